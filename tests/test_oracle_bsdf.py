"""BSDF restatement: energy and pdf checks on the reference's material table (main.cu:443-467)."""
import numpy as np

import bsdf_cases as BC
import bsdf_ref as R
from conftest import golden_scene


def _wi(theta, phi=0.3):
    # local direction INTO the surface (the convention of sample_f_eval's wi argument)
    return -np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], np.float32)


def test_lambert_white_furnace(oracle):
    sc = oracle.OracleScene(golden_scene("cornell32"))
    for mat, albedo in ((2, (0.9, 0.9, 0.9)), (6, (0.9, 0.1, 0.1)), (23, (0.1, 0.9, 0.1))):
        for k in range(200):
            o = sc.bsdf_sample(mat, _wi(0.7), subseq=k)
            wo, f, pdf, draws = o[0:3], o[3:6], o[6], o[7]
            assert draws == 2 and wo[2] > 0 and abs(np.linalg.norm(wo) - 1) < 1e-5
            # f*cos/pdf == albedo for cosine sampling (unless the pdf floor max(z, eps) bites)
            assert np.allclose(f * wo[2] / pdf, albedo, rtol=2e-5)
            ev = sc.bsdf_eval(mat, _wi(0.7), wo)
            assert np.array_equal(ev[:3], f) and ev[3] == pdf


def test_mirror_and_dielectric(oracle):
    sc = oracle.OracleScene(golden_scene("mixed32"))
    wi = _wi(0.5)
    o = sc.bsdf_sample(19, wi, subseq=1)
    assert o[7] == 0 and np.allclose(o[0:3], [wi[0], wi[1], -wi[2]]) and o[6] == 1.0
    assert np.allclose(o[3:6] * o[2], 1.0)          # f * cos = 1
    n_refl = n_refr = 0
    for k in range(400):
        o = sc.bsdf_sample(5, wi, backface=False, subseq=k)
        assert o[7] == 1
        if o[2] > 0:
            n_refl += 1
            assert np.allclose(o[3:6] * o[2] / o[6], 1.0, rtol=1e-5)
        else:
            n_refr += 1
            eta = 1.0 / 1.5
            assert np.allclose(o[3:6] * abs(o[2]) / o[6], eta * eta, rtol=1e-5)
    assert n_refr > n_refl > 0
    # total internal reflection from inside at a grazing angle: no draw, pdf 1
    o = sc.bsdf_sample(5, _wi(1.3), backface=True, subseq=3)
    assert o[7] == 0 and o[6] == 1.0 and o[2] > 0


def test_ggx_metal(oracle):
    sc = oracle.OracleScene(golden_scene("metal32"))
    wi = _wi(0.6)
    n = 300
    out = np.stack([sc.bsdf_sample(7, wi, subseq=k) for k in range(n)])
    for o in out:
        assert o[7] == 2 and o[2] > 0
        ev = sc.bsdf_eval(7, wi, o[0:3])
        assert np.array_equal(ev[:3], o[3:6]) and ev[3] == o[6]
    # Fresnel-weighted reflectance of a rough conductor: the float64 restatement's weights for the same 300 subsequences,
    # each within C_WEIGHT * 2^-24 * kappa * |ref64| (tests/bsdf_ref.py), and so their mean within the mean of those tolerances
    ref = R.sample(sc.array("materials"), np.full(n, 7), np.tile(wi, (n, 1)), np.zeros(n, int), 1.0, BC.uniforms(oracle, np.arange(n)))
    assert not R.branch_excluded(ref).any() and R.weight_resolved(ref).all() and np.all(ref["pdf"] > 0) and np.all(out[:, 6] > 0)
    R.check(ref, BC.unpack_sample(out), what="steel, theta_i = 0.6")
    w = out[:, 3:6].astype(np.float64) * out[:, 2:3] / out[:, 6:7]
    tol = (R.C_WEIGHT * R.EPS24 * ref["weight_a"]).mean(axis=0)
    assert np.all(np.abs(w.mean(axis=0) - ref["weight"].mean(axis=0)) <= tol), (w.mean(axis=0), ref["weight"].mean(axis=0), tol)
    assert np.all(tol < 2e-2 * ref["weight"].mean(axis=0))      # under 2 %, against the 0.2 .. 1.3 this replaces


def test_unhandled_material_types_leave_outputs(oracle):
    sc = oracle.OracleScene(golden_scene("cornell32"))
    ev = sc.bsdf_eval(5, _wi(0.4), np.array([0, 0, 1], np.float32))     # dielectric: f_eval writes nothing, pdf 0
    assert np.array_equal(ev, [0, 0, 0, 0])
