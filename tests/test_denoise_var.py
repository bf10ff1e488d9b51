"""pt_denoise_var on the GPU against its numpy restatement (tests/denoise_var_ref.py), and what it does to image error next to
pt_denoise on the frames of tests/test_denoise.py."""
import os

import numpy as np
import pytest

from denoise_ref import mse, passthrough_mask
from denoise_var_ref import denoise_var as denoise_var_ref
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SEED = 103033


def _cornell(api, scene_dir, name, w, h, **kw):
    from cudapathtracer_amd import scenes
    cfg = scenes.cornell(os.path.join(scene_dir, name), width=w, height=h, name=name, **kw)["config"]
    hs = api.HostScene(cfg)
    return api.Scene(hs), hs.camera()


def _check_against_numpy(api, S, Q, spp, batches, A, N, iterations):
    kw = {} if iterations is None else {"iterations": iterations}
    got = api.denoise_var(S, Q, spp, batches, A, N, **kw)
    d = api.denoise_var_defaults()
    want, skip, L = denoise_var_ref(S, Q, spp, batches, A, N, iterations=d["iterations"] if iterations is None else iterations,
                                    sigma_var=d["sigma_var"], sigma_normal=d["sigma_normal"], sigma_depth=d["sigma_depth"])
    assert_bits_equal(got[skip], S[skip], "pass-through pixels")
    assert_bits_equal(got[..., 3], S[..., 3], "w channel")
    use = ~skip
    err = np.abs(got[use][:, :3] - want[use][:, :3])
    print("iterations %s: max |got - want| = %.3g of atol %.3g; max relative %.3g" % (
        iterations, err.max(), 1e-6 * L * spp, (err / np.maximum(np.abs(want[use][:, :3]), 1e-30)).max()))
    np.testing.assert_allclose(got[use][:, :3], want[use][:, :3], rtol=1e-3, atol=1e-6 * L * spp)
    return got, skip


@pytest.fixture(scope="module")
def frame64(api, gpu_ready, scene_dir):
    gs, cam = _cornell(api, scene_dir, "dv64", 64, 48, spp=4, max_depth=4)
    S, Q = gs.render_moments(cam, 64, 48, 8, 2, 4)
    A, N = gs.render_aovs(cam, 64, 48, aov_spp=2)
    return S, Q, A, N


@pytest.mark.parametrize("iterations", [0, 1, None])
def test_denoise_var_matches_numpy(api, frame64, iterations):
    S, Q, A, N = frame64
    got, skip = _check_against_numpy(api, S, Q, 8, 4, A, N, iterations)
    assert (~skip).sum() > 0.9 * skip.size
    if iterations != 0:
        assert not np.array_equal(got, S)


def test_nan_inf_and_miss_pixels_pass_through(api, frame64):
    S, Q, A, N = frame64
    S = S.copy(); A = A.copy(); Q = Q.copy()
    S[5, 7, 0] = np.nan; S[20, 30, 1] = np.inf; S[40, 2, 2] = -np.inf; S[41, 2, :3] = np.nan
    Q[30, 9, 1] = np.nan; Q[31, 9, 2] = np.inf                # a non-finite variance passes through as well
    A[10:18, 40:52, 3] = 0.0                              # a miss region: coverage 0
    got, skip = _check_against_numpy(api, S, Q, 8, 4, A, N, None)
    assert skip[5, 7] and skip[20, 30] and skip[40, 2] and skip[41, 2] and skip[10:18, 40:52].all() and skip[30, 9] and skip[31, 9]
    fin = api.finalise(got, 8)                            # novum_finalise still paints them
    assert np.allclose(fin[5, 7, :3], (1, 0, 1)) and np.allclose(fin[20, 30, :3], (0, 1, 0))


def test_out_may_alias_in_and_device_form_is_the_host_form(api, gpu_ready, frame64):
    torch = gpu_ready
    S, Q, A, N = frame64
    h, w = S.shape[:2]
    want = api.denoise_var(S, Q, 8, 4, A, N)
    inplace = S.copy()
    api.denoise_var(inplace, Q, 8, 4, A, N, out=inplace)
    assert_bits_equal(inplace, want, "host, out = in")
    dS, dQ, dA, dN = (torch.from_numpy(x.copy()).to("cuda:0") for x in (S, Q, A, N))
    ws = torch.empty(api.denoise_var_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    out = torch.full_like(dS, 3.0)
    api.denoise_var_device(w, h, dS.data_ptr(), dQ.data_ptr(), 8, 4, dA.data_ptr(), dN.data_ptr(), ws.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert_bits_equal(out.cpu().numpy(), want, "device form")
    api.denoise_var_device(w, h, dS.data_ptr(), dQ.data_ptr(), 8, 4, dA.data_ptr(), dN.data_ptr(), ws.data_ptr(), dS.data_ptr())
    torch.cuda.synchronize()
    assert_bits_equal(dS.cpu().numpy(), want, "device form, out = in")


# mse(var) / mse(raw) of the numpy restatement with the library's defaults on exactly these frames (they are the CPU reference's
# frames bit for bit, so the restatement runs without a GPU; the sweep is in DESIGN.md §9): the ceiling is that value times
# 1.05 for the kernel's f32 arithmetic.
RESTATEMENT_RATIO = {"dnq_diffuse": 0.4087, "dnq_specular": 0.5050}     # (pt_denoise on the same frames: 0.739, 0.806)


def _quality(api, scene_dir, name, **kw):
    """The frames of test_denoise.py::_quality: Cornell 128 x 128, depth 8, MIS, raw 16 spp (here as 4 batches of 4), reference
    4096 spp (another seed, here as 16 batches of 256), features at 4 rays per pixel. Returns the MSEs against the reference."""
    gs, cam = _cornell(api, scene_dir, name, 128, 128, spp=16, max_depth=8, **kw)
    raw, Q = gs.render_moments(cam, 128, 128, 16, 4, 8)
    ref, Qref = gs.render_moments(cam, 128, 128, 4096, 256, 8, seed=777)
    A, N = gs.render_aovs(cam, 128, 128, aov_spp=4)
    mask = ~passthrough_mask(raw, 16, A) & ~passthrough_mask(ref, 4096, A)
    refm = ref / 4096
    m = {"raw": mse(raw / 16, refm, mask),
         "classic": mse(api.denoise(raw, 16, A, N) / 16, refm, mask),
         "var": mse(api.denoise_var(raw, Q, 16, 4, A, N) / 16, refm, mask),
         "classic_conv": mse(api.denoise(ref, 4096, A, N) / 4096, refm, mask),
         "var_conv": mse(api.denoise_var(ref, Qref, 4096, 16, A, N) / 4096, refm, mask)}
    print("%s: MSE raw16 %.5g; classic %.5g (ratio %.3f), variance-guided %.5g (ratio %.3f, %.3f of classic); "
          "converged image: classic %.5g (ratio %.4f), variance-guided %.5g (ratio %.4f)" % (
              name, m["raw"], m["classic"], m["classic"] / m["raw"], m["var"], m["var"] / m["raw"], m["var"] / m["classic"],
              m["classic_conv"], m["classic_conv"] / m["raw"], m["var_conv"], m["var_conv"] / m["raw"]))
    assert m["var"] <= 0.85 * m["classic"]
    assert m["var_conv"] <= m["classic_conv"]             # a converged image is blurred less than by the classic filter
    assert m["var"] <= 1.05 * RESTATEMENT_RATIO[name] * m["raw"]
    return m


def test_quality_diffuse_cornell(api, gpu_ready, scene_dir):
    _quality(api, scene_dir, "dnq_diffuse")


def test_quality_specular_cornell(api, gpu_ready, scene_dir):
    _quality(api, scene_dir, "dnq_specular", tall_material=5, short_material=19)     # glass, mirror


def test_full_hd_moments_aovs_and_denoise_var(api, gpu_ready, scene_dir):
    torch = gpu_ready
    w, h = 1920, 1080
    gs, cam = _cornell(api, scene_dir, "dvhd", w, h, spp=4, max_depth=4)
    S, Q = gs.render_moments(cam, w, h, 4, 2, 4)
    A, N = gs.render_aovs(cam, w, h)
    host = api.denoise_var(S, Q, 4, 2, A, N)
    assert not np.array_equal(host, S)
    dS = torch.empty(h, w, 4, device="cuda:0"); dQ = torch.empty(h, w, 4, device="cuda:0")
    gs.render_moments_device(cam, w, h, 4, 2, 4, dS.data_ptr(), dQ.data_ptr())
    dA = torch.empty(h, w, 4, device="cuda:0"); dN = torch.empty(h, w, 4, device="cuda:0")
    gs.render_aovs_device(cam, w, h, dA.data_ptr(), dN.data_ptr())
    ws = torch.empty(api.denoise_var_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    out = torch.empty_like(dS)
    api.denoise_var_device(w, h, dS.data_ptr(), dQ.data_ptr(), 4, 2, dA.data_ptr(), dN.data_ptr(), ws.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert_bits_equal(dS.cpu().numpy(), S, "sums")
    assert_bits_equal(dQ.cpu().numpy(), Q, "squared batch sums")
    assert_bits_equal(out.cpu().numpy(), host, "device vs host denoise_var")
