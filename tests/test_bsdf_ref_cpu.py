"""The CPU oracle's BSDFs against the float64 restatement of the reference's formulas (tests/bsdf_ref.py).

Values: every case set of tests/bsdf_cases.py (both tables, every eta_i, both backface values) under the tolerance
C * 2^-24 * kappa * |ref64| with the C measured from the restatement alone, the exclusion rules and their asserted ceilings per set
and per direction class (bsdf_cases.assert_caps); the exact set is under none of them.
Distributions: the oracle's sampler against the float64 pdf by binned counts.
"""
import numpy as np
import pytest

import bsdf_cases as BC
import bsdf_ref as R

SETS = ["%s/eta_i=%g" % (t, e) for t in ("reference", "synthetic") for e in BC.ETA_I]
BRANCH_CAP, ILL_CAP = BC.BRANCH_CAP, BC.ILL_CAP


@pytest.fixture(scope="module")
def scenes(oracle):
    return {"reference": oracle.OracleScene(BC.SCENES + "/mixed32.rendertron"),
            "synthetic": oracle.OracleScene(arrays=BC.scene_arrays(oracle, BC.synthetic_table()[0]))}


def _set(oracle, name):
    return next(cs for cs in BC.all_sets(oracle) if cs.name == name)


def test_synthetic_table_holds_what_it_must():
    T = R.read_table(BC.synthetic_table()[0])
    m, l, d = T["type"] == R.MAT_METAL, T["type"] == R.MAT_LEAF, T["type"] == R.MAT_SMOOTHDIELECTRIC
    f32 = lambda *x: set(np.float32(x).tolist())
    assert len(T["type"]) <= 64 and set(T["type"]) == {0, 1, 2, 4, 6}
    assert f32(0.02, 0.05, 0.15, 0.5, 1.0) <= set(T["roughness"][m].tolist())
    assert np.any(m & np.all(T["k"] == 0, 1)) and np.any(m & np.all(T["eta"] == 1, 1)) and np.any(m & np.any(T["k"] != T["eta"], 1))
    assert {(r, t) for r, t in zip(T["roughness"][l].tolist(), T["transmission"][l].tolist())} >= \
        {(float(np.float32(r)), float(np.float32(t))) for r in (0.05, 0.3, 0.9) for t in (0, 0.15, 1)}
    assert f32(1.0, 1.0001, 1.31, 2.42, 0.75) <= set(T["ior"][d].tolist())
    dif = T["albedo"][T["type"] == R.MAT_DIFFUSE]
    assert np.any(np.all(dif == 0, 1)) and np.any(np.all(dif == 1, 1))
    raw = BC.synthetic_table()[0].reshape(-1, 176)
    assert not raw[:, 0].any() and not raw[:, 16].any()          # hasTexture = hasTransMap = 0


@pytest.mark.parametrize("kind", ["eval", "sample"])
@pytest.mark.parametrize("name", SETS)
def test_oracle_matches_the_restatement(oracle, scenes, name, kind):
    cs = _set(oracle, name)
    assert set(cs.backface.tolist()) == {0, 1}
    ref = BC.restate(cs, kind)
    # the caps hold for the restatement alone, before the oracle is looked at
    skip = R.branch_excluded(ref) & ~cs.exact
    assert skip.mean() <= BRANCH_CAP, (name, kind, skip.mean())
    sc = scenes[cs.table_name]
    if kind == "eval":
        got = BC.unpack_eval(sc.bsdf_eval_n(cs.material, cs.wi, cs.wo, eta_i=cs.eta_i), cs.wo)
    else:
        got = BC.unpack_sample(sc.bsdf_sample_n(cs.material, cs.wi, cs.backface, cs.subseq, eta_i=cs.eta_i))
    res = R.check(ref, got, cs.exact, "%s %s" % (name, kind), ref32=BC.restate(cs, kind, np.float32), cls=cs.cls)
    print(name, kind, res)
    BC.assert_caps(res, name, kind)


def test_batched_probes_equal_the_single_ones(oracle, scenes):
    cs = _set(oracle, "reference/eta_i=1.2")
    pick = np.random.default_rng(3).choice(cs.n, 200, replace=False)
    sc = scenes["reference"]
    a = sc.bsdf_sample_n(cs.material[pick], cs.wi[pick], cs.backface[pick], cs.subseq[pick], eta_i=cs.eta_i)
    b = np.stack([sc.bsdf_sample(int(cs.material[i]), cs.wi[i], bool(cs.backface[i]), eta_i=cs.eta_i, subseq=int(cs.subseq[i])) for i in pick])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    a = sc.bsdf_eval_n(cs.material[pick], cs.wi[pick], cs.wo[pick], eta_i=cs.eta_i)
    b = np.stack([sc.bsdf_eval(int(cs.material[i]), cs.wi[i], cs.wo[i], eta_i=cs.eta_i) for i in pick])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    with pytest.raises(ValueError):
        sc.bsdf_eval_n([24], cs.wi[:1], cs.wo[:1])


def test_measure_reproduces_the_constants(oracle):
    """`python tests/bsdf_ref.py --measure` prints what the module carries, and the binary32 restatement sits inside it."""
    C, rows = R.measure(oracle)
    assert C == R.constants(), (C, R.constants())
    for name, kind, n, branch, ill, _ in rows:
        assert branch <= BRANCH_CAP and ill <= ILL_CAP, (name, kind, branch, ill)


# ---- sampler against pdf ------------------------------------------------------------------------------------------------

N_SAMPLES, NPHI, NZ, QUAD = 20000, 12, 8, 24
Z999 = 3.0902323                                                # standard normal 0.999 quantile


def chi2_999(k):
    """0.999 quantile of chi-square with k degrees of freedom (exact for k <= 2, Wilson-Hilferty above: within 1 %)."""
    if k <= 2:
        return {0: 0.0, 1: 10.828, 2: 13.816}[k]
    return k * (1.0 - 2.0 / (9.0 * k) + Z999 * np.sqrt(2.0 / (9.0 * k))) ** 3


def _wi(theta, phi=0.3):
    return -np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], np.float32)


def _bin_dirs(q):
    """midpoints of a q x q grid in every one of the NPHI x NZ equal-solid-angle bins: [NZ*NPHI*q*q, 3]"""
    z = -1.0 + (np.arange(NZ * q) + 0.5) * (2.0 / (NZ * q))
    p = (np.arange(NPHI * q) + 0.5) * (2.0 * np.pi / (NPHI * q))
    Z, P = np.meshgrid(z, p, indexing="ij")
    s = np.sqrt(1.0 - Z * Z)
    return np.stack([s * np.cos(P), s * np.sin(P), Z], -1).reshape(-1, 3)


def _bin_masses(pdf, q):
    pdf = np.nan_to_num(np.asarray(pdf, np.float64).reshape(NZ, q, NPHI, q), nan=0.0, posinf=0.0, neginf=0.0)
    return pdf.sum(axis=(1, 3)).reshape(-1) * (2.0 / (NZ * q)) * (2.0 * np.pi / (NPHI * q))


def _counts(wo):
    wo = np.asarray(wo, np.float64)
    ok = np.all(np.isfinite(wo), 1)
    wo = wo[ok] / np.linalg.norm(wo[ok], axis=1, keepdims=True)
    iz = np.clip(((wo[:, 2] + 1.0) * 0.5 * NZ).astype(int), 0, NZ - 1)
    ip = np.clip((np.mod(np.arctan2(wo[:, 1], wo[:, 0]), 2 * np.pi) / (2 * np.pi) * NPHI).astype(int), 0, NPHI - 1)
    return np.bincount(iz * NPHI + ip, minlength=NZ * NPHI).astype(np.float64)


def _chi2(counts, mass):
    """chi-square of the counts against N * mass; bins expecting fewer than 5 are pooled. -> (statistic, dof).
    The counts sum to N, so k bins leave k - 1 degrees of freedom."""
    E = N_SAMPLES * mass
    big = E >= 5.0
    o, e = list(counts[big]), list(E[big])
    if (~big).any() and E[~big].sum() > 0:
        o.append(counts[~big].sum()); e.append(E[~big].sum())
    elif (~big).any() and counts[~big].sum() > 0:
        return np.inf, max(len(e) - 1, 1)
    o, e = np.array(o), np.array(e)
    return float(((o - e) ** 2 / e).sum()), max(len(e) - 1, 1)


# A GGX lobe of roughness <= 0.05 (alpha <= 0.0025 rad) is narrower than the sphere quadrature's spacing (0.01 x 0.02 rad). Its
# core is cut out of the 12 x 8 bins and binned on its own, in the half-vector's coordinates (s, phi_h) with
# s = tan^2 / (alpha^2 + tan^2) of theta_h, s < S_MAX, in which the lobe is flat: LOBE_S x LOBE_PHI bins, each integrated by
# midpoints in (theta_h, phi_h) of pdf(wo(h)) * 4 (wo . h) sin(theta_h) - the 4 (wo . h) is d omega_o / d omega_h of a
# reflection about h, geometry and no part of the reference. The sphere bins then hold (samples and quadrature points alike) only
# what lies outside the core: 0.1 % of the lobe.
LOBE_ROUGHNESS, S_MAX, LOBE_S, LOBE_PHI = 0.05, 0.999, 4, 6


def _lobe_coords(wi, wo, alpha):
    """-> (in the lobe's core, s, phi_h) of directions wo for the incoming wi (into the surface)"""
    h = -np.asarray(wi, np.float64) + np.asarray(wo, np.float64)
    with np.errstate(all="ignore"):
        h = h / np.linalg.norm(h, axis=1, keepdims=True)
        t2 = (1.0 - h[:, 2] ** 2) / h[:, 2] ** 2
        s = t2 / (alpha * alpha + t2)
    core = np.isfinite(s) & (h[:, 2] > 0) & (s < S_MAX)
    return core, s, np.mod(np.arctan2(h[:, 1], h[:, 0]), 2 * np.pi)


def _lobe_counts(wi, wo, alpha):
    wo = np.asarray(wo, np.float64)
    core, s, ph = _lobe_coords(wi, wo, alpha)
    core &= np.all(np.isfinite(wo), 1)
    i = np.clip((s[core] / S_MAX * LOBE_S).astype(int), 0, LOBE_S - 1) * LOBE_PHI + np.clip((ph[core] / (2 * np.pi) * LOBE_PHI).astype(int), 0, LOBE_PHI - 1)
    return np.bincount(i, minlength=LOBE_S * LOBE_PHI).astype(np.float64), core


LOBE_Q_THETA = 8            # theta_h nodes per s-bin, in multiples of q: a bin of the core spans up to 30 alpha


def _lobe_points(wi, alpha, q):
    """midpoints in (theta_h, phi_h) of the core's bins -> (wo [n, 3], weight of each point's pdf in its bin's integral).
    Uniform in theta_h inside every s-bin: that resolves the lobe (scale alpha) and the smooth diffuse part alike."""
    qt = LOBE_Q_THETA * q
    edges = np.arctan(alpha * np.sqrt((np.arange(LOBE_S + 1) * S_MAX / LOBE_S) / (1.0 - np.arange(LOBE_S + 1) * S_MAX / LOBE_S)))
    th = np.concatenate([lo + (np.arange(qt) + 0.5) * (hi - lo) / qt for lo, hi in zip(edges[:-1], edges[1:])])
    dth = np.concatenate([np.full(qt, (hi - lo) / qt) for lo, hi in zip(edges[:-1], edges[1:])])
    p = (np.arange(LOBE_PHI * q) + 0.5) * (2 * np.pi / (LOBE_PHI * q))
    TH, P = (x.reshape(-1) for x in np.meshgrid(th, p, indexing="ij"))
    DTH = np.repeat(dth, len(p))
    h = np.stack([np.sin(TH) * np.cos(P), np.sin(TH) * np.sin(P), np.cos(TH)], 1)
    w = -np.asarray(wi, np.float64)
    wo = 2.0 * (h @ w)[:, None] * h - w
    jac = 4.0 * np.sum(wo * h, 1) * np.sin(TH) * DTH * (2 * np.pi / (LOBE_PHI * q))
    assert np.all(wo[:, 2] > 0)                                 # the core stays above the horizon: no flip inside it
    return wo, jac


def _lobe_masses(pdf, jac, q):
    v = np.nan_to_num(np.asarray(pdf, np.float64) * jac, nan=0.0, posinf=0.0, neginf=0.0)
    return v.reshape(LOBE_S, LOBE_Q_THETA * q, LOBE_PHI, q).sum(axis=(1, 3)).reshape(-1)


# (row, theta_i) whose float64 sampler does not follow the float64 pdf: reference behaviour that is recorded, not fixed.
# mass = the integral of the float64 pdf over the sphere by the quadrature above.
#   "clamp":   leaf_pdf clamps F to 1 - 0.1 roughness (:472) where leaf_sample_f uses F itself (:510)
#   "horizon": leaf_sample_f keeps the specular lobe's directions below the horizon (no flip, :526), and leaf_pdf gives them the
#              transmission arm's pdf, which is 0 where transmission is 0 (statistic inf: samples where the pdf has no mass)
KNOWN_INCONSISTENT = {
    ("reference 16", 0.9): (0.9828, "clamp"),                   # leafAutumn r=0.8 t=0.6   chi2 147.3 / 95 dof
    ("leaf r=0.3 t=0 ior=2.42", 0.3): (0.9986, "horizon"),      # chi2 inf
    ("leaf r=0.3 t=0 ior=2.42", 0.9): (0.9964, "horizon"),      # chi2 inf
    ("leaf r=0.3 t=0.15 ior=2.42", 0.9): (0.9964, "horizon"),   # chi2 165.3 / 95 dof
    ("leaf r=0.9 t=0 ior=1.333", 0.3): (0.9918, "horizon"),     # chi2 inf
    ("leaf r=0.9 t=0 ior=1.333", 0.9): (0.9878, "horizon"),     # chi2 inf
    ("leaf r=0.9 t=0.15 ior=1.333", 0.9): (0.9878, "clamp"),    # chi2 233.0 / 95 dof
}
# (row, theta_i) where the float64 sampler follows the pdf (chi2 22 / 25 dof) and the reference's sampling formula evaluated in
# binary32 does not: at roughness 0.02, alpha^4 = 2.6e-14 and alpha^2 = 1.6e-7 lie below 2^-24, so `1 + (alpha*alpha - 1) u1`
# (:167) is `1 - u1` and `1 - cosTheta*cosTheta` (:168) takes a handful of values: sin(theta_h) is 0, 2.4e-4, 3.5e-4, ... against a
# lobe of width 4e-4. The restatement's own binary32 run shows it (chi2 16695); the oracle has to show the same, bin for bin.
BINARY32_COARSE = {("metal gold r=0.02", 0.3), ("metal gold r=0.02", 0.9)}


def _chi_rows():
    T = R.read_table(BC.synthetic_table()[0])
    syn = [int(i) for i in np.flatnonzero(np.isin(T["type"], (R.MAT_METAL, R.MAT_LEAF)) & (T["roughness"] <= np.float32(0.3)))]
    # the autumn leaf (row 16) and the roughness-0.9 leaves are not among the rows to assert; they are measured as the known examples
    rough = [int(i) for i in np.flatnonzero((T["type"] == R.MAT_LEAF) & (T["roughness"] == np.float32(0.9)))]
    return [("reference", r) for r in (2, 7, 13, 16)] + [("synthetic", r) for r in syn + rough]


@pytest.fixture(scope="module")
def chi_uniforms(oracle):
    return BC.uniforms(oracle, np.arange(N_SAMPLES) + (1 << 20))


def _tables(oracle):
    return {"reference": BC.reference_table(oracle), "synthetic": BC.synthetic_table()[0]}


def _describe(table_name, row):
    return "reference %d" % row if table_name == "reference" else BC.synthetic_table()[1][row]


def chi_case(oracle, scenes, u, table_name, row, theta):
    """-> dict of the float64 sampler's and the oracle's statistics against the float64 pdf."""
    table = _tables(oracle)[table_name]
    T = R.read_table(table)
    alpha = float(T["roughness"][row]) ** 2
    narrow = T["type"][row] in (R.MAT_METAL, R.MAT_LEAF) and T["roughness"][row] <= np.float32(LOBE_ROUGHNESS)
    wi = _wi(theta)
    mats = lambda n: np.full(n, row, np.int32)
    tile = lambda n: np.tile(wi, (n, 1))
    pdf64 = lambda d: R.evaluate(table, mats(len(d)), tile(len(d)), d.astype(np.float32), 1.0)["pdf"][:, 0]
    pdfo = lambda d: scenes[table_name].bsdf_eval_n(mats(len(d)), tile(len(d)), d.astype(np.float32), eta_i=1.0)[:, 3]

    def masses(pdf, q):
        d = _bin_dirs(q)
        v = pdf(d)
        if not narrow:
            return _bin_masses(v, q)
        v = np.where(_lobe_coords(tile(len(d)), d, alpha)[0], 0.0, v)
        lw, jac = _lobe_points(wi, alpha, q)
        return np.concatenate([_bin_masses(v, q), _lobe_masses(pdf(lw), jac, q)])

    def counts(wo):
        if not narrow:
            return _counts(wo)
        lobe, core = _lobe_counts(tile(len(wo)), wo, alpha)
        return np.concatenate([_counts(np.asarray(wo)[~core]), lobe])

    mass, mass2 = masses(pdf64, QUAD), masses(pdf64, QUAD // 2)
    sub = (np.arange(N_SAMPLES) + (1 << 20)).astype(np.uint32)
    back = np.zeros(N_SAMPLES, np.int32)
    s64 = R.sample(table, mats(N_SAMPLES), tile(N_SAMPLES), back, 1.0, u)
    so = scenes[table_name].bsdf_sample_n(mats(N_SAMPLES), tile(N_SAMPLES), back, sub, eta_i=1.0)
    s32 = R.sample(table, mats(N_SAMPLES), tile(N_SAMPLES), back, 1.0, u, np.float32)
    n64, no, n32 = counts(s64["wo"]), counts(so[:, 0:3]), counts(s32["wo"])
    c64, dof = _chi2(n64, mass)
    co, _ = _chi2(no, mass)
    c32, _ = _chi2(n32, mass)
    return dict(chi64=c64, chio=co, dof=dof, mass=float(mass.sum()), quad_err=abs(float(mass.sum() - mass2.sum())),
                mass_oracle=float(masses(pdfo, QUAD).sum()), moved=float(np.abs(n64 - no).sum() / 2), chi32=c32,
                moved32=float(np.abs(n32 - no).sum() / 2))


@pytest.mark.parametrize("theta", [0.3, 0.9])
@pytest.mark.parametrize("table_name,row", _chi_rows())
def test_sampler_follows_the_pdf(oracle, scenes, chi_uniforms, table_name, row, theta):
    r = chi_case(oracle, scenes, chi_uniforms, table_name, row, theta)
    key = (_describe(table_name, row), theta)
    print("%r: chi2 float64 %.1f oracle %.1f / %d dof (limit %.1f), pdf mass %.4f (oracle %.4f, quadrature +- %.4f), %d samples in another bin (binary32 restatement: chi2 %.1f, %d)"
          % (key, r["chi64"], r["chio"], r["dof"], chi2_999(r["dof"]), r["mass"], r["mass_oracle"], r["quad_err"], r["moved"], r["chi32"], r["moved32"]))
    limit = chi2_999(r["dof"])
    # the oracle's samples are the binary32 restatement's: only a sample within rounding of a bin's edge may change bins
    assert r["moved32"] <= 1e-3 * N_SAMPLES, r
    known = KNOWN_INCONSISTENT.get(key)
    assert (r["chi64"] < limit) == (known is None), "KNOWN_INCONSISTENT is out of date for %r: %r" % (key, r)
    if known is not None:
        mass, reason = known
        assert abs(r["mass"] - mass) < 5e-4, r                  # the table carries what the restatement gives
        assert abs(r["mass_oracle"] - mass) <= r["quad_err"] + 5e-4, r
        assert np.isinf(r["chio"]) == np.isinf(r["chi64"]) and (np.isinf(r["chio"]) or abs(r["chio"] - r["chi64"]) <= 0.05 * r["chi64"]), r
    elif key in BINARY32_COARSE:
        assert r["chi32"] >= limit, "BINARY32_COARSE is out of date for %r: %r" % (key, r)
        assert abs(r["chio"] - r["chi32"]) <= 0.05 * r["chi32"], r
    else:
        assert r["chi32"] < limit, "BINARY32_COARSE is out of date for %r: %r" % (key, r)
        assert r["chio"] < limit, r
