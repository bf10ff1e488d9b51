"""Live probe grids without a GPU (pt_grid_classify, pt_grid_update, pt_grid_irradiance_states): the symbols, the
constants and the Python names; every argument check of the six functions in the header's order (they fire before any HIP call,
under the function's name); tests/grid_live_ref.py's f32 restatement against grid_ref's (all states 0, a dead probe against a
zeroed map), against rays.grid_irradiance(states=...) in float64, and on its own rules for update and classify; and the resources of
the new kernels, read from the code-object notes, against §30's table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import grid_live_ref as GL
import grid_ref as GR
from util import assert_bits_equal

F = np.float32
CLS, UPD, LKS = "pt_grid_classify", "pt_grid_update", "pt_grid_irradiance_states"
INF, NAN = float("inf"), float("nan")
GOOD = dict(lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), counts=(2, 2, 2), sh_samples=64, map_res=4, map_samples=2, power=3)


def _err(api):
    return api.lib().pt_last_error().decode()


def _desc(api, **change):
    a = dict(GOOD, **change)
    return api.grid_desc(a["lo"], a["hi"], a["counts"], a["sh_samples"], a["map_res"], a["map_samples"], a["power"])


def test_new_symbols_constants_and_names(api):
    from conftest import ROOT
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for n in ("pt_grid_classify", "pt_grid_classify_device", "pt_grid_update", "pt_grid_update_device", "pt_grid_irradiance_states",
              "pt_grid_irradiance_states_device"):
        assert hasattr(L, n), n
        assert "int " + n + "(" in header, n
        assert getattr(L, n).argtypes, n
    assert "#define PT_PROBE_INSIDE 1u" in header and "#define PT_PROBE_IDLE   2u" in header
    assert (api.PROBE_INSIDE, api.PROBE_IDLE) == (1, 2) == (GL.INSIDE, GL.IDLE)
    for n in ("grid_classify", "grid_update", "grid_irradiance"):
        assert hasattr(api, n), n
    for n in ("classify", "update", "bake", "lookup"):
        assert hasattr(api.ProbeGrid, n), n
    import inspect
    from cudapathtracer_amd import rays
    assert inspect.signature(api.grid_irradiance).parameters["states"].default is None
    assert inspect.signature(rays.grid_irradiance).parameters["states"].default is None
    assert inspect.signature(api.grid_classify).parameters["back_fraction"].default == 0.25
    assert inspect.signature(api.ProbeGrid.update).parameters["hysteresis"].default == 0.9


# ---- the checks -----------------------------------------------------------------------------------------------------------------
# (a desc that one of grid_params' checks refuses, what later desc checks refuse as well, the message), in the checks' order
DESC_CASES = [(dict(counts=(0, 2, 2)), dict(lo=(NAN, 0.0, 0.0), sh_samples=0, power=0), "counts 0 x 2 x 2 must be at least 1 each"),
              (dict(counts=(2048, 2048, 2)), dict(sh_samples=0, map_res=3), "make more than 4194304 probes"),
              (dict(lo=(0.0, NAN, 0.0)), dict(sh_samples=0, power=0), "is not finite"),
              (dict(hi=(0.0, 1.0, 1.0)), dict(map_samples=0, power=0), "hi[0] = 0 must be above lo[0] = 0"),
              (dict(sh_samples=0), dict(map_res=5, power=0), "sh_samples 0 must be at least 1"),
              (dict(map_res=5), dict(map_samples=0, power=0), "map_res 5 must be 0, 4, 8, 16 or 32"),
              (dict(map_samples=0), dict(power=0), "map_samples 0 must be at least 1"),
              (dict(power=9), {}, "power 9 must be 1..8")]


def _buffers():
    """Host buffers of the 2 x 2 x 2 grid at R = 4, pre-filled: nothing a refused call is given may change."""
    b = dict(idx=np.arange(8, dtype=np.int32), sums=np.full(8 * 36, 3.0, F), maps=np.full(8 * 16 * 4, 5.0, F),
             packed=np.full(8 * 36 + 8 * 36 * 2 + 8, 77.0, F), states=np.full(8, 9, np.uint32), recs=np.zeros((5, 8), F), out=np.full((5, 4), 77.0, F))
    return b, {k: v.ctypes.data for k, v in b.items()}


def _unchanged(b):
    return (b["packed"] == 77).all() and (b["out"] == 77).all() and (b["states"] == 9).all() and (b["sums"] == 3).all() and (b["maps"] == 5).all()


def _forms(api, p):
    """name -> (argument names in the call's order, the good arguments, host form, device form)."""
    L = api.lib()
    return {CLS: (("desc", "k", "idx", "maps", "bf", "states"), dict(desc={}, k=8, idx=p["idx"], maps=p["maps"], bf=0.25, states=p["states"]),
                  L.pt_grid_classify, L.pt_grid_classify_device),
            UPD: (("desc", "k", "idx", "sums", "maps", "h", "packed"), dict(desc={}, k=8, idx=p["idx"], sums=p["sums"], maps=p["maps"], h=0.5, packed=p["packed"]),
                  L.pt_grid_update, L.pt_grid_update_device),
            LKS: (("desc", "packed", "states", "m", "recs", "out"), dict(desc={}, packed=p["packed"], states=p["states"], m=5, recs=p["recs"], out=p["out"]),
                  L.pt_grid_irradiance_states, L.pt_grid_irradiance_states_device)}


def _call(api, fn, order, a, tail):
    d = a["desc"]
    return fn(None if d is None else C.byref(_desc(api, **d)), *[a[k] for k in order[1:]], *tail)


def _refused(api, name, forms, a, msg, exact=True):
    order, _, host, dev = forms[name]
    for fn, tail in ((host, ()), (dev, (None,))):
        assert _call(api, fn, order, a, tail) == -1, (name, a)
        e = _err(api)
        assert (e == name + ": " + msg) if exact else (e.startswith(name + ": ") and msg in e), (name, a, e)


# per function its own checks after the desc's, in the header's order: (what breaks, the message)
OWN = {
    CLS: [(dict(desc=dict(map_res=0)), "map_res is 0: a grid without maps has nothing to classify"),
          (dict(k=-1), "k -1 must not be negative"),
          (dict(k=9), "k 9 lists more than the grid's 8 probes"),
          (dict(k=5, idx=None), "null indices need k == 8, the grid's probes, not 5"),
          (dict(bf=NAN), "back_fraction nan must be in [0, 1]"),
          (dict(maps=None), "null maps"),
          (dict(states=None), "null states")],
    UPD: [(dict(k=-3), "k -3 must not be negative"),
          (dict(k=9), "k 9 lists more than the grid's 8 probes"),
          (dict(k=7, idx=None), "null indices need k == 8, the grid's probes, not 7"),
          (dict(h=1.0), "hysteresis 1 must be in [0, 1)"),
          (dict(sums=None), "null coeff_sums"),
          (dict(packed=None), "null packed buffer"),
          (dict(maps=None), "null maps although map_res is 4")],
    LKS: [(dict(m=-1), "m -1 must not be negative"),
          (dict(packed=None), "null packed buffer"),
          (dict(states=None), "null states"),
          (dict(recs=None), "null records"),
          (dict(out=None), "null output buffer")],
}


def _later(breaks):
    """The breaks merged so that the earliest wins each argument: what all the later checks refuse, together."""
    out = {}
    for b, _ in reversed(breaks):
        out.update(b)
    return out


def test_the_desc_checks_come_first_from_all_six_functions(api):
    b, p = _buffers()
    forms = _forms(api, p)
    for name, (order, good, _, _) in forms.items():
        own = _later(OWN[name])
        own.pop("desc", None)
        for a in (dict(good, desc=None), dict(good, **dict(own, desc=None))):
            _refused(api, name, forms, a, "null desc")
        for change, also, msg in DESC_CASES:
            for extra in ({}, also):
                d = dict(extra, **change)
                for a in (dict(good, desc=d), dict(good, **dict(own, desc=d))):
                    _refused(api, name, forms, a, msg, exact=False)
    assert _unchanged(b)


@pytest.mark.parametrize("name", [CLS, UPD, LKS])
def test_each_functions_own_checks_alone_and_in_order(api, name):
    """Each check's break alone, and together with everything the later checks refuse: the earliest broken check answers, from the
    host form and the device form."""
    b, p = _buffers()
    forms = _forms(api, p)
    good = forms[name][1]
    for i, (brk, msg) in enumerate(OWN[name]):
        for a in (dict(good, **brk), dict(dict(good, **_later(OWN[name][i + 1:])), **brk)):
            _refused(api, name, forms, a, msg)
    assert _unchanged(b)


def test_the_ranges_the_count_of_zero_and_the_overlaps(api):
    b, p = _buffers()
    forms = _forms(api, p)
    L = api.lib()
    for bf in (NAN, INF, -INF, -0.125, 1.5):
        _refused(api, CLS, forms, dict(forms[CLS][1], bf=bf), "back_fraction", exact=False)
    for h in (NAN, INF, -INF, -0.125, 1.0, 1.5):
        _refused(api, UPD, forms, dict(forms[UPD][1], h=h), "hysteresis", exact=False)
    _refused(api, UPD, forms, dict(forms[UPD][1], desc=dict(map_res=0)), "maps given although map_res is 0")
    d4, d0 = C.byref(_desc(api)), C.byref(_desc(api, map_res=0, map_samples=0))
    # k == 0 (m == 0): 0 after the desc's checks (and classify's map_res), whatever comes after: NULL buffers, a value out of range
    for d in (d4, d0):
        assert L.pt_grid_update(d, 0, None, None, None, NAN, None) == 0 and L.pt_grid_update_device(d, 0, None, None, None, 2.0, None, None) == 0
        assert L.pt_grid_irradiance_states(d, None, None, 0, None, None) == 0 and L.pt_grid_irradiance_states_device(d, None, None, 0, None, None, None) == 0
    assert L.pt_grid_classify(d4, 0, None, None, NAN, None) == 0 and L.pt_grid_classify_device(d4, 0, None, None, -1.0, None, None) == 0
    assert L.pt_grid_classify(d0, 0, None, None, 0.25, None) == -1 and _err(api).startswith(CLS + ": map_res is 0")
    bad = C.byref(_desc(api, power=0))
    assert L.pt_grid_update(bad, 0, None, None, None, 0.5, None) == -1 and "power 0" in _err(api)
    # the ends of the ranges are inside
    assert L.pt_grid_classify(d4, 8, None, None, 0.0, None) == -1 and _err(api) == CLS + ": null maps"
    assert L.pt_grid_classify(d4, 8, None, None, 1.0, None) == -1 and _err(api) == CLS + ": null maps"
    assert L.pt_grid_update(d4, 8, None, None, None, 0.0, None) == -1 and _err(api) == UPD + ": null coeff_sums"
    # the device forms: a written buffer over a read one, checked last
    pk_bytes = api.grid_packed_bytes(_desc(api))
    for args in ((d4, 8, p["idx"], p["maps"], 0.25, p["maps"]), (d4, 8, p["idx"], p["maps"], 0.25, p["maps"] + 8 * 16 * 16 - 4),
                 (d4, 8, p["idx"], p["maps"], 0.25, p["idx"] + 28), (d4, 2, p["states"] + 24, p["maps"], 0.25, p["states"])):
        assert L.pt_grid_classify_device(*args, None) == -1 and _err(api) == CLS + ": the states overlap an input", (args, _err(api))
    for args in ((d4, 8, p["idx"], p["sums"], p["maps"], 0.5, p["sums"]), (d4, 8, p["idx"], p["sums"], p["maps"], 0.5, p["maps"] + 16),
                 (d4, 8, p["packed"] + pk_bytes - 4, p["sums"], p["maps"], 0.5, p["packed"]), (d0, 8, None, p["sums"] + 8 * 144 - 4, None, 0.5, p["sums"])):
        assert L.pt_grid_update_device(*args, None) == -1 and _err(api) == UPD + ": the packed buffer overlaps an input", (args, _err(api))
    for args in ((d4, p["packed"], p["states"], 5, p["recs"], p["recs"] + 5 * 32 - 4), (d4, p["packed"], p["states"], 5, p["recs"], p["packed"] + pk_bytes - 4),
                 (d4, p["packed"], p["states"], 5, p["recs"], p["states"]), (d4, p["packed"], p["out"] + 76, 5, p["recs"], p["out"])):
        assert L.pt_grid_irradiance_states_device(*args, None) == -1 and _err(api) == LKS + ": the output buffer overlaps an input", (args, _err(api))
    assert _unchanged(b)
    # the Python wrappers refuse what would read or write past an array
    d = _desc(api)
    with pytest.raises(api.PtError, match="maps holds 64 float32 words, the grid needs 512"):
        api.grid_classify(d, np.zeros((1, 4, 4, 4), F))
    with pytest.raises(api.PtError, match="states holds 7 words, the call needs 8"):
        api.grid_classify(d, b["maps"], states=np.zeros(7, np.uint32))
    with pytest.raises(api.PtError, match="states must be a writable C-contiguous uint32 array"):
        api.grid_classify(d, b["maps"], states=[0] * 8)
    with pytest.raises(api.PtError, match="coeff_sums holds 288 float32 words, the grid needs 72"):
        api.grid_update(b["packed"][:-8].copy(), d, b["sums"], b["maps"][:128], indices=[1, 2])
    with pytest.raises(api.PtError, match="maps are missing but desc.map_res is 4"):
        api.grid_update(b["packed"][:-8].copy(), d, b["sums"])
    with pytest.raises(api.PtError, match="packed must be a writable C-contiguous float32 array"):
        api.grid_update(list(b["packed"][:-8]), d, b["sums"], b["maps"])
    with pytest.raises(api.PtError, match="states holds 3 words, the call needs 8"):
        api.grid_irradiance(b["packed"][:-8].copy(), d, b["recs"], states=np.zeros(3, np.uint32))
    assert api.grid_irradiance(b["packed"][:-8].copy(), d, np.zeros((0, 8), F), states=np.zeros(8, np.uint32)).shape == (0, 4)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
# tests/test_grid_api.py's seeded 3 x 2 x 2 data: the same recipe, so the two files' restatements see the same numbers
LO, HI, COUNTS, SH_SAMPLES, MAP_SAMPLES, RES, M, SEED = (-1.0, 0.5, 2.0), (1.5, 1.75, 3.0), (3, 2, 2), 96, 4, 8, 2000, 11
N = 12
PATTERNS = {"one": (4,), "corners": (0, 7), "alternate": (0, 2, 4, 6, 8, 10)}


def _inputs():
    rng = np.random.default_rng(SEED)
    n = N
    sums = np.zeros((n, 9, 4), F)
    sums[:, 0, :3] = rng.uniform(4.0, 12.0, (n, 3))
    sums[:, 1:, :3] = rng.uniform(-3.0, 3.0, (n, 8, 3))
    mean = rng.uniform(0.4, 1.6, (n, RES, RES))
    var = rng.uniform(0.02, 0.3, (n, RES, RES))
    maps = np.zeros((n, RES, RES, 4), F)
    maps[..., 0], maps[..., 1] = mean * MAP_SAMPLES, (mean * mean + var) * MAP_SAMPLES
    lo, hi = np.array(LO), np.array(HI)
    cell = (hi - lo) / (np.array(COUNTS) - 1)
    pts = rng.uniform(lo - cell, hi + cell, (M, 3)).astype(F)
    nrm = rng.standard_normal((M, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F)
    return sums, maps, pts, nrm


def _states(dead, junk=False):
    s = np.zeros(N, np.uint32)
    if junk:
        s[:] = 0xfffffffe
    s[list(dead)] |= 1
    return s


@pytest.mark.parametrize("res,power", [(0, 1), (0, 3), (8, 1), (8, 3)])
def test_with_every_state_clear_the_restatement_is_grid_refs(api, res, power):
    from cudapathtracer_amd import rays
    sums, maps, pts, nrm = _inputs()
    coeff, tex = GR.pack(SH_SAMPLES, sums, maps if res else None, MAP_SAMPLES)
    rec = rays.irradiance_records(pts, nrm)
    rec[5, 0], rec[77, 5] = np.nan, np.inf
    want, fallback = GR.lookup(LO, HI, COUNTS, coeff, tex, power, rec)
    for st in (_states(()), np.full(N, 0xfffffffe, np.uint32), np.full(N, 2, np.uint32)):           # bit 0 alone is read
        got, arm, _ = GL.lookup(LO, HI, COUNTS, coeff, tex, power, rec, st)
        assert_bits_equal(got, want, "all states live, res %d power %d" % (res, power))
        assert set(np.unique(arm)) <= {GL.ARM_WEIGHTED, GL.ARM_PLAIN, GL.ARM_BAD} and (arm == GL.ARM_BAD).sum() == 2
        assert np.array_equal(arm == GL.ARM_PLAIN, fallback if res else arm != GL.ARM_BAD)


@pytest.mark.parametrize("power", [1, 3])
def test_a_dead_probe_is_a_probe_with_a_zeroed_map(api, power):
    """With maps a dead corner adds what a probe whose map is all zero adds: no weight. So wherever neither route takes its fallback
    the masked restatement equals grid_ref.lookup on a pack whose dead probes' maps are zero, in all four words. What is left out are
    the points clamped onto a dead probe (a zero map sees a point at distance 0) and the fallbacks. The arms the mask adds are all in
    this data: the divide arm and the all-dead arm."""
    from cudapathtracer_amd import rays
    sums, maps, pts, nrm = _inputs()
    rec = rays.irradiance_records(pts, nrm)
    arms = set()
    for name in ("one", "corners"):
        dead = PATTERNS[name]
        coeff, tex = GR.pack(SH_SAMPLES, sums, maps, MAP_SAMPLES)
        got, arm, _ = GL.lookup(LO, HI, COUNTS, coeff, tex, power, rec, _states(dead, junk=True))
        zeroed = maps.copy()
        zeroed[list(dead)] = 0
        want, fallback = GR.lookup(LO, HI, COUNTS, *GR.pack(SH_SAMPLES, sums, zeroed, MAP_SAMPLES), power, rec)
        keep = (arm == GL.ARM_WEIGHTED) & ~fallback
        print(name, "power", power, "left out", int((~keep).sum()), "of", M, "arms", np.bincount(arm, minlength=5))
        assert (~keep).sum() <= M // 20
        assert_bits_equal(got[keep], want[keep], "dead probes %s against zeroed maps" % (dead,))
        assert not got[arm == GL.ARM_DEAD].view(np.uint32).any()
        arms |= set(np.unique(arm))
        # without maps the mask renormalises: every point that lost a corner takes the divide arm or has no live weight
        plain, parm, T = GL.lookup(LO, HI, COUNTS, coeff, None, power, rec, _states(dead))
        assert set(np.unique(parm)) <= {GL.ARM_PLAIN, GL.ARM_DIVIDED, GL.ARM_DEAD}
        assert_bits_equal(plain[:, 3], T, "without maps W is the live trilinear sum")
        arms |= set(np.unique(parm))
    assert {GL.ARM_WEIGHTED, GL.ARM_DIVIDED, GL.ARM_DEAD} <= arms


def _sums64(pts, maps, power, dead):
    """(weight sum, live trilinear sum, lost a corner) of rays.grid_irradiance(states=...) in float64, formed from its parts as
    tests/test_grid_api.py's _weight_sum64 forms the first."""
    from cudapathtracer_amd import rays
    p = pts.astype(np.float64)
    i0, f, pos = [], [], []
    for a in range(3):
        step = (HI[a] - LO[a]) / (COUNTS[a] - 1)
        g = (p[:, a] - LO[a]) / step
        low = np.clip(np.floor(g), 0, COUNTS[a] - 2)
        i0.append(low.astype(np.int64)); f.append(np.clip(g - low, 0, 1)); pos.append((LO[a], step))
    den, live, lost = 0, 0, False
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                i = (i0[0] + cx, i0[1] + cy, i0[2] + cz)
                tri = (f[0] if cx else 1 - f[0]) * (f[1] if cy else 1 - f[1]) * (f[2] if cz else 1 - f[2])
                j = (i[2] * COUNTS[1] + i[1]) * COUNTS[0] + i[0]
                gone = dead[j]
                tri = np.where(gone, 0.0, tri)
                live, lost = live + tri, lost | gone
                if maps is not None:
                    v = p - np.stack([pos[a][0] + pos[a][1] * i[a] for a in range(3)], -1)
                    dist = np.sqrt((v * v).sum(-1))
                    d = np.where((dist > 0)[:, None], v, np.array([0.0, 0.0, 1.0])[None, :])
                    den = den + tri * rays.distance_visibility(maps.astype(np.float64)[j], MAP_SAMPLES, d, dist, power)
    return (den if maps is not None else live), live, lost


# The largest |f32 - f64| / max(|f64|, mean |f64|) per case as measured on the seeded data: a few f32 roundings, and the divide arm's
# one more. The test asserts 4x the largest, which covers library drift only, and a quarter of the case's own.
MEASURED = {(0, 1, "one"): 3.69e-7, (0, 1, "corners"): 4.88e-7, (0, 1, "alternate"): 1.45e-6,          # (map_res, power, the dead probes)
            (0, 3, "one"): 3.69e-7, (0, 3, "corners"): 4.88e-7, (0, 3, "alternate"): 1.45e-6,          # without maps the power is not read
            (8, 1, "one"): 3.90e-7, (8, 1, "corners"): 4.43e-7, (8, 1, "alternate"): 1.05e-6,
            (8, 3, "one"): 5.10e-7, (8, 3, "corners"): 5.34e-7, (8, 3, "alternate"): 8.49e-7}
# left out: none of the 2000 points in any case; without live weight: 0 (one), 65 (corners), 323 (alternate) points, in f32 and f64 alike


@pytest.mark.parametrize("res,power,pattern", sorted(MEASURED))
def test_the_masked_restatement_follows_grid_irradiance_in_float64(api, res, power, pattern):
    """As tests/test_grid_api.py compares the plain lookup: the restatement on the f32 inputs, rays.grid_irradiance(states=...) on the
    same values in float64. Left out are the points whose float64 weight sum lies in [0.5e-6, 2e-6] (the fallback threshold) and those
    whose live trilinear sum lies in (0, 1e-3), where the divide amplifies the rounding of the sum: at most 1 % together. The points
    with no live weight at all are the same set in both."""
    from cudapathtracer_amd import rays
    sums, maps, pts, nrm = _inputs()
    st = _states(PATTERNS[pattern])
    coeff, tex = GR.pack(SH_SAMPLES, sums, maps if res else None, MAP_SAMPLES)
    got, arm, T = GL.lookup(LO, HI, COUNTS, coeff, tex, power, rays.irradiance_records(pts, nrm), st)
    want = rays.grid_irradiance(LO, HI, COUNTS, sums.astype(np.float64), SH_SAMPLES, pts.astype(np.float64), nrm.astype(np.float64),
                                maps.astype(np.float64) if res else None, MAP_SAMPLES, power, states=st)
    assert got.dtype == F and got.shape == (M, 4) and want.dtype == np.float64
    w64, live64, lost64 = _sums64(pts, maps if res else None, power, (st & 1) != 0)
    assert np.array_equal(T == 0, live64 == 0)
    dead32, dead64 = arm == GL.ARM_DEAD, lost64 & (live64 == 0)
    print("no live weight:", int(dead32.sum()), "in f32,", int(dead64.sum()), "in f64")
    assert np.array_equal(dead32, dead64) and not want[dead64].any() and not got[dead32].view(np.uint32).any()
    keep = ~((live64 > 0) & (live64 < 1e-3))
    if res:
        keep &= ~((w64 >= 0.5e-6) & (w64 <= 2e-6))
        assert np.array_equal((arm == GL.ARM_WEIGHTED)[keep], w64[keep] >= 1e-6)
    print("left out", int((~keep).sum()), "of", M, "; arms", np.bincount(arm, minlength=5))
    assert (~keep).sum() <= M // 100
    assert np.abs(got[keep, 3] - w64[keep]).max() <= 1e-5
    err = np.abs(got[keep, :3] - want[keep]) / np.maximum(np.abs(want[keep]), np.abs(want[keep]).mean())
    print("res", res, "power", power, "pattern", pattern, "max relative error %.3g" % err.max())
    assert err.max() <= 4 * max(MEASURED.values())
    assert 0.25 * MEASURED[(res, power, pattern)] <= err.max()


def test_update_restated():
    sums, maps, _, _ = _inputs()
    rng = np.random.default_rng(3)
    fresh_s = (sums * rng.uniform(0.5, 1.5, sums.shape)).astype(F)
    fresh_m = (maps * rng.uniform(0.5, 1.5, maps.shape)).astype(F)
    coeff, tex = GR.pack(SH_SAMPLES, sums, maps, MAP_SAMPLES)
    # h = 0 over all probes is the pack, whatever was there (a NaN included), with the fresh sums' own sample counts
    junk_c, junk_t = np.full_like(coeff, np.nan), np.full_like(tex, -7.0)
    c0, t0 = GL.update(junk_c, junk_t, 48, fresh_s, fresh_m, 2, 0.0)
    want_c, want_t = GR.pack(48, fresh_s, fresh_m, 2)
    assert_bits_equal(c0, want_c, "h = 0: the coefficients")
    assert_bits_equal(t0, want_t, "h = 0: the texels")
    c0, _ = GL.update(junk_c, None, 48, fresh_s, None, 1, 0.0, np.arange(N)[::-1])
    assert_bits_equal(c0, want_c[::-1], "h = 0 through a permuted list")
    # a blend keeps the gutter rule and touches the listed probes alone; rows out of range touch nothing
    sy, sx = GR.border_source(RES)
    assert np.array_equal(tex, tex[:, 1:-1, 1:-1][:, sy, sx])
    idx = np.array([7, -1, 2, N, 11])
    rows = [0, 2, 4]
    for h in (0.5, 0.96875):
        c1, t1 = GL.update(coeff, tex, 48, fresh_s[:5], fresh_m[:5], 2, h, idx)
        assert np.array_equal(t1, t1[:, 1:-1, 1:-1][:, sy, sx]), "the gutter rule after a blend"
        rest = np.setdiff1d(np.arange(N), idx[rows])
        assert_bits_equal(c1[rest], coeff[rest], "unlisted coefficients")
        assert_bits_equal(t1[rest], tex[rest], "unlisted texels")
        fc, ft = GR.pack(48, fresh_s[:5], fresh_m[:5], 2)
        hh = np.float64(h)
        for got, old, fresh in ((c1[idx[rows]][..., :3], coeff[idx[rows]][..., :3], fc[rows][..., :3]), (t1[idx[rows]], tex[idx[rows]], ft[rows])):
            exact = fresh.astype(np.float64) + hh * (old.astype(np.float64) - fresh.astype(np.float64))
            assert (got != old).any() and (got != fresh).any()
            assert np.abs(got - exact).max() <= 2.0 ** -22 * np.abs(exact).max()                  # two roundings: the difference and the fma
        assert not c1[..., 3].any()


def test_classify_restated():
    R = 4
    maps = np.zeros((6, R, R, 4), F)
    maps[..., :2] = 3.0
    maps[0, :, :, 2] = 4; maps[0, 0, :, 3] = 4                       # Hs = 64, Ks = 16: the tie at 0.25 is not inside
    maps[1, :, :, 2] = 4; maps[1, 0, :, 3] = 4; maps[1, 3, 3, 3] = 1  # Ks = 17: inside
    # probe 2: nothing hit: idle, and 0 > 0 is false
    maps[3, :, :, 2] = 2; maps[3, :, :, 3] = 2                       # every hit from behind
    maps[4, :, :, 2] = 1; maps[4, 1, 1, 2] = np.nan                  # a NaN count: every comparison false
    maps[5, :, :, 2] = 1; maps[5, 2, 2, 3] = np.nan
    got = GL.classify(maps, 0.25, 6)
    assert got.dtype == np.uint32 and list(got) == [0, GL.INSIDE, GL.IDLE, GL.INSIDE, 0, 0]
    assert list(GL.classify(maps, 1.0, 6)) == [0, 0, GL.IDLE, 0, 0, 0] and list(GL.classify(maps, 0.0, 6)) == [1, 1, GL.IDLE, 1, 0, 0]
    # a list writes its own words alone, rows out of range none
    before = np.full(9, 0xabcd0000, np.uint32)
    got = GL.classify(maps[[1, 2, 0, 3]], 0.25, 9, [8, -1, 3, 9], before)
    assert list(got[[8, 3]]) == [GL.INSIDE, 0] and (np.delete(got, [8, 3]) == 0xabcd0000).all() and (before == 0xabcd0000).all()
    # the product is rounded once in f32: 0.1f * 30 = 3.0000001192...; in f32 it is 3, and Ks = 3 is a tie
    m = np.zeros((1, R, R, 4), F)
    m[0, 0, 0, 2], m[0, 0, 0, 3] = 30, 3
    assert F(0.1) * F(30) == F(3) and float(F(0.1)) * 30 > 3 and list(GL.classify(m, F(0.1), 1)) == [0]


# DESIGN.md §30's table: kernel -> (VGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes per workgroup, waves per SIMD that fit)
TABLE = {"live_classify": (10, 0, 0, 0, 8), "live_update": (16, 0, 0, 0, 8), "live_lookup_maps": (84, 0, 0, 0, 5), "live_lookup_plain": (70, 0, 0, 0, 7)}
# and §29's, which the new unit leaves as it was
GRID_TABLE = {"grid_pack": (16, 0, 0, 0, 8), "grid_irradiance_maps": (89, 0, 0, 0, 5), "grid_irradiance_plain": (66, 0, 0, 0, 7)}


def test_each_kernel_has_the_tables_resources():
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import grid_live_time
    import grid_time
    for res, table in ((grid_live_time.live_kernel_resources(), TABLE), (grid_time.grid_kernel_resources(), GRID_TABLE)):
        print(res)
        assert set(res) == set(table)
        for k, (vgprs, scratch, spills, lds, waves) in table.items():
            r = res[k]
            assert r["vgpr_count"] == vgprs and r["private_segment_fixed_size"] == scratch and r["vgpr_spill_count"] == spills, (k, r)
            assert r["sgpr_spill_count"] == 0 and r["group_segment_fixed_size"] == lds, (k, r)
            assert min(512 // ((r["vgpr_count"] + 7) // 8 * 8), 8) == waves, (k, r)
