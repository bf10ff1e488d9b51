"""Probe relocation without a GPU (pt_grid_relocate, pt_grid_irradiance_offsets): the symbols and the Python names;
every argument check of the four functions in the header's order (they fire before any HIP call, under the function's name);
tests/grid_relocate_ref.py's f32 restatement of the lookup against grid_ref's and grid_live_ref's at zero offsets, and against
rays.grid_irradiance(offsets=...) in float64; the restated relocation on synthetic maps, rule by rule; and the resources of the new
kernels, read from the code-object notes, against §31's table."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

import grid_live_ref as GL
import grid_ref as GR
import grid_relocate_ref as RR
import test_grid_live_api as TL
from util import assert_bits_equal

F = np.float32
RLC, LKO = "pt_grid_relocate", "pt_grid_irradiance_offsets"
INF, NAN = float("inf"), float("nan")
_desc, _err, _later = TL._desc, TL._err, TL._later


def test_new_symbols_and_names(api):
    from conftest import ROOT
    from cudapathtracer_amd import rays
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for n in ("pt_grid_relocate", "pt_grid_relocate_device", "pt_grid_irradiance_offsets", "pt_grid_irradiance_offsets_device"):
        assert hasattr(L, n), n
        assert "int " + n + "(" in header, n
        assert getattr(L, n).argtypes, n
    assert header.index("int pt_grid_irradiance_states(") < header.index("int pt_grid_relocate_device(")
    for n in ("grid_relocate", "grid_relocate_defaults", "grid_irradiance"):
        assert hasattr(api, n), n
    assert hasattr(api.ProbeGrid, "relocate")
    par = inspect.signature(api.grid_relocate).parameters
    assert list(par) == ["desc", "maps", "offsets", "back_fraction", "min_dist", "max_offset", "indices"]
    assert par["offsets"].default is None and par["back_fraction"].default == 0.25 and par["indices"].default is None
    assert inspect.signature(api.grid_irradiance).parameters["offsets"].default is None
    assert inspect.signature(rays.grid_irradiance).parameters["offsets"].default is None
    assert inspect.signature(rays.sh_grid).parameters["offsets"].default is None
    assert inspect.signature(api.ProbeGrid.relocate).parameters["iterations"].default == 4
    assert (RR.KEPT, RR.PUSHED_OUT, RR.PUSHED_OFF) == (0, 1, 2)
    # the defaults: 0.2 of the smallest step; 0.45 of each axis' step, an axis with one probe takes the smallest of the others
    mn, mx = api.grid_relocate_defaults(api.grid_desc((0, 0, 0), (4, 1, 9), (5, 3, 1), 64, 8))
    assert np.isclose(mn, 0.2 * 0.5) and np.allclose(mx, [0.45, 0.225, 0.225])
    with pytest.raises(api.PtError, match="one probe"):
        api.grid_relocate_defaults(api.grid_desc((0, 0, 0), (1, 1, 1), (1, 1, 1), 64, 8))
    g = rays.sh_grid((0, 0, 0), (1, 1, 1), (2, 1, 1), 3.0, offsets=np.array([[0.25, 0, -0.5, 1], [0, 0.125, 0, 2]], F))
    assert g.dtype == F and np.array_equal(g[:, :4], np.array([[0.25, 0, -0.5, 3], [1, 0.125, 0, 3]], F))


# ---- the checks -----------------------------------------------------------------------------------------------------------------
def _buffers():
    """Host buffers of the 2 x 2 x 2 grid at R = 4, pre-filled: nothing a refused call is given may change."""
    b = dict(idx=np.arange(8, dtype=np.int32), maps=np.full(8 * 16 * 4, 5.0, F), packed=np.full(8 * 36 + 8 * 36 * 2 + 8, 77.0, F),
             states=np.full(8, 9, np.uint32), off=np.full(8 * 4 + 8, 4.0, F), mx=np.full(3, 0.25, F), bad=np.array([0.25, -1.0, NAN], F),
             recs=np.zeros((5, 8), F), out=np.full((5, 4), 77.0, F))
    return b, {k: v.ctypes.data for k, v in b.items()}


def _unchanged(b):
    return (b["packed"] == 77).all() and (b["out"] == 77).all() and (b["states"] == 9).all() and (b["maps"] == 5).all() and (b["off"] == 4).all()


def _forms(api, p):
    L = api.lib()
    return {RLC: (("desc", "k", "idx", "maps", "bf", "md", "mx", "off"),
                  dict(desc={}, k=8, idx=p["idx"], maps=p["maps"], bf=0.25, md=0.1, mx=p["mx"], off=p["off"]), L.pt_grid_relocate, L.pt_grid_relocate_device),
            LKO: (("desc", "packed", "states", "off", "m", "recs", "out"),
                  dict(desc={}, packed=p["packed"], states=p["states"], off=p["off"], m=5, recs=p["recs"], out=p["out"]),
                  L.pt_grid_irradiance_offsets, L.pt_grid_irradiance_offsets_device)}


def _refused(api, name, forms, a, msg, exact=True):
    order, _, host, dev = forms[name]
    for fn, tail in ((host, ()), (dev, (None,))):
        assert TL._call(api, fn, order, a, tail) == -1, (name, a)
        e = _err(api)
        assert (e == name + ": " + msg) if exact else (e.startswith(name + ": ") and msg in e), (name, a, e)


def _own(p):
    """Per function its own checks after the desc's, in the header's order: (what breaks, the message)."""
    no_maps = "map_res is 0: a grid without maps has no positions to read"
    return {RLC: [(dict(desc=dict(map_res=0)), no_maps),
                  (dict(k=-1), "k -1 must not be negative"),
                  (dict(k=9), "k 9 lists more than the grid's 8 probes"),
                  (dict(k=5, idx=None), "null indices need k == 8, the grid's probes, not 5"),
                  (dict(bf=NAN), "back_fraction nan must be in [0, 1]"),
                  (dict(md=NAN), "min_dist nan must be finite and not negative"),
                  (dict(mx=p["bad"]), "max_offset[1] = -1 must be finite and not negative"),
                  (dict(maps=None), "null maps"),
                  (dict(mx=None), "null max_offset"),
                  (dict(off=None), "null offsets")],
            LKO: [(dict(desc=dict(map_res=0)), no_maps),
                  (dict(m=-1), "m -1 must not be negative"),
                  (dict(packed=None), "null packed buffer"),
                  (dict(off=None), "null offsets"),
                  (dict(recs=None), "null records"),
                  (dict(out=None), "null output buffer")]}


def test_the_desc_checks_come_first_from_all_four_functions(api):
    b, p = _buffers()
    forms = _forms(api, p)
    for name, (order, good, _, _) in forms.items():
        own = _later(_own(p)[name])
        own.pop("desc", None)
        for a in (dict(good, desc=None), dict(good, **dict(own, desc=None))):
            _refused(api, name, forms, a, "null desc")
        for change, also, msg in TL.DESC_CASES:
            for extra in ({}, also):
                d = dict(extra, **change)
                for a in (dict(good, desc=d), dict(good, **dict(own, desc=d))):
                    _refused(api, name, forms, a, msg, exact=False)
    assert _unchanged(b)


@pytest.mark.parametrize("name", [RLC, LKO])
def test_each_functions_own_checks_alone_and_in_order(api, name):
    """Each check's break alone, and together with everything the later checks refuse: the earliest broken check answers, from the
    host form and the device form."""
    b, p = _buffers()
    forms = _forms(api, p)
    good = forms[name][1]
    own = _own(p)[name]
    for i, (brk, msg) in enumerate(own):
        for a in (dict(good, **brk), dict(dict(good, **_later(own[i + 1:])), **brk)):
            _refused(api, name, forms, a, msg)
    assert _unchanged(b)


def test_the_ranges_the_count_of_zero_the_overlaps_and_the_wrappers(api):
    b, p = _buffers()
    forms = _forms(api, p)
    L = api.lib()
    good = forms[RLC][1]
    for bf in (NAN, INF, -INF, -0.125, 1.5):
        _refused(api, RLC, forms, dict(good, bf=bf), "back_fraction", exact=False)
    for md in (NAN, INF, -INF, -0.125):
        _refused(api, RLC, forms, dict(good, md=md), "min_dist", exact=False)
    for a, v in ((0, NAN), (1, INF), (2, -INF), (0, -1e-3)):
        mx = np.full(3, 0.25, F)
        mx[a] = v
        _refused(api, RLC, forms, dict(good, mx=mx.ctypes.data), "max_offset[%d]" % a, exact=False)
    d4, d0 = C.byref(_desc(api)), C.byref(_desc(api, map_res=0, map_samples=0))
    # k == 0 (m == 0): 0 after the desc's checks and map_res, whatever comes after
    assert L.pt_grid_relocate(d4, 0, None, None, NAN, NAN, None, None) == 0 and L.pt_grid_relocate_device(d4, 0, None, None, 2.0, -1.0, None, None, None) == 0
    assert L.pt_grid_irradiance_offsets(d4, None, None, None, 0, None, None) == 0
    assert L.pt_grid_irradiance_offsets_device(d4, None, None, None, 0, None, None, None) == 0
    assert L.pt_grid_relocate(d0, 0, None, None, 0.25, 0.1, None, None) == -1 and _err(api).startswith(RLC + ": map_res is 0")
    assert L.pt_grid_irradiance_offsets(d0, None, None, None, 0, None, None) == -1 and _err(api).startswith(LKO + ": map_res is 0")
    bad = C.byref(_desc(api, power=0))
    assert L.pt_grid_relocate(bad, 0, None, None, 0.25, 0.1, None, None) == -1 and "power 0" in _err(api)
    # the ends of the ranges are inside: back_fraction 0 and 1, min_dist 0, a max_offset of 0
    zero = np.zeros(3, F)
    for bf in (0.0, 1.0):
        assert L.pt_grid_relocate(d4, 8, None, None, bf, 0.0, zero.ctypes.data, None) == -1 and _err(api) == RLC + ": null maps"
    # states may be NULL in the lookup: the next check answers
    assert L.pt_grid_irradiance_offsets(d4, p["packed"], None, None, 5, p["recs"], p["out"]) == -1 and _err(api) == LKO + ": null offsets"
    # the device forms: a written buffer over a read one, checked last
    pk_bytes = api.grid_packed_bytes(_desc(api))
    for args in ((d4, 8, p["idx"], p["maps"], 0.25, 0.1, p["mx"], p["maps"]), (d4, 8, p["idx"], p["maps"], 0.25, 0.1, p["mx"], p["maps"] + 8 * 16 * 16 - 4),
                 (d4, 8, p["idx"], p["maps"], 0.25, 0.1, p["mx"], p["idx"] + 28), (d4, 2, p["off"] + 8 * 16 - 4, p["maps"], 0.25, 0.1, p["mx"], p["off"])):
        assert L.pt_grid_relocate_device(*args, None) == -1 and _err(api) == RLC + ": the offsets overlap an input", (args, _err(api))
    for args in ((d4, p["packed"], p["states"], p["off"], 5, p["recs"], p["recs"] + 5 * 32 - 4), (d4, p["packed"], p["states"], p["off"], 5, p["recs"], p["packed"] + pk_bytes - 4),
                 (d4, p["packed"], p["states"], p["off"], 5, p["recs"], p["states"]), (d4, p["packed"], None, p["off"], 5, p["recs"], p["off"] + 8 * 16 - 4),
                 (d4, p["packed"], p["out"] + 76, p["off"], 5, p["recs"], p["out"])):
        assert L.pt_grid_irradiance_offsets_device(*args, None) == -1 and _err(api) == LKO + ": the output buffer overlaps an input", (args, _err(api))
    assert _unchanged(b)
    # the Python wrappers refuse what would read or write past an array
    d = _desc(api)
    with pytest.raises(api.PtError, match="maps holds 64 float32 words, the grid needs 512"):
        api.grid_relocate(d, np.zeros((1, 4, 4, 4), F))
    with pytest.raises(api.PtError, match="offsets holds 28 float32 words, the grid needs 32"):
        api.grid_relocate(d, b["maps"], offsets=np.zeros((7, 4), F))
    with pytest.raises(api.PtError, match="offsets must be a writable C-contiguous float32 array"):
        api.grid_relocate(d, b["maps"], offsets=[[0.0] * 4] * 8)
    with pytest.raises(api.PtError, match="maps holds 512 float32 words, the grid needs 128"):
        api.grid_relocate(d, b["maps"], indices=[1, 2])
    with pytest.raises(api.PtError, match="offsets holds 12 float32 words, the grid needs 32"):
        api.grid_irradiance(b["packed"][:-8].copy(), d, b["recs"], offsets=np.zeros((3, 4), F))
    with pytest.raises(api.PtError, match="states holds 3 words, the call needs 8"):
        api.grid_irradiance(b["packed"][:-8].copy(), d, b["recs"], states=np.zeros(3, np.uint32), offsets=np.zeros((8, 4), F))
    assert api.grid_irradiance(b["packed"][:-8].copy(), d, np.zeros((0, 8), F), offsets=np.zeros((8, 4), F)).shape == (0, 4)


# ---- the restated lookup ----------------------------------------------------------------------------------------------------------
LO, HI, COUNTS, SH_SAMPLES, MAP_SAMPLES, RES, M, N = TL.LO, TL.HI, TL.COUNTS, TL.SH_SAMPLES, TL.MAP_SAMPLES, TL.RES, TL.M, TL.N
OFFSET_SEED = 1
DEAD = {"none": None, "two": (4, 9)}


def _offsets(seed=OFFSET_SEED):
    """Seeded offsets within 0.45 of a step per axis; the fourth word is junk the lookup must not read."""
    rng = np.random.default_rng(seed)
    step = (np.array(HI) - np.array(LO)) / (np.array(COUNTS) - 1)
    off = np.zeros((N, 4), F)
    off[:, :3] = rng.uniform(-0.45, 0.45, (N, 3)) * step
    off[:, 3] = TL.NAN
    return off


@pytest.mark.parametrize("power", [1, 3])
def test_with_zero_offsets_the_restatement_is_both_older_ones(api, power):
    from cudapathtracer_amd import rays
    sums, maps, pts, nrm = TL._inputs()
    coeff, tex = GR.pack(SH_SAMPLES, sums, maps, MAP_SAMPLES)
    rec = rays.irradiance_records(pts, nrm)
    rec[5, 0], rec[77, 5] = np.nan, np.inf
    assert RR.fma_of_the_grid_is_never_minus_zero(LO, HI, COUNTS)
    assert RR.fma_of_the_grid_is_never_minus_zero((-0.0, -1.0, 0.0), (1.0, 1.0, 0.0), (3, 3, 1))        # a cancelling sum and a -0 corner
    plus, minus = np.zeros((N, 4), F), np.zeros((N, 4), F)
    minus[:, :3] = -0.0
    minus[:, 3] = TL.NAN
    want, _ = GR.lookup(LO, HI, COUNTS, coeff, tex, power, rec)
    for off in (plus, minus):
        got, arm, _ = RR.lookup(LO, HI, COUNTS, coeff, tex, power, rec, off)
        assert_bits_equal(got, want, "zero offsets, no states: grid_ref's lookup")
        assert set(np.unique(arm)) <= {GL.ARM_WEIGHTED, GL.ARM_PLAIN, GL.ARM_BAD}
        for pattern in ("one", "corners", "alternate"):
            st = TL._states(TL.PATTERNS[pattern], junk=True)
            live_want, live_arm, live_T = GL.lookup(LO, HI, COUNTS, coeff, tex, power, rec, st)
            got, arm, T = RR.lookup(LO, HI, COUNTS, coeff, tex, power, rec, off, st)
            assert_bits_equal(got, live_want, "zero offsets, states %s: grid_live_ref's lookup" % pattern)
            assert np.array_equal(arm, live_arm) and np.array_equal(T, live_T)


def _weight_sum64(pts, maps, power, off, dead):
    """The float64 weight sum of rays.grid_irradiance(offsets=...), formed from its parts."""
    from cudapathtracer_amd import rays
    p = pts.astype(np.float64)
    i0, f, pos = [], [], []
    for a in range(3):
        step = (HI[a] - LO[a]) / (COUNTS[a] - 1)
        g = (p[:, a] - LO[a]) / step
        low = np.clip(np.floor(g), 0, COUNTS[a] - 2)
        i0.append(low.astype(np.int64)); f.append(np.clip(g - low, 0, 1)); pos.append((LO[a], step))
    den = 0
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                i = (i0[0] + cx, i0[1] + cy, i0[2] + cz)
                tri = (f[0] if cx else 1 - f[0]) * (f[1] if cy else 1 - f[1]) * (f[2] if cz else 1 - f[2])
                j = (i[2] * COUNTS[1] + i[1]) * COUNTS[0] + i[0]
                tri = np.where(dead[j], 0.0, tri)
                v = p - (np.stack([pos[a][0] + pos[a][1] * i[a] for a in range(3)], -1) + off[j, :3].astype(np.float64))
                dist = np.sqrt((v * v).sum(-1))
                d = np.where((dist > 0)[:, None], v, np.array([0.0, 0.0, 1.0])[None, :])
                den = den + tri * rays.distance_visibility(maps.astype(np.float64)[j], MAP_SAMPLES, d, dist, power)
    return den


# The largest |f32 - f64| / max(|f64|, mean |f64|) per case as measured on the seeded data (power, the dead probes): a few f32 roundings
# more than the lookup without offsets has, the rounded add of the offset among them. The test asserts 4x the largest.
MEASURED = {(1, "none"): 6.29e-7, (1, "two"): 6.50e-7, (3, "none"): 9.74e-7, (3, "two"): 9.68e-7}
# left out: none of the 2000 points in any case; with two probes dead 70 points have no live weight, in f32 and f64 alike


@pytest.mark.parametrize("power,pattern", sorted(MEASURED))
def test_the_restatement_follows_grid_irradiance_with_offsets_in_float64(api, power, pattern):
    """The restatement on the f32 inputs, rays.grid_irradiance(offsets=...) on the same values in float64. Left out are the points
    whose float64 weight sum lies in [0.5e-6, 2e-6], the fallback threshold: at most 1 %, which the seed is chosen to keep."""
    from cudapathtracer_amd import rays
    sums, maps, pts, nrm = TL._inputs()
    off = _offsets()
    st = None if DEAD[pattern] is None else TL._states(DEAD[pattern])
    dead = np.zeros(N, bool) if st is None else (st & 1) != 0
    coeff, tex = GR.pack(SH_SAMPLES, sums, maps, MAP_SAMPLES)
    got, arm, _ = RR.lookup(LO, HI, COUNTS, coeff, tex, power, rays.irradiance_records(pts, nrm), off, st)
    want = rays.grid_irradiance(LO, HI, COUNTS, sums.astype(np.float64), SH_SAMPLES, pts.astype(np.float64), nrm.astype(np.float64),
                                maps.astype(np.float64), MAP_SAMPLES, power, states=st, offsets=off[:, :3].astype(np.float64))
    plain = rays.grid_irradiance(LO, HI, COUNTS, sums.astype(np.float64), SH_SAMPLES, pts.astype(np.float64), nrm.astype(np.float64),
                                 maps.astype(np.float64), MAP_SAMPLES, power, states=st)
    assert got.dtype == F and got.shape == (M, 4) and want.dtype == np.float64
    assert np.abs(want - plain).max() > 1e-2 * np.abs(plain).mean()                     # the offsets matter to the reference
    w64 = _weight_sum64(pts, maps, power, off, dead)
    keep = ~((w64 >= 0.5e-6) & (w64 <= 2e-6))
    print("left out", int((~keep).sum()), "of", M, "; arms", np.bincount(arm, minlength=5))
    assert (~keep).sum() <= M // 100
    assert np.array_equal((arm == GL.ARM_WEIGHTED)[keep], w64[keep] >= 1e-6)
    assert np.abs(got[keep, 3] - w64[keep]).max() <= 1e-5
    err = np.abs(got[keep, :3] - want[keep]) / np.maximum(np.abs(want[keep]), np.abs(want[keep]).mean())
    print("power", power, "pattern", pattern, "max relative error %.3g" % err.max())
    assert err.max() <= 4 * max(MEASURED.values())
    assert 0.25 * MEASURED[(power, pattern)] <= err.max()


# ---- the restated relocation ------------------------------------------------------------------------------------------------------
SPP = 2


def _front_map(res, mean=1.0):
    """One probe's map: every texel hit from the front, SPP samples, at distance `mean`."""
    m = np.zeros((res, res, 4), F)
    m[..., 0], m[..., 1], m[..., 2] = mean * SPP, mean * mean * SPP, SPP
    return m


def _set(m, l, mean, hits=SPP, back=0):
    res = m.shape[0]
    m[l // res, l % res] = (mean * SPP, mean * mean * SPP, hits, back)


def _relocate_one(m, min_dist=0.25, max_offset=(9.0, 9.0, 9.0), old=(0.0, 0.0, 0.0, 7.0), bf=0.25):
    return RR.relocate(m[None], SPP, bf, min_dist, max_offset, np.array([old], F))[0]


def test_relocate_restated_the_choice_and_the_move():
    R = 8
    # inside: every hit from behind; the nearest back texel wins although a front texel is nearer, and the move is c (m + min / 2)
    m = _front_map(R, 2.0)
    m[..., 3] = SPP
    _set(m, 21, 0.5, SPP, SPP); _set(m, 40, 0.75, SPP, SPP); _set(m, 3, 0.125, SPP, 0)
    assert RR.chosen_texel(m, SPP, 0.25) == (True, 21, F(0.5))
    got = _relocate_one(m)
    c = RR.centre_direction(21, R)
    assert abs(float(np.linalg.norm(c.astype(np.float64))) - 1) < 1e-6
    assert_bits_equal(got[:3], (c * F(0.625)).astype(F), "pushed out through the nearest back face")
    assert got[3] == RR.PUSHED_OUT
    # with an offset there already the move is one fma per axis
    got = _relocate_one(m, old=(0.5, -0.25, 0.125, 0.0))
    exact = np.array([0.5, -0.25, 0.125]) + c.astype(np.float64) * 0.625
    assert np.abs(got[:3] - exact).max() <= 2.0 ** -24 and got[3] == RR.PUSHED_OUT
    # not inside: the nearest front texel under min_dist pushes away by min - m; back texels are not looked at
    m = _front_map(R, 1.0)
    _set(m, 50, 0.0625); _set(m, 9, 0.125); _set(m, 60, 0.03125, SPP, SPP)
    assert RR.chosen_texel(m, SPP, 0.25) == (False, 50, F(0.0625))
    got = _relocate_one(m)
    c = RR.centre_direction(50, R)
    assert c[2] == 0 and np.array_equal(got[:3], (-c * F(0.1875)).astype(F))      # by value: fma(-0, t, +0) is +0, the product -0
    assert got[3] == RR.PUSHED_OFF
    # at min_dist and beyond nothing moves: the offset's bits stay, the code is 0
    old = (0.01, -0.02, 0.3, 2.0)
    for nearest in (0.25, 0.5):
        m = _front_map(R, 1.0)
        _set(m, 50, nearest)
        got = _relocate_one(m, old=old)
        assert_bits_equal(got[:3], np.array(old[:3], F), "nothing nearer than min_dist")
        assert got[3] == RR.KEPT
    _set(m, 50, np.nextafter(F(0.25), F(0)))
    assert _relocate_one(m, old=old)[3] == RR.PUSHED_OFF
    # a texel without a hit is neither front nor back
    m = _front_map(R, 1.0)
    _set(m, 50, 0.0625, 0, 0)
    assert _relocate_one(m)[3] == RR.KEPT


def test_relocate_restated_ties_nan_and_negative_means():
    # ties go to the lower l: neighbours, and l and l + 64 (one lane's stride at R = 16)
    R = 16
    for pair in ((70, 71), (5, 69), (200, 8)):
        m = _front_map(R, 1.0)
        for l in pair:
            _set(m, l, 0.0625)
        assert RR.chosen_texel(m, SPP, 0.25)[1] == min(pair)
        m[..., 3] = SPP
        assert RR.chosen_texel(m, SPP, 0.25)[:2] == (True, min(pair))
    # +0 and -0 are equal: the lower l wins whichever it holds
    m = _front_map(R, 1.0)
    _set(m, 30, 0.0); _set(m, 12, -0.0)
    assert RR.chosen_texel(m, SPP, 0.25)[1] == 12
    # a NaN or a negative mean is no candidate
    m = _front_map(8, 1.0)
    _set(m, 3, np.nan); _set(m, 4, -0.5); _set(m, 40, 0.125)
    assert RR.chosen_texel(m, SPP, 0.25) == (False, 40, F(0.125))
    m[..., 3] = SPP
    assert RR.chosen_texel(m, SPP, 0.25) == (True, 40, F(0.125))
    # no candidate at all
    m = _front_map(8, np.nan)
    got = _relocate_one(m, old=(0.5, 0.25, -0.125, 1.0))
    assert_bits_equal(got, np.array([0.5, 0.25, -0.125, 0.0], F), "no candidate: kept")


def test_relocate_restated_inside_without_a_back_texel_the_clamp_and_the_list():
    R = 4
    # every texel half from behind: Ks = Hs / 2 passes back_fraction, but no texel has a back majority: kept, code 0
    m = _front_map(R, 0.0625)
    m[..., 2], m[..., 3] = 4, 2
    inside, l, _ = RR.chosen_texel(m, SPP, 0.25)
    assert inside and l is None
    got = _relocate_one(m, old=(0.5, 0.25, -0.125, 1.0))
    assert_bits_equal(got, np.array([0.5, 0.25, -0.125, 0.0], F), "inside without a back texel")
    # the clamp holds on each axis, also when nothing moved, and a NaN in the old offset ends inside the box
    m = _front_map(R, 2.0)
    m[..., 3] = SPP
    for l in range(R * R):                                                      # a move of 0.625 along every texel's direction
        one = m.copy()
        _set(one, l, 0.5, SPP, SPP)
        far = _relocate_one(one, max_offset=(0.25, 0.5, 0.125))
        assert far[3] == RR.PUSHED_OUT and (np.abs(far[:3]) <= np.array([0.25, 0.5, 0.125], F)).all()
    _set(m, 5, 0.5, SPP, SPP)
    c = RR.centre_direction(5, R)
    got = _relocate_one(m, max_offset=(0.25, 0.5, 0.125))
    assert_bits_equal(np.abs(got[:3]), np.minimum(np.abs(c * F(0.625)), np.array([0.25, 0.5, 0.125], F)).astype(F), "the clamp, axis by axis")
    kept = _relocate_one(_front_map(R, 1.0), max_offset=(0.25, 0.5, 0.125), old=(3.0, -3.0, 0.0625, 1.0))
    assert_bits_equal(kept, np.array([0.25, -0.5, 0.0625, 0.0], F), "kept, but clamped")
    for a in range(3):
        old = [0.01, 0.02, 0.03, 0.0]
        old[a] = np.nan
        for mm in (m, _front_map(R, 1.0)):
            got = _relocate_one(mm, max_offset=(0.25, 0.5, 0.125), old=old)
            assert np.isfinite(got).all() and (np.abs(got[:3]) <= np.array([0.25, 0.5, 0.125], F)).all()
    assert not _relocate_one(m, max_offset=(0.0, 0.0, 0.0))[:3].any()
    # a list writes its own probes' rows alone; rows out of range write none
    maps = np.stack([m, _front_map(R, 1.0), m, m])
    before = np.full((6, 4), 0.015625, F)
    got = RR.relocate(maps, SPP, 0.25, 0.25, (9, 9, 9), before, [5, -1, 2, 6])
    assert (before == 0.015625).all()
    assert (got[[0, 1, 3, 4]] == 0.015625).all() and got[5, 3] == RR.PUSHED_OUT and got[2, 3] == RR.PUSHED_OUT
    assert_bits_equal(got[5], got[2], "the same map, the same move")
    assert list(RR.relocate(maps, SPP, 0.25, 0.25, (9, 9, 9), np.zeros((4, 4), F))[:, 3]) == [1, 0, 1, 1]


# ---- resources ----------------------------------------------------------------------------------------------------------------------
# DESIGN.md §31's table: kernel -> (VGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes per workgroup, waves per SIMD that fit)
TABLE = {"reloc": (19, 0, 0, 0, 8), "reloc_lookup_states": (86, 0, 0, 0, 5), "reloc_lookup_none": (92, 0, 0, 0, 5)}


def test_each_new_kernel_has_the_tables_resources():
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import grid_relocate_time
    res = grid_relocate_time.relocate_kernel_resources()
    print(res)
    assert set(res) == set(TABLE)
    for k, (vgprs, scratch, spills, lds, waves) in TABLE.items():
        r = res[k]
        assert r["vgpr_count"] == vgprs and r["private_segment_fixed_size"] == scratch and r["vgpr_spill_count"] == spills, (k, r)
        assert r["sgpr_spill_count"] == 0 and r["group_segment_fixed_size"] == lds, (k, r)
        assert min(512 // ((r["vgpr_count"] + 7) // 8 * 8), 8) == waves, (k, r)
        assert waves >= 5
