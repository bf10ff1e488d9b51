"""Probe-grid lookups without a GPU: the symbols, pt_grid_desc's layout and the Python names; every argument check of the five
pt_grid_* functions in the header's order (they fire before any HIP call, under the function's name); pt_grid_packed_bytes against
the layout; tests/grid_ref.py's f32 restatement of the header's arithmetic against rays.grid_irradiance in float64 on the same
inputs; and the resources of the three kernels read from the code-object notes against DESIGN.md §29's table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import grid_ref as GR

PACK, LOOK, BYTES = "pt_grid_pack", "pt_grid_irradiance", "pt_grid_packed_bytes"


def _err(api):
    return api.lib().pt_last_error().decode()


def test_new_symbols_struct_and_names(api):
    from conftest import ROOT
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for n in ("pt_grid_packed_bytes", "pt_grid_pack", "pt_grid_pack_device", "pt_grid_irradiance", "pt_grid_irradiance_device"):
        assert hasattr(L, n), n
        assert n + "(" in header, n
    assert "} pt_grid_desc;" in header
    D = api.GridDesc
    assert C.sizeof(D) == 52
    assert [(f, getattr(D, f).offset) for f, _ in D._fields_] == [("lo", 0), ("hi", 12), ("counts", 24), ("sh_samples", 36), ("map_res", 40),
                                                                  ("map_samples", 44), ("power", 48)]
    for n in ("grid_desc", "grid_packed_bytes", "grid_pack", "grid_irradiance", "ProbeGrid"):
        assert hasattr(api, n), n
    for n in ("bake", "irradiance", "shade"):
        assert hasattr(api.ProbeGrid, n), n
    d = api.grid_desc((0, 1, 2), (3, 4, 5), (2, 3, 4), 64, 8, 4)
    assert list(d.lo) == [0, 1, 2] and list(d.hi) == [3, 4, 5] and list(d.counts) == [2, 3, 4]
    assert (d.sh_samples, d.map_res, d.map_samples, d.power) == (64, 8, 4, 3)


GOOD = dict(lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), counts=(2, 2, 2), sh_samples=64, map_res=4, map_samples=2, power=3)
INF, NAN = float("inf"), float("nan")
# (what breaks, what later checks refuse as well, the message): the header's order, desc checks first
DESC_CASES = [
    # 2. the counts
    (dict(counts=(0, 2, 2)), dict(lo=(NAN, 0, 0), sh_samples=0, map_res=5, map_samples=0, power=0), "counts 0 x 2 x 2 must be at least 1 each"),
    (dict(counts=(2, -3, 2)), dict(hi=(0, 0, 0), power=9), "counts 2 x -3 x 2 must be at least 1"),
    (dict(counts=(2, 2, 0)), dict(sh_samples=-1), "must be at least 1 each"),
    (dict(counts=(2048, 2048, 2)), dict(lo=(INF, 0, 0), sh_samples=0, map_res=3), "make more than 4194304 probes"),
    (dict(counts=(1 << 30, 1 << 30, 1 << 30)), dict(power=0), "make more than 4194304 probes"),
    (dict(counts=(1 << 22, 1, 2)), dict(map_samples=0), "make more than 4194304 probes"),
    # 3. the corners
    (dict(lo=(0.0, NAN, 0.0)), dict(sh_samples=0, map_res=5, map_samples=0, power=0), "is not finite"),
    (dict(hi=(1.0, 1.0, INF)), dict(sh_samples=0, power=9), "is not finite"),
    (dict(lo=(-INF, 0.0, 0.0)), dict(map_res=64), "is not finite"),
    (dict(hi=(0.0, 1.0, 1.0)), dict(sh_samples=0, map_res=5, map_samples=0, power=0), "hi[0] = 0 must be above lo[0] = 0"),
    (dict(hi=(1.0, 1.0, -1.0)), dict(map_samples=-1), "hi[2] = -1 must be above"),
    # 4. sh_samples
    (dict(sh_samples=0), dict(map_res=5, map_samples=0, power=0), "sh_samples 0 must be at least 1"),
    (dict(sh_samples=-7), dict(map_res=2, power=9), "sh_samples -7 must be"),
    # 5. map_res
    (dict(map_res=5), dict(map_samples=0, power=0), "map_res 5 must be 0, 4, 8, 16 or 32"),
    (dict(map_res=2), dict(power=9), "map_res 2 must be"),
    (dict(map_res=64), dict(map_samples=0), "map_res 64 must be"),
    (dict(map_res=-4), {}, "map_res -4 must be"),
    # 6. map_samples, with maps
    (dict(map_samples=0), dict(power=0), "map_samples 0 must be at least 1"),
    (dict(map_samples=-2, map_res=32), dict(power=9), "map_samples -2 must be"),
    # 7. power
    (dict(power=0), {}, "power 0 must be 1..8"),
    (dict(power=9), {}, "power 9 must be 1..8"),
    (dict(power=-1, map_res=0, map_samples=0), {}, "power -1 must be"),
]


def _desc(api, a):
    return api.grid_desc(a["lo"], a["hi"], a["counts"], a["sh_samples"], a["map_res"], a["map_samples"], a["power"])


def _buffers():
    sums = np.full(8 * 36, 3.0, np.float32)
    maps = np.full(8 * 16 * 4, 5.0, np.float32)
    packed = np.full(8 * 36 + 8 * 36 * 2 + 8, 77.0, np.float32)
    recs = np.zeros((5, 8), np.float32)
    out = np.full((5, 4), 77.0, np.float32)
    return sums, maps, packed, recs, out


def _calls(api, a, bufs, m=5):
    """(function name, thunk) for the five functions on desc fields a and the buffers: the later checks' arguments come with `a`."""
    L = api.lib()
    p = lambda k: a.get(k, bufs[k])
    d = lambda: (None if a.get("null_desc") else C.byref(_desc(api, a)))
    mm = a.get("m", m)
    return [(BYTES, lambda: -1 if L.pt_grid_packed_bytes(d()) == 0 else 0),
            (PACK, lambda: L.pt_grid_pack(d(), p("sums"), p("maps"), p("packed"))),
            (PACK, lambda: L.pt_grid_pack_device(d(), p("sums"), p("maps"), p("packed"), None)),
            (LOOK, lambda: L.pt_grid_irradiance(d(), p("packed"), mm, p("recs"), p("out"))),
            (LOOK, lambda: L.pt_grid_irradiance_device(d(), p("packed"), mm, p("recs"), p("out"), None))]


def test_desc_checks_in_order_for_all_five_functions(api):
    """Each case breaks one field, alone and then together with fields and arguments that later checks refuse: the earliest broken
    check answers, under the function's name, from each of the five functions."""
    sums, maps, packed, recs, out = _buffers()
    bufs = dict(sums=sums.ctypes.data, maps=maps.ctypes.data, packed=packed.ctypes.data, recs=recs.ctypes.data, out=out.ctypes.data)
    later = dict(m=-1, sums=None, maps=None, packed=None, recs=None, out=None)
    for name, call in _calls(api, dict(GOOD, null_desc=True), bufs) + _calls(api, dict(GOOD, null_desc=True, counts=(0, 0, 0), **later), bufs):
        assert call() == -1 and _err(api) == name + ": null desc", (name, _err(api))
    for change, also, msg in DESC_CASES:
        for extra in ({}, also, dict(also, **later)):
            a = dict(GOOD, **extra)
            a.update(change)
            for name, call in _calls(api, a, bufs):
                assert call() == -1, (change, extra, name)
                assert _err(api).startswith(name + ": ") and msg in _err(api), (change, extra, name, _err(api))
    assert (packed == 77).all() and (out == 77).all()


def test_buffer_checks_in_order(api):
    L = api.lib()
    sums, maps, packed, recs, out = _buffers()
    s, mp, pk, r, o = (v.ctypes.data for v in (sums, maps, packed, recs, out))
    d4, d0 = C.byref(_desc(api, GOOD)), C.byref(_desc(api, dict(GOOD, map_res=0, map_samples=0)))
    pack_cases = [
        ((d4, None, mp, pk), "null coeff_sums"), ((d4, None, None, None), "null coeff_sums"), ((d0, None, mp, None), "null coeff_sums"),
        ((d4, s, mp, None), "null packed buffer"), ((d4, s, None, None), "null packed buffer"), ((d0, s, mp, None), "null packed buffer"),
        ((d0, s, mp, pk), "maps given although map_res is 0"), ((d4, s, None, pk), "null maps although map_res is 4"),
    ]
    for args, msg in pack_cases:
        for fn, tail in ((L.pt_grid_pack, ()), (L.pt_grid_pack_device, (None,))):
            assert fn(*args, *tail) == -1 and _err(api) == PACK + ": " + msg, (msg, _err(api))
    # the device form: the packed buffer over an input, checked last
    for args in ((d4, s, mp, s), (d4, s, mp, mp + 16), (d0, s, None, s + 8 * 36 * 4 - 4), (d4, pk + 16, mp, pk)):
        assert L.pt_grid_pack_device(*args, None) == -1 and _err(api) == PACK + ": the packed buffer overlaps an input", (args, _err(api))
    look_cases = [
        ((d4, pk, -1, r, o), "m -1 must not be negative"), ((d4, None, -5, None, None), "m -5 must not be negative"),
        ((d4, None, 5, r, o), "null packed buffer"), ((d4, None, 5, None, None), "null packed buffer"),
        ((d4, pk, 5, None, o), "null records"), ((d4, pk, 5, None, None), "null records"),
        ((d4, pk, 5, r, None), "null output buffer"),
    ]
    for args, msg in look_cases:
        for fn, tail in ((L.pt_grid_irradiance, ()), (L.pt_grid_irradiance_device, (None,))):
            assert fn(*args, *tail) == -1 and _err(api) == LOOK + ": " + msg, (msg, _err(api))
    for args in ((d4, pk, 5, r, r), (d4, pk, 5, r, r + 5 * 32 - 4), (d4, pk, 5, r, pk), (d4, pk, 5, r, pk + api.grid_packed_bytes(_desc(api, GOOD)) - 4),
                 (d0, pk, 5, r + 16, r)):
        assert L.pt_grid_irradiance_device(*args, None) == -1 and _err(api) == LOOK + ": the output buffer overlaps an input", (args, _err(api))
    # m == 0: 0 after the desc checks, whatever the buffers; nothing is looked at or written
    for d in (d4, d0):
        assert L.pt_grid_irradiance(d, None, 0, None, None) == 0 and L.pt_grid_irradiance_device(d, None, 0, None, None, None) == 0
        assert L.pt_grid_irradiance(d, pk, 0, r, o) == 0 and L.pt_grid_irradiance_device(d, pk, 0, r, r, None) == 0
    bad = C.byref(_desc(api, dict(GOOD, power=0)))
    assert L.pt_grid_irradiance(bad, None, 0, None, None) == -1 and "power 0" in _err(api)
    assert (packed == 77).all() and (out == 77).all() and (sums == 3).all() and (maps == 5).all()
    # the Python wrappers refuse what would read past an array
    d = _desc(api, GOOD)
    with pytest.raises(api.PtError, match="coeff_sums holds 36 float32 words, the grid needs 288"):
        api.grid_pack(d, np.zeros((1, 9, 4), np.float32), maps.reshape(8, 4, 4, 4))
    with pytest.raises(api.PtError, match="maps are missing but desc.map_res is 4"):
        api.grid_pack(d, sums)
    with pytest.raises(api.PtError, match="packed holds 7 float32 words"):
        api.grid_irradiance(np.zeros(7, np.float32), d, recs)
    with pytest.raises(api.PtError, match="pt_grid_packed_bytes: power 11"):
        api.grid_packed_bytes(_desc(api, dict(GOOD, power=11)))
    assert api.grid_irradiance(np.zeros(api.grid_packed_bytes(d) // 4, np.float32), d, np.zeros((0, 8), np.float32)).shape == (0, 4)


@pytest.mark.parametrize("res", [0, 4, 32])
def test_packed_bytes_is_the_layouts(api, res):
    for counts in ((1, 1, 1), (3, 2, 2), (7, 5, 3), (1 << 22, 1, 1)):
        n = counts[0] * counts[1] * counts[2]
        want = n * 9 * 16 + (n * (res + 2) ** 2 * 8 if res else 0)
        assert api.grid_packed_bytes(_desc(api, dict(GOOD, counts=counts, map_res=res))) == want == GR.packed_bytes(counts, res)
        assert want % 16 == 0 and (n * 9 * 16) % 16 == 0


def test_the_restated_gutter_is_oct_borders(api):
    from cudapathtracer_amd import rays
    for res in (4, 8, 16, 32):
        idx = np.arange(res * res, dtype=np.float64).reshape(1, res, res, 1)
        sy, sx = GR.border_source(res)
        assert np.array_equal(rays.oct_border(idx)[0, :, :, 0], sy * res + sx)
    sums = np.random.default_rng(5).standard_normal((3, 9, 4)).astype(np.float32)
    coeff, tex = GR.pack(48, sums)
    assert tex is None and coeff.dtype == np.float32 and not coeff[..., 3].any()
    assert np.abs(coeff[..., :3] - rays._sh_convolved(sums.astype(np.float64), 48)).max() <= 4 * 2.0 ** -24 * np.abs(coeff).max()


# ---- the restatement against rays.grid_irradiance in float64 ----------------------------------------------------------------
LO, HI, COUNTS, SH_SAMPLES, MAP_SAMPLES, RES, M, SEED = (-1.0, 0.5, 2.0), (1.5, 1.75, 3.0), (3, 2, 2), 96, 4, 8, 2000, 11
# The largest |f32 - f64| / max(|f64|, mean |f64|) of this file's four cases as measured on the seeded data (per case below); the
# test asserts 4x the largest, which covers library drift only.
MEASURED = {(0, 1): 3.83e-7, (0, 3): 3.83e-7, (8, 1): 3.67e-7, (8, 3): 5.10e-7}          # (map_res, power): a few f32 roundings; none of the 2000 points is left out


def _inputs():
    rng = np.random.default_rng(SEED)
    n = COUNTS[0] * COUNTS[1] * COUNTS[2]
    sums = np.zeros((n, 9, 4), np.float32)
    sums[:, 0, :3] = rng.uniform(4.0, 12.0, (n, 3))
    sums[:, 1:, :3] = rng.uniform(-3.0, 3.0, (n, 8, 3))
    mean = rng.uniform(0.4, 1.6, (n, RES, RES))
    var = rng.uniform(0.02, 0.3, (n, RES, RES))
    maps = np.zeros((n, RES, RES, 4), np.float32)
    maps[..., 0], maps[..., 1] = mean * MAP_SAMPLES, (mean * mean + var) * MAP_SAMPLES
    lo, hi = np.array(LO), np.array(HI)
    cell = (hi - lo) / (np.array(COUNTS) - 1)
    pts = rng.uniform(lo - cell, hi + cell, (M, 3)).astype(np.float32)
    nrm = rng.standard_normal((M, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    return sums, maps, pts, nrm


def _weight_sum64(pts, maps, power):
    """rays.grid_irradiance's weight sum in float64: the function itself on probes whose E is 1 times the same on probes whose E is
    the weight's indicator would need its internals, so the sum is formed from its parts, distance_visibility and the trilinear
    weights, as the function forms it."""
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
                v = p - np.stack([pos[a][0] + pos[a][1] * i[a] for a in range(3)], -1)
                dist = np.sqrt((v * v).sum(-1))
                d = np.where((dist > 0)[:, None], v, np.array([0.0, 0.0, 1.0])[None, :])
                den = den + tri * rays.distance_visibility(maps.astype(np.float64)[j], MAP_SAMPLES, d, dist, power)
    return den


@pytest.mark.parametrize("res,power", sorted(MEASURED))
def test_the_restatement_follows_grid_irradiance_in_float64(api, res, power):
    """A seeded 3 x 2 x 2 grid, maps with variance, 2000 points inside and up to a cell outside the grid. The restatement runs on the
    f32 inputs, rays.grid_irradiance on the same values in float64. Points whose float64 weight sum lies in [0.5e-6, 2e-6] are left
    out (the fallback threshold is the lookup's one discontinuity), at most 1 % of them."""
    from cudapathtracer_amd import rays
    sums, maps, pts, nrm = _inputs()
    lo32, hi32 = np.array(LO, np.float32), np.array(HI, np.float32)
    assert np.array_equal(lo32.astype(np.float64), LO) and np.array_equal(hi32.astype(np.float64), HI)          # the corners are exact in f32
    coeff, tex = GR.pack(SH_SAMPLES, sums, maps if res else None, MAP_SAMPLES)
    got, fallback = GR.lookup(LO, HI, COUNTS, coeff, tex, power, rays.irradiance_records(pts, nrm))
    want = rays.grid_irradiance(LO, HI, COUNTS, sums.astype(np.float64), SH_SAMPLES, pts.astype(np.float64), nrm.astype(np.float64),
                                maps.astype(np.float64) if res else None, MAP_SAMPLES, power)
    assert got.dtype == np.float32 and got.shape == (M, 4) and want.dtype == np.float64
    keep = np.ones(M, bool)
    if res:
        w64 = _weight_sum64(pts, maps, power)
        keep = ~((w64 >= 0.5e-6) & (w64 <= 2e-6))
        print("left out", int((~keep).sum()), "of", M, "; fallback taken by", int(fallback.sum()), "; smallest kept weight sum", w64[keep].min())
        assert (~keep).sum() <= M // 100
        assert np.array_equal(fallback[keep], w64[keep] < 1e-6)
        assert np.abs(got[keep, 3] - w64[keep]).max() <= 1e-5
    else:
        assert not fallback.any() and np.abs(got[:, 3] - 1.0).max() <= 4 * 2.0 ** -23
    err = np.abs(got[keep, :3] - want[keep]) / np.maximum(np.abs(want[keep]), np.abs(want[keep]).mean())
    print("res", res, "power", power, "max relative error", err.max())
    assert err.max() <= 4 * max(MEASURED.values())
    assert 0.25 * MEASURED[(res, power)] <= err.max()                                        # the table above is this data's, not a guess


# DESIGN.md §29's table: kernel -> (VGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes per workgroup, waves per SIMD that fit)
TABLE = {"grid_pack": (16, 0, 0, 0, 8), "grid_irradiance_maps": (89, 0, 0, 0, 5), "grid_irradiance_plain": (66, 0, 0, 0, 7)}


def test_each_grid_kernel_has_the_tables_resources():
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import grid_time
    res = grid_time.grid_kernel_resources()
    print(res)
    assert set(res) == set(TABLE)
    for k, (vgprs, scratch, spills, lds, waves) in TABLE.items():
        r = res[k]
        assert r["vgpr_count"] == vgprs and r["private_segment_fixed_size"] == scratch and r["vgpr_spill_count"] == spills, (k, r)
        assert r["sgpr_spill_count"] == 0 and r["group_segment_fixed_size"] == lds, (k, r)
        assert min(512 // ((r["vgpr_count"] + 7) // 8 * 8), 8) == waves, (k, r)
