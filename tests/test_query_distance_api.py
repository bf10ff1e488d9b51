"""Distance probes without a GPU: the new symbols of the C ABI and of the Python wrapper, every argument check of pt_query_distance and
pt_query_distance_rays_device in the header's order (they fire before any HIP call, under the function's name; n == 0 returns 0 before
the scene or anything else is looked at), the record builder, the octahedral helpers of cudapathtracer_amd/rays.py (round trip,
gutter, visibility, the grid lookup), the f32 restatement of the device's map, and the resources of the two trace kernels read from
the code-object notes against DESIGN.md §28's table."""
import os
import sys

import numpy as np
import pytest

import distance_ref as DR

N = 5
WALK, RAYS = "pt_query_distance", "pt_query_distance_rays_device"
CENTRE = 4


def _err(api):
    return api.lib().pt_last_error().decode()


def test_new_symbols_are_declared_and_exported(api):
    from conftest import ROOT
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for n in ("pt_query_distance_device", "pt_query_distance", "pt_query_distance_rays_device"):
        assert hasattr(L, n), n
        assert n + "(" in header, n
    assert "#define PT_QUERY_TEXEL_CENTRE 4u" in header and api.QUERY_TEXEL_CENTRE == CENTRE
    assert hasattr(api.Scene, "query_distance") and hasattr(api.Scene, "query_distance_rays")
    from cudapathtracer_amd import rays
    for n in ("distance_records", "oct_decode", "oct_encode", "oct_border", "distance_visibility", "grid_irradiance"):
        assert hasattr(rays, n), n


def _buffers():
    recs = np.zeros((N, 8), np.float32)
    out = np.full((N * 16 * 2, 4), 77.0, np.float32)           # holds N * 16 float4, and N * 16 rays
    fake = np.zeros(4096, np.uint8)                            # stands for a scene where a check before the scene's must fire
    return recs, out, fake


def test_distance_argument_checks_in_order(api):
    """Each case breaks one argument, alone and then together with arguments that later checks of the header's list refuse (`also`):
    the earliest broken check answers, so the message shows the order."""
    L = api.lib()
    recs, out, fake = _buffers()
    r, o, s = recs.ctypes.data, out.ctypes.data, fake.ctypes.data
    good = dict(scene=s, n=N, recs=r, res=4, spp_lane=2, seed=1, first_stream=0, out=o, flags=0)
    far = 0xffffffff
    cases = [
        # 1. n < 0 or n * R * R > 1 << 28
        (dict(n=-1), dict(scene=None, res=3, spp_lane=0, flags=8, first_stream=far), "n -1 at"),
        (dict(n=(1 << 24) + 1), dict(recs=None, spp_lane=0, flags=1), "n 16777217 at res 4 must be 0..268435456"),
        (dict(n=(1 << 18) + 1, res=32), dict(out=None, flags=CENTRE), "n 262145 at res 32 must be"),
        (dict(res=1 << 30), dict(scene=None, spp_lane=0), "n 5 at res 1073741824 must be"),
        # 2. a NULL scene, records or maps buffer
        (dict(scene=None), dict(res=3, spp_lane=0, flags=8, first_stream=far), "null scene"),
        (dict(recs=None), dict(res=0, spp_lane=0, flags=8, first_stream=far), "null records"),
        (dict(out=None), dict(res=64, spp_lane=0, flags=1, first_stream=far), "null output buffer"),
        # 3. res
        (dict(res=0), dict(spp_lane=0, flags=8, first_stream=far), "res 0 must be 4, 8, 16 or 32"),
        (dict(res=3), dict(spp_lane=0, flags=8, first_stream=far), "res 3 must be"),
        (dict(res=2), dict(spp_lane=-1, flags=1), "res 2 must be"),
        (dict(res=64), dict(spp_lane=-1), "res 64 must be"),
        (dict(res=12), dict(flags=CENTRE), "res 12 must be"),
        (dict(res=-4), dict(flags=8), "res -4 must be"),
        # 4. spp_lane < 1 or R * R * spp_lane > 1 << 22
        (dict(spp_lane=0), dict(flags=8, first_stream=far), "spp_lane 0 at res 4 must be 1..4194304"),
        (dict(spp_lane=-2, res=8), dict(flags=CENTRE | 8, first_stream=far), "spp_lane -2 at res 8"),
        (dict(spp_lane=(1 << 18) + 1), dict(flags=1), "spp_lane 262145 at res 4"),
        (dict(spp_lane=(1 << 12) + 1, res=32), dict(flags=CENTRE), "spp_lane 4097 at res 32"),
        # 5. the flags
        (dict(flags=api.QUERY_REORDER), dict(first_stream=far), "PT_QUERY_REORDER"),
        (dict(flags=api.QUERY_REORDER | api.QUERY_STREAM_PAD | CENTRE), {}, "PT_QUERY_REORDER"),
        (dict(flags=8), dict(first_stream=far), "unknown flag bits 0x8"),
        (dict(flags=0x80000002), dict(res=16), "unknown flag bits 0x80000000"),
        (dict(flags=CENTRE | 8), dict(first_stream=far), "unknown flag bits 0x8"),               # ... before centre mode's spp_lane = 2
        # 6. centre mode has one sample a texel
        (dict(flags=CENTRE), dict(first_stream=far), "spp_lane 2 must be 1"),
        (dict(flags=CENTRE | api.QUERY_STREAM_PAD, spp_lane=3), dict(res=32), "spp_lane 3 must be 1"),
        # 7. the stream range, without PT_QUERY_STREAM_PAD
        (dict(first_stream=(1 << 31) - 16 * N + 1), {}, "pass 2^31"),
        (dict(first_stream=far), dict(res=32), "pass 2^31"),
        (dict(n=1 << 24, first_stream=(1 << 31) - (1 << 28) + 1), {}, "pass 2^31"),
    ]

    def args(a):
        return (a["scene"], a["n"], a["recs"], a["res"], a["spp_lane"], a["seed"], a["first_stream"], a["out"], a["flags"])

    for change, also, msg in cases:
        for extra in ({}, also):
            a = dict(good, **extra)
            a.update(change)
            assert L.pt_query_distance(*args(a)) == -1, (change, extra)
            assert WALK + ": " in _err(api) and msg in _err(api), (change, extra, _err(api))
            assert L.pt_query_distance_device(*args(a), None) == -1, (change, extra)
            assert WALK + ": " in _err(api) and msg in _err(api), (change, extra, _err(api))
    # n == 0: 0 with a NULL scene, whatever else is passed; nothing is looked at or written
    for z in ((None, 0, None, 0, 0, 0, 0, None), (s, 0, r, 4, 2, 1, 0, o), (None, 0, None, 1 << 30, 0, 0, far, None)):
        assert L.pt_query_distance(*z, 0xff) == 0 and L.pt_query_distance_device(*z, 0xff, None) == 0
    assert (out == 77).all() and not fake.any()
    sc = api.Scene.__new__(api.Scene)                          # no device scene: the checks fire before it is looked at
    sc.h = None
    with pytest.raises(api.PtError, match="pt_query_distance: null scene"):
        sc.query_distance(recs, 4, 2)
    with pytest.raises(api.PtError, match="pt_query_distance: n 5 at res 1073741824"):
        sc.query_distance(recs, 1 << 30)
    assert sc.query_distance(np.zeros((0, 8), np.float32), 8).shape == (0, 8, 8, 4)


def test_centre_mode_skips_the_stream_range_check(api):
    """The device check is the only one behind the stream range. It is reached with a stand-in scene whose first word, the scene's
    device index, names a device no machine has: the check fails there, with or without a device, before anything is launched."""
    L = api.lib()
    recs, out, _ = _buffers()
    nowhere = np.full(4096, 0x7f, np.uint8)
    r, o, s = recs.ctypes.data, out.ctypes.data, nowhere.ctypes.data
    far = 0xffffffff
    for flags, msg in ((0, "pass 2^31"), (CENTRE, "scene lives on HIP device 2139062143"), (CENTRE | api.QUERY_STREAM_PAD, "scene lives on HIP device"),
                       (api.QUERY_STREAM_PAD, "scene lives on HIP device")):
        assert L.pt_query_distance(s, N, r, 4, 1, 1, far, o, flags) == -1 and WALK + ": " in _err(api) and msg in _err(api), (flags, _err(api))
        assert L.pt_query_distance_device(s, N, r, 4, 1, 1, far, o, flags, None) == -1 and msg in _err(api), (flags, _err(api))
        assert L.pt_query_distance_rays_device(s, N, r, 4, 1, far, None, o, flags, None) == -1 and RAYS + ": " in _err(api) and msg in _err(api), (flags, _err(api))
    assert (out == 77).all() and (nowhere == 0x7f).all()


def test_distance_rays_argument_checks_in_order(api):
    """pt_query_distance_rays_device has the checks of the list that its arguments can fail, in the same order."""
    L = api.lib()
    recs, out, fake = _buffers()
    off = np.zeros(N * 16, np.uint32)
    r, o, s, d = recs.ctypes.data, out.ctypes.data, fake.ctypes.data, off.ctypes.data
    good = dict(scene=s, n=N, recs=r, res=4, seed=1, first_stream=0, off=d, rays=o, flags=0)
    far = 0xffffffff
    cases = [
        (dict(n=-1), dict(scene=None, res=3, flags=8, first_stream=far), "n -1 at"),
        (dict(n=(1 << 24) + 1), dict(recs=None, flags=1), "n 16777217 at res 4 must be 0..268435456"),
        (dict(scene=None), dict(res=3, flags=8, first_stream=far), "null scene"),
        (dict(recs=None), dict(res=0, flags=8), "null records"),
        (dict(rays=None), dict(res=64, flags=1), "null output buffer"),
        (dict(res=0), dict(flags=8, first_stream=far), "res 0 must be 4, 8, 16 or 32"),
        (dict(res=6), dict(flags=1), "res 6 must be"),
        (dict(res=64), {}, "res 64 must be"),
        (dict(flags=api.QUERY_REORDER), dict(first_stream=far), "PT_QUERY_REORDER"),
        (dict(flags=8), dict(first_stream=far), "unknown flag bits 0x8"),
        (dict(flags=16 | CENTRE), {}, "unknown flag bits 0x10"),
        (dict(first_stream=(1 << 31) - 16 * N + 1), {}, "pass 2^31"),
        (dict(first_stream=far, res=32), {}, "pass 2^31"),
    ]
    for change, also, msg in cases:
        for extra in ({}, also):
            a = dict(good, **extra)
            a.update(change)
            got = L.pt_query_distance_rays_device(a["scene"], a["n"], a["recs"], a["res"], a["seed"], a["first_stream"], a["off"], a["rays"], a["flags"], None)
            assert got == -1, (change, extra)
            assert RAYS + ": " in _err(api) and msg in _err(api), (change, extra, _err(api))
    assert L.pt_query_distance_rays_device(None, 0, None, 0, 0, 0, None, None, 0xff, None) == 0
    assert (out == 77).all() and not fake.any()


def test_the_record_builder(api):
    from cudapathtracer_amd import rays
    p = np.array([(0.5, -0.25, 1.5), (1.0, 2.0, 3.0)], np.float32)
    r = rays.distance_records(p, 7.5)
    assert r.shape == (2, 8) and r.dtype == np.float32
    assert np.array_equal(r[:, 0:3].view(np.uint32), p.view(np.uint32)) and (r[:, 3] == 7.5).all() and not r[:, 4:].view(np.uint32).any()
    assert np.array_equal(r.view(np.uint32), rays.sh_records(p, 7.5).view(np.uint32))
    assert np.array_equal(rays.distance_records(p, 7.5, device="cpu").numpy().view(np.uint32), r.view(np.uint32))
    g = rays.sh_grid((0.0, 10.0, 100.0), (1.0, 12.0, 103.0), (2, 3, 4), 2.5)                 # the grid is sh_grid's, with the lookups' max_t
    assert g.shape == (24, 8) and (g[:, 3] == 2.5).all()


def _square(n=257):
    g = np.linspace(0.0, 1.0, n)
    u, v = np.meshgrid(g, g, indexing="xy")
    return np.stack([u.ravel(), v.ravel()], 1)


def test_encode_inverts_decode_on_the_whole_square(api):
    """A 257 x 257 grid of float64 points: it holds the corners (all four are -z, told apart by the signs of the zeros), the edges'
    middles (+-x, +-y), the centre (+z) and the fold lines |2u - 1| + |2v - 1| = 1, which pass through grid points exactly."""
    from cudapathtracer_amd import rays
    uv = _square()
    f = 2 * uv - 1
    assert (np.abs(f[:, 0]) + np.abs(f[:, 1]) == 1).sum() >= 4 * 128
    d = rays.oct_decode(uv)
    assert d.dtype == np.float64 and d.shape == (len(uv), 3)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-15
    back = rays.oct_encode(d)
    print("max |encode(decode(uv)) - uv|", np.abs(back - uv).max())
    assert np.abs(back - uv).max() <= 1e-12
    at = lambda u, v: rays.oct_decode(np.array([[u, v]], np.float64))[0]
    assert np.allclose(at(0.5, 0.5), (0, 0, 1)) and np.allclose(at(1.0, 0.5), (1, 0, 0)) and np.allclose(at(0.5, 1.0), (0, 1, 0))
    assert np.allclose(at(0.0, 0.5), (-1, 0, 0)) and np.allclose(at(0.5, 0.0), (0, -1, 0))
    for c in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert np.allclose(at(*map(float, c)), (0, 0, -1))
    assert np.allclose(rays.oct_encode(7.0 * d), uv, rtol=0, atol=1e-12)                       # any length
    import torch
    assert np.allclose(rays.oct_decode(torch.from_numpy(uv)).numpy(), d, rtol=0, atol=1e-15)
    assert np.allclose(rays.oct_encode(torch.from_numpy(d)).numpy(), back, rtol=0, atol=1e-15)
    assert rays.oct_decode(uv.astype(np.float32)).dtype == np.float32


def test_the_devices_map_is_unit_and_stays_in_its_texel(api):
    """tests/distance_ref.py's f32 restatement of the header's arithmetic, on every texel of all four map sizes at a grid of uniforms
    that holds rng_uniform's extremes (2^-33, and 1.0, which the largest draw rounds to) and values next to the fold: |d| is within
    4 ulp of 1, and rays.oct_encode(d), in float64, lies in the texel's square to within one ulp of its edges; the ulp is 1's, 2^-23
    (the three components of d carry at most a rounding each from the reciprocal, its square root and the product).
    Largest deviations found: | |d| - 1 | = 1.21 ulp; encode(d) past an edge of its texel: 0.083 ulp."""
    from cudapathtracer_amd import rays
    ulp = 2.0 ** -23
    us = np.array([2.0 ** -33, 1e-6, 0.125, 0.3333, 0.5, 0.6667, 0.875, 1.0 - 2.0 ** -24, 1.0], np.float32)
    worst_norm = worst_edge = 0.0
    for res in (4, 8, 16, 32):
        ty, tx, a, b = (v.ravel() for v in np.meshgrid(np.arange(res), np.arange(res), us, us, indexing="ij"))
        d = DR.oct_map(tx, ty, a, b, res)
        assert d.dtype == np.float32 and d.shape == (len(tx), 3)
        d64 = d.astype(np.float64)
        worst_norm = max(worst_norm, np.abs(np.sqrt((d64 ** 2).sum(1)) - 1.0).max())
        uv = rays.oct_encode(d64)
        lo, hi = np.stack([tx, ty], 1) / res, np.stack([tx + 1, ty + 1], 1) / res
        worst_edge = max(worst_edge, (lo - uv).max(), (uv - hi).max())
        # the restatement against the float64 map: the same directions to f32 accuracy
        want = rays.oct_decode(np.stack([(tx + a.astype(np.float64)) / res, (ty + b.astype(np.float64)) / res], 1))
        assert np.abs(d64 - want).max() <= 4 * ulp
        centre = DR.oct_map(tx, ty, np.float32(0.5), np.float32(0.5), res)
        assert np.abs(centre.astype(np.float64) - rays.oct_decode(np.stack([(tx + 0.5) / res, (ty + 0.5) / res], 1))).max() <= 2 * ulp
    print("max | |d| - 1 | / ulp", worst_norm / ulp, "max excursion of encode(d) past its texel / ulp", worst_edge / ulp)
    assert worst_norm <= 4 * ulp
    assert worst_edge <= ulp
    assert tuple(DR.oct_map([3], [3], np.float32(1.0), np.float32(1.0), 4)[0]) == (0.0, 0.0, -1.0)               # the square's corner
    assert tuple(DR.oct_map([1], [1], np.float32(1.0), np.float32(1.0), 4)[0]) == (0.0, 0.0, 1.0)                # the centre, from texel (1, 1)'s far corner


@pytest.mark.parametrize("res", [4, 8])
def test_the_gutter_copies_the_texel_the_wrap_names(api, res):
    from cudapathtracer_amd import rays
    idx = np.arange(res * res, dtype=np.float64).reshape(res, res)                              # texel (tx, ty) holds ty * res + tx
    maps = np.stack([idx, -idx], -1)[None]                                                      # [1, R, R, 2]
    b = rays.oct_border(maps)
    assert b.shape == (1, res + 2, res + 2, 2)
    assert np.array_equal(b[:, 1:-1, 1:-1], maps)

    def wrap(u, v):
        if u < 0: u, v = -u, 1 - v
        elif u > 1: u, v = 2 - u, 1 - v
        if v < 0: u, v = 1 - u, -v
        elif v > 1: u, v = 1 - u, 2 - v
        return u, v

    seen = 0
    for gy in range(res + 2):
        for gx in range(res + 2):
            if 1 <= gx <= res and 1 <= gy <= res:
                continue
            u, v = wrap((gx - 0.5) / res, (gy - 0.5) / res)
            tx, ty = int(np.floor(u * res)), int(np.floor(v * res))
            assert 0 <= tx < res and 0 <= ty < res
            assert b[0, gy, gx, 0] == ty * res + tx and b[0, gy, gx, 1] == -(ty * res + tx), (gx, gy)
            seen += 1
    assert seen == 4 * res + 4
    r = res - 1
    assert b[0, 0, 0, 0] == idx[r, r] and b[0, 0, res + 1, 0] == idx[r, 0] and b[0, res + 1, 0, 0] == idx[0, r] and b[0, res + 1, res + 1, 0] == idx[0, 0]
    assert b[0, 1, 0, 0] == idx[r, 0] and b[0, 1, res + 1, 0] == idx[r, r] and b[0, 0, 1, 0] == idx[0, r] and b[0, res + 1, 1, 0] == idx[r, r]
    import torch
    assert np.array_equal(rays.oct_border(torch.from_numpy(maps)).numpy(), b)
    # the wrap is the map's own: a point just outside the square decodes, by the wrapped point, to the direction next to the edge
    eps = 1e-9
    for u, v in ((-eps, 0.3), (1 + eps, 0.8), (0.4, -eps), (0.9, 1 + eps)):
        inside = rays.oct_decode(np.array([wrap(u, v)]))[0]
        edge = rays.oct_decode(np.array([[min(max(u, 0.0), 1.0), min(max(v, 0.0), 1.0)]]))[0]
        assert np.abs(inside - edge).max() < 1e-8


def test_visibility_of_a_flat_map_is_a_step_and_of_a_spread_map_chebyshevs_bound(api):
    from cudapathtracer_amd import rays
    res, samples, D = 8, 4, 2.5
    flat = np.zeros((3, res, res, 4))
    flat[..., 0], flat[..., 1] = D * samples, D * D * samples
    rng = np.random.default_rng(3)
    d = rng.standard_normal((3, 3))
    for dist, want in ((2.5, 1.0), (1.0, 1.0), (0.0, 1.0), (np.nextafter(2.5, 3.0), 0.0), (2.6, 0.0), (100.0, 0.0)):
        got = rays.distance_visibility(flat, samples, d, np.full(3, dist))
        assert got.shape == (3,) and (got == want).all(), (dist, got)
    # a map with variance, looked up at a texel's centre: no neighbour enters, and the closed form holds
    spread = np.zeros((1, res, res, 4))
    mean, msq = rng.uniform(1.0, 2.0, (res, res)), None
    msq = mean * mean + rng.uniform(0.01, 0.5, (res, res))
    spread[0, ..., 0], spread[0, ..., 1] = mean * samples, msq * samples
    worst = 0.0
    for ty, tx in ((0, 0), (3, 5), (7, 7), (7, 0), (4, 4)):
        c = rays.oct_decode(np.array([[(tx + 0.5) / res, (ty + 0.5) / res]]))
        for dist in (0.5, mean[ty, tx], 2.5, 4.0):
            for power in (1, 3):
                got = rays.distance_visibility(spread, samples, c, np.array([dist]), power)[0]
                var = msq[ty, tx] - mean[ty, tx] ** 2
                want = 1.0 if dist <= mean[ty, tx] + 1e-13 else (var / (var + (dist - mean[ty, tx]) ** 2)) ** power
                worst = max(worst, abs(got - want))
    print("max error at texel centres", worst)
    assert worst <= 1e-12
    import torch
    t = rays.distance_visibility(torch.from_numpy(flat), samples, torch.from_numpy(d), torch.full((3,), 2.6, dtype=torch.float64))
    assert (t.numpy() == 0).all()
    t = rays.distance_visibility(torch.from_numpy(spread), samples, torch.from_numpy(c), torch.tensor([4.0], dtype=torch.float64), 3)
    assert abs(t.item() - got) <= 1e-12


def test_grid_irradiance_drops_the_probe_that_does_not_see_the_point(api):
    """Two probes on x, A at 0 with E = 1 and B at 1 with E = 0 (band 0 only), the point at x = 0.25: trilinear 0.75."""
    from cudapathtracer_amd import rays
    lo, hi, counts, samples, res, ms = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2, 1, 1), 64, 4, 2
    sums = np.zeros((2, 9, 4))
    sums[0, 0, :3] = samples / (4.0 * np.pi) / (rays.SH_LOBE[0] * rays.SH_C[0])               # E_A(n) = 1 for every n
    p = np.array([[0.25, 0.0, 0.0], [0.75, 0.0, 0.0]])
    nrm = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    tri = np.array([[0.75], [0.25]]) * np.ones((1, 3))
    assert np.abs(rays.sh_irradiance(sums, samples, nrm)[0] - 1.0).max() < 1e-12
    plain = rays.grid_irradiance(lo, hi, counts, sums, samples, p, nrm)
    assert plain.shape == (2, 3) and np.abs(plain - tri).max() <= 1e-12

    def maps(da, db):
        m = np.zeros((2, res, res, 4))
        for j, dd in enumerate((da, db)):
            m[j, ..., 0], m[j, ..., 1] = dd * ms, dd * dd * ms
        return m

    q = lambda m: rays.grid_irradiance(lo, hi, counts, sums, samples, p, nrm, m, ms)
    assert np.array_equal(q(maps(0.1, 5.0)), np.zeros((2, 3)))                                # A ends before the points, B sees them: B's light alone
    assert np.abs(q(maps(5.0, 0.1)) - 1.0).max() <= 1e-12                                     # and the other way round: A's alone
    assert np.abs(q(maps(5.0, 5.0)) - tri).max() <= 1e-12                                     # both see them: trilinear
    assert np.abs(q(maps(0.1, 0.1)) - tri).max() <= 1e-12                                     # neither: the weights vanish, the fallback
    outside = rays.grid_irradiance(lo, hi, counts, sums, samples, np.array([[-3.0, 2.0, 1.0], [9.0, 0.0, 0.0]]), nrm)
    assert np.abs(outside - np.array([[1.0], [0.0]])).max() <= 1e-12                          # clamped at the faces
    import torch
    t = rays.grid_irradiance(lo, hi, counts, torch.from_numpy(sums), samples, torch.from_numpy(p), torch.from_numpy(nrm), torch.from_numpy(maps(0.1, 5.0)), ms)
    assert t.shape == (2, 3) and not t.numpy().any()
    t = rays.grid_irradiance(lo, hi, counts, torch.from_numpy(sums), samples, torch.from_numpy(p), torch.from_numpy(nrm))
    assert np.abs(t.numpy() - tri).max() <= 1e-12


# DESIGN.md §28's table: kernel -> (VGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes per workgroup, waves per SIMD it is launched at)
TABLE = {"distance_jittered": (66, 0, 0, 16384, 7), "distance_centre": (54, 0, 0, 16384, 8)}


def test_each_distance_kernel_fits_the_waves_it_declares():
    """What the compile gives, pinned as tests/test_query_sh_api.py pins sh_kernel's: both kernels fit the waves per SIMD they are
    launched at in VGPRs and LDS (the traversal stack's 16 KB and nothing else), and need no scratch."""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import distance_time
    res, waves = distance_time.distance_kernel_resources(), distance_time.declared_waves()
    print(res, waves)
    assert set(res) == set(TABLE) == set(waves)
    for k, (vgprs, scratch, spills, lds, w) in TABLE.items():
        r = res[k]
        assert waves[k] == w, (k, waves[k])
        assert r["vgpr_count"] == vgprs and r["private_segment_fixed_size"] == scratch and r["vgpr_spill_count"] == spills, (k, r)
        assert r["group_segment_fixed_size"] == lds, (k, r)
        fit = min(512 // ((r["vgpr_count"] + 7) // 8 * 8), (160 * 1024) // r["group_segment_fixed_size"], 8)
        assert fit == w, (k, r, fit)
