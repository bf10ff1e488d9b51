"""Irradiance queries without a GPU: the new symbols of the C ABI and of the Python wrapper, every argument check of
pt_query_irradiance and pt_query_irradiance_rays_device in the header's order (they fire before any HIP call, under the function's
name; n == 0 returns 0 before the scene or anything else is looked at), the record builders of cudapathtracer_amd/rays.py, the host
restatement of the sums' tree on a hand-worked example, its fma against exact rational arithmetic, and the resources of the six
irradiance kernels read from the code-object notes against DESIGN.md §26's table."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import irradiance_ref as IR

N = 5
WALK, RAYS = "pt_query_irradiance", "pt_query_irradiance_rays_device"


def _err(api):
    return api.lib().pt_last_error().decode()


def test_new_symbols_are_declared_and_exported(api):
    from conftest import ROOT
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for n in ("pt_query_irradiance", "pt_query_irradiance_device", "pt_query_irradiance_rays_device"):
        assert hasattr(L, n), n
        assert n + "(" in header, n
    assert hasattr(api.Scene, "query_irradiance") and hasattr(api.Scene, "query_irradiance_rays")
    from cudapathtracer_amd import rays
    assert hasattr(rays, "irradiance_records") and hasattr(rays, "records_from_surfaces")


def _buffers():
    recs = np.zeros((N, 8), np.float32)
    out = np.full((N * 64, 8), 77.0, np.float32)
    sq = np.full((N, 4), 78.0, np.float32)
    fake = np.zeros(4096, np.uint8)                            # stands for a scene where a check before the scene's must fire
    return recs, out, sq, fake


def test_irradiance_argument_checks_in_order(api):
    """Each case breaks one argument, alone and then together with arguments that later checks of the header's list refuse (`also`):
    the earliest broken check answers, so the message shows the order."""
    L = api.lib()
    recs, out, sq, fake = _buffers()
    r, o, q, s = recs.ctypes.data, out.ctypes.data, sq.ctypes.data, fake.ctypes.data
    good = dict(scene=s, n=N, recs=r, lanes=4, spp_lane=2, max_depth=8, integrator=0, use_mis=1, seed=1, first_stream=0, out=o, sq=q, flags=0)
    far = 0xffffffff
    cases = [
        # 1. n < 0 or n * L > 1 << 28
        (dict(n=-1), dict(scene=None, lanes=3, spp_lane=0, integrator=1, flags=4, first_stream=far), "n -1 at"),
        (dict(n=(1 << 26) + 1), dict(recs=None, spp_lane=0, integrator=1, flags=1), "n 67108865 at 4 lanes must be 0..268435456"),
        (dict(n=(1 << 22) + 1, lanes=64), dict(out=None, integrator=3), "n 4194305 at 64 lanes must be"),
        # 2. a NULL scene, records or sum buffer
        (dict(scene=None), dict(lanes=3, spp_lane=0, integrator=1, flags=4, first_stream=far), "null scene"),
        (dict(recs=None), dict(lanes=0, spp_lane=0, integrator=1, flags=4, first_stream=far), "null records"),
        (dict(out=None), dict(lanes=128, spp_lane=0, integrator=1, flags=1, first_stream=far), "null output buffer"),
        # 3. lanes
        (dict(lanes=0), dict(spp_lane=0, integrator=1, flags=4, first_stream=far), "lanes 0 must be a power of two in 1..64"),
        (dict(lanes=3), dict(spp_lane=0, integrator=1, flags=4, first_stream=far), "lanes 3 must be"),
        (dict(lanes=128), dict(spp_lane=-1, integrator=1, flags=1), "lanes 128 must be"),
        (dict(lanes=-4), dict(integrator=1, flags=4), "lanes -4 must be"),
        # 4. spp_lane < 1 or L * spp_lane > 1 << 22
        (dict(spp_lane=0), dict(integrator=1, flags=4, first_stream=far), "spp_lane 0 at 4 lanes must be 1..4194304"),
        (dict(spp_lane=-2, lanes=1), dict(integrator=1, flags=4, first_stream=far), "spp_lane -2 at 1 lanes"),
        (dict(spp_lane=(1 << 20) + 1), dict(integrator=3, flags=1), "spp_lane 1048577 at 4 lanes"),
        (dict(spp_lane=(1 << 16) + 1, lanes=64), dict(integrator=-1), "spp_lane 65537 at 64 lanes"),
        # 5. the integrator
        (dict(integrator=1), dict(lanes=1, flags=4, first_stream=far), "integrator 1 is out of scope"),
        (dict(integrator=3), dict(flags=1, first_stream=far), "integrator 3 is out of scope"),
        (dict(integrator=-1), dict(lanes=1), "integrator -1"),
        # 6. sq_sum with one lane
        (dict(lanes=1), dict(flags=4, first_stream=far), "sq_sum needs lanes >= 2"),
        (dict(lanes=1), dict(flags=1), "sq_sum needs lanes >= 2"),
        # 7. the flags
        (dict(flags=api.QUERY_REORDER), dict(first_stream=far), "PT_QUERY_REORDER"),
        (dict(flags=api.QUERY_REORDER | api.QUERY_STREAM_PAD), {}, "PT_QUERY_REORDER"),
        (dict(flags=4), dict(first_stream=far), "unknown flag bits 0x4"),
        (dict(flags=0x80000002), {}, "unknown flag bits 0x80000000"),
        # 8. the stream range, without PT_QUERY_STREAM_PAD
        (dict(first_stream=(1 << 31) - 4 * N + 1), {}, "pass 2^31"),
        (dict(first_stream=far), {}, "pass 2^31"),
        (dict(n=1 << 26, first_stream=(1 << 31) - (1 << 28) + 1), {}, "pass 2^31"),
    ]

    def args(a):
        return (a["scene"], a["n"], a["recs"], a["lanes"], a["spp_lane"], a["max_depth"], a["integrator"], a["use_mis"], a["seed"], a["first_stream"],
                a["out"], a["sq"], a["flags"])

    for change, also, msg in cases:
        for extra in ({}, also):
            a = dict(good, **extra)
            a.update(change)
            assert L.pt_query_irradiance(*args(a)) == -1, (change, extra)
            assert WALK + ": " in _err(api) and msg in _err(api), (change, extra, _err(api))
            assert L.pt_query_irradiance_device(*args(a), None) == -1, (change, extra)
            assert WALK + ": " in _err(api) and msg in _err(api), (change, extra, _err(api))
    # without sq_sum one lane is allowed: the next check answers
    a = dict(good, lanes=1, sq=None, flags=4)
    assert L.pt_query_irradiance(*args(a)) == -1 and "unknown flag bits 0x4" in _err(api)
    # n == 0: 0 with a NULL scene, whatever else is passed; nothing is looked at or written
    for z in ((None, 0, None, 0, 0, 0, 7, 0, 0, 0, None, None, 0xff), (s, 0, r, 4, 2, 8, 0, 1, 1, 0, o, q, api.QUERY_STREAM_PAD)):
        assert L.pt_query_irradiance(*z) == 0 and L.pt_query_irradiance_device(*z, None) == 0
    assert (out == 77).all() and (sq == 78).all() and not fake.any()
    sc = api.Scene.__new__(api.Scene)                          # no device scene: the checks fire before it is looked at
    sc.h = None
    with pytest.raises(api.PtError, match="pt_query_irradiance: null scene"):
        sc.query_irradiance(recs, 4, 2, 8)
    with pytest.raises(api.PtError, match="pt_query_irradiance: n 5 at 1073741824 lanes"):
        sc.query_irradiance(recs, 1 << 30, 2, 8)
    assert sc.query_irradiance(np.zeros((0, 8), np.float32), 4, 2, 8).shape == (0, 4)
    s0, q0 = sc.query_irradiance(np.zeros((0, 8), np.float32), 4, 2, 8, moments=True)
    assert s0.shape == (0, 4) and q0.shape == (0, 4)


def test_irradiance_rays_argument_checks_in_order(api):
    """pt_query_irradiance_rays_device has the checks of the list that its arguments can fail, in the same order."""
    L = api.lib()
    recs, out, _, fake = _buffers()
    off = np.zeros(N * 64, np.uint32)
    r, o, s, d = recs.ctypes.data, out.ctypes.data, fake.ctypes.data, off.ctypes.data
    good = dict(scene=s, n=N, recs=r, lanes=4, seed=1, first_stream=0, off=d, rays=o, flags=0)
    far = 0xffffffff
    cases = [
        (dict(n=-1), dict(scene=None, lanes=3, flags=4, first_stream=far), "n -1 at"),
        (dict(n=(1 << 26) + 1), dict(recs=None, flags=1), "n 67108865 at 4 lanes must be 0..268435456"),
        (dict(scene=None), dict(lanes=3, flags=4, first_stream=far), "null scene"),
        (dict(recs=None), dict(lanes=0, flags=4), "null records"),
        (dict(rays=None), dict(lanes=128, flags=1), "null output buffer"),
        (dict(lanes=0), dict(flags=4, first_stream=far), "lanes 0 must be a power of two in 1..64"),
        (dict(lanes=6), dict(flags=1), "lanes 6 must be"),
        (dict(lanes=128), {}, "lanes 128 must be"),
        (dict(flags=api.QUERY_REORDER), dict(first_stream=far), "PT_QUERY_REORDER"),
        (dict(flags=8), dict(first_stream=far), "unknown flag bits 0x8"),
        (dict(first_stream=(1 << 31) - 4 * N + 1), {}, "pass 2^31"),
        (dict(first_stream=far), {}, "pass 2^31"),
    ]
    for change, also, msg in cases:
        for extra in ({}, also):
            a = dict(good, **extra)
            a.update(change)
            got = L.pt_query_irradiance_rays_device(a["scene"], a["n"], a["recs"], a["lanes"], a["seed"], a["first_stream"], a["off"], a["rays"],
                                                    a["flags"], None)
            assert got == -1, (change, extra)
            assert RAYS + ": " in _err(api) and msg in _err(api), (change, extra, _err(api))
    assert L.pt_query_irradiance_rays_device(None, 0, None, 0, 0, 0, None, None, 0xff, None) == 0
    assert (out == 77).all() and not fake.any()


def test_record_builders(api):
    from cudapathtracer_amd import rays
    p = np.array([(0.5, -0.25, 1.5), (1.0, 2.0, 3.0)], np.float32)
    nrm = np.array([(0.0, 1.0, 0.0), (0.6, 0.0, 0.8)], np.float32)
    r = rays.irradiance_records(p, nrm, 7.5)
    assert r.shape == (2, 8) and r.dtype == np.float32
    assert np.array_equal(r[:, 0:3].view(np.uint32), p.view(np.uint32)) and np.array_equal(r[:, 4:7].view(np.uint32), nrm.view(np.uint32))
    assert (r[:, 3] == 7.5).all() and not r[:, 7].view(np.uint32).any()
    assert (rays.irradiance_records(p, nrm)[:, 3] == np.float32(999999.0)).all()
    assert np.array_equal(rays.irradiance_records(p, nrm, 7.5, device="cpu").numpy().view(np.uint32), r.view(np.uint32))
    with pytest.raises(ValueError):
        rays.irradiance_records(p, nrm[:1])
    surf = np.zeros(3, api.RAY_SURFACE_DTYPE)
    surf["px"], surf["py"], surf["pz"] = (1.0, 0.0, 4.0), (2.0, 0.0, 5.0), (3.0, 0.0, 6.0)
    surf["nx"], surf["ny"], surf["nz"] = (0.0, 0.0, 0.6), (1.0, 0.0, 0.0), (0.0, 0.0, 0.8)
    surf["uvx"], surf["uvy"] = 0.25, 0.75
    surf["material"], surf["light"] = (2, -1, 7), (-1, -1, 0)
    s = rays.records_from_surfaces(surf, 3.0)
    want = np.array([(1, 2, 3, 3, 0, 1, 0, 0), (0, 0, 0, 0, 0, 0, 1, 0), (4, 5, 6, 3, 0.6, 0, 0.8, 0)], np.float32)
    assert np.array_equal(s.view(np.uint32), want.view(np.uint32))
    import torch
    t = rays.records_from_surfaces(torch.from_numpy(surf.view(np.float32).reshape(3, 12).copy()), 3.0)
    assert np.array_equal(t.numpy().view(np.uint32), want.view(np.uint32))


def test_the_tree_on_a_hand_worked_example():
    """L = 4, values chosen so that the order of the sums shows: in f32, (2^24 + 1) + 1 is 2^24 + 2 with the pair (1 + 1) formed
    first, and 2^24 when the ones are added to 2^24 one after the other."""
    big = np.float32(2.0 ** 24)
    a = np.zeros((2, 4, 3), np.float32)
    a[0, :, 0] = (big, 0.0, 1.0, 1.0)              # (big + 0) + (1 + 1) = big + 2, exactly; left to right it stays big
    a[0, :, 1] = (1.0, big, 1.0, 0.0)              # (1 + big) + (1 + 0) = big + 1 -> big (ties to even)
    a[0, :, 2] = (0.5, 0.25, 0.125, 0.0625)
    a[1, :, 0] = (3.0, 0.0, 0.0, 4.0)
    s, q = IR.sums(a)
    assert s.shape == (2, 4) and q.shape == (2, 4) and s.dtype == np.float32
    assert s[0, 0] == big + np.float32(2.0) and ((big + np.float32(1.0)) + np.float32(1.0)) == big
    assert s[0, 1] == big
    assert s[0, 2] == np.float32(0.9375) and s[0, 3] == 0 and s[1, 0] == 7.0
    assert q[1, 0] == 25.0 and q[0, 3] == 4.0 and q[1, 3] == 4.0
    assert q[0, 2] == np.float32(0.25 + 0.0625 + 0.015625 + 0.00390625)
    assert q[0, 0] == np.float32(2.0 ** 48) + np.float32(2.0)       # (2^48 + 0) + (1 + 1): the 2 is lost only in the last sum
    assert q[0, 0] == np.float32(2.0 ** 48)
    one = IR.sums(a[:, :1])
    assert np.array_equal(one[0][:, :3], a[:, 0]) and (one[1][:, 3] == 1).all()
    assert np.array_equal(IR.tree(np.arange(8, dtype=np.float32).reshape(1, 8)), np.array([28.0], np.float32))
    li = [np.array([[big, 1.0, 0.0]], np.float32), np.array([[1.0, 1.0, 0.0]], np.float32), np.array([[1.0, 1.0, 2.0]], np.float32)]
    assert np.array_equal(IR.lane_sum(li), np.array([[big, 3.0, 2.0]], np.float32))        # ((0 + big) + 1) + 1 = big
    assert np.array_equal(IR.advance(np.array([0, 2, 4], np.uint32), [True, False, True]), np.array([4, 4, 8], np.uint32))


def test_fma32_is_the_exactly_rounded_fma():
    rng = np.random.default_rng(11)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1.0 + rng.standard_normal(4000) * 1e-7)).astype(np.float32)   # near cancellation
    c[::3] = rng.standard_normal(len(c[::3])).astype(np.float32)
    # halfway cases of the f32 rounding that a double rounding gets wrong: a * b = 1 + 2^-24 exactly, c tiny
    a[:2], b[:2] = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 - 2.0 ** -12 + 2.0 ** -23)
    c[:2] = (np.float32(2.0 ** -60), np.float32(-2.0 ** -60))
    got = IR.fma32(a, b, c)

    def exact(x, y, z):
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        if v == 0:
            return np.float32(0.0)
        # round the rational to f32, to nearest even, through its two f32 neighbours
        f = np.float32(float(v))
        lo, hi = (np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf)))
        best = min((lo, f, hi), key=lambda t: (abs(Fraction(float(t)) - v), int(np.float32(t).view(np.uint32)) & 1))
        return np.float32(best)

    want = np.array([exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# DESIGN.md §26's table: kernel -> (VGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes per workgroup, waves per SIMD it is launched at)
TABLE = {
    "irradiance_naive_simple": (80, 16, 3, 16384, 6), "irradiance_naive_lean": (95, 20, 6, 20480, 5), "irradiance_naive_generic": (100, 0, 0, 20480, 4),
    "irradiance_mis_simple": (80, 40, 11, 16384, 6), "irradiance_mis_lean": (96, 100, 40, 20480, 5), "irradiance_mis_generic": (128, 8, 1, 20480, 4),
}


def test_each_irradiance_kernel_fits_the_waves_it_declares():
    """What the compile gives, pinned as tests/test_radiance_api.py pins radiance_kernel's: each of the six kernels fits the waves per
    SIMD it is launched at (radiance_kernel's of the same class) in VGPRs and LDS, its LDS is radiance_kernel's (the tree uses none),
    and scratch and spills are §26's table."""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import irradiance_time
    import radiance_time
    res, waves = irradiance_time.irradiance_kernel_resources(), irradiance_time.declared_waves()
    print(res, waves)
    assert set(res) == set(TABLE) == set(waves)
    rad = radiance_time.declared_waves()
    for k, (vgprs, scratch, spills, lds, w) in TABLE.items():
        r = res[k]
        assert waves[k] == w == rad[k.replace("irradiance", "radiance")], (k, waves[k])
        assert r["vgpr_count"] == vgprs and r["private_segment_fixed_size"] == scratch and r["vgpr_spill_count"] == spills, (k, r)
        assert r["group_segment_fixed_size"] == lds, (k, r)
        fit = min(512 // ((r["vgpr_count"] + 7) // 8 * 8), (160 * 1024) // r["group_segment_fixed_size"], 8)
        assert fit >= w, (k, r, fit)
