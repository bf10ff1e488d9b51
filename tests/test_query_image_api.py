"""Denoisable ray queries without a GPU: the four new symbols of the C ABI and the Python wrapper's two methods, every argument check
of pt_query_radiance_moments and pt_query_guides (they fire before any HIP call, under the function's own name, with a NULL scene
where the check precedes the scene's), n == 0, and the resources of the eight new kernels read from the code-object notes against
DESIGN.md §25's tables and the waves per SIMD each is launched at."""
import os
import sys

import numpy as np
import pytest

N = 5


def _err(api):
    return api.lib().pt_last_error().decode()


def test_new_symbols_are_declared_and_exported(api):
    from conftest import ROOT
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for n in ("pt_query_radiance_moments", "pt_query_radiance_moments_device", "pt_query_guides", "pt_query_guides_device"):
        assert hasattr(L, n), n
        assert "int " + n + "(" in header, n
    assert hasattr(api.Scene, "query_radiance_moments") and hasattr(api.Scene, "query_guides")
    assert L.pt_api_version() == 1


def test_radiance_moments_argument_checks(api):
    L = api.lib()
    rays = np.zeros((N, 8), np.float32)
    out = np.full((N, 4), 77.0, np.float32)
    sq = np.full((N, 4), 78.0, np.float32)
    fake = np.zeros(4096, np.uint8)                            # stands for a scene where a check before the scene's must fire
    r, o, q, s = rays.ctypes.data, out.ctypes.data, sq.ctypes.data, fake.ctypes.data
    good = dict(scene=s, n=N, rays=r, spp=4, batch_spp=2, max_depth=8, integrator=0, use_mis=1, seed=1, first_stream=0, out=o, sq=q, flags=0)
    cases = [
        # pt_query_radiance's, in its order
        (dict(n=-1, scene=None), "n -1 must be 0..268435456"), (dict(n=(1 << 28) + 1, scene=None), "n 268435457 must be 0..268435456"),
        (dict(scene=None), "null scene"), (dict(rays=None), "null rays"), (dict(out=None), "null output buffer"),
        (dict(spp=0), "spp 0 must be 1..4194304"), (dict(spp=(1 << 22) + 1), "spp 4194305 must be 1..4194304"),
        (dict(integrator=1), "integrator 1 is out of scope"), (dict(integrator=3), "integrator 3 is out of scope"),
        (dict(flags=api.QUERY_REORDER), "PT_QUERY_REORDER"), (dict(flags=api.QUERY_REORDER | api.QUERY_STREAM_PAD), "PT_QUERY_REORDER"),
        (dict(flags=4), "unknown flag bits 0x4"),
        (dict(first_stream=(1 << 31) - N + 1), "pass 2^31"),
        # an earlier check wins over a later one
        (dict(scene=None, batch_spp=0, sq=None), "null scene"), (dict(spp=0, batch_spp=0), "spp 0 must be"),
        # its own
        (dict(batch_spp=0), "batch_spp 0 must be positive"), (dict(batch_spp=-2), "batch_spp -2 must be positive"),
        (dict(spp=7, batch_spp=2), "spp 7 is not a multiple of batch_spp 2"), (dict(spp=4, batch_spp=3), "spp 4 is not a multiple of batch_spp 3"),
        (dict(spp=4, batch_spp=4), "1 batch(es)"), (dict(spp=1, batch_spp=1), "1 batch(es)"),
        (dict(sq=None), "null sq_sum buffer"), (dict(spp=4, batch_spp=4, sq=None), "1 batch(es)"),
    ]
    for change, msg in cases:
        a = dict(good, **change)
        args = (a["scene"], a["n"], a["rays"], a["spp"], a["batch_spp"], a["max_depth"], a["integrator"], a["use_mis"], a["seed"], a["first_stream"],
                a["out"], a["sq"], a["flags"])
        for fn, more in ((L.pt_query_radiance_moments, ()), (L.pt_query_radiance_moments_device, (None,))):
            assert fn(*args, *more) == -1, change
            assert "pt_query_radiance_moments: " in _err(api) and msg in _err(api), (change, _err(api))
    # n == 0: 0 with a NULL scene, whatever else is passed; nothing is looked at or written
    for args in ((None, 0, None, 0, 0, 0, 7, 0, 0, 0, None, None, 0xff), (s, 0, r, 4, 2, 8, 0, 1, 1, 0, o, q, api.QUERY_STREAM_PAD)):
        assert L.pt_query_radiance_moments(*args) == 0 and L.pt_query_radiance_moments_device(*args, None) == 0
    assert (out == 77).all() and (sq == 78).all() and not fake.any()
    sc = api.Scene.__new__(api.Scene)                          # no device scene: the checks fire before it is looked at
    sc.h = None
    with pytest.raises(api.PtError, match="pt_query_radiance_moments: null scene"):
        sc.query_radiance_moments(rays, 4, 2, 8)
    S, Q = sc.query_radiance_moments(np.zeros((0, 8), np.float32), 4, 2, 8)
    assert S.shape == (0, 4) and Q.shape == (0, 4)


def test_guides_argument_checks(api):
    L = api.lib()
    rays = np.zeros((N, 8), np.float32)
    alb = np.full((N, 4), 77.0, np.float32)
    nd = np.full((N, 4), 78.0, np.float32)
    ln = np.full(N, 79.0, np.float32)
    fake = np.zeros(4096, np.uint8)
    r, pa, pn, pl, s = rays.ctypes.data, alb.ctypes.data, nd.ctypes.data, ln.ctypes.data, fake.ctypes.data
    good = dict(scene=s, n=N, rays=r, max_links=4, alb=pa, nd=pn, ln=pl, flags=0)
    cases = [
        (dict(n=-1, scene=None), "n -1 must be 0..268435456"), (dict(n=(1 << 28) + 1, scene=None), "n 268435457 must be 0..268435456"),
        (dict(scene=None), "null scene"), (dict(rays=None), "null rays"), (dict(alb=None), "null output buffer"), (dict(nd=None), "null output buffer"),
        (dict(max_links=-1), "max_links -1 must be 0..16"), (dict(max_links=17), "max_links 17 must be 0..16"),
        (dict(flags=1), "flags 0x1"), (dict(flags=api.QUERY_STREAM_PAD), "flags 0x2"), (dict(flags=0x80000000), "flags 0x80000000"),
        (dict(scene=None, max_links=17, flags=1), "null scene"),
        (dict(n=0, max_links=17), "max_links 17"), (dict(n=0, flags=1), "flags 0x1"),       # n == 0 does not pass a bad argument
    ]
    for change, msg in cases:
        a = dict(good, **change)
        args = (a["scene"], a["n"], a["rays"], a["max_links"], a["alb"], a["nd"], a["ln"], a["flags"])
        for fn, more in ((L.pt_query_guides, ()), (L.pt_query_guides_device, (None,))):
            assert fn(*args, *more) == -1, change
            assert "pt_query_guides: " in _err(api) and msg in _err(api), (change, _err(api))
    # n == 0: 0, with and without a links buffer; nothing of the scene is looked at, nothing written
    for links in (pl, None):
        for m in (0, 4, 16):
            assert L.pt_query_guides(s, 0, r, m, pa, pn, links, 0) == 0 and L.pt_query_guides_device(s, 0, r, m, pa, pn, links, 0, None) == 0
    assert (alb == 77).all() and (nd == 78).all() and (ln == 79).all() and not fake.any()
    sc = api.Scene.__new__(api.Scene)
    sc.h = None
    with pytest.raises(api.PtError, match="pt_query_guides: null scene"):
        sc.query_guides(rays, 4)


# DESIGN.md §25's tables: kernel -> (VGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes per workgroup, waves per SIMD it is launched at)
MOMENTS_TABLE = {
    "radiance_moments_naive_simple": (80, 0, 0, 23552, 6), "radiance_moments_naive_lean": (95, 0, 0, 27648, 5),
    "radiance_moments_naive_generic": (97, 0, 0, 27648, 4), "radiance_moments_mis_simple": (80, 36, 10, 23552, 6),
    "radiance_moments_mis_lean": (96, 88, 33, 27648, 5), "radiance_moments_mis_generic": (128, 12, 2, 27648, 4),
}
GUIDES_TABLE = {"query_guides_kernel": (55, 0, 0, 16384, 8), "query_guides_chain_kernel": (60, 0, 0, 23552, 6)}
# DESIGN.md §24's scratch bytes per lane of the parent kernels (tests/test_radiance_api.py pins them)
PARENT_SCRATCH = {"naive_simple": 0, "naive_lean": 0, "naive_generic": 0, "mis_simple": 28, "mis_lean": 84, "mis_generic": 12}


def test_each_new_kernel_fits_the_waves_it_declares():
    """What the compile gives, pinned: each kernel needs at most 512 / waves VGPRs (in granules of 8) and waves x its LDS within the
    CU's 160 KB at the waves per SIMD pt_feature_host.h launches it at. The moments kernels run at their parent kernel's waves; four
    of the six have the parent's scratch, MIS SIMPLE and MIS LEAN 8 and 4 bytes a lane more (the register form had 36 and 28 more)."""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import query_image_time as T
    import radiance_time
    res = dict(T.radiance_moments_kernel_resources(), **T.guides_kernel_resources())
    waves = T.declared_waves()
    table = dict(MOMENTS_TABLE, **GUIDES_TABLE)
    print(res, waves)
    assert set(res) == set(table) == set(waves)
    for k, (vgprs, scratch, spills, lds, w) in table.items():
        r = res[k]
        assert waves[k] == w, (k, waves[k])
        assert r["vgpr_count"] == vgprs and r["private_segment_fixed_size"] == scratch and r["vgpr_spill_count"] == spills, (k, r)
        assert r["group_segment_fixed_size"] == lds, (k, r)
        fit = min(512 // ((r["vgpr_count"] + 7) // 8 * 8), (160 * 1024) // r["group_segment_fixed_size"], 8)
        assert fit >= w, (k, r, fit)
    parent = radiance_time.declared_waves()
    for k in MOMENTS_TABLE:
        short = k[len("radiance_moments_"):]
        assert waves[k] == parent["radiance_" + short], k
        assert res[k]["private_segment_fixed_size"] - PARENT_SCRATCH[short] == {"mis_simple": 8, "mis_lean": 4}.get(short, 0), k
