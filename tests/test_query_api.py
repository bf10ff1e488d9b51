"""Ray queries without a GPU: the new symbols of the C ABI and of the Python wrapper, the three record layouts against the header's,
the argument checks of the pt_query_* calls (they fire before any HIP call; n == 0 returns 0 before the scene is looked at), and the
resources of the query kernels, read from the code-object notes."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

NEW_SYMBOLS = ("pt_query_closest", "pt_query_closest_device", "pt_query_shadow", "pt_query_shadow_device", "pt_query_camera_rays_device")
N = 5


def _err(api):
    return api.lib().pt_last_error().decode()


def test_new_symbols_are_declared_and_exported(api):
    from conftest import ROOT
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert n + "(" in header, n
    for t in ("pt_ray", "pt_ray_hit", "pt_ray_surface"):
        assert "} %s;" % t in header, t
    assert "#define PT_QUERY_REORDER 1u" in header and api.QUERY_REORDER == 1
    assert all(hasattr(api.Scene, n) for n in ("query_closest", "query_shadow", "query_camera_rays", "trace_closest", "trace_shadow"))
    assert all(hasattr(api, n) for n in ("Ray", "RayHit", "RaySurface", "RAY_DTYPE", "RAY_HIT_DTYPE", "RAY_SURFACE_DTYPE", "query_camera_rays"))


def test_record_layouts_are_the_headers(api, tmp_path):
    from conftest import ROOT
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    fields = {"pt_ray": ("ox", "oy", "oz", "max_t", "dx", "dy", "dz", "pad"), "pt_ray_hit": ("t", "u", "v", "tri"),
              "pt_ray_surface": ("px", "py", "pz", "uvx", "nx", "ny", "nz", "uvy", "material", "light", "backface", "pad")}
    structs = {"pt_ray": (api.Ray, api.RAY_DTYPE, 32), "pt_ray_hit": (api.RayHit, api.RAY_HIT_DTYPE, 16),
               "pt_ray_surface": (api.RaySurface, api.RAY_SURFACE_DTYPE, 48)}
    body = "".join('printf("%%zu", sizeof(%s)); %s printf("\\n");\n' % (t, " ".join('printf(" %%zu", offsetof(%s, %s));' % (t, f) for f in fs))
                   for t, fs in fields.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void) {\n%sreturn 0; }\n' % body)
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    for (t, fs), line in zip(fields.items(), lines):
        got = [int(v) for v in line.split()]
        S, dt, size = structs[t]
        assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fs], (t, got)
        assert got == [dt.itemsize] + [dt.fields[f][1] for f in fs], (t, got)
        assert got[0] == size and got[1:] == list(range(0, size, 4)), (t, got)
    assert [f[0] for f in api.Ray._fields_] == list(fields["pt_ray"])


def test_query_argument_checks(api):
    L = api.lib()
    rays = np.zeros((N, 8), np.float32)
    hits, surf, thr = np.full((N, 4), 77.0, np.float32), np.full((N, 12), 77.0, np.float32), np.full((N, 4), 77.0, np.float32)
    fake = np.zeros(4096, np.uint8)                            # stands for a scene where a check before the scene's must fire
    r, o, sf, t, s = rays.ctypes.data, hits.ctypes.data, surf.ctypes.data, thr.ctypes.data, fake.ctypes.data
    closest = [
        ((None, N, r, o, sf, 0), "null scene"), ((None, 0, r, o, None, 0), "null scene"),
        ((s, N, None, o, sf, 0), "null rays"), ((s, N, r, None, sf, 0), "null output buffer"),
        ((s, -1, r, o, sf, 0), "n -1 must be 0..268435456"), ((s, (1 << 28) + 1, r, o, None, 0), "n 268435457 must be 0..268435456"),
        ((s, N, r, o, sf, 2), "unknown flag bits 0x2"), ((s, N, r, o, None, 0x80000001), "unknown flag bits 0x80000000"),
        ((s, 0, None, o, sf, 0), "null rays"), ((s, 0, r, o, sf, 4), "unknown flag bits 0x4"),      # n == 0 does not skip a check
    ]
    for args, msg in closest:
        assert L.pt_query_closest(*args) == -1, args
        assert "pt_query_closest: " in _err(api) and msg in _err(api), (args, _err(api))
        assert L.pt_query_closest_device(*args, None) == -1, args
        assert "pt_query_closest: " in _err(api) and msg in _err(api), (args, _err(api))
    shadow = [
        ((None, N, r, t, 0), "null scene"), ((s, N, None, t, 0), "null rays"), ((s, N, r, None, 1), "null output buffer"),
        ((s, -7, r, t, 0), "n -7 must be 0..268435456"), ((s, (1 << 28) + 1, r, t, 1), "n 268435457"), ((s, N, r, t, 3), "unknown flag bits 0x2"),
    ]
    for args, msg in shadow:
        assert L.pt_query_shadow(*args) == -1, args
        assert "pt_query_shadow: " in _err(api) and msg in _err(api), (args, _err(api))
        assert L.pt_query_shadow_device(*args, None) == -1, args
        assert "pt_query_shadow: " in _err(api) and msg in _err(api), (args, _err(api))
    # n == 0: 0, nothing launched, the scene not looked at, with and without the flag
    for flags in (0, api.QUERY_REORDER):
        assert L.pt_query_closest(s, 0, r, o, sf, flags) == 0 and L.pt_query_closest_device(s, 0, r, o, None, flags, None) == 0
        assert L.pt_query_shadow(s, 0, r, t, flags) == 0 and L.pt_query_shadow_device(s, 0, r, t, flags, None) == 0
    assert (hits == 77).all() and (surf == 77).all() and (thr == 77).all() and not fake.any()
    sc = api.Scene.__new__(api.Scene)                        # no device scene: the checks fire before it is looked at
    sc.h = None
    with pytest.raises(api.PtError, match="pt_query_closest: null scene"):
        sc.query_closest(rays, surfaces=True)
    with pytest.raises(api.PtError, match="pt_query_shadow: null scene"):
        sc.query_shadow(rays, reorder=True)
    assert sc.query_closest(np.zeros((0, 8), np.float32)).shape == (0,) and sc.query_shadow(np.zeros((0, 8), np.float32)).shape == (0, 4)


def test_camera_rays_argument_checks(api):
    L = api.lib()
    cam = api.make_camera(True, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 45.0, 16, 8)
    c = ctypes.byref(cam)
    buf = np.full((16 * 8, 8), 77.0, np.float32)
    o = buf.ctypes.data
    cases = [
        ((None, 16, 8, 1.0, o), "null camera"), ((c, 0, 8, 1.0, o), "size"), ((c, 16, -1, 1.0, o), "size"),
        ((c, 1 << 15, 1 << 14, 1.0, o), "too large"), ((c, 16, 9, 1.0, o), "camera is 16 x 8"), ((c, 16, 8, 1.0, None), "null rays buffer"),
    ]
    for args, msg in cases:
        assert L.pt_query_camera_rays_device(*args, None) == -1, args
        assert "pt_query_camera_rays_device: " in _err(api) and msg in _err(api), (args, _err(api))
    assert (buf == 77).all()


def test_the_query_kernels_fit_eight_waves_per_simd():
    """What the compile gives, pinned: the three trace kernels are launched 8 workgroups of four waves per CU (8 waves per SIMD), as
    aov_centre_kernel and ids_kernel. That needs at most 64 VGPRs (512 / 8) and 8 x the LDS within 160 KB: the four waves' stacks,
    16 384 B. No kernel has scratch or spills. Hits only: 59 VGPRs; with surfaces: 55; shadow: 56."""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import denoise_time
    import query_time
    r = query_time.query_kernel_resources()
    c = denoise_time.aov_kernel_resources()["aov_centre_kernel"]
    print(r, c)
    assert set(r) == {"query_closest_kernel", "query_closest_surface_kernel", "query_shadow_kernel", "query_camera_rays_kernel", "query_keys_kernel"}
    for k, v in r.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
    waves = lambda k: min(512 // ((k["vgpr_count"] + 7) // 8 * 8), (160 * 1024) // k["group_segment_fixed_size"], 8)
    assert waves(c) == 8, c
    for k, vgprs in (("query_closest_kernel", 59), ("query_closest_surface_kernel", 55), ("query_shadow_kernel", 56)):
        assert r[k]["vgpr_count"] == vgprs and r[k]["vgpr_count"] <= 64, (k, r[k])
        assert r[k]["group_segment_fixed_size"] == 16384 and waves(r[k]) == 8, (k, r[k])
    assert r["query_closest_kernel"]["vgpr_count"] <= c["vgpr_count"], (r["query_closest_kernel"], c)
    for k in ("query_camera_rays_kernel", "query_keys_kernel"):
        assert r[k]["group_segment_fixed_size"] == 0 and r[k]["vgpr_count"] <= 32, (k, r[k])
    src = open(os.path.join(ROOT, "cudapathtracer_amd", "csrc", "pt_feature_host.h")).read()
    assert all(s in src for s in ("kQueryClosestWavesPerSimd = 8;", "kQuerySurfaceWavesPerSimd = 8;", "kQueryShadowWavesPerSimd = 8;"))
