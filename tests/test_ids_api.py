"""Picking without a GPU: every new symbol of the C ABI and of the Python wrapper, the argument checks of pt_render_ids, pt_pick,
pt_select_overlay and the session's calls (they fire before any HIP call), pt_select_entry's layout against the header's, and the
resources of the two ID kernels next to the centre pass's, read from the code-object notes."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

NEW_SYMBOLS = ("pt_render_ids", "pt_render_ids_device", "pt_pick", "pt_select_overlay", "pt_select_overlay_device", "pt_preview_set_selection",
               "pt_preview_pick", "pt_preview_read_ids", "pt_preview_device_ids", "pt_preview_id_passes")
W, H = 16, 8


def _err(api):
    return api.lib().pt_last_error().decode()


def _cam(api, w=W, h=H):
    return api.make_camera(True, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 45.0, w, h)


def test_new_symbols_are_declared_and_exported(api):
    from conftest import ROOT
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert n + "(" in header, n
    assert "} pt_select_entry;" in header
    assert all(hasattr(api.Scene, n) for n in ("render_ids", "render_ids_device", "pick"))
    assert all(hasattr(api, n) for n in ("select_overlay", "select_overlay_device", "SelectEntry"))
    assert all(hasattr(api.Preview, n) for n in ("set_selection", "pick", "read_ids", "device_ids", "id_passes"))


def test_select_entry_layout_is_the_headers(api, tmp_path):
    from conftest import ROOT
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(pt_select_entry), offsetof(pt_select_entry, component), offsetof(pt_select_entry, lo), offsetof(pt_select_entry, hi), "
                   "offsetof(pt_select_entry, colour), offsetof(pt_select_entry, radius), offsetof(pt_select_entry, fill_alpha)); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    E = api.SelectEntry
    assert got == [ctypes.sizeof(E), E.component.offset, E.lo.offset, E.hi.offset, E.colour.offset, E.radius.offset, E.fill_alpha.offset], got
    assert got[0] == 24


def test_render_ids_argument_checks(api):
    L = api.lib()
    ids = np.zeros((H, W, 4), np.int32)
    o = ids.ctypes.data
    c = ctypes.byref(_cam(api))
    cases = [
        ((None, c, W, H, -1, o), "max_links -1 must be 0..16"), ((None, c, W, H, 17, o), "max_links 17 must be 0..16"),
        ((None, c, 0, H, 0, o), "size"), ((None, c, W, -1, 0, o), "size"),
        ((None, None, W, H, 0, o), "null camera"),
        ((None, c, W, H + 1, 0, o), "camera is 16 x 8"), ((None, ctypes.byref(_cam(api, 17, 8)), W, H, 4, o), "camera is 17 x 8"),
        ((None, c, W, H, 0, None), "null ids output"),
        ((None, c, W, H, 0, o), "null scene"), ((None, c, W, H, 16, o), "null scene"),     # everything else in order
    ]
    for args, msg in cases:
        assert L.pt_render_ids(*args) == -1, args
        assert "pt_render_ids: " in _err(api) and msg in _err(api), (args, _err(api))
        assert L.pt_render_ids_device(*args, None) == -1, args
        assert "pt_render_ids: " in _err(api) and msg in _err(api), (args, _err(api))
    assert not ids.any()
    sc = api.Scene.__new__(api.Scene)                        # no device scene: the checks fire before it is looked at
    sc.h = None
    with pytest.raises(api.PtError, match="pt_render_ids: null scene"):
        sc.render_ids(_cam(api), W, H, 4)
    with pytest.raises(api.PtError, match="null ids output"):
        sc.render_ids_device(_cam(api), W, H, 0, 0)


def test_pick_argument_checks(api):
    L = api.lib()
    xy = np.array([(0, 0), (W - 1, H - 1), (3, 4)], np.int32)
    ids, hit = np.full((3, 4), 77, np.int32), np.full((3, 4), 77.0, np.float32)
    q, oi, oh = xy.ctypes.data, ids.ctypes.data, hit.ctypes.data
    c = ctypes.byref(_cam(api))

    def bad(x, y):
        b = xy.copy(); b[1] = (x, y)
        return b

    outside = [bad(-1, 0), bad(W, 0), bad(0, -1), bad(0, H), bad(2 ** 31 - 1, 0)]
    cases = [
        ((None, c, W, H, 0, q, 0, oi, oh), "n 0 must be positive"), ((None, c, W, H, -2, q, 0, oi, oh), "n -2 must be positive"),
        ((None, c, W, H, 3, None, 0, oi, oh), "null pixel list"), ((None, c, W, H, 3, q, 0, oi, None), "null hit output"),
        ((None, c, W, H, 3, q, 0, None, oh), "null ids output"),
        ((None, c, W, H, 3, q, 17, oi, oh), "max_links 17 must be 0..16"), ((None, c, W, 0, 3, q, 0, oi, oh), "size"),
        ((None, None, W, H, 3, q, 0, oi, oh), "null camera"), ((None, c, W + 1, H, 3, q, 0, oi, oh), "camera is 16 x 8"),
        ((None, c, W, H, 3, q, 4, oi, oh), "null scene"),
    ]
    cases += [((None, c, W, H, 3, b.ctypes.data, 0, oi, oh), "pixel 1 is (%d, %d), outside the 16 x 8 image" % tuple(b[1])) for b in outside]
    for args, msg in cases:
        assert L.pt_pick(*args) == -1, args
        assert "pt_pick: " in _err(api) and msg in _err(api), (args, _err(api))
    assert (ids == 77).all() and (hit == 77.0).all()         # nothing was written
    sc = api.Scene.__new__(api.Scene)
    sc.h = None
    with pytest.raises(api.PtError, match="outside the 16 x 8 image"):
        sc.pick(_cam(api), W, H, [(0, 0), (16, 0)])


def test_select_overlay_argument_checks(api):
    L = api.lib()
    ids = np.zeros((H, W, 4), np.int32)
    rgba = np.full((H, W, 4), 9, np.uint8)
    i, o = ids.ctypes.data, rgba.ctypes.data
    E = api.SelectEntry
    col = (ctypes.c_uint8 * 4)(1, 2, 3, 4)

    def ent(*over, n=1):
        arr = (E * 4)()
        for k in range(4):
            arr[k] = E(0, 0, 5, col, 1, 0)
        for k, field, v in over:
            setattr(arr[k], field, v)
        return arr

    ok = ent()
    cases = [
        ((0, H, i, 1, ok, o), "size"), ((W, -3, i, 1, ok, o), "size"),
        ((W, H, None, 1, ok, o), "null ids buffer"), ((W, H, i, 1, ok, None), "null rgba8 buffer"), ((W, H, None, 0, None, o), "null ids buffer"),
        ((W, H, i, -1, ok, o), "n -1 must be 0..4"), ((W, H, i, 5, ok, o), "n 5 must be 0..4"), ((W, H, i, 2, None, o), "null entries"),
        ((W, H, i, 1, ent((0, "component", 3)), o), "entry 0: component 3"), ((W, H, i, 2, ent((1, "component", -1)), o), "entry 1: component -1"),
        ((W, H, i, 1, ent((0, "lo", -1)), o), "entry 0: range [-1, 5]"), ((W, H, i, 4, ent((3, "hi", -2)), o), "entry 3: range [0, -2]"),
        ((W, H, i, 1, ent((0, "lo", 6)), o), "entry 0: range [6, 5]"),
        ((W, H, i, 1, ent((0, "radius", 0)), o), "entry 0: radius 0 must be 1..4"), ((W, H, i, 3, ent((2, "radius", 5)), o), "entry 2: radius 5 must be 1..4"),
        ((W, H, i, 1, ent((0, "fill_alpha", 256)), o), "fill_alpha 256 must be 0..255"), ((W, H, i, 1, ent((0, "fill_alpha", -1)), o), "fill_alpha -1"),
        ((W, H, i, 1, ok, i), "must not overlap"), ((W, H, i, 1, ok, i + 16 * W * H - 1), "must not overlap"), ((W, H, o + 4 * W * H - 1, 1, ok, o), "must not overlap"),
    ]
    for args, msg in cases:
        assert L.pt_select_overlay(*args) == -1, args
        assert "pt_select_overlay: " in _err(api) and msg in _err(api), (args, _err(api))
        assert L.pt_select_overlay_device(*args, None) == -1, args
        assert "pt_select_overlay: " in _err(api) and msg in _err(api), (args, _err(api))
    assert (rgba == 9).all()
    # an entry beyond n is not looked at, and n = 0 takes no entries and writes nothing: both succeed without a device
    assert L.pt_select_overlay(W, H, i, 0, None, o) == 0 and L.pt_select_overlay_device(W, H, i, 0, ent((0, "radius", 9)), o, None) == 0
    assert (rgba == 9).all()
    assert np.array_equal(api.select_overlay(ids, rgba, []), rgba)
    with pytest.raises(api.PtError, match="int32"):
        api.select_overlay(ids.astype(np.int64), rgba, [])
    with pytest.raises(api.PtError, match="ids' shape"):
        api.select_overlay(ids, rgba[:, :-1], [])
    with pytest.raises(api.PtError, match="radius 7 must be 1..4"):
        api.select_overlay(ids, rgba, [("tri", 0, 3, (1, 2, 3, 4), 7, 0)])


def test_the_sessions_calls_refuse_null(api):
    L = api.lib()
    E = api.SelectEntry
    e = (E * 1)(E(1, 0, 0, (ctypes.c_uint8 * 4)(255, 128, 0, 255), 2, 64))
    out4, hit4 = np.zeros(4, np.int32), np.zeros(4, np.float32)
    assert L.pt_preview_set_selection(None, 1, e, 0) == -1 and "pt_preview_set_selection: null session" in _err(api)
    assert L.pt_preview_set_selection(None, 0, None, 0) == -1 and "pt_preview_set_selection: null session" in _err(api)
    assert L.pt_preview_pick(None, 0, 0, 0, out4.ctypes.data, hit4.ctypes.data) == -1 and "pt_preview_pick: null session" in _err(api)
    assert L.pt_preview_read_ids(None, out4.ctypes.data) == -1 and "pt_preview_read_ids: null session" in _err(api)
    assert L.pt_preview_device_ids(None) is None
    assert L.pt_preview_id_passes(None) == -1 and "pt_preview_id_passes: null session" in _err(api)


def test_the_id_kernels_fit_where_the_centre_kernels_fit():
    """ids_kernel is launched 8 workgroups per CU, as aov_centre_kernel: at most its VGPRs and at most 64, 8 x its LDS within 160 KB.
    ids_chain_kernel is launched 6 per CU, as aov_centre_chain_kernel: at most 80 VGPRs (512 / 6, in allocation units of 8) and
    6 x its LDS within 160 KB. Neither has scratch or spills. LDS: the four waves' stacks (16 384 B); the chain kernel adds IdsChain's
    two words per lane (2 048 B: 18 432 B) — follow_chain's seven-word record is written but never read there, and the compiler drops
    it; were it kept, 25 600 B would still fit six times."""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import denoise_time
    import pick_time
    r = pick_time.ids_kernel_resources()
    c = denoise_time.aov_kernel_resources()
    print(r, {k: c[k] for k in ("aov_centre_kernel", "aov_centre_chain_kernel")})
    for k in ("ids_kernel", "ids_chain_kernel"):
        assert r[k]["private_segment_fixed_size"] == 0 and r[k]["vgpr_spill_count"] == 0 and r[k]["sgpr_spill_count"] == 0, r[k]
    m, cc = r["ids_kernel"], c["aov_centre_kernel"]
    assert m["vgpr_count"] <= cc["vgpr_count"] and m["vgpr_count"] <= 64, (m, cc)
    assert m["group_segment_fixed_size"] == 16384 and 8 * m["group_segment_fixed_size"] <= 160 * 1024
    m, cc = r["ids_chain_kernel"], c["aov_centre_chain_kernel"]
    waves = lambda k, per_cu_cap: min(512 // ((k["vgpr_count"] + 7) // 8 * 8), (160 * 1024) // k["group_segment_fixed_size"], per_cu_cap)
    assert waves(cc, 8) == 6, cc
    assert waves(m, 8) >= waves(cc, 8), (m, cc)
    assert m["group_segment_fixed_size"] == 18432, m
    src = open(os.path.join(ROOT, "cudapathtracer_amd", "csrc", "pt_feature_host.h")).read()
    assert "kIdsWavesPerSimd = 8;" in src and "kIdsChainWavesPerSimd = 6;" in src
