"""Motion vectors without a GPU: every new symbol of the C ABI and of the Python wrapper, the argument checks of pt_render_motion,
pt_temporal_accumulate_motion, pt_temporal_accumulate_cur_motion, pt_scene_has_motion and pt_preview_set_motion (they fire before
any HIP call), and the resources of the motion kernel next to aov_centre_kernel's, read from the code-object notes."""
import ctypes
import os
import sys

import numpy as np
import pytest

NEW_SYMBOLS = ("pt_scene_has_motion", "pt_render_motion", "pt_render_motion_device", "pt_temporal_accumulate_motion",
               "pt_temporal_accumulate_motion_device", "pt_temporal_accumulate_cur_motion", "pt_temporal_accumulate_cur_motion_device",
               "pt_preview_set_motion", "pt_preview_motion")
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
    assert all(hasattr(api.Scene, n) for n in ("render_motion", "render_motion_device", "has_motion"))
    assert all(hasattr(api, n) for n in ("temporal_accumulate_motion", "temporal_accumulate_motion_device", "temporal_accumulate_cur_motion",
                                         "temporal_accumulate_cur_motion_device"))
    assert all(hasattr(api.Preview, n) for n in ("set_motion", "motion"))


def test_render_motion_argument_checks(api):
    L = api.lib()
    buf = np.zeros((3, H, W, 4), np.float32)
    a, n, m = (buf[i].ctypes.data for i in range(3))
    c = ctypes.byref(_cam(api))
    cases = [
        ((None, c, W, H, a, None, m), "both NULL or both set"),          # one guide output without the other
        ((None, c, W, H, None, n, m), "both NULL or both set"),
        ((None, c, W, H, a, n, None), "null motion output"),
        ((None, c, W, H, None, None, None), "null motion output"),
        ((None, c, 0, H, a, n, m), "size"),
        ((None, c, W, -1, None, None, m), "size"),
        ((None, None, W, H, a, n, m), "null camera"),
        ((None, c, W, H + 1, a, n, m), "camera is 16 x 8"),
        ((None, ctypes.byref(_cam(api, 17, 8)), W, H, None, None, m), "camera is 17 x 8"),
        # everything else in order, with and without guides: the scene is what is refused
        ((None, c, W, H, a, n, m), "null scene"),
        ((None, c, W, H, None, None, m), "null scene"),
    ]
    for args, msg in cases:
        assert L.pt_render_motion(*args) == -1, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_render_motion_device(*args, None) == -1, args
        assert msg in _err(api), (args, _err(api))
    sc = api.Scene.__new__(api.Scene)                        # no device scene: the checks fire before it is looked at
    sc.h = None
    with pytest.raises(api.PtError, match="null scene"):
        sc.render_motion(_cam(api), W, H, guides=True)
    with pytest.raises(api.PtError, match="both NULL or both set"):
        sc.render_motion_device(_cam(api), W, H, a, 0, m)


def test_has_motion_and_the_preview_setter_refuse_null(api):
    L = api.lib()
    assert L.pt_scene_has_motion(None) == -1 and "pt_scene_has_motion: null scene" in _err(api)
    for on in (0, 1):
        assert L.pt_preview_set_motion(None, on) == -1 and "pt_preview_set_motion: null session" in _err(api)
    for on in (2, -1):
        assert L.pt_preview_set_motion(None, on) == -1 and "pt_preview_set_motion: on %d must be 0 or 1" % on in _err(api)
    assert L.pt_preview_motion(None) == -1 and "pt_preview_motion: null session" in _err(api)


def test_accumulate_motion_argument_checks(api):
    """The base functions' checks, and an output that overlaps the motion buffer; all before any HIP call."""
    L = api.lib()
    n = W * H
    f4 = np.zeros((9, H, W, 4), np.float32)
    S, Q, A, N, PN, Hs, Mv, O, cur = (f4[i].ctypes.data for i in range(9))
    ln = np.zeros((2, H, W), np.float32)
    HL, OL = ln[0].ctypes.data, ln[1].ctypes.data
    c = ctypes.byref(_cam(api))

    def full(motion=Mv, out=O, out_len=OL, cam=c, spp=4, batches=2, hist=(PN, Hs, HL), s=S):
        return (W, H, cam, None, s, Q, spp, batches, A, N) + tuple(hist) + (motion, None, out, out_len)

    def curf(motion=Mv, out=O, out_len=OL, cam=c, hist=(PN, Hs, HL), e=cur):
        return (W, H, cam, None, e, N) + tuple(hist) + (motion, None, out, out_len)

    for fn, dev in ((L.pt_temporal_accumulate_motion, L.pt_temporal_accumulate_motion_device),):
        cases = [
            (full(out=Mv), "alias the motion"), (full(out=Mv + 16 * (n - 1)), "alias the motion"), (full(out_len=Mv + 16), "alias the motion"),
            (full(out=Hs), "alias"), (full(cam=None), "null camera"), (full(spp=3), "must divide"), (full(batches=1), "at least 2"),
            (full(hist=(PN, None, HL)), "all NULL"), (full(s=None), "null buffer"), (full(out=None), "null output"),
            (full(motion=None, out=None), "null output"),
        ]
        for args, msg in cases:
            assert fn(*args) == -1, args
            assert msg in _err(api), (args, _err(api))
            assert dev(*args, None) == -1, args
            assert msg in _err(api), (args, _err(api))
    cases = [
        (curf(out=Mv), "alias the motion"), (curf(out_len=Mv + 16 * n - 4), "alias the motion"), (curf(out=Hs), "alias"),
        (curf(cam=None), "null camera"), (curf(hist=(None, Hs, HL)), "all NULL"), (curf(e=None), "null buffer"), (curf(out_len=None), "null output"),
    ]
    for args, msg in cases:
        assert L.pt_temporal_accumulate_cur_motion(*args) == -1, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_temporal_accumulate_cur_motion_device(*args, None) == -1, args
        assert msg in _err(api), (args, _err(api))
    cam = _cam(api)
    z = f4[0]
    with pytest.raises(api.PtError, match="alias the motion"):
        # (the wrapper allocates its own outputs: the raw call shows the check)
        api._check(L.pt_temporal_accumulate_motion(*full(out=Mv)), "pt_temporal_accumulate_motion")
    with pytest.raises(api.PtError, match="shapes differ"):
        api.temporal_accumulate_motion(cam, z, z, 4, 2, z, z, None, z, z, ln[0], motion=np.zeros((H, W + 1, 4), np.float32))
    with pytest.raises(api.PtError, match="shapes differ"):
        api.temporal_accumulate_cur_motion(cam, z, z, None, z, z, ln[0], motion=np.zeros((H + 1, W, 4), np.float32))


def test_the_motion_kernel_needs_no_more_than_the_centre_pass():
    """motion_blocks launches 8 workgroups per CU, as aov_centre_blocks does: 8 waves per SIMD need at most 64 VGPRs, 8 workgroups at
    most 160 KB / 8 of LDS each; no scratch. The nine loads after the traversal add no register that is live across it."""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import denoise_time
    import motion_time
    m = motion_time.motion_kernel_resources()
    c = denoise_time.aov_kernel_resources()["aov_centre_kernel"]
    print(m, c)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["vgpr_count"] <= c["vgpr_count"] and m["vgpr_count"] <= 64, (m, c)
    assert m["group_segment_fixed_size"] <= c["group_segment_fixed_size"] and 8 * m["group_segment_fixed_size"] <= 160 * 1024, (m, c)
