"""The responsive history without a GPU: every new symbol of the C ABI and of the Python wrapper, the argument checks of
pt_temporal_accumulate_respond and pt_preview_set_respond (they fire before any HIP call), the workspace size, the defaults against
the pick of tests/respond_seq.py's sweep, and the two kernels' resources read from the code-object notes."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

NEW_SYMBOLS = ("pt_respond_defaults", "pt_temporal_respond_workspace_bytes", "pt_temporal_accumulate_respond",
               "pt_temporal_accumulate_respond_device", "pt_preview_set_respond", "pt_preview_respond")
W, H = 16, 8
PICK = {"radius": 3, "power": 4, "threshold": 2.0}           # the sweep's pick


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
    assert "typedef struct pt_respond_params" in header
    assert all(hasattr(api, n) for n in ("RespondParams", "respond_defaults", "temporal_respond_workspace_bytes", "temporal_accumulate_respond",
                                         "temporal_accumulate_respond_device"))
    assert all(hasattr(api.Preview, n) for n in ("set_respond", "respond"))
    assert ctypes.sizeof(api.RespondParams) == 12
    assert "respond" in api.TemporalHistory.__init__.__code__.co_varnames


def test_defaults_are_the_sweeps_pick_and_the_workspace_is_36_bytes_a_pixel(api):
    import respond_ref as R
    assert api.respond_defaults() == PICK == R.DEFAULTS
    assert api.temporal_respond_workspace_bytes(W, H) == 36 * W * H
    assert api.temporal_respond_workspace_bytes(1920, 1080) == 36 * 1920 * 1080
    assert api.temporal_respond_workspace_bytes(37, 21) == 36 * 37 * 21
    assert api.temporal_respond_workspace_bytes(0, 8) == 0 and api.temporal_respond_workspace_bytes(8, -1) == 0
    api.lib().pt_respond_defaults(None)                      # (a NULL out is ignored)


def test_accumulate_respond_argument_checks(api):
    """The base functions' checks, the new parameters' ranges, exactly one frame form, and a workspace and an out_scale that stay
    clear of every other buffer; all before any HIP call, host and device form alike."""
    L = api.lib()
    n = W * H
    f4 = np.zeros((10, H, W, 4), np.float32)
    S, Q, A, N, PN, Hs, Mv, O, cur, spare = (f4[i].ctypes.data for i in range(10))
    ln = np.zeros((3, H, W), np.float32)
    HL, OL, SC = (ln[i].ctypes.data for i in range(3))
    ws = np.zeros(36 * n + 64, np.uint8)
    WS = ws.ctypes.data
    c = ctypes.byref(_cam(api))

    def rp(radius=2, power=2, threshold=3.0):
        return ctypes.byref(api.RespondParams(radius, power, threshold))

    def tp(max_history=32, depth_tol=0.1, normal_tol=0.9):
        return ctypes.byref(api.TemporalParams(max_history, depth_tol, normal_tol))

    def call(s=S, q=Q, a=A, e=None, spp=4, batches=2, cam=c, nd=N, hist=(PN, Hs, HL), motion=Mv, t=None, r=None, w=W, h=H, work=WS, out=O,
             out_len=OL, scale=SC):
        head = (w, h, cam, None, s, q, spp, batches, a, e, nd) + tuple(hist) + (motion, t, r)
        return head + (out, out_len, scale), head + (work, out, out_len, scale, None)

    cases = [
        # the frame forms
        (call(e=cur), "exactly one frame form"), (call(s=None, q=None, a=None), "exactly one frame form"),
        (call(s=None, q=None, e=cur), "exactly one frame form"), (call(s=None, e=None), "null buffer"), (call(a=None), "null buffer"),
        # the base function's
        (call(w=0), "size"), (call(cam=None), "null camera"), (call(cam=ctypes.byref(_cam(api, 17, 8))), "camera is 17 x 8"),
        (call(spp=3), "must divide"), (call(batches=1), "at least 2"), (call(spp=0), "must be positive"), (call(nd=None), "null buffer"),
        (call(hist=(PN, None, HL)), "all NULL"), (call(out=None), "null output"), (call(out_len=None), "null output"),
        (call(out=Hs), "alias the input history"), (call(out_len=HL), "alias the input history"), (call(out=Mv), "alias the motion"),
        (call(t=tp(max_history=0)), "max_history"), (call(t=tp(depth_tol=-1.0)), "depth_tol"), (call(t=tp(normal_tol=1.5)), "normal_tol"),
        # the new parameters
        (call(r=rp(radius=0)), "radius 0 must be 1..3"), (call(r=rp(radius=4)), "radius 4 must be 1..3"),
        (call(r=rp(power=3)), "power 3 must be 1, 2 or 4"), (call(r=rp(power=0)), "power 0"), (call(r=rp(power=8)), "power 8"),
        (call(r=rp(threshold=0.0)), "threshold must be positive"), (call(r=rp(threshold=-2.0)), "threshold must be positive"),
        (call(r=rp(threshold=math.nan)), "threshold must be positive"),
        # out_scale against the other buffers
        (call(scale=S), "out_scale must not alias"), (call(scale=Hs + 16 * (n - 1)), "out_scale must not alias"), (call(scale=OL), "out_scale must not alias"),
        (call(scale=O + 16), "out_scale must not alias"), (call(scale=N), "out_scale must not alias"), (call(scale=Mv), "out_scale must not alias"),
        (call(s=None, q=None, a=None, e=cur, scale=cur), "out_scale must not alias"),
    ]
    for (host, dev), msg in cases:
        assert L.pt_temporal_accumulate_respond(*host) == -1, (host, msg)
        assert msg in _err(api), (msg, _err(api))
        assert L.pt_temporal_accumulate_respond_device(*dev) == -1, (dev, msg)
        assert msg in _err(api), (msg, _err(api))
    # the workspace: the device form's alone
    dev_cases = [
        (call(work=None), "null workspace"), (call(work=S), "workspace must not alias"), (call(work=O), "workspace must not alias"),
        (call(work=Hs - 36 * n + 4), "workspace must not alias"), (call(work=HL), "workspace must not alias"),
        (call(work=OL), "workspace must not alias"), (call(work=Mv), "workspace must not alias"), (call(work=N), "workspace must not alias"),
        (call(scale=WS + 36 * n - 4), "workspace must not alias"), (call(s=None, q=None, a=None, e=cur, work=cur), "workspace must not alias"),
    ]
    for (_, dev), msg in dev_cases:
        assert L.pt_temporal_accumulate_respond_device(*dev) == -1, (dev, msg)
        assert msg in _err(api), (msg, _err(api))
    # the wrapper reaches the same checks, and makes its own on the shapes
    cam = _cam(api)
    z = f4[0]
    with pytest.raises(api.PtError, match="exactly one frame form"):
        api.temporal_accumulate_respond(cam, z, z, z, 4, 2, z, cur=z)
    with pytest.raises(api.PtError, match="radius 7"):
        api.temporal_accumulate_respond(cam, z, z, z, 4, 2, z, radius=7)
    with pytest.raises(api.PtError, match="shapes differ"):
        api.temporal_accumulate_respond(cam, z, cur=z, motion=np.zeros((H, W + 1, 4), np.float32))
    with pytest.raises(api.PtError, match="all None or all given"):
        api.temporal_accumulate_respond(cam, z, cur=z, hist=z)


def test_the_preview_option_refuses_null_and_bad_parameters(api):
    L = api.lib()
    good = api.RespondParams(2, 2, 3.0)
    assert L.pt_preview_set_respond(None, ctypes.byref(good)) == -1 and "pt_preview_set_respond: null session" in _err(api)
    assert L.pt_preview_set_respond(None, None) == -1 and "pt_preview_set_respond: null session" in _err(api)
    assert L.pt_preview_respond(None, None) == -1 and "pt_preview_respond: null session" in _err(api)
    assert L.pt_preview_respond(None, ctypes.byref(good)) == -1


def test_the_two_kernels_resources():
    """From the compile: no scratch and no spills; the gather at the base kernel's register budget (8 waves per SIMD
    need at most 64 VGPRs); the walk's LDS is the two staged float4 arrays of 22 rows of 24 entries, 16896 bytes, of which 9
    workgroups fit a CU's 160 KB: more than its 8 waves per SIMD can use."""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import respond_time
    res = respond_time.respond_kernel_resources()
    print(res)
    gather = {k: v for k, v in res.items() if "temporal_gather_kernel" in k}
    walk = {k: v for k, v in res.items() if "temporal_respond_kernel" in k}
    assert len(gather) == 8 and len(walk) == 2, sorted(res)
    for k, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (k, r)
        assert r["vgpr_count"] <= 64, (k, r)
    for k, r in gather.items():
        assert r["group_segment_fixed_size"] == 0, (k, r)
    for k, r in walk.items():
        assert r["group_segment_fixed_size"] == 2 * 22 * 24 * 16 == 16896, (k, r)
        assert r["vgpr_count"] <= respond_time.WALK_VGPRS, (k, r)
    assert max(r["vgpr_count"] for r in gather.values()) <= respond_time.GATHER_VGPRS, gather
