"""Motion through mirrors and glass without a GPU: the new symbols of the C ABI and of the Python wrapper, the argument checks of
pt_render_motion_chain (they fire before a scene is looked at, each under the function's own name), the refusals of
pt_preview_set_motion_chain, and the resources of motion_chain_kernel next to aov_centre_chain_kernel's, read from the code-object
notes."""
import ctypes
import os
import sys

import numpy as np
import pytest

NEW_SYMBOLS = ("pt_render_motion_chain", "pt_render_motion_chain_device", "pt_preview_set_motion_chain", "pt_preview_motion_chain")
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
    assert all(hasattr(api.Scene, n) for n in ("render_motion_chain", "render_motion_chain_device"))
    assert all(hasattr(api.Preview, n) for n in ("set_motion_chain", "motion_chain"))


def test_render_motion_chain_argument_checks(api):
    L = api.lib()
    buf = np.zeros((4, H, W, 4), np.float32)
    a, n, l, m = (buf[i].ctypes.data for i in range(4))
    c = ctypes.byref(_cam(api))
    cases = [
        ((None, c, W, H, -1, a, n, l, m), "max_links -1 must be 0..16"),
        ((None, c, W, H, 17, None, None, None, m), "max_links 17 must be 0..16"),
        ((None, c, W, H, 2, a, None, None, m), "both NULL or both set"),      # one guide output without the other
        ((None, c, W, H, 2, None, n, None, m), "both NULL or both set"),
        ((None, c, W, H, 2, None, None, l, m), "links needs albedo and normal_depth"),
        ((None, c, W, H, 2, a, n, l, None), "null motion output"),
        ((None, c, W, H, 0, None, None, None, None), "null motion output"),
        ((None, c, 0, H, 2, a, n, l, m), "size"),
        ((None, c, W, -1, 2, None, None, None, m), "size"),
        ((None, c, 65536, 65536, 2, None, None, None, m), "too large"),
        ((None, None, W, H, 2, a, n, l, m), "null camera"),
        ((None, c, W, H + 1, 2, a, n, None, m), "camera is 16 x 8"),
        ((None, ctypes.byref(_cam(api, 17, 8)), W, H, 2, None, None, None, m), "camera is 17 x 8"),
        # everything else in order, with and without guides and links, at both ends of max_links: the scene is what is refused
        ((None, c, W, H, 0, a, n, l, m), "null scene"),
        ((None, c, W, H, 16, a, n, None, m), "null scene"),
        ((None, c, W, H, 2, None, None, None, m), "null scene"),
    ]
    for args, msg in cases:
        assert L.pt_render_motion_chain(*args) == -1, args
        assert msg in _err(api) and _err(api).startswith("pt_render_motion_chain: "), (args, _err(api))
        assert L.pt_render_motion_chain_device(*args, None) == -1, args
        assert msg in _err(api) and _err(api).startswith("pt_render_motion_chain: "), (args, _err(api))
    sc = api.Scene.__new__(api.Scene)                        # no device scene: the checks fire before it is looked at
    sc.h = None
    with pytest.raises(api.PtError, match="null scene"):
        sc.render_motion_chain(_cam(api), W, H, 2, guides=True, links=True)
    with pytest.raises(api.PtError, match="links needs"):
        sc.render_motion_chain(_cam(api), W, H, 2, links=True)
    with pytest.raises(api.PtError, match="both NULL or both set"):
        sc.render_motion_chain_device(_cam(api), W, H, 2, a, 0, 0, m)
    with pytest.raises(api.PtError, match="max_links 99"):
        sc.render_motion_chain_device(_cam(api), W, H, 99, 0, 0, 0, m)


def test_the_preview_setter_refuses_null_and_other_values(api):
    L = api.lib()
    for on in (0, 1):
        assert L.pt_preview_set_motion_chain(None, on) == -1 and "pt_preview_set_motion_chain: null session" in _err(api)
    for on in (2, -1):
        assert L.pt_preview_set_motion_chain(None, on) == -1 and "pt_preview_set_motion_chain: on %d must be 0 or 1" % on in _err(api)
    assert L.pt_preview_motion_chain(None) == -1 and "pt_preview_motion_chain: null session" in _err(api)
    # (pt_preview_set_motion keeps refusing 2: the chain is a switch of its own, not a third value)
    assert L.pt_preview_set_motion(None, 2) == -1 and "pt_preview_set_motion: on 2 must be 0 or 1" in _err(api)


def test_the_kernel_fits_the_waves_it_is_launched_with():
    """motion_chain_kernel keeps the unfolding matrix in registers: 93 VGPRs, 5 waves per SIMD (at most 96), which is what
    kMotionChainWavesPerSimd launches. No scratch. LDS: the four waves' stacks (16 384 B) and ten words per lane, follow_chain's
    seven and the centre ray's direction (10 240 B): 26 624 B, of which six workgroups fit a CU's 160 KB, so the registers decide.
    aov_centre_chain_kernel next to it stays at its 69 VGPRs and 23 552 B."""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import denoise_time
    import motion_time
    m = motion_time.motion_chain_kernel_resources()
    c = denoise_time.aov_kernel_resources()["aov_centre_chain_kernel"]
    print(m, c)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["vgpr_count"] <= 96, m                          # (93 from this compile; 5 waves per SIMD hold up to 96)
    assert m["group_segment_fixed_size"] == 4 * 64 * 4 * (16 + 10) == 26624 and 5 * m["group_segment_fixed_size"] <= 160 * 1024, m
    assert c["vgpr_count"] <= 80 and c["group_segment_fixed_size"] == 23552, c      # (69: 6 waves per SIMD, as before)
    src = open(os.path.join(ROOT, "cudapathtracer_amd", "csrc", "pt_feature_host.h")).read()
    assert "kMotionChainWavesPerSimd = 5;" in src
