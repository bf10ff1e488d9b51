"""Centre guides without a GPU: every new symbol of the C ABI and of the Python wrapper, the argument checks of
pt_render_aovs_centre, pt_guide_subsample, pt_probe_centre_rays and pt_preview_set_guide_centre (they fire before any HIP call),
and the resources of the two centre kernels next to their jittered counterparts, read from the same code-object notes."""
import ctypes
import os
import sys

import numpy as np
import pytest

NEW_SYMBOLS = ("pt_render_aovs_centre", "pt_render_aovs_centre_device", "pt_probe_centre_rays", "pt_guide_subsample",
               "pt_guide_subsample_device", "pt_preview_set_guide_centre", "pt_preview_guide_centre", "pt_preview_guide_passes")


def _err(api):
    return api.lib().pt_last_error().decode()


def _cam(api, w=16, h=8):
    return api.make_camera(True, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 45.0, w, h)


def test_new_symbols_are_declared_and_exported(api):
    from conftest import ROOT
    L = api.lib()
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert n + "(" in header, n
    assert all(hasattr(api.Scene, n) for n in ("render_aovs_centre", "render_aovs_centre_device"))
    assert all(hasattr(api, n) for n in ("guide_subsample", "guide_subsample_device", "probe_centre_rays"))
    assert all(hasattr(api.Preview, n) for n in ("set_guide_centre", "guide_centre", "guide_passes"))


def test_render_aovs_centre_argument_checks(api):
    L = api.lib()
    buf = np.zeros((8, 16, 4), np.float32)
    links = np.zeros((8, 16), np.float32)
    cam = _cam(api)
    c = ctypes.byref(cam)
    p, q = buf.ctypes.data, links.ctypes.data
    cases = [
        ((None, c, 0, 8, 4, p, p, q), "size"),
        ((None, c, 16, -1, 4, p, p, q), "size"),
        ((None, c, 16, 8, -1, p, p, q), "max_links -1 must be 0..16"),
        ((None, c, 16, 8, 17, p, p, q), "max_links 17 must be 0..16"),
        ((None, None, 16, 8, 4, p, p, q), "null camera"),
        ((None, c, 16, 9, 4, p, p, q), "camera is 16 x 8"),
        ((None, ctypes.byref(_cam(api, 17, 8)), 16, 8, 4, p, p, q), "camera is 17 x 8"),
        ((None, c, 16, 8, 4, None, p, q), "null output"),
        ((None, c, 16, 8, 4, p, None, q), "null output"),
        # everything else in order, links given or NULL: the scene is what is refused
        ((None, c, 16, 8, 0, p, p, q), "null scene"),
        ((None, c, 16, 8, 16, p, p, None), "null scene"),
    ]
    for args, msg in cases:
        assert L.pt_render_aovs_centre(*args) == -1, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_render_aovs_centre_device(*args, None) == -1, args
        assert msg in _err(api), (args, _err(api))


def test_probe_centre_rays_argument_checks(api):
    L = api.lib()
    xy = np.zeros(2, np.int32)
    out = np.zeros(6, np.float32)
    c = ctypes.byref(_cam(api))
    for args in ((None, 1, xy.ctypes.data, out.ctypes.data), (c, 0, xy.ctypes.data, out.ctypes.data), (c, 1, None, out.ctypes.data),
                 (c, 1, xy.ctypes.data, None)):
        assert L.pt_probe_centre_rays(*args) == -1, args
        assert "pt_probe_centre_rays" in _err(api)


def test_guide_subsample_argument_checks(api):
    L = api.lib()
    w, h = 24, 12
    full = np.zeros((2, h, w, 4), np.float32)
    lo = np.zeros((2, h // 2, w // 2, 4), np.float32)
    A, N, Al, Nl = full[0].ctypes.data, full[1].ctypes.data, lo[0].ctypes.data, lo[1].ctypes.data
    lo_bytes = (w // 2) * (h // 2) * 16
    cases = [
        ((0, h, 2, A, N, Al, Nl), "size"),
        ((w, -3, 2, A, N, Al, Nl), "size"),
        ((w, h, 1, A, N, Al, Nl), "scale 1 must be 2..8"),
        ((w, h, 9, A, N, Al, Nl), "scale 9 must be 2..8"),
        ((w, h, 5, A, N, Al, Nl), "scale 5 must divide the image size 24 x 12"),
        ((w, h, 8, A, N, Al, Nl), "scale 8 must divide"),
        ((w, h, 2, None, N, Al, Nl), "null buffer"),
        ((w, h, 2, A, None, Al, Nl), "null buffer"),
        ((w, h, 2, A, N, None, Nl), "null output"),
        ((w, h, 2, A, N, Al, None), "null output"),
        ((w, h, 2, A, N, A, Nl), "alias"),                             # an output on an input
        ((w, h, 2, A, N, Al, N + 16), "alias"),
        ((w, h, 2, A, N, Al, A + w * h * 16 - 16), "alias"),           # ... on its last pixel
        ((w, h, 2, A, N, Al, Al), "alias"),                            # the outputs on each other
        ((w, h, 2, A, N, Al, Al + lo_bytes - 16), "alias"),
    ]
    for args, msg in cases:
        assert L.pt_guide_subsample(*args) == -1, args
        assert "pt_guide_subsample" in _err(api) and msg in _err(api), (args, _err(api))
        assert L.pt_guide_subsample_device(*args, None) == -1, args
        assert msg in _err(api), (args, _err(api))
    with pytest.raises(api.PtError, match="scale 5 must divide"):
        api.guide_subsample(5, full[0], full[1])
    with pytest.raises(api.PtError, match="float32"):
        api.guide_subsample(2, full[0].astype(np.float64), full[1])


def test_guide_centre_setter_refuses_a_null_session(api):
    L = api.lib()
    for on in (0, 1):
        assert L.pt_preview_set_guide_centre(None, on) == -1 and "pt_preview_set_guide_centre: null session" in _err(api)
    for on in (2, -1):                                       # the value is checked first: no session is needed to see it refused
        assert L.pt_preview_set_guide_centre(None, on) == -1 and "pt_preview_set_guide_centre: on %d must be 0 or 1" % on in _err(api)
    assert L.pt_preview_guide_centre(None) == -1 and "pt_preview_guide_centre: null session" in _err(api)
    assert L.pt_preview_guide_passes(None) == -1 and "pt_preview_guide_passes: null session" in _err(api)


def test_python_wrapper_refuses_what_the_library_refuses(api):
    cam = _cam(api)
    sc = api.Scene.__new__(api.Scene)                        # no device scene: the checks fire before it is looked at
    sc.h = None
    with pytest.raises(api.PtError, match="max_links 17"):
        sc.render_aovs_centre(cam, 16, 8, 17)
    with pytest.raises(api.PtError, match="null scene"):
        sc.render_aovs_centre(cam, 16, 8, 4, links=True)


def test_the_centre_kernels_need_no_more_than_their_jittered_counterparts():
    """No scratch, and neither more VGPRs nor more LDS than aov_kernel / aov_chain_kernel: the launch shapes are theirs, and a
    centre pass is the same traversal without the seeding. aov_centre_blocks launches 8 workgroups per CU for the first-hit kernel:
    8 waves per SIMD need at most 64 VGPRs, 8 workgroups at most 160 KB / 8 of LDS each."""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import denoise_time
    res = denoise_time.aov_kernel_resources()
    print(res)
    for centre, jittered in (("aov_centre_kernel", "aov_kernel"), ("aov_centre_chain_kernel", "aov_chain_kernel")):
        c, j = res[centre], res[jittered]
        assert c["private_segment_fixed_size"] == 0 and c["vgpr_spill_count"] == 0, c
        assert c["vgpr_count"] <= j["vgpr_count"], (c, j)
        assert c["group_segment_fixed_size"] <= j["group_segment_fixed_size"], (c, j)
    first = res["aov_centre_kernel"]
    assert first["vgpr_count"] <= 64 and 8 * first["group_segment_fixed_size"] <= 160 * 1024, first
