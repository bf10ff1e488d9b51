"""Feature buffers and denoiser: the C ABI and the Python wrappers without a GPU (symbols, struct layout, defaults,
workspace size, argument checks that must fire before any HIP call)."""
import ctypes

import numpy as np
import pytest

NEW_SYMBOLS = ("pt_render_aovs", "pt_render_aovs_device", "pt_denoise_defaults", "pt_denoise_workspace_bytes", "pt_denoise",
               "pt_denoise_device")


def _err(api):
    return api.lib().pt_last_error().decode()


def _cam(api, w=16, h=8):
    return api.make_camera(True, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 45.0, w, h)


def test_new_symbols_are_exported(api):
    L = api.lib()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    assert L.pt_api_version() == 1


def test_denoise_params_layout_and_defaults(api):
    assert ctypes.sizeof(api.DenoiseParams) == 16
    assert [api.DenoiseParams.iterations.offset, api.DenoiseParams.sigma_color.offset, api.DenoiseParams.sigma_normal.offset,
            api.DenoiseParams.sigma_depth.offset] == [0, 4, 8, 12]
    buf = (ctypes.c_uint8 * 32)(*([0xAB] * 32))           # the C side writes exactly 16 bytes
    api.lib().pt_denoise_defaults(ctypes.cast(buf, ctypes.POINTER(api.DenoiseParams)))
    assert bytes(buf[16:]) == b"\xab" * 16
    p = api.DenoiseParams.from_buffer_copy(bytes(buf[:16]))
    d = api.denoise_defaults()
    assert d == {"iterations": p.iterations, "sigma_color": p.sigma_color, "sigma_normal": p.sigma_normal, "sigma_depth": p.sigma_depth}
    assert d["iterations"] == 5
    assert np.float32(d["sigma_color"]) == np.float32(1.0)
    assert np.float32(d["sigma_normal"]) == np.float32(64.0)
    assert np.float32(d["sigma_depth"]) == np.float32(0.02)
    api.lib().pt_denoise_defaults(None)                   # ignored


@pytest.mark.parametrize("w,h", [(1, 1), (64, 48), (255, 3), (256, 1), (257, 1), (1920, 1080)])
def test_workspace_bytes_match_the_layout(api, w, h):
    n = w * h
    parts = (n + 255) // 256
    assert api.denoise_workspace_bytes(w, h) == 3 * n * 16 + ((parts * 8 + 15) & ~15) + 16


def test_workspace_bytes_of_an_empty_image_are_zero(api):
    assert api.denoise_workspace_bytes(0, 10) == 0 and api.denoise_workspace_bytes(10, -1) == 0


def test_render_aovs_argument_checks(api):
    L = api.lib()
    buf = np.zeros((8, 16, 4), np.float32)
    cam = _cam(api)
    p = buf.ctypes.data
    cases = [
        ((None, ctypes.byref(cam), 0, 8, 1, 1, p, p), "size"),
        ((None, ctypes.byref(cam), 16, -1, 1, 1, p, p), "size"),
        ((None, ctypes.byref(cam), 16, 8, 0, 1, p, p), "aov_spp"),
        ((None, ctypes.byref(cam), 16, 8, -3, 1, p, p), "aov_spp"),
        ((None, None, 16, 8, 1, 1, p, p), "null camera"),
        ((None, ctypes.byref(cam), 16, 9, 1, 1, p, p), "camera is 16 x 8"),
        ((None, ctypes.byref(_cam(api, 17, 8)), 16, 8, 1, 1, p, p), "camera is 17 x 8"),
        ((None, ctypes.byref(cam), 16, 8, 1, 1, None, p), "null output"),
        ((None, ctypes.byref(cam), 16, 8, 1, 1, p, None), "null output"),
        ((None, ctypes.byref(cam), 16, 8, 1, 1, p, p), "null scene"),
    ]
    for args, msg in cases:
        assert L.pt_render_aovs(*args) < 0, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_render_aovs_device(*args, None) < 0, args
        assert msg in _err(api), (args, _err(api))


def test_denoise_argument_checks(api):
    L = api.lib()
    buf = np.zeros((8, 16, 4), np.float32)
    p = buf.ctypes.data
    good = api.DenoiseParams(5, 1.0, 64.0, 0.1)

    def params(**kw):
        q = api.DenoiseParams(good.iterations, good.sigma_color, good.sigma_normal, good.sigma_depth)
        for k, v in kw.items():
            setattr(q, k, v)
        return ctypes.byref(q)

    cases = [
        ((0, 8, p, 4, p, p, params(), p), "size"),
        ((16, 0, p, 4, p, p, params(), p), "size"),
        ((16, 8, p, 0, p, p, params(), p), "spp"),
        ((16, 8, p, -1, p, p, params(), p), "spp"),
        ((16, 8, None, 4, p, p, params(), p), "null"),
        ((16, 8, p, 4, None, p, params(), p), "null"),
        ((16, 8, p, 4, p, None, params(), p), "null"),
        ((16, 8, p, 4, p, p, params(), None), "null"),
        ((16, 8, p, 4, p, p, params(iterations=-1), p), "iterations"),
        ((16, 8, p, 4, p, p, params(iterations=17), p), "iterations"),
        ((16, 8, p, 4, p, p, params(sigma_color=0.0), p), "sigma_color"),
        ((16, 8, p, 4, p, p, params(sigma_color=float("nan")), p), "sigma_color"),
        ((16, 8, p, 4, p, p, params(sigma_normal=-1.0), p), "sigma_normal"),
        ((16, 8, p, 4, p, p, params(sigma_depth=0.0), p), "sigma_depth"),
        ((16, 8, p, 4, p, p, params(sigma_depth=float("inf")), p), "sigma_depth"),
    ]
    for args, msg in cases:
        assert L.pt_denoise(*args) < 0, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_denoise_device(*args[:7], p, args[7], None) < 0, args
        assert msg in _err(api), (args, _err(api))
    assert L.pt_denoise_device(16, 8, p, 4, p, p, params(), None, p, None) < 0
    assert "workspace" in _err(api)


def test_python_wrappers_reject_bad_shapes_and_dtypes(api):
    f4 = np.zeros((8, 16, 4), np.float32)
    bad = [
        (np.zeros((8, 16, 3), np.float32), f4, f4),
        (f4, np.zeros((8, 15, 4), np.float32), f4),
        (f4, f4, np.zeros((16, 8, 4), np.float32)),
        (f4.astype(np.float64), f4, f4),
        (f4, f4.astype(np.float16), f4),
        (f4.reshape(-1, 4), f4, f4),
        ([[0.0] * 4], f4, f4),
    ]
    for s, a, n in bad:
        with pytest.raises(api.PtError):
            api.denoise(s, 4, a, n)
    with pytest.raises(api.PtError):
        api.denoise(f4, 4, f4, f4, out=np.zeros((8, 16, 4), np.float64))
    with pytest.raises(api.PtError):                      # the library's own checks surface as PtError too
        api.denoise(f4, 0, f4, f4)
    with pytest.raises(api.PtError):
        api.denoise(f4, 4, f4, f4, iterations=-1)
