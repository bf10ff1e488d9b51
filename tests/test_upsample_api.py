"""The render scale without a GPU: the C ABI and the Python wrappers of pt_upsample, pt_temporal_accumulate_cur, pt_camera_scaled
and pt_preview_set_scale (symbols, struct layout against the header, defaults, argument checks that must fire before any HIP
call), and the numpy restatement (tests/upsample_ref.py) on hand-made buffers with a known answer."""
import ctypes

import numpy as np
import pytest

import temporal_ref as T
import upsample_ref as U
from test_preview_api import _header_fields

NEW_SYMBOLS = ("pt_upsample_defaults", "pt_upsample", "pt_upsample_device", "pt_camera_scaled", "pt_temporal_accumulate_cur",
               "pt_temporal_accumulate_cur_device", "pt_preview_set_scale", "pt_preview_scale")
f32 = np.float32


def _err(api):
    return api.lib().pt_last_error().decode()


def _cam(api, w=16, h=8):
    return api.make_camera(True, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 45.0, w, h)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported(api):
    L = api.lib()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    assert L.pt_api_version() == 1
    for name in ("UpsampleParams", "upsample_defaults", "scaled_camera", "upsample", "upsample_device", "temporal_accumulate_cur",
                 "temporal_accumulate_cur_device"):
        assert hasattr(api, name), name
    assert hasattr(api.TemporalHistory, "push_cur") and hasattr(api.Preview, "set_scale") and hasattr(api.Preview, "scale")


def test_upsample_params_layout_and_defaults(api):
    P = api.UpsampleParams
    assert ctypes.sizeof(P) == 8 and ctypes.alignment(P) == 4
    assert [f for f, _ in P._fields_] == _header_fields("pt_upsample_params") == ["sigma_normal", "sigma_depth"]
    assert [P.sigma_normal.offset, P.sigma_depth.offset] == [0, 4]
    buf = (ctypes.c_uint8 * 32)(*([0xAB] * 32))           # the C side writes exactly 8 bytes
    api.lib().pt_upsample_defaults(ctypes.cast(buf, ctypes.POINTER(P)))
    assert bytes(buf[8:]) == b"\xab" * 24
    p = P.from_buffer_copy(bytes(buf[:8]))
    d = api.upsample_defaults()
    assert d == {"sigma_normal": p.sigma_normal, "sigma_depth": p.sigma_depth}
    assert f32(d["sigma_normal"]) == f32(U.DEFAULTS["sigma_normal"]) and f32(d["sigma_depth"]) == f32(U.DEFAULTS["sigma_depth"])
    api.lib().pt_upsample_defaults(None)                  # ignored
    # the session's structs keep their layouts: the scale is not a parameter
    assert ctypes.sizeof(api.PreviewParams) == 68 and ctypes.sizeof(api.PreviewStats) == 28


def test_camera_scaled_round_trip(api):
    L = api.lib()
    cam = api.make_camera(False, (0.1, 0.2, 1.0), (3.0, 4.0, 5.0), 50.0, 1920, 1080, 0.02, 2.0)
    for s in (1, 2, 3, 4, 5, 6, 8):
        lo = api.scaled_camera(cam, s)
        assert (lo.w, lo.h) == (1920 // s, 1080 // s)
        back = api.Camera.frombytes(lo.tobytes()); back.w, back.h = cam.w, cam.h
        assert back.tobytes() == cam.tobytes()            # nothing but the size changed
        # the claim the upsampling rests on: both sizes have the same aspect, bit for bit
        assert f32(1920) / f32(1080) == f32(lo.w) / f32(lo.h)
    assert api.scaled_camera(cam, 1).tobytes() == cam.tobytes()
    out = api.Camera()
    for s, msg in ((0, "scale 0 must be 1..8"), (-2, "scale -2"), (9, "scale 9"), (7, "scale 7 must divide the camera's size 1920 x 1080"),
                   (16, "scale 16")):
        assert L.pt_camera_scaled(ctypes.byref(cam), s, ctypes.byref(out)) == -1
        assert msg in _err(api) and "pt_camera_scaled" in _err(api), _err(api)
    assert L.pt_camera_scaled(None, 2, ctypes.byref(out)) == -1 and "null" in _err(api)
    assert L.pt_camera_scaled(ctypes.byref(cam), 2, None) == -1 and "null" in _err(api)
    with pytest.raises(api.PtError, match="must divide"):
        api.scaled_camera(_cam(api, 63, 45), 2)


def test_upsample_argument_checks(api):
    L = api.lib()
    w, h, s = 16, 8, 2
    lo = np.ones((h // s, w // s, 4), f32); full = np.ones((h, w, 4), f32); out = np.zeros((h, w, 4), f32)
    l, f, o = lo.ctypes.data, full.ctypes.data, out.ctypes.data

    def params(sigma_normal=64.0, sigma_depth=0.02):
        return ctypes.byref(api.UpsampleParams(sigma_normal, sigma_depth))

    # (w, h, scale, S_lo, Q_lo, spp, batches, albedo_lo, nd_lo, albedo, nd, params, out)
    cases = [
        ((0, h, s, l, l, 4, 2, l, l, f, f, params(), o), "size"),
        ((w, -1, s, l, l, 4, 2, l, l, f, f, params(), o), "size"),
        ((1 << 16, 1 << 16, s, l, l, 4, 2, l, l, f, f, params(), o), "too large"),
        ((w, h, 1, l, l, 4, 2, l, l, f, f, params(), o), "scale 1 must be 2..8"),
        ((w, h, 0, l, l, 4, 2, l, l, f, f, params(), o), "scale 0 must be 2..8"),
        ((w, h, 9, l, l, 4, 2, l, l, f, f, params(), o), "scale 9 must be 2..8"),
        ((w, h, 3, l, l, 4, 2, l, l, f, f, params(), o), "scale 3 must divide the image size 16 x 8"),
        ((w, 9, 2, l, l, 4, 2, l, l, f, f, params(), o), "scale 2 must divide the image size 16 x 9"),
        ((w, h, s, l, l, 0, 2, l, l, f, f, params(), o), "spp 0 must be positive"),
        ((w, h, s, l, l, 4, 1, l, l, f, f, params(), o), "batches 1 must be at least 2"),
        ((w, h, s, l, l, 4, 3, l, l, f, f, params(), o), "batches 3 must divide spp 4"),
        ((w, h, s, None, l, 4, 2, l, l, f, f, params(), o), "null buffer"),
        ((w, h, s, l, None, 4, 2, l, l, f, f, params(), o), "null buffer"),
        ((w, h, s, l, l, 4, 2, None, l, f, f, params(), o), "null buffer"),
        ((w, h, s, l, l, 4, 2, l, None, f, f, params(), o), "null buffer"),
        ((w, h, s, l, l, 4, 2, l, l, None, f, params(), o), "null buffer"),
        ((w, h, s, l, l, 4, 2, l, l, f, None, params(), o), "null buffer"),
        ((w, h, s, l, l, 4, 2, l, l, f, f, params(), None), "null output"),
        ((w, h, s, l, l, 4, 2, l, l, f, f, params(), f), "alias"),
        ((w, h, s, l, l, 4, 2, l, l, f, o, params(), o), "alias"),
        ((w, h, s, l, l, 4, 2, l, l, f, f, params(), f + 64), "alias"),                  # a partial overlap is one too
        ((w, h, s, o + 16, l, 4, 2, l, l, f, f, params(), o), "alias"),                  # a low-res input inside the output
        ((w, h, s, l, l, 4, 2, l, o + 256, f, f, params(), o), "alias"),
        ((w, h, s, l, l, 4, 2, l, l, f, f, params(sigma_normal=-1.0), o), "sigma_normal"),
        ((w, h, s, l, l, 4, 2, l, l, f, f, params(sigma_normal=float("nan")), o), "sigma_normal"),
        ((w, h, s, l, l, 4, 2, l, l, f, f, params(sigma_normal=float("inf")), o), "sigma_normal"),
        ((w, h, s, l, l, 4, 2, l, l, f, f, params(sigma_depth=0.0), o), "sigma_depth"),
        ((w, h, s, l, l, 4, 2, l, l, f, f, params(sigma_depth=-0.1), o), "sigma_depth"),
        ((w, h, s, l, l, 4, 2, l, l, f, f, params(sigma_depth=float("nan")), o), "sigma_depth"),
        ((w, h, s, l, l, 4, 2, l, l, f, f, params(sigma_depth=float("inf")), o), "sigma_depth"),
    ]
    for args, msg in cases:
        assert L.pt_upsample(*args) == -1, args
        assert msg in _err(api) and "pt_upsample" in _err(api), (args, _err(api))
        assert L.pt_upsample_device(*args, None) == -1, args
        assert msg in _err(api), (args, _err(api))
    assert not out.any() and (full == 1).all() and (lo == 1).all()      # nothing ran
    # the wrapper's array checks (denoise_var's)
    good = dict(scale=2, rgba_sum_lo=lo, sq_sum_lo=lo, spp=4, batches=2, albedo_lo=lo, normal_depth_lo=lo, albedo=full, normal_depth=full)
    for kw in (dict(albedo=np.zeros((h, w, 3), f32)), dict(normal_depth=full.astype(np.float64)), dict(normal_depth=np.zeros((h, w + 2, 4), f32)),
               dict(rgba_sum_lo=full), dict(sq_sum_lo=lo.reshape(-1, 4)), dict(albedo_lo=lo.astype(np.float16)), dict(scale=4), dict(scale=3),
               dict(scale=1), dict(spp=0), dict(batches=3), dict(sigma_depth=0.0)):
        with pytest.raises(api.PtError):
            api.upsample(**{**good, **kw})


def test_temporal_accumulate_cur_argument_checks(api):
    L = api.lib()
    buf = np.zeros((8, 16, 4), f32); other = np.zeros((8, 16, 4), f32); ln = np.zeros((8, 16), f32); ln2 = np.zeros((8, 16), f32)
    p, o, l, l2 = buf.ctypes.data, other.ctypes.data, ln.ctypes.data, ln2.ctypes.data
    cam = ctypes.byref(_cam(api)); cam17 = ctypes.byref(_cam(api, 17, 8))

    def params(**kw):
        q = api.TemporalParams(8, 0.05, 0.9)
        for k, v in kw.items():
            setattr(q, k, v)
        return ctypes.byref(q)

    # (w, h, cam, cam_prev, cur, nd, prev_nd, hist, hist_len, params, out_hist, out_len)
    cases = [
        ((0, 8, cam, cam, p, p, p, p, l, params(), o, l2), "size"),
        ((16, -1, cam, cam, p, p, p, p, l, params(), o, l2), "size"),
        ((1 << 16, 1 << 16, cam, cam, p, p, p, p, l, params(), o, l2), "too large"),
        ((16, 8, None, cam, p, p, p, p, l, params(), o, l2), "null camera"),
        ((16, 8, cam17, cam, p, p, p, p, l, params(), o, l2), "camera is 17 x 8"),
        ((16, 8, cam, cam17, p, p, p, p, l, params(), o, l2), "previous camera is 17 x 8"),
        ((16, 8, cam, cam, None, p, p, p, l, params(), o, l2), "null buffer"),
        ((16, 8, cam, cam, p, None, p, p, l, params(), o, l2), "null buffer"),
        ((16, 8, cam, cam, p, p, p, p, l, params(), None, l2), "null output"),
        ((16, 8, cam, cam, p, p, p, p, l, params(), o, None), "null output"),
        ((16, 8, cam, cam, p, p, None, p, l, params(), o, l2), "all NULL"),
        ((16, 8, cam, cam, p, p, p, None, l, params(), o, l2), "all NULL"),
        ((16, 8, cam, cam, p, p, p, p, None, params(), o, l2), "all NULL"),
        ((16, 8, cam, cam, p, p, p, o, l, params(), o, l2), "alias"),
        ((16, 8, cam, cam, p, p, p, p, l, params(), o, l), "alias"),
        ((16, 8, cam, cam, p, p, p, o, l, params(), o + 64, l2), "alias"),
        ((16, 8, cam, cam, p, p, p, p, l, params(max_history=0), o, l2), "max_history 0"),
        ((16, 8, cam, cam, p, p, p, p, l, params(depth_tol=0.0), o, l2), "depth_tol"),
        ((16, 8, cam, cam, p, p, p, p, l, params(depth_tol=float("nan")), o, l2), "depth_tol"),
        ((16, 8, cam, cam, p, p, p, p, l, params(normal_tol=0.0), o, l2), "normal_tol"),
        ((16, 8, cam, cam, p, p, p, p, l, params(normal_tol=1.5), o, l2), "normal_tol"),
    ]
    for args, msg in cases:
        assert L.pt_temporal_accumulate_cur(*args) == -1, args
        assert msg in _err(api) and "pt_temporal_accumulate_cur:" in _err(api), (args, _err(api))
        assert L.pt_temporal_accumulate_cur_device(*args, None) == -1, args
        assert msg in _err(api), (args, _err(api))
    assert not other.any() and not ln2.any()              # nothing ran
    f4 = np.zeros((8, 16, 4), f32)
    c = _cam(api)
    for kw in (dict(cur=np.zeros((8, 16, 3), f32)), dict(normal_depth=np.zeros((8, 15, 4), f32)), dict(prev_normal_depth=f4, hist=f4),
               dict(prev_normal_depth=f4, hist=f4, hist_len=np.zeros((16, 8), f32)), dict(max_history=0)):
        with pytest.raises(api.PtError):
            api.temporal_accumulate_cur(c, **{**dict(cur=f4, normal_depth=f4), **kw})
    with pytest.raises(api.PtError):
        api.TemporalHistory(16, 8).push_cur(c, np.zeros((8, 17, 4), f32), f4)


def test_preview_set_scale_null_session(api):
    L = api.lib()
    assert L.pt_preview_set_scale(None, 2) == -1 and "pt_preview_set_scale: null session" in _err(api)
    assert L.pt_preview_scale(None) == -1 and "pt_preview_scale: null session" in _err(api)


# ---- the restatement on hand-made buffers with a known answer -------------------------------------------------------------------
@pytest.mark.parametrize("wl,hl,s", [(8, 8, 2), (8, 4, 3)])
def test_constant_guides_give_the_bilinear_interpolation(wl, hl, s):
    S, Q, Al, Nl, A, N = U.synthetic(wl, hl, s, 1)
    cur, kind, fragile = U.upsample(s, S, Q, 4, 2, Al, Nl, A, N)
    _, e, V, skip = T.frame_ev(S, Q, 4, 2, Al)
    assert not skip.any() and (kind == U.WEIGHTED).all() and not fragile.any()
    want_e, want_V, W = U.bilinear_closed_form(s, e.astype(np.float64), V.astype(np.float64))
    np.testing.assert_allclose(cur[..., :3], want_e, rtol=1e-6)
    np.testing.assert_allclose(cur[..., 3], want_V, rtol=1e-6)
    # on the low-res grid the frame itself; between two samples their mean at a quarter of the summed variance (scale 2)
    assert np.array_equal(cur[::s, ::s, :3], e) and np.array_equal(cur[::s, ::s, 3], V)
    inner = W[:, :-s] if s > 1 else W
    np.testing.assert_allclose(inner[:-s], 1.0, rtol=1e-6)                  # plain bilinear away from the high edges
    if s == 2:
        np.testing.assert_allclose(cur[0, 1, :3], 0.5 * (e[0, 0].astype(np.float64) + e[0, 1]), rtol=1e-6)
        np.testing.assert_allclose(cur[0, 1, 3], 0.25 * (float(V[0, 0]) + float(V[0, 1])), rtol=1e-6)
    # past the last low-res sample only the taps inside the image remain
    np.testing.assert_allclose(cur[0, -1, :3], e[0, -1], rtol=1e-6)


@pytest.mark.parametrize("wl,hl,s", [(8, 8, 2), (8, 4, 3)])
def test_no_value_crosses_a_depth_step(wl, hl, s):
    S, Q, Al, Nl, A, N = U.synthetic(wl, hl, s, 2, depth_split=True)
    cur, kind, _ = U.upsample(s, S, Q, 4, 2, Al, Nl, A, N)
    _, e, V, _ = T.frame_ev(S, Q, 4, 2, Al)
    assert (kind == U.WEIGHTED).all()
    w = wl * s
    for side, lo_side in ((np.s_[:, :w // 2], np.s_[:, :wl // 2]), (np.s_[:, w // 2:], np.s_[:, wl // 2:])):
        lo_min, lo_max = e[lo_side].min(), e[lo_side].max()
        assert cur[side][..., :3].min() >= lo_min - 1e-6 and cur[side][..., :3].max() <= lo_max + 1e-6
    assert cur[:, :w // 2, :3].max() < 0.5 < cur[:, w // 2:, :3].min()     # (left e in [0.18, 0.22], right e in [0.9, 1.1])


def test_branches_of_the_restatement():
    s, wl, hl = 2, 8, 8
    S, Q, Al, Nl, A, N = U.synthetic(wl, hl, s, 3)
    _, e, V, _ = T.frame_ev(S, Q, 4, 2, Al)
    m = S[..., :3] / f32(4)
    A[5, 7, 3] = 0.0                                      # nothing hit at display resolution: the nearest candidate's raw mean
    A[4, 9, 3] = 0.0                                      # fx = 0.5: a tie, tap (0,0) wins
    S[1, 1, 0] = np.nan                                   # a pass-through low-res pixel is no tap
    N[10, 12, :3] = 0.0                                   # a zero normal: every w_k is 0, the nearest usable tap is copied
    Nl[6, 6, 3] = 3.0                                     # a low-res pixel at another depth: display pixel (12, 12) falls back to it
    cur, kind, fragile = U.upsample(s, S, Q, 4, 2, Al, Nl, A, N)
    assert kind[5, 7] == U.PASS and np.array_equal(cur[5, 7, :3], m[2, 3]) and cur[5, 7, 3] == -1
    assert kind[4, 9] == U.PASS and np.array_equal(cur[4, 9, :3], m[2, 4])
    assert kind[2, 2] == U.PASS and np.isnan(cur[2, 2, 0]) and cur[2, 2, 3] == -1          # its only tap (b = 1) is pass-through
    assert kind[2, 3] == U.WEIGHTED and np.isfinite(cur[2, 3]).all()                       # ... its neighbours have another one
    np.testing.assert_allclose(cur[2, 3, :3], e[1, 2], rtol=1e-6)
    assert np.isfinite(np.delete(cur.reshape(-1, 4), 2 * 16 + 2, 0)).all()                 # the NaN reached nobody else
    assert kind[10, 12] == U.FALLBACK and np.array_equal(cur[10, 12], np.append(e[5, 6], V[5, 6]))
    assert kind[12, 12] == U.FALLBACK and np.array_equal(cur[12, 12], np.append(e[6, 6], V[6, 6]))
    assert kind[12, 13] == U.WEIGHTED
    np.testing.assert_allclose(cur[12, 13, :3], e[6, 7], rtol=1e-6)                        # (6, 6) is rejected by depth, (6, 7) remains
    assert not fragile.any()
    # scale 3: fx = 2 / 3 makes tap (1, 0) the nearest candidate
    S, Q, Al, Nl, A, N = U.synthetic(8, 4, 3, 4)
    A[4, 5, 3] = 0.0; A[4, 4, 3] = 0.0
    cur, kind, _ = U.upsample(3, S, Q, 4, 2, Al, Nl, A, N)
    m = S[..., :3] / f32(4)
    assert np.array_equal(cur[4, 5, :3], m[1, 2]) and np.array_equal(cur[4, 4, :3], m[1, 1]) and kind[4, 5] == U.PASS


def test_accumulate_cur_is_accumulate_from_step_two_on(api):
    h, w = 6, 10
    cam = _cam(api, w, h)
    S, Q, Al, Nl, A, N = U.synthetic(w, h, 1, 5)
    S2, Q2, _, _, _, _ = U.synthetic(w, h, 1, 6)
    S2[2, 3, 0] = np.nan; A[4, 5, 3] = 0.0
    h0, l0, _ = T.accumulate(cam, None, S, Q, 4, 2, Al, N)
    want, want_len, _ = T.accumulate(cam, cam, S2, Q2, 4, 2, A, N, N, h0, l0)
    m, e, V, skip = T.frame_ev(S2, Q2, 4, 2, A)
    cur = np.concatenate([np.where(skip[..., None], m, e), np.where(skip, f32(-1), V)[..., None]], -1).astype(f32)
    got, got_len, _ = U.accumulate_cur(cam, cam, cur, N, N, h0, l0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got_len, want_len)
    assert got_len[2, 3] == 0 and got[2, 3, 3] == -1 and np.isnan(got[2, 3, 0]) and got_len[4, 5] == 0 and got_len.max() == 2
    first, first_len, _ = U.accumulate_cur(cam, None, cur, N)
    assert np.array_equal(first.view(np.uint32), cur.view(np.uint32)) and np.array_equal(first_len, np.where(skip, 0, 1))
    assert T.frame_ev is not None and T.accumulate(cam, None, S, Q, 4, 2, Al, N)[0].shape == (h, w, 4)      # temporal_ref is as it was
