"""Temporal accumulation and the history filter without a GPU: the C ABI and the Python wrappers (symbols, struct layout,
defaults, workspace size, argument checks that must fire before any HIP call), and the numpy restatement itself
(tests/temporal_ref.py) on hand-made buffers with a known answer."""
import ctypes

import numpy as np
import pytest

import temporal_ref as T
from denoise_var_ref import moments_from_partial_sums

NEW_SYMBOLS = ("pt_temporal_defaults", "pt_temporal_accumulate", "pt_temporal_accumulate_device", "pt_denoise_hist_workspace_bytes",
               "pt_denoise_hist", "pt_denoise_hist_device")
f32 = np.float32


def _err(api):
    return api.lib().pt_last_error().decode()


def _cam(api, w=16, h=8, pos=(0.0, 0.0, 3.0), rot=(0.0, 0.0, 0.0)):
    return api.make_camera(True, pos, rot, 45.0, w, h)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported(api):
    L = api.lib()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    assert L.pt_api_version() == 1
    for name in ("TemporalParams", "TemporalHistory", "temporal_defaults", "temporal_accumulate", "temporal_accumulate_device", "denoise_hist",
                 "denoise_hist_device", "denoise_hist_workspace_bytes"):
        assert hasattr(api, name), name


def test_temporal_params_layout_and_defaults(api):
    P = api.TemporalParams
    assert ctypes.sizeof(P) == 12
    assert [P.max_history.offset, P.depth_tol.offset, P.normal_tol.offset] == [0, 4, 8]
    buf = (ctypes.c_uint8 * 32)(*([0xAB] * 32))           # the C side writes exactly 12 bytes
    api.lib().pt_temporal_defaults(ctypes.cast(buf, ctypes.POINTER(P)))
    assert bytes(buf[12:]) == b"\xab" * 20
    p = P.from_buffer_copy(bytes(buf[:12]))
    d = api.temporal_defaults()
    assert d == {"max_history": p.max_history, "depth_tol": p.depth_tol, "normal_tol": p.normal_tol}
    assert d["max_history"] == T.DEFAULTS["max_history"]
    assert f32(d["depth_tol"]) == f32(T.DEFAULTS["depth_tol"]) and f32(d["normal_tol"]) == f32(T.DEFAULTS["normal_tol"])
    api.lib().pt_temporal_defaults(None)                  # ignored
    assert api.denoise_var_defaults()["iterations"] == 3  # pt_denoise_var's own defaults are untouched


@pytest.mark.parametrize("w,h", [(1, 1), (64, 48), (255, 3), (257, 1), (1920, 1080), (0, 10), (10, -1)])
def test_hist_workspace_is_the_variance_filters(api, w, h):
    assert api.denoise_hist_workspace_bytes(w, h) == api.denoise_var_workspace_bytes(w, h)


def test_temporal_accumulate_argument_checks(api):
    L = api.lib()
    buf = np.zeros((8, 16, 4), f32); other = np.zeros((8, 16, 4), f32); ln = np.zeros((8, 16), f32); ln2 = np.zeros((8, 16), f32)
    p, o, l, l2 = buf.ctypes.data, other.ctypes.data, ln.ctypes.data, ln2.ctypes.data
    cam = ctypes.byref(_cam(api))
    cam17 = ctypes.byref(_cam(api, 17, 8))
    good = api.TemporalParams(8, 0.05, 0.9)

    def params(**kw):
        q = api.TemporalParams(good.max_history, good.depth_tol, good.normal_tol)
        for k, v in kw.items():
            setattr(q, k, v)
        return ctypes.byref(q)

    # (w, h, cam, cam_prev, S, Q, spp, batches, albedo, nd, prev_nd, hist, hist_len, params, out_hist, out_len)
    cases = [
        ((0, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(), o, l2), "size"),
        ((16, -1, cam, cam, p, p, 4, 2, p, p, p, p, l, params(), o, l2), "size"),
        ((16, 8, cam, cam, p, p, 0, 2, p, p, p, p, l, params(), o, l2), "spp 0 must be positive"),
        ((16, 8, cam, cam, p, p, -4, 2, p, p, p, p, l, params(), o, l2), "spp -4 must be positive"),
        ((16, 8, cam, cam, p, p, 4, 1, p, p, p, p, l, params(), o, l2), "batches 1 must be at least 2"),
        ((16, 8, cam, cam, p, p, 4, 3, p, p, p, p, l, params(), o, l2), "batches 3 must divide spp 4"),
        ((16, 8, None, cam, p, p, 4, 2, p, p, p, p, l, params(), o, l2), "null camera"),
        ((16, 8, cam17, cam, p, p, 4, 2, p, p, p, p, l, params(), o, l2), "camera is 17 x 8"),
        ((16, 8, cam, cam17, p, p, 4, 2, p, p, p, p, l, params(), o, l2), "previous camera is 17 x 8"),
        ((16, 9, cam, cam, p, p, 4, 2, p, p, p, p, l, params(), o, l2), "camera is 16 x 8"),
        ((16, 8, cam, cam, None, p, 4, 2, p, p, p, p, l, params(), o, l2), "null buffer"),
        ((16, 8, cam, cam, p, None, 4, 2, p, p, p, p, l, params(), o, l2), "null buffer"),
        ((16, 8, cam, cam, p, p, 4, 2, None, p, p, p, l, params(), o, l2), "null buffer"),
        ((16, 8, cam, cam, p, p, 4, 2, p, None, p, p, l, params(), o, l2), "null buffer"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(), None, l2), "null output"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(), o, None), "null output"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, None, p, l, params(), o, l2), "all NULL"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, None, l, params(), o, l2), "all NULL"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, None, params(), o, l2), "all NULL"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, None, None, l, params(), o, l2), "all NULL"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, o, l, params(), o, l2), "alias"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(), o, l), "alias"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, o, l, params(), o + 64, l2), "alias"),        # a partial overlap is one too
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(max_history=0), o, l2), "max_history 0"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(max_history=-3), o, l2), "max_history -3"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(depth_tol=0.0), o, l2), "depth_tol"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(depth_tol=-0.1), o, l2), "depth_tol"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(depth_tol=float("nan")), o, l2), "depth_tol"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(normal_tol=0.0), o, l2), "normal_tol"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(normal_tol=-0.5), o, l2), "normal_tol"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(normal_tol=float("nan")), o, l2), "normal_tol"),
        ((16, 8, cam, cam, p, p, 4, 2, p, p, p, p, l, params(normal_tol=1.5), o, l2), "normal_tol"),
    ]
    for args, msg in cases:
        assert L.pt_temporal_accumulate(*args) < 0, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_temporal_accumulate_device(*args, None) < 0, args
        assert msg in _err(api), (args, _err(api))
    assert not other.any() and not ln2.any()              # nothing ran


def test_denoise_hist_argument_checks(api):
    L = api.lib()
    buf = np.zeros((8, 16, 4), f32)
    p = buf.ctypes.data

    def params(**kw):
        q = api.DenoiseVarParams(3, 6.0, 64.0, 0.02)
        for k, v in kw.items():
            setattr(q, k, v)
        return ctypes.byref(q)

    # (w, h, hist, albedo, nd, params, out)
    cases = [
        ((0, 8, p, p, p, params(), p), "size"),
        ((16, 0, p, p, p, params(), p), "size"),
        ((16, 8, None, p, p, params(), p), "null"),
        ((16, 8, p, None, p, params(), p), "null"),
        ((16, 8, p, p, None, params(), p), "null"),
        ((16, 8, p, p, p, params(), None), "null"),
        ((16, 8, p, p, p, params(iterations=-1), p), "iterations"),
        ((16, 8, p, p, p, params(iterations=17), p), "iterations"),
        ((16, 8, p, p, p, params(sigma_var=0.0), p), "sigma_var"),
        ((16, 8, p, p, p, params(sigma_normal=-1.0), p), "sigma_normal"),
        ((16, 8, p, p, p, params(sigma_depth=float("inf")), p), "sigma_depth"),
    ]
    for args, msg in cases:
        assert L.pt_denoise_hist(*args) < 0, args
        assert msg in _err(api) and "pt_denoise_hist" in _err(api), (args, _err(api))
        assert L.pt_denoise_hist_device(*args[:6], p, args[6], None) < 0, args
        assert msg in _err(api), (args, _err(api))
    assert L.pt_denoise_hist_device(16, 8, p, p, p, params(), None, p, None) < 0
    assert "workspace" in _err(api)


def test_python_wrappers_reject_bad_shapes_and_dtypes(api):
    f4 = np.zeros((8, 16, 4), f32)
    ln = np.zeros((8, 16), f32)
    cam = _cam(api)
    bad = [
        dict(rgba_sum=np.zeros((8, 16, 3), f32)), dict(sq_sum=np.zeros((8, 15, 4), f32)), dict(albedo=f4.astype(np.float64)),
        dict(normal_depth=f4.reshape(-1, 4)), dict(prev_normal_depth=f4, hist=f4), dict(hist=f4, hist_len=ln),
        dict(prev_normal_depth=f4, hist=np.zeros((8, 17, 4), f32), hist_len=ln), dict(prev_normal_depth=f4, hist=f4, hist_len=np.zeros((16, 8), f32)),
        dict(prev_normal_depth=f4, hist=f4, hist_len=ln.astype(np.float64)), dict(spp=0), dict(batches=3), dict(max_history=0),
        dict(prev_normal_depth=f4, hist=f4, hist_len=ln, normal_tol=2.0),
    ]
    for kw in bad:
        a = dict(rgba_sum=f4, sq_sum=f4, spp=4, batches=2, albedo=f4, normal_depth=f4)
        a.update(kw)
        with pytest.raises(api.PtError):
            api.temporal_accumulate(cam, **a)
    for h_, a_, n_ in ((np.zeros((8, 16, 3), f32), f4, f4), (f4, f4.astype(np.float16), f4), (f4, f4, np.zeros((16, 8, 4), f32))):
        with pytest.raises(api.PtError):
            api.denoise_hist(h_, a_, n_)
    with pytest.raises(api.PtError):
        api.denoise_hist(f4, f4, f4, out=np.zeros((8, 16, 4), np.float64))
    with pytest.raises(api.PtError):
        api.denoise_hist(f4, f4, f4, iterations=-1)
    with pytest.raises(api.PtError):
        api.TemporalHistory(16, 8).push(cam, np.zeros((8, 17, 4), f32), f4, 4, 2, f4, f4)


# ---- the restatement on hand-made buffers with a known answer -------------------------------------------------------------------
def _frame(h, w, seed, spp=4, batches=2, albedo=0.5, depth=2.0):
    """S, Q of a synthetic frame with per-pixel noise; flat albedo, a +z normal of length 0.5 (not unit on purpose) and flat depth."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((h, w, 4), f32); partial = []
    for _ in range(batches):
        acc = acc.copy()
        acc[..., :3] = (acc[..., :3] + rng.uniform(0.2, 1.0, (h, w, 3)).astype(f32) * f32(spp // batches)).astype(f32)
        partial.append(acc)
    A = np.zeros((h, w, 4), f32); A[..., :3] = albedo; A[..., 3] = 1.0
    N = np.zeros((h, w, 4), f32); N[..., 2] = 0.5; N[..., 3] = depth
    return partial[-1], moments_from_partial_sums(partial), A, N


def test_first_frame_is_the_frames_own_estimate(api):
    S, Q, A, N = _frame(6, 10, 1)
    S[2, 3, 0] = np.nan; A[4, 5, 3] = 0.0
    hist, ln, fragile = T.accumulate(_cam(api, 10, 6), None, S, Q, 4, 2, A, N)
    m, e, V, skip = T.frame_ev(S, Q, 4, 2, A)
    assert skip[2, 3] and skip[4, 5] and skip.sum() == 2
    use = ~skip
    assert np.array_equal(hist[use][:, :3], e[use]) and np.array_equal(hist[use][:, 3], V[use]) and np.all(ln[use] == 1)
    # a pass-through pixel holds the raw mean, the mark and length 0
    assert np.array_equal(hist[4, 5, :3], m[4, 5]) and hist[4, 5, 3] == -1 and ln[4, 5] == 0
    assert np.isnan(hist[2, 3, 0]) and hist[2, 3, 3] == -1 and ln[2, 3] == 0
    assert not fragile.any()
    assert np.allclose(e[use], S[use][:, :3] / 4 / 0.5) and (V[use] > 0).all()


def test_identity_with_equal_frames_counts_up_and_the_variance_falls_as_one_over_n(api):
    S, Q, A, N = _frame(5, 7, 2)
    cam = _cam(api, 7, 5)
    hist, ln, _ = T.accumulate(cam, None, S, Q, 4, 2, A, N)
    e0, V0 = hist[..., :3].copy(), hist[..., 3].copy()
    max_history = 5
    for k in range(2, 9):
        prev = cam if k % 2 else None                    # the same bytes and NULL are both the identity
        hist, ln, fragile = T.accumulate(cam, prev, S, Q, 4, 2, A, N, N, hist, ln, max_history=max_history)
        n = min(k, max_history)
        assert np.all(ln == n) and not fragile.any()
        np.testing.assert_allclose(hist[..., :3], e0, rtol=1e-6)          # the mean of equal estimates
        if k <= max_history:
            np.testing.assert_allclose(hist[..., 3], V0 / n, rtol=1e-5)   # independent estimates of equal variance: V / N
    # capped: the exponential average's fixed point alpha / (2 - alpha) V is approached from above
    assert np.all(hist[..., 3] < V0 / max_history) and np.all(hist[..., 3] > V0 / (2 * max_history - 1))


def test_a_depth_jump_or_a_turned_normal_drops_the_tap(api):
    S, Q, A, N = _frame(4, 6, 3)
    cam = _cam(api, 6, 4)
    hist, ln, _ = T.accumulate(cam, None, S, Q, 4, 2, A, N)
    S2, Q2, _, _ = _frame(4, 6, 4)
    N2 = N.copy()
    N2[1, 2, 3] = 2.0 * 1.06             # beyond a depth_tol of 0.05 of the expected depth
    N2[1, 3, 3] = 2.0 * 1.04             # inside it
    N2[2, 2, :3] = (0.5, 0.0, 0.5)       # 45 degrees: cos 0.707 < 0.9
    N2[2, 3, :3] = (0.1, 0.0, 0.5)       # cos 0.98
    N2[3, 3, :3] = 0.0                   # a zero normal has no history
    out, ln2, fragile = T.accumulate(cam, cam, S2, Q2, 4, 2, A, N2, N, hist, ln, depth_tol=0.05)
    _, e2, V2, _ = T.frame_ev(S2, Q2, 4, 2, A)
    for y, x in ((1, 2), (2, 2), (3, 3)):
        assert ln2[y, x] == 1 and np.array_equal(out[y, x, :3], e2[y, x]) and out[y, x, 3] == V2[y, x]
    for y, x in ((1, 3), (2, 3), (0, 0)):
        assert ln2[y, x] == 2 and not np.array_equal(out[y, x, :3], e2[y, x])
    assert not fragile.any()
    # exactly at the threshold the mask reports the pixel
    N3 = N.copy(); N3[1, 2, 3] = f32(2.0 / 0.95)          # |2 - z| = 0.05 z
    assert T.accumulate(cam, cam, S2, Q2, 4, 2, A, N3, N, hist, ln, depth_tol=0.05)[2][1, 2]
    # a pass-through pixel in the history is no tap, and its NaN goes nowhere
    hist_bad = hist.copy(); hist_bad[0, 0] = (np.nan, np.nan, np.nan, -1.0)
    out, ln3, _ = T.accumulate(cam, cam, S2, Q2, 4, 2, A, N, N, hist_bad, ln)
    assert ln3[0, 0] == 1 and np.isfinite(out).all()


def test_a_one_pixel_shift_lands_on_integer_taps(api):
    """A camera that looks down -z at a wall z = 0 parallel to the image plane, moved sideways by exactly one pixel's footprint:
    every pixel's history is its right neighbour's, with bilinear weight 1 on one tap up to the projection's rounding."""
    w, h = 16, 8
    cam0 = _cam(api, w, h, pos=(0.0, 0.0, 4.0))
    c = T.camera_fields(cam0)
    assert np.allclose(c["forward"], (0, 0, -1), atol=1e-6) or np.allclose(c["forward"], (0, 0, 1), atol=1e-6)
    dist = 4.0
    # one pixel is du = 2 / w * aspect * fovScale in image-plane units, i.e. du * dist on the wall
    step = 2.0 / w * (w / h) * float(c["fovScale"]) * dist
    pos1 = np.array([0.0, 0.0, 4.0]) + step * c["right"].astype(np.float64)
    cam1 = _cam(api, w, h, pos=tuple(pos1))
    # depth along each pixel's own centre ray to the wall, for both cameras (the wall is parallel: the same per-pixel depths)
    ys, xs = np.mgrid[0:h, 0:w]
    u = (2.0 * xs / w - 1.0) * (w / h) * float(c["fovScale"]); v = (2.0 * ys / h - 1.0) * float(c["fovScale"])
    depth = (dist * np.sqrt(u * u + v * v + 1.0)).astype(f32)
    S, Q, A, N = _frame(h, w, 5)
    N[..., 3] = depth
    hist0, len0, _ = T.accumulate(cam0, None, S, Q, 4, 2, A, N)
    xp, yp, zexp, ok = T.reproject(cam1, cam0, depth)
    assert ok.all()
    np.testing.assert_allclose(xp, xs + 1.0, atol=2e-4)   # moving right by a pixel: the point was one pixel further right before
    np.testing.assert_allclose(yp, ys, atol=2e-4)
    np.testing.assert_allclose(zexp[:, :-1], depth[:, 1:], rtol=1e-5)
    S1, Q1, _, _ = _frame(h, w, 6)
    out, ln, fragile = T.accumulate(cam1, cam0, S1, Q1, 4, 2, A, N, N, hist0, len0)
    _, e1, V1, _ = T.frame_ev(S1, Q1, 4, 2, A)
    assert not fragile.any()
    assert np.all(ln[:, :-1] == 2) and np.all(ln[:, -1] == 1)            # the last column's history lies outside the image
    want = 0.5 * (hist0[:, 1:, :3].astype(np.float64) + e1[:, :-1])
    np.testing.assert_allclose(out[:, :-1, :3], want, rtol=1e-3, atol=1e-4)   # neighbours differ by O(1): weight error 2e-4
    np.testing.assert_allclose(out[:, :-1, 3], 0.25 * (hist0[:, 1:, 3] + V1[:, :-1]), rtol=1e-3)
    assert np.array_equal(out[:, -1, :3], e1[:, -1])


def test_denoise_hist_restatement_on_flat_buffers():
    S, Q, A, N = _frame(12, 12, 7)
    m, e, V, skip = T.frame_ev(S, Q, 4, 2, A)
    hist = np.concatenate([e, V[..., None]], -1).astype(f32)
    hist[3, 4] = (7.0, 8.0, 9.0, -1.0)                    # pass-through: returned as it is
    hist[6, 6, 1] = np.inf                                # not finite: pass-through too
    out0, skip0, _ = T.denoise_hist(hist, A, N, iterations=0)
    assert skip0[3, 4] and skip0[6, 6] and skip0.sum() == 2
    np.testing.assert_allclose(out0[~skip0][:, :3], (0.5 * e[~skip0]).astype(np.float64), rtol=1e-7)
    assert np.array_equal(out0[3, 4, :3], (7.0, 8.0, 9.0)) and np.all(out0[..., 3] == 0) and np.isinf(out0[6, 6, 1])
    out3, _, _ = T.denoise_hist(hist, A, N, iterations=3)
    use = ~skip0
    assert out3[use][:, :3].var() < 0.5 * out0[use][:, :3].var()           # flat guides: the filter averages
    assert np.isfinite(out3[use]).all() and np.array_equal(out3[3, 4], out0[3, 4])
