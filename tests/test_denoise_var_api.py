"""Per-pixel moments and the variance-guided denoiser without a GPU: the C ABI and the Python wrappers (symbols, struct layout,
defaults, workspace size, argument checks that must fire before any HIP call), and the numpy restatement itself
(tests/denoise_var_ref.py) on cases with a known answer."""
import ctypes

import numpy as np
import pytest

import denoise_var_ref as R
from denoise_ref import H5

NEW_SYMBOLS = ("pt_render_moments", "pt_render_moments_device", "pt_denoise_var_defaults", "pt_denoise_var_workspace_bytes",
               "pt_denoise_var", "pt_denoise_var_device")


def _err(api):
    return api.lib().pt_last_error().decode()


def _cam(api, w=16, h=8):
    return api.make_camera(True, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 45.0, w, h)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported(api):
    L = api.lib()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    assert L.pt_api_version() == 1


def test_denoise_var_params_layout_and_defaults(api):
    P = api.DenoiseVarParams
    assert ctypes.sizeof(P) == 16
    assert [P.iterations.offset, P.sigma_var.offset, P.sigma_normal.offset, P.sigma_depth.offset] == [0, 4, 8, 12]
    buf = (ctypes.c_uint8 * 32)(*([0xAB] * 32))           # the C side writes exactly 16 bytes
    api.lib().pt_denoise_var_defaults(ctypes.cast(buf, ctypes.POINTER(P)))
    assert bytes(buf[16:]) == b"\xab" * 16
    p = P.from_buffer_copy(bytes(buf[:16]))
    d = api.denoise_var_defaults()
    assert d == {"iterations": p.iterations, "sigma_var": p.sigma_var, "sigma_normal": p.sigma_normal, "sigma_depth": p.sigma_depth}
    assert d["iterations"] == 3
    assert np.float32(d["sigma_var"]) == np.float32(6.0)
    assert np.float32(d["sigma_normal"]) == np.float32(64.0)
    assert np.float32(d["sigma_depth"]) == np.float32(0.02)
    api.lib().pt_denoise_var_defaults(None)               # ignored
    assert api.denoise_defaults()["sigma_color"] == 1.0   # pt_denoise's own defaults are untouched


@pytest.mark.parametrize("w,h", [(1, 1), (64, 48), (255, 3), (256, 1), (257, 1), (1920, 1080)])
def test_workspace_bytes_match_the_layout(api, w, h):
    n = w * h
    parts = (n + 255) // 256
    assert api.denoise_var_workspace_bytes(w, h) == 3 * n * 16 + ((parts * 8 + 15) & ~15) + 16


def test_workspace_bytes_of_an_empty_image_are_zero(api):
    assert api.denoise_var_workspace_bytes(0, 10) == 0 and api.denoise_var_workspace_bytes(10, -1) == 0


def test_render_moments_argument_checks(api):
    L = api.lib()
    buf = np.zeros((8, 16, 4), np.float32)
    cam = ctypes.byref(_cam(api))
    p = buf.ctypes.data
    # (scene, camera, w, h, spp, batch_spp, max_depth, integrator, use_mis, seed, S, Q)
    cases = [
        ((None, cam, 0, 8, 16, 4, 4, 0, 1, 1, p, p), "size"),
        ((None, cam, 16, -1, 16, 4, 4, 0, 1, 1, p, p), "size"),
        ((None, cam, 16, 8, 0, 4, 4, 0, 1, 1, p, p), "spp 0 must be positive"),
        ((None, cam, 16, 8, -4, 4, 4, 0, 1, 1, p, p), "spp -4 must be positive"),
        ((None, cam, 16, 8, 16, 0, 4, 0, 1, 1, p, p), "batch_spp 0 must be positive"),
        ((None, cam, 16, 8, 16, -2, 4, 0, 1, 1, p, p), "batch_spp -2 must be positive"),
        ((None, cam, 16, 8, 16, 3, 4, 0, 1, 1, p, p), "multiple of batch_spp"),
        ((None, cam, 16, 8, 16, 16, 4, 0, 1, 1, p, p), "at least 2 batches"),
        ((None, cam, 16, 8, 16, 4, 4, 1, 1, 1, p, p), "integrator"),
        ((None, None, 16, 8, 16, 4, 4, 0, 1, 1, p, p), "null camera"),
        ((None, cam, 16, 9, 16, 4, 4, 0, 1, 1, p, p), "camera is 16 x 8"),
        ((None, ctypes.byref(_cam(api, 17, 8)), 16, 8, 16, 4, 4, 0, 1, 1, p, p), "camera is 17 x 8"),
        ((None, cam, 16, 8, 16, 4, 4, 0, 1, 1, None, p), "null output"),
        ((None, cam, 16, 8, 16, 4, 4, 0, 1, 1, p, None), "null output"),
        ((None, cam, 16, 8, 16, 4, 4, 0, 1, 1, p, p), "null scene"),
    ]
    for args, msg in cases:
        assert L.pt_render_moments(*args) < 0, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_render_moments_device(*args, None) < 0, args
        assert msg in _err(api), (args, _err(api))


def test_denoise_var_argument_checks(api):
    L = api.lib()
    buf = np.zeros((8, 16, 4), np.float32)
    p = buf.ctypes.data
    good = api.DenoiseVarParams(5, 6.0, 64.0, 0.1)

    def params(**kw):
        q = api.DenoiseVarParams(good.iterations, good.sigma_var, good.sigma_normal, good.sigma_depth)
        for k, v in kw.items():
            setattr(q, k, v)
        return ctypes.byref(q)

    # (w, h, S, Q, spp, batches, albedo, normal_depth, params, out)
    cases = [
        ((0, 8, p, p, 16, 4, p, p, params(), p), "size"),
        ((16, 0, p, p, 16, 4, p, p, params(), p), "size"),
        ((16, 8, p, p, 0, 4, p, p, params(), p), "spp"),
        ((16, 8, p, p, -1, 4, p, p, params(), p), "spp"),
        ((16, 8, p, p, 16, 1, p, p, params(), p), "batches 1 must be at least 2"),
        ((16, 8, p, p, 16, 0, p, p, params(), p), "batches 0 must be at least 2"),
        ((16, 8, p, p, 16, 3, p, p, params(), p), "batches 3 must divide spp 16"),
        ((16, 8, None, p, 16, 4, p, p, params(), p), "null"),
        ((16, 8, p, None, 16, 4, p, p, params(), p), "null"),
        ((16, 8, p, p, 16, 4, None, p, params(), p), "null"),
        ((16, 8, p, p, 16, 4, p, None, params(), p), "null"),
        ((16, 8, p, p, 16, 4, p, p, params(), None), "null"),
        ((16, 8, p, p, 16, 4, p, p, params(iterations=-1), p), "iterations"),
        ((16, 8, p, p, 16, 4, p, p, params(iterations=17), p), "iterations"),
        ((16, 8, p, p, 16, 4, p, p, params(sigma_var=0.0), p), "sigma_var"),
        ((16, 8, p, p, 16, 4, p, p, params(sigma_var=float("nan")), p), "sigma_var"),
        ((16, 8, p, p, 16, 4, p, p, params(sigma_normal=-1.0), p), "sigma_normal"),
        ((16, 8, p, p, 16, 4, p, p, params(sigma_depth=0.0), p), "sigma_depth"),
        ((16, 8, p, p, 16, 4, p, p, params(sigma_depth=float("inf")), p), "sigma_depth"),
    ]
    for args, msg in cases:
        assert L.pt_denoise_var(*args) < 0, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_denoise_var_device(*args[:9], p, args[9], None) < 0, args
        assert msg in _err(api), (args, _err(api))
    assert L.pt_denoise_var_device(16, 8, p, p, 16, 4, p, p, params(), None, p, None) < 0
    assert "workspace" in _err(api)


def test_python_wrappers_reject_bad_shapes_and_dtypes(api):
    f4 = np.zeros((8, 16, 4), np.float32)
    bad = [
        (np.zeros((8, 16, 3), np.float32), f4, f4, f4),
        (f4, np.zeros((8, 15, 4), np.float32), f4, f4),
        (f4, f4, np.zeros((16, 8, 4), np.float32), f4),
        (f4, f4, f4, np.zeros((8, 17, 4), np.float32)),
        (f4.astype(np.float64), f4, f4, f4),
        (f4, f4.astype(np.float64), f4, f4),
        (f4, f4, f4.astype(np.float16), f4),
        (f4.reshape(-1, 4), f4, f4, f4),
        ([[0.0] * 4], f4, f4, f4),
    ]
    for s, q, a, n in bad:
        with pytest.raises(api.PtError):
            api.denoise_var(s, q, 16, 4, a, n)
    with pytest.raises(api.PtError):
        api.denoise_var(f4, f4, 16, 4, f4, f4, out=np.zeros((8, 16, 4), np.float64))
    with pytest.raises(api.PtError):                      # the library's own checks surface as PtError too
        api.denoise_var(f4, f4, 0, 4, f4, f4)
    with pytest.raises(api.PtError):
        api.denoise_var(f4, f4, 16, 3, f4, f4)
    with pytest.raises(api.PtError):
        api.denoise_var(f4, f4, 16, 4, f4, f4, iterations=-1)


# ---- the restatement on cases with a known answer -------------------------------------------------------------------------------
def test_moments_replay_matches_a_hand_computed_case():
    f = np.float32
    # one pixel, three batches; partial sums chosen so that every step rounds: 0.1f, 0.1f + 0.2f, ... in float32
    s1 = np.array([[f(0.1), f(1.0), f(3.0), f(0.0)]], f)
    s2 = np.array([[f(0.1) + f(0.2), f(1.5), f(3.0), f(0.0)]], f)
    s3 = np.array([[f(0.7), f(4.0), f(1.0), f(0.0)]], f)
    Q = R.moments_from_partial_sums([s1, s2, s3])
    want = np.zeros((1, 4), f)
    for c in range(3):
        d1 = f(s1[0, c] - f(0)); d2 = f(s2[0, c] - s1[0, c]); d3 = f(s3[0, c] - s2[0, c])
        q = f(f(0) + f(d1 * d1)); q = f(q + f(d2 * d2)); q = f(q + f(d3 * d3))
        want[0, c] = q
    want[0, 3] = f(3)
    assert np.array_equal(Q.view(np.uint32), want.view(np.uint32))
    # the exactly representable channel by hand: batch sums 1, 0.5, 2.5 -> 1 + 0.25 + 6.25; 3, 0, -2 -> 9 + 0 + 4
    assert Q[0, 1] == f(7.5) and Q[0, 2] == f(13.0)
    # f32, not f64: the rounded product differs from the float64 one
    d = np.float64(s2[0, 0]) - np.float64(s1[0, 0])
    assert np.float64(Q[0, 0]) != np.float64(s1[0, 0]) ** 2 + d * d + (np.float64(s3[0, 0]) - np.float64(s2[0, 0])) ** 2
    # NaN / Inf propagate
    bad = R.moments_from_partial_sums([np.array([[np.inf, np.nan, 1.0, 0.0]], f), np.array([[np.inf, np.nan, 2.0, 0.0]], f)])
    assert np.isnan(bad[0, 0]) and np.isnan(bad[0, 1]) and bad[0, 2] == f(2.0)


def test_variance_of_mean_known_values():
    f = np.float32
    # batch sums (2, 4) per channel: S = 6, Q = 20, B = 2, spp = 4: max(0, 20 - 36 / 2) / 1 * 2 / 16 = 0.25 per channel
    S = np.full((1, 1, 4), 6.0, f); Q = np.full((1, 1, 4), 20.0, f)
    A = np.array([[[0.5, 1.0, 0.001, 1.0]]], f)          # albedo below 0.01 demodulates by 1
    V = R.variance_of_mean(S, Q, 4, 2, A)
    assert V.dtype == np.float32 and V[0, 0] == f(0.25 / 0.25 + 0.25 + 0.25)
    # the numpy variance of the batch means / B agrees: means (0.5, 1.0) -> var(ddof 1) / 2 = 0.0625 ... per unit albedo
    assert np.isclose(np.var([2 / 2, 4 / 2], ddof=1) / 2, 0.25)
    # identical batches: Q - S^2 / B cancels to 0 (or rounds below it): V = 0, never negative
    S = np.full((1, 1, 4), 0.3 * 4, f); Q = R.moments_from_partial_sums([np.full((1, 1, 4), 0.3 * (j + 1), f) for j in range(4)])
    assert R.variance_of_mean(S, Q, 16, 4, A)[0, 0] >= 0
    # NaN stays NaN (and makes the pixel pass through)
    Qn = Q.copy(); Qn[0, 0, 1] = np.nan
    assert np.isnan(R.variance_of_mean(S, Qn, 16, 4, A)[0, 0])
    assert R.passthrough_mask_var(S, Qn, 16, 4, A)[0, 0] and not R.passthrough_mask_var(S, Q, 16, 4, A)[0, 0]


def _flat_frame(h, w, spp, batches, colour, noise_sigma, seed=1):
    """S, Q of a synthetic frame: per-pixel batch sums around `colour` * spp / batches; flat albedo, normal and depth."""
    f = np.float32
    rng = np.random.default_rng(seed)
    c = spp // batches
    partial = []
    acc = np.zeros((h, w, 4), f)
    for _ in range(batches):
        b = (np.asarray(colour, np.float64) * c + noise_sigma * rng.standard_normal((h, w, 3))).astype(f)
        acc = acc.copy(); acc[..., :3] = (acc[..., :3] + b).astype(f)
        partial.append(acc)
    A = np.zeros((h, w, 4), f); A[..., :3] = 0.5; A[..., 3] = 1.0
    N = np.zeros((h, w, 4), f); N[..., 2] = 1.0; N[..., 3] = 2.0
    return partial[-1], R.moments_from_partial_sums(partial), A, N


def test_zero_iterations_is_the_identity_up_to_rounding():
    S, Q, A, N = _flat_frame(12, 20, 16, 4, (0.4, 0.3, 0.2), 0.3)
    A[..., :3] = np.random.default_rng(2).uniform(0.05, 0.9, (12, 20, 3)).astype(np.float32)
    out, skip, _ = R.denoise_var(S, Q, 16, 4, A, N, iterations=0)
    assert not skip.any()
    np.testing.assert_allclose(out[..., :3], S[..., :3], rtol=4e-7)       # spp * a * ((S / spp) / a): three f32 roundings
    assert np.array_equal(out[..., 3], S[..., 3])


def test_a_constant_image_is_a_fixed_point():
    S, Q, A, N = _flat_frame(16, 16, 16, 4, (0.4, 0.3, 0.2), 0.0)
    out, skip, L, v = R.denoise_var(S, Q, 16, 4, A, N, iterations=3, return_variance=True)
    assert not skip.any() and L > 0
    np.testing.assert_allclose(out[..., :3], S[..., :3].astype(np.float64), rtol=1e-6)
    assert np.all(v <= 1e-12)
    black = np.zeros_like(S)
    out, skip, L = R.denoise_var(black, black, 16, 4, A, N, iterations=2)  # L = 0 and V = 0: the quotient stays defined
    assert L == 0 and np.array_equal(out, black.astype(np.float64))


def test_an_edge_between_flat_regions_without_variance_is_kept_exactly():
    f = np.float32
    h, w = 16, 24
    S = np.zeros((h, w, 4), f)
    S[:, :12, :3] = (f(1.6), f(3.2), f(4.8)); S[:, 12:, :3] = (f(6.4), f(1.6), f(0.8))
    Q = np.zeros((h, w, 4), f)
    Q[..., :3] = (S[..., :3] / f(4)) ** 2 * f(4)          # four equal batch sums: Q = S^2 / B exactly, V = 0
    A = np.zeros((h, w, 4), f); A[..., :3] = 0.5; A[..., 3] = 1.0
    N = np.zeros((h, w, 4), f); N[..., 2] = 1.0; N[..., 3] = 2.0
    assert np.all(R.variance_of_mean(S, Q, 16, 4, A) == 0)
    out, skip, L = R.denoise_var(S, Q, 16, 4, A, N, iterations=5)
    # the colour weight across the edge is exp(-|de| / (1e-3 L)) = exp(-thousands) = 0: no tap crosses it
    np.testing.assert_allclose(out[..., :3], S[..., :3].astype(np.float64), rtol=1e-6)


def test_equal_variance_on_a_flat_region_shrinks_by_the_kernel_norm():
    """All edge-stopping weights 1 (sigma_var huge, flat features): one iteration leaves V (sum_k h_k^2)^2 = V (70/256)^2
    away from the border, the variance of a B3-spline average of independent pixels."""
    h = w = 12
    f = np.float32
    S, _, A, N = _flat_frame(h, w, 16, 4, (0.4, 0.3, 0.2), 0.0)
    Q = np.zeros((h, w, 4), f)
    Q[..., :3] = ((S[..., :3] * S[..., :3]) / f(4) + f(0.75)).astype(f)   # the same excess everywhere
    V0 = R.variance_of_mean(S, Q, 16, 4, A)
    assert np.all(V0 == V0[0, 0]) and V0[0, 0] > 0
    _, _, _, v = R.denoise_var(S, Q, 16, 4, A, N, iterations=1, sigma_var=1e9, sigma_normal=0.0, return_variance=True)
    assert np.isclose((H5 ** 2).sum(), 70.0 / 256.0)
    np.testing.assert_allclose(v[2:-2, 2:-2], float(V0[0, 0]) * (70.0 / 256.0) ** 2, rtol=1e-9)
    assert np.all(v[0, :] > v[5, 5])                      # fewer taps at the border: less averaging
