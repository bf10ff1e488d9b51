"""Adaptive frames with their variance, without a GPU: the C ABI of pt_render_adaptive_moments and pt_denoise_var_tiles (symbols,
argument checks that fire before any HIP call), the Python wrappers' own checks, and the numpy restatement
(tests/adaptive_moments_ref.py) against the restatements it is built on."""
import ctypes

import numpy as np
import pytest

import adaptive_moments_ref as R
import adaptive_ref
from denoise_var_ref import denoise_var, moments_from_partial_sums
from test_abi import _declared_functions

NEW_SYMBOLS = ("pt_render_adaptive_moments", "pt_render_adaptive_moments_device", "pt_denoise_var_tiles", "pt_denoise_var_tiles_device",
               "pt_denoise_var_tiles_workspace_bytes", "pt_probe_adaptive_moments")


def _err(api):
    return api.lib().pt_last_error().decode()


def _cam(api, w=16, h=8):
    return api.make_camera(True, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 45.0, w, h)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported(api):
    L = api.lib()
    declared = _declared_functions()
    for n in NEW_SYMBOLS:
        assert n in declared, n
        assert hasattr(L, n), n
    assert all(hasattr(api.Scene, n) for n in ("render_adaptive_moments", "render_adaptive_moments_device"))
    assert all(hasattr(api, n) for n in ("denoise_var_tiles", "denoise_var_tiles_device", "denoise_var_tiles_workspace_bytes"))
    assert L.pt_api_version() == 1


@pytest.mark.parametrize("w,h", [(1, 1), (61, 43), (257, 1), (1920, 1080), (0, 10), (10, -1)])
def test_workspace_is_pt_denoise_var_devices(api, w, h):
    assert api.denoise_var_tiles_workspace_bytes(w, h) == api.denoise_var_workspace_bytes(w, h)


def test_render_adaptive_moments_argument_checks_both_forms(api):
    L = api.lib()
    col = np.zeros((8, 16, 4), np.float32)
    sq = np.zeros((8, 16, 4), np.float32)
    spp = np.zeros((1, 2), np.int32)
    cam = ctypes.byref(_cam(api))
    c, q, t = col.ctypes.data, sq.ctypes.data, spp.ctypes.data
    P = lambda mn, mx, ch, th: ctypes.byref(api.AdaptiveParams(mn, mx, ch, th))          # noqa: E731
    ok = P(4, 16, 2, 0.1)
    # (scene, camera, w, h, max_depth, integrator, use_mis, seed, params, S, Q, tile_spp, tile_err, stats)
    cases = [
        # pt_render_adaptive's own checks, in its order
        ((None, cam, 0, 8, 4, 0, 1, 1, ok, c, q, t, None, None), "image size", -1),
        ((None, cam, 70000, 70000, 4, 0, 1, 1, ok, c, q, t, None, None), "too large", -1),
        ((None, cam, 16, 8, 4, 0, 1, 1, None, c, q, t, None, None), "null params", -1),
        ((None, cam, 16, 8, 4, 0, 1, 1, P(0, 1, 1, 0.1), c, q, t, None, None), "max_spp 1", -1),
        ((None, cam, 16, 8, 4, 0, 1, 1, P(9, 8, 1, 0.1), c, q, t, None, None), "min_spp 9", -1),
        ((None, cam, 16, 8, 4, 0, 1, 1, P(0, 18, 0, 0.1), c, q, t, None, None), "chunk_spp 0", -1),        # (before the new check divides by it)
        ((None, cam, 16, 8, 4, 0, 1, 1, P(0, 18, 4, float("nan")), c, q, t, None, None), "threshold", -1),
        # the new check: every half-round must render chunk_spp samples
        ((None, cam, 16, 8, 4, 0, 1, 1, P(4, 18, 4, 0.1), c, q, t, None, None), "max_spp 18 must be a multiple of 2 * chunk_spp (8)", -1),
        ((None, cam, 16, 8, 4, 0, 1, 1, P(0, 7, 2, 0.1), c, q, t, None, None), "max_spp 7 must be a multiple of 2 * chunk_spp (4)", -1),
        ((None, cam, 16, 8, 4, 0, 1, 1, P(0, 6, 2, 0.1), c, q, t, None, None), "max_spp 6 must be a multiple of 2 * chunk_spp (4)", -1),
        ((None, cam, 16, 8, 4, 1, 1, 1, P(4, 18, 4, 0.1), c, q, t, None, None), "multiple of 2 * chunk_spp", -1),     # before the integrator's
        ((None, cam, 16, 8, 4, 1, 1, 1, ok, c, q, t, None, None), "integrator 1", -3),
        ((None, None, 16, 8, 4, 0, 1, 1, ok, c, q, t, None, None), "null camera", -1),
        ((None, cam, 16, 8, 4, 0, 1, 1, ok, None, q, t, None, None), "null output", -1),
        ((None, cam, 16, 8, 4, 0, 1, 1, ok, c, None, t, None, None), "null output", -1),                   # the new output
        ((None, cam, 16, 8, 4, 0, 1, 1, ok, c, q, None, None, None), "null output", -1),
        ((None, cam, 16, 8, 4, 0, 1, 1, ok, c, q, t, None, None), "null scene", -1),
        ((None, cam, 16, 8, 4, 0, 1, 1, P(8, 32, 4, 0.1), c, q, t, None, None), "null scene", -1),         # 32 = 4 * 8: accepted
    ]
    for args, msg, code in cases:
        assert L.pt_render_adaptive_moments(*args) == code, (args, _err(api))
        assert msg in _err(api) and _err(api).startswith("pt_render_adaptive"), (msg, _err(api))
        assert L.pt_render_adaptive_moments_device(*args, None) == code, (args, _err(api))
        assert msg in _err(api), (msg, _err(api))
    # pt_render_adaptive itself still takes an odd budget: the next check to fire is the scene's
    args = (None, cam, 16, 8, 4, 0, 1, 1, P(4, 18, 4, 0.1), c, t, None, None)
    assert L.pt_render_adaptive(*args) == -1 and "null scene" in _err(api)
    assert not col.any() and not sq.any() and not spp.any()


def test_probe_argument_checks(api):
    L = api.lib()
    ms = ctypes.c_float(-1.0)
    for args, msg in [((0, 8, 1, 1, ctypes.byref(ms)), "image size"), ((16, 8, 0, 1, ctypes.byref(ms)), "live 0 must lie in 1..2"),
                      ((16, 8, 3, 1, ctypes.byref(ms)), "live 3 must lie in 1..2"), ((16, 8, 2, 0, ctypes.byref(ms)), "reps 0"),
                      ((16, 8, 2, 1, None), "null output")]:
        assert L.pt_probe_adaptive_moments(*args) == -1 and msg in _err(api), (args, _err(api))
    assert ms.value == -1.0


def test_denoise_var_tiles_argument_checks(api):
    L = api.lib()
    buf = np.zeros((8, 16, 4), np.float32)
    p = buf.ctypes.data
    good_map = np.full((1, 2), 8, np.int32)
    m = good_map.ctypes.data
    good = api.DenoiseVarParams(5, 6.0, 64.0, 0.1)

    def params(**kw):
        q = api.DenoiseVarParams(good.iterations, good.sigma_var, good.sigma_normal, good.sigma_depth)
        for k, v in kw.items():
            setattr(q, k, v)
        return ctypes.byref(q)

    def tiles(a, b):
        arr = np.array([[a, b]], np.int32)
        keep.append(arr)
        return arr.ctypes.data
    keep = []

    # (w, h, S, Q, tile_spp, batch_spp, albedo, normal_depth, params, out)
    both = [
        ((0, 8, p, p, m, 2, p, p, params(), p), "size"),
        ((16, 0, p, p, m, 2, p, p, params(), p), "size"),
        ((70000, 70000, p, p, m, 2, p, p, params(), p), "too large"),
        ((16, 8, None, p, m, 2, p, p, params(), p), "null buffer"),
        ((16, 8, p, None, m, 2, p, p, params(), p), "null buffer"),
        ((16, 8, p, p, m, 2, None, p, params(), p), "null buffer"),
        ((16, 8, p, p, m, 2, p, None, params(), p), "null buffer"),
        ((16, 8, p, p, m, 2, p, p, params(), None), "null buffer"),
        ((16, 8, p, p, m, 2, p, p, params(iterations=-1), p), "iterations"),
        ((16, 8, p, p, m, 2, p, p, params(iterations=17), p), "iterations"),
        ((16, 8, p, p, m, 2, p, p, params(sigma_var=0.0), p), "sigma_var"),
        ((16, 8, p, p, m, 2, p, p, params(sigma_normal=-1.0), p), "sigma_normal"),
        ((16, 8, p, p, m, 2, p, p, params(sigma_depth=float("inf")), p), "sigma_depth"),
        ((16, 8, p, p, m, 0, p, p, params(), p), "batch_spp 0 must be positive"),
        ((16, 8, p, p, m, -2, p, p, params(), p), "batch_spp -2 must be positive"),
        ((16, 8, p, p, None, 2, p, p, params(), p), "null tile map"),
    ]
    for args, msg in both:
        assert L.pt_denoise_var_tiles(*args) == -1, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_denoise_var_tiles_device(*args[:-1], p, args[-1], None) == -1, args
        assert msg in _err(api), (args, _err(api))
    assert L.pt_denoise_var_tiles_device(16, 8, p, p, m, 2, p, p, params(), None, p, None) == -1 and "null workspace" in _err(api)
    # the host form reads its map: no samples, no multiple of batch_spp, a single batch (B = 1 has no variance)
    host = [
        ((16, 8, p, p, tiles(8, 0), 2, p, p, params(), p), "tile_spp[1] = 0"),
        ((16, 8, p, p, tiles(-4, 8), 2, p, p, params(), p), "tile_spp[0] = -4"),
        ((16, 8, p, p, tiles(8, 3), 2, p, p, params(), p), "tile_spp[1] = 3"),
        ((16, 8, p, p, tiles(2, 8), 2, p, p, params(), p), "tile_spp[0] = 2"),
        ((16, 8, p, p, tiles(8, 8), 8, p, p, params(), p), "tile_spp[0] = 8"),
    ]
    for args, msg in host:
        assert L.pt_denoise_var_tiles(*args) == -1, args
        assert msg in _err(api) and _err(api).startswith("pt_denoise_var_tiles"), (args, _err(api))
    assert not buf.any()


def test_python_wrapper_rejects_bad_maps_and_frames(api):
    f = np.zeros((12, 20, 4), np.float32)
    good = np.full((2, 3), 8, np.int32)
    for tm in (good.astype(np.int64), good[:, :2], good.T.copy(), [[8] * 3] * 2, None):
        with pytest.raises(api.PtError, match="tile_spp"):
            api.denoise_var_tiles(f, f, tm, 2, f, f)
    with pytest.raises(api.PtError):
        api.denoise_var_tiles(f.astype(np.float64), f, good, 2, f, f)
    with pytest.raises(api.PtError, match="shapes differ"):
        api.denoise_var_tiles(f, f[:8], good, 2, f, f)
    with pytest.raises(api.PtError, match="out must be"):
        api.denoise_var_tiles(f, f, good, 2, f, f, out=np.zeros((12, 20, 3), np.float32))
    with pytest.raises(api.PtError, match=r"tile_spp\[0\] = 8"):         # the library's own check of the map, through the wrapper
        api.denoise_var_tiles(f, f, good, 8, f, f)


# ---- the restatement against the restatements it is built on ---------------------------------------------------------------------
def _noisy(w, h, seed=1):
    """frame_at(n) of a synthetic renderer: per-pixel sums of n iid samples (frame_at(n) is a prefix of frame_at(m) for n < m),
    the left half quiet and the right half noisy, so tiles stop in different rounds."""
    rng = np.random.default_rng(seed)
    mean = (0.2 + rng.random((h, w, 1))).astype(np.float32)
    spread = np.where(np.arange(w)[None, :, None] < w // 2, 0.05, 2.0).astype(np.float32)
    draws = (mean + spread * rng.standard_normal((64, h, w, 3))).clip(0).astype(np.float32)
    cache = {}

    def frame_at(n):
        if n not in cache:
            s = np.zeros((h, w, 4), np.float32)
            for k in range(n):
                s[..., :3] += draws[k]
            cache[n] = s
        return cache[n]
    return frame_at


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_replay_moments_with_threshold_zero_is_moments_over_all_batches():
    w, h = 21, 13
    fa = _noisy(w, h)
    r = R.replay_moments(fa, w, h, 4, 16, 2, 0.0)
    assert (r["tile_spp"] == 16).all()
    want = moments_from_partial_sums([fa(2 * j) for j in range(1, 9)])
    assert np.array_equal(_bits(r["sq"]), _bits(want)) and (r["sq"][..., 3] == 8).all()
    assert np.array_equal(_bits(r["colors"]), _bits(fa(16)))
    plain = adaptive_ref.replay(fa, w, h, 4, 16, 2, 0.0)
    assert np.array_equal(_bits(plain["tile_err"]), _bits(r["tile_err"]))


def test_replay_moments_gives_every_tile_the_moments_at_its_own_count():
    w, h = 37, 19                                                        # ragged last tile row and column
    fa = _noisy(w, h)
    t = adaptive_ref.pick_threshold(fa, w, h, 4, 32, 2)
    assert t is not None
    r = R.replay_moments(fa, w, h, 4, 32, 2, t)
    assert np.unique(r["tile_spp"]).size >= 3
    for (j, i), n in np.ndenumerate(r["tile_spp"]):
        want = moments_from_partial_sums([fa(2 * k) for k in range(1, int(n) // 2 + 1)])
        sl = (slice(8 * j, 8 * j + 8), slice(8 * i, 8 * i + 8))
        assert np.array_equal(_bits(r["sq"][sl]), _bits(want[sl]))
        assert (r["sq"][sl][..., 3] == n // 2).all()
    with pytest.raises(AssertionError):
        R.replay_moments(fa, w, h, 4, 18, 4, t)                          # batches of unequal size: the entry point refuses them too


def _frame(w, h, spp, batches, seed=5):
    """A frame with moments, guides, a miss region, a NaN and an Inf: S and Q of `batches` batch sums per pixel."""
    rng = np.random.default_rng(seed)
    batch = (0.5 + 0.3 * rng.standard_normal((batches, h, w, 3))).clip(0).astype(np.float32) * np.float32(spp / batches)
    S = np.zeros((h, w, 4), np.float32)
    S[..., :3] = batch.sum(0, dtype=np.float32)
    Q = np.zeros((h, w, 4), np.float32)
    Q[..., :3] = (batch * batch).sum(0, dtype=np.float32)
    Q[..., 3] = batches
    A = np.ones((h, w, 4), np.float32)
    A[..., :3] = (0.2 + 0.6 * rng.random((h, w, 3))).astype(np.float32)
    A[2:5, 3:9, 3] = 0.0
    N = np.zeros((h, w, 4), np.float32)
    N[..., 2] = 1.0
    N[:, w // 2:, :3] = (0.0, 0.6, 0.8)
    N[..., 3] = (2.0 + 0.01 * np.arange(w)[None, :]).astype(np.float32)
    S[7, 11, 0] = np.nan
    S[9, 2, 1] = np.inf
    return S, Q, A, N


def test_a_uniform_map_is_the_scalar_restatement_bit_for_bit():
    w, h = 29, 18
    S, Q, A, N = _frame(w, h, 8, 4)
    tm = np.full(((h + 7) // 8, (w + 7) // 8), 8, np.int32)
    for it in (0, 2):
        want, skip0, L0, v0 = denoise_var(S, Q, 8, 4, A, N, iterations=it, return_variance=True)
        got, skip1, L1, v1 = R.denoise_var_tiles(S, Q, tm, 2, A, N, iterations=it, return_variance=True)
        assert np.array_equal(skip0, skip1) and L0 == L1 and skip0[7, 11] and skip0[9, 2] and skip0[2:5, 3:9].all()
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got.view(np.uint64)[~np.isnan(got)], want.view(np.uint64)[~np.isnan(want)])
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(v0.view(np.uint64), v1.view(np.uint64))


def test_the_map_is_read_per_tile_with_the_frames_own_tile_columns():
    """Constant S and constant per-sample variance: V differs between the tiles of a checkerboard map by the factor the counts
    imply, and a pixel reads tile (y // 8) * ceil(w / 8) + x // 8 (w = 29: four tile columns, not three)."""
    w, h = 29, 18
    ty, tx = (h + 7) // 8, (w + 7) // 8
    tm = np.where((np.arange(ty)[:, None] + np.arange(tx)[None, :]) % 2 == 0, 8, 16).astype(np.int32)
    n = R.pixel_map(tm, w, h).astype(np.float32)
    assert n.shape == (h, w) and n[0, 7] == 8 and n[0, 8] == 16 and n[8, 0] == 16 and n[17, 28] == tm[2, 3]
    S = np.zeros((h, w, 4), np.float32)
    Q = np.zeros((h, w, 4), np.float32)
    B = n / 2                                                            # batches of 2 samples, alternately 0 and 2 in sum: mean 1/2
    S[..., :3] = (B / 2 * 2)[..., None]
    Q[..., :3] = (B / 2 * 4)[..., None]
    A = np.ones((h, w, 4), np.float32)
    N = np.zeros((h, w, 4), np.float32)
    N[..., 2] = 1.0
    N[..., 3] = 2.0
    out, skip, L, v = R.denoise_var_tiles(S, Q, tm, 2, A, N, iterations=0, return_variance=True)
    assert not skip.any() and np.allclose(out[..., :3], S[..., :3])
    # per channel: batch variance 1 (sums 0 / 2 around 1) times B / (B - 1), over B batches, over c^2 = 4; three channels
    want = 3.0 * (B / (B - 1)) / B / 4.0
    np.testing.assert_allclose(v, want, rtol=1e-6)
    assert np.isclose(v[0, 7] / v[0, 8], (1 / 3) / (1 / 7)) and np.isclose(v[7, 0] / v[8, 0], (1 / 3) / (1 / 7))
