"""Adaptive sampling without a GPU: the C ABI (symbols, struct layouts, argument checks that fire before any HIP call), the
Python wrappers' own checks, and properties of the numpy restatement of the schedule (tests/adaptive_ref.py)."""
import ctypes

import numpy as np
import pytest

import adaptive_ref as R

NEW_SYMBOLS = ("pt_render_adaptive", "pt_render_adaptive_device")


def _err(api):
    return api.lib().pt_last_error().decode()


def _cam(api, w=16, h=8):
    return api.make_camera(True, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 45.0, w, h)


def test_new_symbols_are_exported(api):
    L = api.lib()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    assert L.pt_api_version() == 1


def test_params_and_stats_layouts(api):
    assert ctypes.sizeof(api.AdaptiveParams) == 16
    assert [api.AdaptiveParams.min_spp.offset, api.AdaptiveParams.max_spp.offset, api.AdaptiveParams.chunk_spp.offset,
            api.AdaptiveParams.threshold.offset] == [0, 4, 8, 12]
    assert ctypes.sizeof(api.AdaptiveStats) == 16 and ctypes.alignment(api.AdaptiveStats) == 8
    assert [api.AdaptiveStats.rounds.offset, api.AdaptiveStats.tiles_at_max.offset, api.AdaptiveStats.pixel_samples.offset] == [0, 4, 8]
    p = api.adaptive_params(4, 64, 8, 0.25)
    assert (p.min_spp, p.max_spp, p.chunk_spp) == (4, 64, 8) and np.float32(p.threshold) == np.float32(0.25)


def _cases(api, buf, spp, cam):
    P = lambda mn, mx, c, t: ctypes.byref(api.AdaptiveParams(mn, mx, c, t))          # noqa: E731
    ok = P(4, 16, 2, 0.1)
    return [
        ((None, ctypes.byref(cam), 0, 8, 4, 0, 1, 1, ok, buf, spp, None, None), "image size", -1),
        ((None, ctypes.byref(cam), 16, -2, 4, 0, 1, 1, ok, buf, spp, None, None), "image size", -1),
        ((None, ctypes.byref(cam), 70000, 70000, 4, 0, 1, 1, ok, buf, spp, None, None), "too large", -1),
        ((None, ctypes.byref(cam), 16, 8, 4, 0, 1, 1, None, buf, spp, None, None), "null params", -1),
        ((None, ctypes.byref(cam), 16, 8, 4, 0, 1, 1, P(0, 1, 1, 0.1), buf, spp, None, None), "max_spp 1", -1),
        ((None, ctypes.byref(cam), 16, 8, 4, 0, 1, 1, P(-1, 8, 1, 0.1), buf, spp, None, None), "min_spp -1", -1),
        ((None, ctypes.byref(cam), 16, 8, 4, 0, 1, 1, P(9, 8, 1, 0.1), buf, spp, None, None), "min_spp 9", -1),
        ((None, ctypes.byref(cam), 16, 8, 4, 0, 1, 1, P(0, 8, 0, 0.1), buf, spp, None, None), "chunk_spp 0", -1),
        ((None, ctypes.byref(cam), 16, 8, 4, 0, 1, 1, P(0, 8, 1, float("nan")), buf, spp, None, None), "threshold", -1),
        ((None, ctypes.byref(cam), 16, 8, 4, 0, 1, 1, P(0, 8, 1, -0.5), buf, spp, None, None), "threshold", -1),
        ((None, ctypes.byref(cam), 16, 8, 4, 1, 1, 1, ok, buf, spp, None, None), "integrator 1", -3),
        ((None, None, 16, 8, 4, 0, 1, 1, ok, buf, spp, None, None), "null camera", -1),
        ((None, ctypes.byref(cam), 16, 8, 4, 0, 1, 1, ok, None, spp, None, None), "null output", -1),
        ((None, ctypes.byref(cam), 16, 8, 4, 0, 1, 1, ok, buf, None, None, None), "null output", -1),
        ((None, ctypes.byref(cam), 16, 8, 4, 0, 1, 1, ok, buf, spp, None, None), "null scene", -1),
    ]


def test_argument_checks_both_forms(api):
    L = api.lib()
    col = np.zeros((8, 16, 4), np.float32)
    spp = np.zeros((1, 2), np.int32)
    cam = _cam(api)
    for args, msg, code in _cases(api, col.ctypes.data, spp.ctypes.data, cam):
        assert L.pt_render_adaptive(*args) == code, (args, _err(api))
        assert msg in _err(api) and _err(api).startswith("pt_render_adaptive"), (msg, _err(api))
        assert L.pt_render_adaptive_device(*args, None) == code, (args, _err(api))
        assert msg in _err(api), (msg, _err(api))
    # an infinite threshold (every tile stops at its first chance) is a valid value: the next check to fire is the scene's
    args = (None, ctypes.byref(cam), 16, 8, 4, 0, 1, 1, ctypes.byref(api.AdaptiveParams(0, 8, 1, float("inf"))), col.ctypes.data,
            spp.ctypes.data, None, None)
    assert L.pt_render_adaptive(*args) == -1 and "null scene" in _err(api)


def test_python_wrappers_reject_bad_shapes_and_dtypes(api):
    col = np.zeros((12, 20, 4), np.float32)
    spp = np.full((2, 3), 4, np.int32)
    m = api.adaptive_mean(col, spp)
    assert m.shape == col.shape and m.dtype == np.float32
    for c, s in [(col.astype(np.float64), spp), (col[..., :3], spp), (col.reshape(-1, 4), spp), ([[0.0] * 4], spp),
                 (col, spp.astype(np.int64)), (col, spp[:, :2]), (col, spp.T.copy()), (col, np.zeros((2, 3), np.int32))]:
        with pytest.raises(api.PtError):
            api.adaptive_mean(c, s)


def test_adaptive_mean_divides_by_the_tile_count(api):
    rng = np.random.default_rng(3)
    col = rng.random((12, 20, 4)).astype(np.float32)
    spp = np.array([[2, 4, 6], [8, 10, 12]], np.int32)
    m = api.adaptive_mean(col, spp)
    for y in range(12):
        for x in range(20):
            assert np.array_equal(m[y, x], col[y, x] / np.float32(spp[y // 8, x // 8]))


# ---- properties of the restatement ----------------------------------------------------------------------------------------
def _noisy(w, h, seed=1):
    """frame_at(n) of a synthetic renderer: per-pixel sums of n iid samples (the streams are per pixel, so frame_at(n) is a
    prefix of frame_at(m) for n < m), mean set per region so that tiles converge at different speeds."""
    rng = np.random.default_rng(seed)
    mean = (0.2 + rng.random((h, w, 1))).astype(np.float32)
    spread = np.where(np.arange(w)[None, :, None] < w // 2, 0.05, 2.0).astype(np.float32)
    draws = (mean + spread * rng.standard_normal((512, h, w, 3))).clip(0).astype(np.float32)
    cache = {}

    def frame_at(n):
        if n not in cache:
            s = np.zeros((h, w, 4), np.float32)
            for k in range(n):
                s[..., :3] += draws[k]
            cache[n] = s
        return cache[n]
    return frame_at


def test_noise_free_frame_stops_every_tile_at_the_first_round_past_min_spp():
    w, h = 24, 20
    const = np.zeros((h, w, 4), np.float32)
    const[..., :3] = 0.5
    r = R.replay(lambda n: const * np.float32(n), w, h, min_spp=10, max_spp=64, chunk_spp=2, threshold=1e-6)
    assert (r["tile_spp"] == 12).all() and r["rounds"] == 3 and (r["tile_err"] == 0).all()
    r = R.replay(lambda n: const * np.float32(n), w, h, min_spp=0, max_spp=64, chunk_spp=2, threshold=1e-6)
    assert (r["tile_spp"] == 4).all() and r["rounds"] == 1


def test_threshold_zero_gives_max_spp_everywhere():
    w, h = 20, 12
    fa = _noisy(w, h)
    r = R.replay(fa, w, h, min_spp=0, max_spp=16, chunk_spp=3, threshold=0.0)
    assert (r["tile_spp"] == 16).all()
    assert r["ns"] == [6, 12, 16]                                  # c = 3, 3, then the budget: (16 - 12) / 2 = 2
    assert np.array_equal(r["colors"].view(np.uint32), fa(16).view(np.uint32))
    assert R.stats(r["tile_spp"], w, h, 16) == (6, 16 * w * h)


def test_budget_cut_for_an_odd_max_spp():
    w, h = 16, 8
    r = R.replay(_noisy(w, h), w, h, min_spp=0, max_spp=7, chunk_spp=2, threshold=0.0)
    assert r["ns"] == [4, 6] and (r["tile_spp"] == 6).all()
    r = R.replay(_noisy(w, h), w, h, min_spp=7, max_spp=7, chunk_spp=8, threshold=1e30)
    assert r["ns"] == [6] and (r["tile_spp"] == 6).all()


def test_a_nan_pixel_never_holds_its_tile_back():
    w, h = 16, 16
    const = np.zeros((h, w, 4), np.float32)
    const[..., :3] = 0.5

    def fa(n):
        f = const * np.float32(n)
        f[3, 5, 1] = np.nan                                        # tile 0
        f[9, 12, 0] = np.inf                                       # tile 3
        return f
    r = R.replay(fa, w, h, min_spp=0, max_spp=32, chunk_spp=2, threshold=1e-6)
    assert (r["tile_spp"] == 4).all() and (r["tile_err"] == 0).all()
    assert np.isnan(r["colors"][3, 5, 1]) and np.isinf(r["colors"][9, 12, 0])


def test_noisy_tiles_take_more_samples_and_the_threshold_picker_spreads_rounds():
    w, h = 32, 16
    fa = _noisy(w, h)
    t = R.pick_threshold(fa, w, h, 4, 64, 4)
    assert t is not None
    r = R.replay(fa, w, h, 4, 64, 4, t)
    assert np.unique(r["tile_spp"]).size >= 3
    assert r["tile_spp"][:, :2].mean() < r["tile_spp"][:, 2:].mean()  # the quiet left half stops first
    # every tile's sums are the frame at its own count; every tile's error is below the threshold or it ran to the end
    for (j, i), n in np.ndenumerate(r["tile_spp"]):
        assert np.array_equal(r["colors"][8 * j:8 * j + 8, 8 * i:8 * i + 8], fa(int(n))[8 * j:8 * j + 8, 8 * i:8 * i + 8])
        assert r["tile_err"][j, i] < np.float32(t) or n == r["ns"][-1]


def test_pixel_error_follows_the_stated_order():
    S = np.array([[[3.0, 1.0, 0.25]]], np.float32)
    H = np.array([[[1.0, 1.0, 0.0]]], np.float32)
    d = np.float32(1.0) + np.float32(1.0) + np.float32(0.25)
    inv = np.float32(1) / np.float32(6)
    want = (d * inv) / (np.float32(1e-4) + np.sqrt(np.float32(4.25) * inv))
    assert R.pixel_error(S, H, 6)[0, 0] == want
    assert R.pixel_error(S * np.float32(np.nan), H, 6)[0, 0] == 0
    assert R.pixel_error(-S, H, 6)[0, 0] == 0                      # sqrt of a negative sum: NaN, counts as 0
