"""The converge stages without a GPU: the C ABI and the Python wrappers (symbols, struct layout, defaults, the argument checks that
must fire before any HIP call), and the numpy restatement itself (tests/converge_ref.py) on hand-made histories with a known
answer."""
import ctypes

import numpy as np
import pytest

import converge_ref as R

NEW_SYMBOLS = ("pt_converge_defaults", "pt_temporal_select", "pt_temporal_select_device", "pt_render_moments_tiles",
               "pt_render_moments_tiles_device", "pt_temporal_accumulate_live", "pt_temporal_accumulate_live_device",
               "pt_preview_set_converge", "pt_preview_last_live", "pt_preview_read_tiles")
f32 = np.float32


def _err(api):
    return api.lib().pt_last_error().decode()


def _cam(api, w=16, h=8, pos=(0.0, 0.0, 3.0)):
    return api.make_camera(True, pos, (0.0, 0.0, 0.0), 45.0, w, h)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported(api):
    L = api.lib()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    assert L.pt_api_version() == 1
    for name in ("ConvergeParams", "converge_defaults", "temporal_select", "temporal_select_device", "temporal_accumulate_live",
                 "temporal_accumulate_live_device"):
        assert hasattr(api, name), name
    for name in ("render_moments_tiles", "render_moments_tiles_device"):
        assert hasattr(api.Scene, name), name
    for name in ("set_converge", "last_live", "read_tiles"):
        assert hasattr(api.Preview, name), name


def test_converge_params_layout_and_defaults(api):
    P = api.ConvergeParams
    assert ctypes.sizeof(P) == 8
    assert [P.threshold.offset, P.min_history.offset] == [0, 4]
    buf = (ctypes.c_uint8 * 32)(*([0xAB] * 32))           # the C side writes exactly 8 bytes
    api.lib().pt_converge_defaults(ctypes.cast(buf, ctypes.POINTER(P)))
    assert bytes(buf[8:]) == b"\xab" * 24
    p = P.from_buffer_copy(bytes(buf[:8]))
    d = api.converge_defaults()
    assert d == {"threshold": p.threshold, "min_history": p.min_history}
    assert d["min_history"] == R.DEFAULTS["min_history"] == 8 and f32(d["threshold"]) == f32(R.DEFAULTS["threshold"]) and d["threshold"] > 0
    api.lib().pt_converge_defaults(None)                  # ignored
    assert api.temporal_defaults()["max_history"] == 32   # pt_temporal_accumulate's own defaults are untouched


def test_temporal_select_argument_checks(api):
    L = api.lib()
    w, h = 16, 8                                          # T = 2
    hist = np.zeros((h, w, 4), f32); ln = np.zeros((h, w), f32)
    out = np.full(16, 7, np.int32)                        # err, live, list, count at [0:2], [4:6], [8:10], [12]
    H, N, o = hist.ctypes.data, ln.ctypes.data, out.ctypes.data
    E, V, I, K = o, o + 16, o + 32, o + 48

    def params(threshold=0.05, min_history=4):
        return ctypes.byref(api.ConvergeParams(threshold, min_history))

    # (w, h, hist, hist_len, params, tile_err, tile_live, list, count)
    cases = [
        ((0, h, H, N, params(), E, V, I, K), "size"),
        ((w, -2, H, N, params(), E, V, I, K), "size"),
        ((65536, 65536, H, N, params(), E, V, I, K), "too large"),
        ((w, h, None, N, params(), E, V, I, K), "null buffer"),
        ((w, h, H, None, params(), E, V, I, K), "null buffer"),
        ((w, h, H, N, params(), None, V, I, K), "null output"),
        ((w, h, H, N, params(), E, None, I, K), "null output"),
        ((w, h, H, N, params(), E, V, None, K), "null output"),
        ((w, h, H, N, params(), E, V, I, None), "null output"),
        ((w, h, H, N, params(threshold=-0.1), E, V, I, K), "threshold"),
        ((w, h, H, N, params(threshold=float("nan")), E, V, I, K), "threshold"),
        ((w, h, H, N, params(threshold=float("inf")), E, V, I, K), "threshold"),
        ((w, h, H, N, params(min_history=0), E, V, I, K), "min_history 0"),
        ((w, h, H, N, params(min_history=-3), E, V, I, K), "min_history -3"),
        ((w, h, H, N, params(), H, V, I, K), "alias"),                     # an output on the history
        ((w, h, H, N, params(), E, N + 8, I, K), "alias"),                 # ... inside the lengths
        ((w, h, H, N, params(), E, V, H + w * h * 16 - 4, K), "alias"),    # ... on the history's last bytes
        ((w, h, H, N, params(), E, V, I, N), "alias"),
        ((w, h, H, N, params(), E, E + 4, I, K), "alias"),                 # two outputs on each other
        ((w, h, H, N, params(), E, V, I, I + 4), "alias"),
    ]
    for args, msg in cases:
        assert L.pt_temporal_select(*args) == -1, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_temporal_select_device(*args, None) == -1, args
        assert msg in _err(api), (args, _err(api))
    assert (out == 7).all() and not hist.any()            # nothing ran
    with pytest.raises(api.PtError, match="float32"):
        api.temporal_select(hist.astype(np.float64), ln)
    with pytest.raises(api.PtError, match="hist_len"):
        api.temporal_select(hist, ln[:, :-1])
    with pytest.raises(api.PtError, match="threshold"):
        api.temporal_select(hist, ln, threshold=-1.0)


def test_render_moments_tiles_argument_checks(api):
    L = api.lib()
    w, h = 24, 16                                         # T = 6
    cam = ctypes.byref(_cam(api, w, h))
    S = np.full((h, w, 4), 5, f32); Q = np.full((h, w, 4), 5, f32)
    s, q = S.ctypes.data, Q.ctypes.data

    def lst(*v):
        a = np.array(v, np.int32)
        return a, a.ctypes.data

    ok, okp = lst(0, 2, 5)
    # (scene, cam, w, h, spp, batch_spp, depth, integrator, mis, seed, list, count, S, Q): the scene is NULL throughout, the last check
    both = [
        ((None, cam, 0, h, 4, 2, 4, 0, 1, 1, okp, 3, s, q), "size"),
        ((None, cam, w, h, 4, 2, 4, 0, 1, 1, okp, -1, s, q), "count -1 must lie in 0..6"),
        ((None, cam, w, h, 4, 2, 4, 0, 1, 1, okp, 7, s, q), "count 7 must lie in 0..6"),
        ((None, cam, w, h, 4, 2, 4, 0, 1, 1, None, 2, s, q), "null tile list"),
        ((None, cam, w, h, 0, 2, 4, 0, 1, 1, okp, 3, s, q), "spp 0 must be positive"),
        ((None, cam, w, h, 4, 3, 4, 0, 1, 1, okp, 3, s, q), "multiple of batch_spp 3"),
        ((None, cam, w, h, 4, 4, 4, 0, 1, 1, okp, 3, s, q), "at least 2 batches"),
        ((None, cam, w, h, 4, 2, 4, 1, 1, 1, okp, 3, s, q), "integrator 1"),
        ((None, None, w, h, 4, 2, 4, 0, 1, 1, okp, 3, s, q), "null camera"),
        ((None, cam, w, h + 8, 4, 2, 4, 0, 1, 1, okp, 3, s, q), "camera is 24 x 16"),
        ((None, cam, w, h, 4, 2, 4, 0, 1, 1, okp, 3, None, q), "null output"),
        ((None, cam, w, h, 4, 2, 4, 0, 1, 1, okp, 3, s, None), "null output"),
        ((None, cam, w, h, 4, 2, 4, 0, 1, 1, okp, 3, s, q), "null scene"),
        ((None, cam, w, h, 4, 2, 4, 0, 1, 1, None, 0, s, q), "null scene"),       # an empty list needs no pointer
    ]
    for args, msg in both:
        assert L.pt_render_moments_tiles(*args) < 0, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_render_moments_tiles_device(*args, None) < 0, args
        assert msg in _err(api), (args, _err(api))
    # the host form reads its list: unsorted, duplicate, out of range
    for bad, msg in (((2, 0, 5), "tile_list[1] = 0"), ((0, 2, 2), "tile_list[2] = 2"), ((0, 2, 6), "tile_list[2] = 6"), ((-1, 2, 5), "tile_list[0] = -1")):
        a, p = lst(*bad)
        assert L.pt_render_moments_tiles(None, cam, w, h, 4, 2, 4, 0, 1, 1, p, 3, s, q) == -1
        assert msg in _err(api) and "strictly ascending within 0..5" in _err(api), _err(api)
    assert (S == 5).all() and (Q == 5).all()              # nothing ran


def test_accumulate_live_argument_checks(api):
    L = api.lib()
    w, h = 16, 8
    buf = np.zeros((h, w, 4), f32); other = np.zeros((h, w, 4), f32); ln = np.zeros((h, w), f32); ln2 = np.zeros((h, w), f32)
    live = np.ones(2, np.int32)
    p, o, l, l2, m = buf.ctypes.data, other.ctypes.data, ln.ctypes.data, ln2.ctypes.data, live.ctypes.data
    cam, same, moved = ctypes.byref(_cam(api)), ctypes.byref(_cam(api)), ctypes.byref(_cam(api, pos=(0.1, 0.0, 3.0)))
    par = ctypes.byref(api.TemporalParams(8, 0.05, 0.9))
    # (w, h, cam, cam_prev, S, Q, spp, batches, albedo, nd, prev_nd, hist, hist_len, tile_live, params, out_hist, out_len)
    cases = [
        ((w, h, cam, moved, p, p, 4, 2, p, p, p, p, l, m, par, o, l2), "unchanged camera"),
        ((w, h, cam, None, p, p, 4, 2, p, p, None, None, None, m, par, o, l2), "needs a history"),
        ((w, h, cam, same, p, p, 4, 2, p, p, None, None, None, m, par, o, l2), "needs a history"),
        ((w, h, cam, None, p, p, 4, 2, p, p, p, p, l, o + 32, par, o, l2), "alias the tile map"),
        ((w, h, cam, None, p, p, 4, 2, p, p, p, p, l, l2, par, o, l2), "alias the tile map"),
        # pt_temporal_accumulate's own checks come first
        ((0, h, cam, None, p, p, 4, 2, p, p, p, p, l, m, par, o, l2), "size"),
        ((w, h, cam, None, p, p, 4, 3, p, p, p, p, l, m, par, o, l2), "batches 3 must divide spp 4"),
        ((w, h, None, None, p, p, 4, 2, p, p, p, p, l, m, par, o, l2), "null camera"),
        ((w, h, cam, None, None, p, 4, 2, p, p, p, p, l, m, par, o, l2), "null buffer"),
        ((w, h, cam, None, p, p, 4, 2, p, p, p, p, l, m, par, None, l2), "null output"),
        ((w, h, cam, None, p, p, 4, 2, p, p, p, None, l, m, par, o, l2), "all NULL"),
        ((w, h, cam, None, p, p, 4, 2, p, p, p, o, l, m, par, o, l2), "alias"),
        ((w, h, cam, None, p, p, 4, 2, p, p, p, p, l, m, ctypes.byref(api.TemporalParams(0, 0.05, 0.9)), o, l2), "max_history 0"),
    ]
    for args, msg in cases:
        assert L.pt_temporal_accumulate_live(*args) == -1, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_temporal_accumulate_live_device(*args, None) == -1, args
        assert msg in _err(api), (args, _err(api))
    assert not other.any() and not ln2.any()              # nothing ran
    with pytest.raises(api.PtError, match="tile_live must be an int32 \\[1, 2\\]"):
        api.temporal_accumulate_live(_cam(api), buf, buf, 4, 2, buf, buf, buf, buf, ln, np.ones((2, 2), np.int32))


def test_preview_converge_null_session(api):
    L = api.lib()
    assert L.pt_preview_set_converge(None, None) == -1 and "pt_preview_set_converge: null session" in _err(api)
    assert L.pt_preview_set_converge(None, ctypes.byref(api.ConvergeParams(0.05, 8))) == -1
    n = ctypes.c_int(5)
    assert L.pt_preview_last_live(None, ctypes.byref(n), ctypes.byref(n)) == -1 and "pt_preview_last_live: null session" in _err(api) and n.value == 5
    assert L.pt_preview_read_tiles(None, None, None) == -1 and "pt_preview_read_tiles: null session" in _err(api)


# ---- the restatement on hand-made histories -------------------------------------------------------------------------------------
def _flat(h, w, e=0.25, V=0.0, n=16.0):
    hist = np.zeros((h, w, 4), f32); hist[..., :3] = e; hist[..., 3] = V
    return hist, np.full((h, w), n, f32)


def _r(e, V):
    """r of a grey pixel, float32 step by step."""
    lum = f32(f32(f32(f32(0.2126) * f32(e)) + f32(f32(0.7152) * f32(e))) + f32(f32(0.0722) * f32(e)))
    return f32(np.sqrt(f32(V)) / f32(f32(1e-4) + np.sqrt(lum)))


def test_a_tile_exactly_at_the_threshold_is_live():
    hist, ln = _flat(16, 16)                              # four tiles, all at V = 0: E = 0
    hist[3, 12, 3] = 0.01                                 # tile 1
    hist[10, 2, 3] = 0.0025                               # tile 2
    thr = _r(0.25, 0.01)
    err, live, lst = R.select(hist, ln, float(thr), 8)
    assert err.dtype == f32 and live.dtype == np.int32 and lst.dtype == np.int32
    assert err[0, 1] == thr and err[1, 0] == _r(0.25, 0.0025) and err[0, 0] == 0 and err[1, 1] == 0
    assert live.tolist() == [[0, 1], [0, 0]] and lst.tolist() == [1]          # E == threshold is not below it
    err2, live2, lst2 = R.select(hist, ln, float(np.nextafter(thr, f32(1))), 8)
    assert live2.tolist() == [[0, 0], [0, 0]] and lst2.size == 0 and np.array_equal(err2, err)


def test_threshold_zero_keeps_every_tile_live():
    hist, ln = _flat(16, 24)
    err, live, lst = R.select(hist, ln, 0.0, 1)
    assert not err.any() and live.all() and lst.tolist() == [0, 1, 2, 3, 4, 5]


def test_an_exempt_pixel_does_not_hold_its_tile_back():
    hist, ln = _flat(8, 32, V=1e-6)
    hist[1, 1] = (np.nan, 0.25, 0.25, 1e-6)               # tile 0: NaN colour
    hist[2, 9] = (0.25, 0.25, 0.25, np.inf)               # tile 1: Inf variance
    hist[3, 17] = (5.0, 5.0, 5.0, -1.0)                   # tile 2: pass-through, and it would be young
    ln[3, 17] = 0
    ln[1, 1] = 0                                          # (an exempt pixel is never young)
    hist[4, 25] = (0.25, 0.25, 0.25, np.nan)              # tile 3: NaN variance
    hist[5, 26] = (-1.0, -1.0, -1.0, 1e-6)                # ... and a negative mean: r is NaN, counts as 0
    err, live, lst = R.select(hist, ln, 0.05, 8)
    assert np.isfinite(err).all() and (err == _r(0.25, 1e-6)).all()
    assert not live.any() and lst.size == 0


def test_one_young_pixel_holds_its_tile_back():
    hist, ln = _flat(16, 16, V=1e-6)
    ln[9, 9] = 7                                          # tile 3
    err, live, lst = R.select(hist, ln, 0.05, 8)
    assert live.tolist() == [[0, 0], [0, 1]] and lst.tolist() == [3] and (err < 0.05).all()
    assert not R.select(hist, ln, 0.05, 7)[1].any()       # young means hist_len < min_history
    ln[9, 9] = np.nan                                     # a NaN length is not below anything
    assert not R.select(hist, ln, 0.05, 8)[1].any()


def test_a_partial_edge_tile_ignores_pixels_outside_the_image():
    hist, ln = _flat(11, 13, V=1e-6)                      # 2 x 2 tiles, the right column 5 wide, the top row 3 high
    err, live, lst = R.select(hist, ln, 0.05, 8)
    assert err.shape == (2, 2) and (err == _r(0.25, 1e-6)).all() and not live.any()
    hist[10, 12, 3] = 4.0                                 # the corner tile's last in-image pixel
    err, live, lst = R.select(hist, ln, 0.05, 8)
    assert live.tolist() == [[0, 0], [0, 1]] and lst.tolist() == [3] and err[1, 1] == _r(0.25, 4.0)


def test_accumulate_live_restatement_carries_and_blends(api):
    import temporal_ref as T
    rng = np.random.default_rng(3)
    h, w = 11, 13
    cam = api.make_camera(True, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 45.0, w, h)
    S = rng.uniform(0.5, 2.0, (h, w, 4)).astype(f32)
    Qm = (S * S / 2 * rng.uniform(1.0, 1.2, (h, w, 4))).astype(f32)
    A = np.ones((h, w, 4), f32); N = np.zeros((h, w, 4), f32); N[..., 2] = 1; N[..., 3] = 3
    hist = rng.uniform(0.1, 0.5, (h, w, 4)).astype(f32); ln = np.full((h, w), 5, f32)
    hist[0, 0, 0] = np.nan                                # carried with its payload
    live = np.array([[0, 1], [1, 0]], np.int32)
    out, out_len = R.accumulate_live(cam, S, Qm, 4, 2, A, N, N, hist, ln, live)
    full, full_len, _ = T.accumulate(cam, None, S, Qm, 4, 2, A, N, N, hist, ln)
    m = R.per_pixel(live != 0, h, w)
    assert np.array_equal(out[~m].view(np.uint32), hist[~m].view(np.uint32)) and (out_len[~m] == 5).all()
    assert np.array_equal(out[m].view(np.uint32), full[m].view(np.uint32)) and (out_len[m] == 6).all()
    S2, Q2 = R.moments_tiles(S, Qm, live)
    assert not S2[~m].any() and not Q2[~m][:, :3].any() and np.array_equal(Q2[..., 3], Qm[..., 3]) and np.array_equal(S2[m], S[m])
