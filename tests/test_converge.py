"""The converge stages on the GPU: pt_temporal_select against its numpy restatement (tests/converge_ref.py), pt_render_moments_tiles
against pt_render_moments, pt_temporal_accumulate_live against pt_temporal_accumulate, and a converging pt_preview session
against the chain of host calls it stands for, bit for bit.

Sizes: 64 x 48, and 61 x 43 (48 tiles, the last tile column and row partial)."""
import ctypes

import numpy as np
import pytest

import converge_ref as R
import converge_seq as CS
import temporal_ref as T
import temporal_seq as Q
from test_temporal import _cams, _cornell, _frame
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SPP, BATCHES, DEPTH = 4, 2, 4
f32 = np.float32


@pytest.fixture(scope="module")
def scenes_by_size(api, gpu_ready, scene_dir):
    return {(w, h): _cornell(api, scene_dir, "cv%dx%d" % (w, h), w, h, spp=SPP, max_depth=DEPTH)[0] for w, h in ((64, 48), (61, 43))}


@pytest.fixture(scope="module")
def full_moments(api, scenes_by_size):
    """pt_render_moments of the 61 x 43 frame, once: what every list is compared with."""
    w, h = 61, 43
    cam = _cams(api, "identity", w, h, 1)[0]
    S, Qm = scenes_by_size[(w, h)].render_moments(cam, w, h, SPP, SPP // BATCHES, DEPTH, seed=41)
    S.setflags(write=False); Qm.setflags(write=False)
    return cam, S, Qm


# ---- 1. select --------------------------------------------------------------------------------------------------------------------
def _synthetic_history(w=61, h=43):
    """Tiles of small and of large variance, NaN, Inf, pass-through and V = 0 with e = 0 pixels, young pixels, and one tile whose
    error is exactly the threshold. Returns (hist, hist_len, threshold, that tile's number)."""
    rng = np.random.default_rng(7)
    ty, tx = R.tile_grid(h, w)
    hist = np.empty((h, w, 4), f32)
    hist[..., :3] = rng.uniform(0.05, 1.0, (h, w, 3))
    noisy = R.per_pixel(rng.integers(0, 2, (ty, tx)).astype(bool), h, w)
    hist[..., 3] = np.where(noisy, rng.uniform(1e-3, 1e-2, (h, w)), rng.uniform(1e-8, 1e-7, (h, w)))
    ln = rng.integers(8, 30, (h, w)).astype(f32)
    hist[2, 3, 0] = np.nan; hist[2, 4, 3] = np.nan; hist[12, 20, 1] = np.inf; hist[13, 21, 3] = np.inf; hist[h - 1, w - 1, 2] = -np.inf
    hist[20, 5] = (3.0, 2.0, 1.0, -1.0); ln[20, 5] = 0                     # pass-through: it would be young, and is exempt
    hist[21, 6] = (0.0, 0.0, 0.0, 0.0)                                     # black and exact: 0 / 1e-4
    hist[22, 7] = (-0.5, -0.5, -0.5, 1e-3)                                 # a negative mean: r is NaN
    ln[30, 40] = 7; ln[h - 2, 1] = 1; ln[5, w - 1] = np.nan                # two young pixels; a NaN length is not young
    exact = 2 * tx + 2                                                     # tile (2, 2): flat but for one pixel
    hist[16:24, 16:24, :3] = 0.25; hist[16:24, 16:24, 3] = 0; ln[16:24, 16:24] = 16
    hist[18, 19, 3] = 4e-4
    thr = float(R.pixel_error(hist)[0][18, 19])
    return hist, ln, thr, exact


def test_select_device_host_and_restatement_are_bit_equal(api, gpu_ready):
    torch = gpu_ready
    w, h = 61, 43
    hist, ln, thr, exact = _synthetic_history(w, h)
    want_err, want_live, want_list = R.select(hist, ln, thr, 8)
    T_ = want_live.size
    assert 0 < want_list.size < T_ and want_live.ravel()[exact] == 1 and want_err.ravel()[exact] == f32(thr)
    err, live, lst = api.temporal_select(hist, ln, thr, 8)
    assert_bits_equal(err, want_err, "host tile_err"); assert np.array_equal(live, want_live) and np.array_equal(lst, want_list)
    dH, dL = torch.from_numpy(hist).to("cuda:0"), torch.from_numpy(ln).to("cuda:0")
    dE = torch.full((T_,), -1.0, device="cuda:0"); dV = torch.full((T_,), -1, dtype=torch.int32, device="cuda:0")
    dI = torch.full((T_,), -1, dtype=torch.int32, device="cuda:0"); dC = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream()
    api.temporal_select_device(w, h, dH.data_ptr(), dL.data_ptr(), dE.data_ptr(), dV.data_ptr(), dI.data_ptr(), dC.data_ptr(), thr, 8, stream=s.cuda_stream)
    s.synchronize()
    n = int(dC.cpu()[0])
    assert n == want_list.size
    assert_bits_equal(dE.cpu().numpy().reshape(want_err.shape), want_err, "device tile_err")
    assert np.array_equal(dV.cpu().numpy().reshape(want_live.shape), want_live)
    got = dI.cpu().numpy()
    assert np.array_equal(got[:n], want_list) and (got[n:] == -1).all()       # the list's tail is left alone
    assert_bits_equal(dH.cpu().numpy(), hist, "the input is left as it was")
    # threshold 0: every tile; a threshold above every error: only the tiles with a young pixel
    e0, l0, i0 = api.temporal_select(hist, ln, 0.0, 8)
    assert l0.all() and np.array_equal(i0, np.arange(T_, dtype=np.int32)); assert_bits_equal(e0, want_err, "tile_err does not depend on the threshold")
    e1, l1, i1 = api.temporal_select(hist, ln, 100.0, 8)
    w1 = R.select(hist, ln, 100.0, 8)
    assert np.array_equal(l1, w1[1]) and np.array_equal(i1, w1[2]) and i1.size == 2
    assert not api.temporal_select(hist, ln, 100.0, 1)[1].any()


# ---- 2. moments on a list -----------------------------------------------------------------------------------------------------------
def _lists(w, h):
    ty, tx = R.tile_grid(h, w)
    n = ty * tx
    return {"every tile": np.arange(n, dtype=np.int32), "one interior tile": np.array([2 * tx + 3], np.int32),
            "the partial corner tile": np.array([n - 1], np.int32), "every other tile": np.arange(0, n, 2, dtype=np.int32),
            "empty": np.zeros(0, np.int32)}


@pytest.mark.parametrize("onchip", [1, 0])
def test_moments_on_a_list_equal_the_full_frame_on_the_listed_tiles(api, gpu_ready, scene_dir, scenes_by_size, full_moments, onchip):
    torch = gpu_ready
    w, h = 61, 43
    cam, S, Qm = full_moments
    gs = scenes_by_size[(w, h)] if onchip else _cornell(api, scene_dir, "cv_hbm", w, h, spp=SPP, max_depth=DEPTH)[0]
    if not onchip:
        gs.set_option("onchip", 0)                        # the kernel for scenes in HBM
    assert gs.flags()["onchip"] == bool(onchip)
    for name, lst in _lists(w, h).items():
        live = np.zeros(R.tile_grid(h, w), np.int32); live.ravel()[lst] = 1
        wantS, wantQ = R.moments_tiles(S, Qm, live)
        gotS, gotQ = gs.render_moments_tiles(cam, w, h, SPP, SPP // BATCHES, DEPTH, lst, seed=41)
        assert_bits_equal(gotS, wantS, "onchip %d, %s: S" % (onchip, name)); assert_bits_equal(gotQ, wantQ, "onchip %d, %s: Q" % (onchip, name))
        assert (gotQ[..., 3] == BATCHES).all()
        if lst.size:
            assert gotS[R.per_pixel(live != 0, h, w)].any()
    # the device form, from a device list
    lst = _lists(w, h)["every other tile"]
    live = np.zeros(R.tile_grid(h, w), np.int32); live.ravel()[lst] = 1
    dI = torch.from_numpy(lst).to("cuda:0")
    dS = torch.full((h, w, 4), 9.0, device="cuda:0"); dQ = torch.full((h, w, 4), 9.0, device="cuda:0")
    s = torch.cuda.Stream()
    gs.render_moments_tiles_device(cam, w, h, SPP, SPP // BATCHES, DEPTH, dI.data_ptr(), lst.size, dS.data_ptr(), dQ.data_ptr(), seed=41, stream=s.cuda_stream)
    wantS, wantQ = R.moments_tiles(S, Qm, live)
    assert_bits_equal(dS.cpu().numpy(), wantS, "device form: S"); assert_bits_equal(dQ.cpu().numpy(), wantQ, "device form: Q")
    gs.render_moments_tiles_device(cam, w, h, SPP, SPP // BATCHES, DEPTH, 0, 0, dS.data_ptr(), dQ.data_ptr(), seed=41)     # an empty list, no pointer
    assert not dS.cpu().numpy().any() and (dQ.cpu().numpy()[..., 3] == BATCHES).all()
    # ... and a later full frame is what it was
    S2, Q2 = gs.render_moments(cam, w, h, SPP, SPP // BATCHES, DEPTH, seed=41)
    assert_bits_equal(S2, S, "pt_render_moments after list renders"); assert_bits_equal(Q2, Qm, "its Q")
    if not onchip:
        gs.close()


def test_moments_on_a_list_refuse_the_wavefront_variant(api, scenes_by_size):
    w, h = 61, 43
    gs = scenes_by_size[(w, h)]
    cam = _cams(api, "identity", w, h, 1)[0]
    S = np.full((h, w, 4), 5, f32); Qm = np.full((h, w, 4), 5, f32)
    lst = np.array([0, 3], np.int32)
    gs.set_variant(1)
    try:
        rc = api.lib().pt_render_moments_tiles(gs.h, ctypes.byref(cam), w, h, SPP, SPP // BATCHES, DEPTH, 0, 1, 41, lst.ctypes.data, 2, S.ctypes.data,
                                               Qm.ctypes.data)
        assert rc == -1 and "wavefront" in api.lib().pt_last_error().decode()
        assert (S == 5).all() and (Qm == 5).all()
    finally:
        gs.set_variant(0)


# ---- 3. accumulate with a map -----------------------------------------------------------------------------------------------------------
def test_accumulate_with_a_map_carries_and_blends(api, gpu_ready, scenes_by_size):
    torch = gpu_ready
    w, h = 61, 43
    gs = scenes_by_size[(w, h)]
    cam = _cams(api, "identity", w, h, 1)[0]
    f0, f1 = _frame(gs, cam, w, h, 51), _frame(gs, cam, w, h, 52)
    hist, ln = api.temporal_accumulate(cam, *f0[:2], SPP, BATCHES, *f0[2:])
    hist[4, 4] = (np.nan, 1.0, 1.0, 0.5); hist[40, 58] = (1.0, 2.0, 3.0, -1.0); ln[40, 58] = 0       # carried with their payloads
    live = np.random.default_rng(5).integers(0, 2, R.tile_grid(h, w)).astype(np.int32)
    live[0, 0] = 0; live[-1, -1] = 0; live[0, -1] = 1
    m = R.per_pixel(live != 0, h, w)
    full, full_len = api.temporal_accumulate(cam, *f1[:2], SPP, BATCHES, *f1[2:], None, f0[3], hist, ln)
    got, got_len = api.temporal_accumulate_live(cam, *f1[:2], SPP, BATCHES, *f1[2:], f0[3], hist, ln, live)
    assert_bits_equal(got[~m], hist[~m], "carried tiles: hist"); assert_bits_equal(got_len[~m], ln[~m], "carried tiles: hist_len")
    assert_bits_equal(got[m], full[m], "live tiles: hist"); assert_bits_equal(got_len[m], full_len[m], "live tiles: hist_len")
    assert (full_len[~m] != ln[~m]).any()                 # the full frame would have aged them
    want, want_len = R.accumulate_live(cam, *f1[:2], SPP, BATCHES, *f1[2:], f0[3], hist, ln, live)
    assert_bits_equal(got_len, want_len, "restatement: hist_len")
    # carried tiles read neither S, Q nor albedo: the zero frame of moments on a list is as good
    S2, Q2 = R.moments_tiles(f1[0], f1[1], live)
    got2, got2_len = api.temporal_accumulate_live(cam, S2, Q2, SPP, BATCHES, *f1[2:], f0[3], hist, ln, live, camera_prev=cam)
    assert_bits_equal(got2, got, "with the list's moments"); assert_bits_equal(got2_len, got_len, "its lengths")
    # no map: pt_temporal_accumulate
    none, none_len = api.temporal_accumulate_live(cam, *f1[:2], SPP, BATCHES, *f1[2:], f0[3], hist, ln, None)
    assert_bits_equal(none, full, "NULL map: hist"); assert_bits_equal(none_len, full_len, "NULL map: hist_len")
    # the device form is the host form
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (f1[0], f1[1], f1[2], f1[3], f0[3], hist, ln, live)]
    dO = torch.zeros(h, w, 4, device="cuda:0"); dOL = torch.zeros(h, w, device="cuda:0")
    s = torch.cuda.Stream()
    api.temporal_accumulate_live_device(w, h, cam, None, dev[0].data_ptr(), dev[1].data_ptr(), SPP, BATCHES, dev[2].data_ptr(), dev[3].data_ptr(),
                                        dev[4].data_ptr(), dev[5].data_ptr(), dev[6].data_ptr(), dev[7].data_ptr(), dO.data_ptr(), dOL.data_ptr(),
                                        stream=s.cuda_stream)
    s.synchronize()
    assert_bits_equal(dO.cpu().numpy(), got, "device form: hist"); assert_bits_equal(dOL.cpu().numpy(), got_len, "device form: hist_len")
    with pytest.raises(api.PtError, match="unchanged camera"):
        api.temporal_accumulate_live(cam, *f1[:2], SPP, BATCHES, *f1[2:], f0[3], hist, ln, live, camera_prev=_cams(api, "pinhole", w, h, 2)[1])


# ---- 4. the session is the chain ---------------------------------------------------------------------------------------------------------
# Chosen on the CPU (python tests/converge_seq.py): the restatement over the CPU reference's frames of this very sequence, at the
# library's default threshold 0.5 and min_history 8. Frame 0 has no history and frame 12 a moved camera: they render every tile.
# Tiles stop from frame 8 on, the count never grows while the camera rests, and 0 < live < 48 on six frames.
SESSION_LIVE = [48, 48, 48, 48, 48, 48, 48, 48, 43, 42, 41, 40, 48, 39, 38]


def _chain_frame(api, gs, cam, w, h, seed, state, threshold, min_history, scale=1):
    """One frame of what a session computes, through the host API. state: (hist, hist_len, prev_n, prev_cam) or None. Returns
    (mean, hist, hist_len, filt, tiles or None, live count), and the next state."""
    hist, ln, prev_n, prev_cam = state if state else (None, None, None, None)
    total = api.n_tiles(w, h)
    A, N = gs.render_aovs(cam, w, h, aov_spp=1, seed=seed)
    tiles, count = None, total
    if threshold and scale == 1 and hist is not None and prev_cam.tobytes() == cam.tobytes():
        err, live, lst = api.temporal_select(hist, ln, threshold, min_history)
        S, Qm = gs.render_moments_tiles(cam, w, h, SPP, SPP // BATCHES, DEPTH, lst, seed=seed) if lst.size else (np.zeros((h, w, 4), f32),) * 2
        hist, ln = api.temporal_accumulate_live(cam, S, Qm, SPP, BATCHES, A, N, prev_n, hist, ln, live, camera_prev=prev_cam)
        tiles, count = (err, live), int(lst.size)
    elif scale == 1:
        S, Qm = gs.render_moments(cam, w, h, SPP, SPP // BATCHES, DEPTH, seed=seed)
        hist, ln = api.temporal_accumulate(cam, S, Qm, SPP, BATCHES, A, N, prev_cam, prev_n, hist, ln)
    else:
        lo = api.scaled_camera(cam, scale)
        S, Qm = gs.render_moments(lo, w // scale, h // scale, SPP, SPP // BATCHES, DEPTH, seed=seed)
        Al, Nl = gs.render_aovs(lo, w // scale, h // scale, aov_spp=1, seed=seed)
        hist, ln = api.temporal_accumulate_cur(cam, api.upsample(scale, S, Qm, SPP, BATCHES, Al, Nl, A, N), N, prev_cam, prev_n, hist, ln)
    filt = api.denoise_hist(hist, A, N)
    return (api.finalise(filt, 1), hist, ln, filt, tiles, count), (hist, ln, N, cam)


def _assert_session_frame(api, pv, want, what):
    mean, hist, ln, filt, tiles, count = want
    got = pv.read()
    assert_bits_equal(got["mean"], mean, what + ": mean"); assert_bits_equal(got["hist"], hist, what + ": hist")
    assert_bits_equal(got["hist_len"], ln, what + ": hist_len")
    assert np.array_equal(got["rgba8"], api.resolve(filt, 1)[0]), what
    assert pv.last_live() == (count, api.n_tiles(pv.w, pv.h)), what
    if tiles is not None:
        err, live = pv.read_tiles()
        assert_bits_equal(err, tiles[0], what + ": tile_err"); assert np.array_equal(live, tiles[1]), what


def test_converging_session_equals_the_host_chain_after_every_frame(api, scenes_by_size):
    w, h = CS.SW, CS.SH
    gs = scenes_by_size[(w, h)]
    cams, seeds = CS.session_cameras(api, w, h), CS.session_seeds()
    thr, mh = CS.SESSION_THRESHOLD, CS.MIN_HISTORY
    kw = dict(spp=SPP, batches=BATCHES, max_depth=CS.SDEPTH)
    pv, plain = api.Preview(gs, w, h, **kw), api.Preview(gs, w, h, **kw)
    with pytest.raises(api.PtError, match="threshold"):
        pv.set_converge(-0.5, mh)
    with pytest.raises(api.PtError, match="min_history 0"):
        pv.set_converge(thr, 0)
    pv.set_converge(thr, mh)
    with pytest.raises(api.PtError, match="no converging frame"):
        pv.read_tiles()
    state = plain_state = None
    counts = []
    for t, (cam, seed) in enumerate(zip(cams, seeds)):
        want, state = _chain_frame(api, gs, cam, w, h, seed, state, thr, mh)
        pv.frame(cam, seed)
        _assert_session_frame(api, pv, want, "frame %d" % t)
        counts.append(pv.last_live()[0])
        if t == 0:
            with pytest.raises(api.PtError, match="no converging frame"):
                pv.read_tiles()
        # a session that never called set_converge is today's session
        wantp, plain_state = _chain_frame(api, gs, cam, w, h, seed, plain_state, 0, mh)
        plain.frame(cam, seed)
        _assert_session_frame(api, plain, wantp, "plain session, frame %d" % t)
    print("live tiles per frame:", counts)
    assert counts == SESSION_LIVE
    still = counts[1:CS.S_STILL]
    assert all(a >= b for a, b in zip(still, still[1:])) and any(0 < c < api.n_tiles(w, h) for c in counts)
    assert (pv.read()["hist_len"] < plain.read()["hist_len"]).any()        # carried pixels did not age
    # a frame at scale 2 renders everything, through the upsample chain
    t = len(cams)
    pv.set_scale(2)
    want, state = _chain_frame(api, gs, cams[-1], w, h, Q.SEED0 + t, state, thr, mh, scale=2)
    pv.frame(cams[-1], Q.SEED0 + t)
    _assert_session_frame(api, pv, want, "frame %d at scale 2" % t)
    assert want[5] == api.n_tiles(w, h)
    # converge off: a resting camera at scale 1 renders every tile again
    pv.set_scale(1).set_converge(0.0)
    want, state = _chain_frame(api, gs, cams[-1], w, h, Q.SEED0 + t + 1, state, 0, mh)
    pv.frame(cams[-1], Q.SEED0 + t + 1)
    _assert_session_frame(api, pv, want, "frame %d, converge off" % (t + 1))
    # ... and on again with NULL-equivalent arguments of the wrapper
    pv.set_converge(False)
    pv.frame(cams[-1], Q.SEED0 + t + 2)
    assert pv.last_live() == (api.n_tiles(w, h),) * 2
    pv.close(); plain.close()


def test_a_failed_frame_leaves_a_converging_session_where_it_was(api, scenes_by_size):
    w, h = 64, 48
    gs = scenes_by_size[(w, h)]
    cam = _cams(api, "identity", w, h, 1)[0]
    # every tile stops once none of its pixels is young: from frame 2 on only tiles in which a pixel lost its history stay live
    pv = api.Preview(gs, w, h, spp=SPP, batches=BATCHES, max_depth=DEPTH).set_converge(100.0, 2)
    clean = api.Preview(gs, w, h, spp=SPP, batches=BATCHES, max_depth=DEPTH).set_converge(100.0, 2)
    for t in range(3):
        pv.frame(cam, 80 + t); clean.frame(cam, 80 + t)
    n_live = pv.last_live()
    print("live tiles of frame 2:", n_live)
    assert 0 <= n_live[0] < 48 and n_live[1] == 48
    before, tiles = pv.read(), pv.read_tiles()
    with pytest.raises(api.PtError, match="camera is 61 x 43"):
        pv.frame(_cams(api, "identity", 61, 43, 1)[0], 83)
    after, tiles_after = pv.read(), pv.read_tiles()
    assert_bits_equal(after["hist"], before["hist"], "hist after a failed frame"); assert_bits_equal(after["hist_len"], before["hist_len"], "hist_len")
    assert_bits_equal(tiles_after[0], tiles[0], "tile_err"); assert np.array_equal(tiles_after[1], tiles[1]) and pv.last_live() == n_live
    assert pv.stats()["frames"] == 3
    # the camera is still the last good frame's: the next frame converges, and equals the session that never failed
    got, want = pv.frame(cam, 83).read(), clean.frame(cam, 83).read()
    assert pv.last_live() == clean.last_live() and pv.last_live()[0] < 48
    assert_bits_equal(got["hist"], want["hist"], "the next good frame"); assert_bits_equal(got["mean"], want["mean"], "its mean")
    carried = ~R.per_pixel(pv.read_tiles()[1] != 0, h, w)
    assert carried.any()
    assert_bits_equal(got["hist"][carried], before["hist"][carried], "the tiles that were not rendered keep their history")
    assert_bits_equal(got["hist_len"][carried], before["hist_len"][carried], "... and its length")
    pv.reset()
    with pytest.raises(api.PtError, match="no converging frame"):
        pv.read_tiles()
    pv.close(); clean.close()


# ---- 5. quality -----------------------------------------------------------------------------------------------------------------------
# mse / mse(raw 4 spp) of history + filter on the last of CS.N_FRAMES still frames, by the numpy restatement at the library's
# defaults on exactly these frames (python tests/converge_seq.py). 24 frames: tiles may stop from frame 8 on, so
# sixteen frames carry tiles, twice the history a tile needs before it may stop. The ceiling is that value times 1.05 for the
# kernels' f32 arithmetic, §11's margin. (Not converging: 0.05071; 33.3 % of the tile-frames are not rendered.)
RESTATEMENT_RATIO = 0.05158


def test_quality_of_a_converging_session(api, gpu_ready, scene_dir):
    w, h = Q.W, Q.H
    gs = _cornell(api, scene_dir, "cvq", w, h, spp=Q.SPP, max_depth=Q.DEPTH)[0]
    cam = Q.camera(api, 0, False, w, h)
    kw = dict(spp=Q.SPP, batches=Q.BATCHES, max_depth=Q.DEPTH)
    pv, plain = api.Preview(gs, w, h, **kw).set_converge(), api.Preview(gs, w, h, **kw)
    live = []
    for t in range(CS.N_FRAMES):
        pv.frame(cam, Q.SEED0 + t); plain.frame(cam, Q.SEED0 + t)
        live.append(pv.last_live()[0])
    last = _frame(gs, cam, w, h, Q.SEED0 + CS.N_FRAMES - 1, depth=Q.DEPTH)
    ref, _ = gs.render_moments(cam, w, h, Q.REF_SPP, Q.REF_SPP // 16, Q.DEPTH, seed=Q.REF_SEED)
    got, base = pv.read(), plain.read()
    m = Q.errors([last], ref, got["hist"], got["mean"])
    b = Q.errors([last], ref, base["hist"], base["mean"])
    saved = CS.pixel_samples_saved(live, h, w)
    print("converging: history + filter / raw %.4f (restatement %.4f); not converging %.4f; live tiles per frame %s; tile-frames saved %.1f %%" % (
        m["hist_filter"] / m["raw"], RESTATEMENT_RATIO, b["hist_filter"] / b["raw"], live, 100 * saved))
    assert 0 < live[-1] < api.n_tiles(w, h)
    assert m["hist_filter"] <= 1.05 * RESTATEMENT_RATIO * m["raw"]
    pv.close(); plain.close(); gs.close()
