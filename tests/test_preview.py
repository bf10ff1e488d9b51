"""pt_resolve on the GPU against its numpy restatement (tests/preview_ref.py), and the pt_preview session against the chain of
host calls it stands for: render_moments -> render_aovs -> temporal_accumulate -> denoise_hist -> finalise, bit for bit. Every
link of that chain has its own device-equals-host test (test_moments.py, test_aov.py, test_temporal.py, test_denoise_var.py).

Sizes: 64 x 48, and 61 x 43, the smallest whose last tile column and row are partial for both the 8 x 8 and the 16 x 16 tiling."""
import os

import numpy as np
import pytest

import preview_ref as R
import temporal_seq as Q
from test_temporal import _cams
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SPP, BATCHES, DEPTH = 4, 2, 4
SIZES = [(64, 48), (61, 43)]
MAX_DIFFERING_BYTES = 0.001          # device powf vs libm's can only move a value across a rounding boundary of the byte conversion


def _scene(api, scene_dir, w, h):
    from cudapathtracer_amd import scenes
    name = "pv%dx%d" % (w, h)
    return api.Scene(api.HostScene(scenes.cornell(os.path.join(scene_dir, name), width=w, height=h, name=name, spp=SPP, max_depth=DEPTH)["config"]))


@pytest.fixture(scope="module")
def scenes_by_size(api, gpu_ready, scene_dir):
    return {(w, h): _scene(api, scene_dir, w, h) for w, h in SIZES}


def _assert_bytes_close(got, want, what):
    """Every byte within one code of the restatement, and at most MAX_DIFFERING_BYTES of them different at all."""
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print("%s: %d of %d bytes differ from the restatement (%.4f %%), largest difference %d" % (what, (d > 0).sum(), d.size, 100 * (d > 0).mean(), d.max()))
    assert d.max() <= 1, what
    assert (d > 0).mean() <= MAX_DIFFERING_BYTES, what


def _host_chain(api, gs, cams, w, h, seeds, temporal=1, filter=1):
    """What a session computes, through the host API: per frame (mean, hist, hist_len, filtered)."""
    hist = ln = prev_n = prev_cam = None
    out = []
    for cam, seed in zip(cams, seeds):
        S, Qs = gs.render_moments(cam, w, h, SPP, SPP // BATCHES, DEPTH, seed=seed)
        A, N = gs.render_aovs(cam, w, h, aov_spp=1, seed=seed)
        if temporal:
            hist, ln = api.temporal_accumulate(cam, S, Qs, SPP, BATCHES, A, N, prev_cam, prev_n, hist, ln)
            prev_n, prev_cam = N, cam
            filt = api.denoise_hist(hist, A, N, **({} if filter else {"iterations": 0}))
            mean = api.finalise(filt, 1)
        else:
            filt = api.denoise_var(S, Qs, SPP, BATCHES, A, N) if filter else S
            mean = api.finalise(filt, SPP)
        out.append((mean, hist, ln, filt))
    return out


def _assert_frame(got, want, what):
    mean, hist, ln, _ = want
    assert_bits_equal(got["mean"], mean, what + ": mean")
    if hist is not None:
        assert_bits_equal(got["hist"], hist, what + ": hist")
        assert_bits_equal(got["hist_len"], ln, what + ": hist_len")


# ---- 1. the resolve -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_resolve_matches_the_restatement(api, gpu_ready, scenes_by_size, w, h):
    torch = gpu_ready
    gs = scenes_by_size[(w, h)]
    cam = _cams(api, "pinhole", w, h, 1)[0]
    S = gs.render(cam, w, h, SPP, DEPTH)[0].copy()
    S[5, 7, 0] = np.nan; S[20, 40, 1] = np.inf; S[h - 1, w - 1, 2] = -np.inf; S[9, 3, :3] = (-2.0, 0.5, 3e4 * SPP); S[0, 0, :3] = (np.nan, np.inf, 1.0)
    S[..., 3] = 3.0
    b8, mean = api.resolve(S, SPP)
    assert_bits_equal(mean, api.finalise(S, SPP), "mean vs finalise")
    assert tuple(mean[5, 7]) == (1, 0, 1, 0) and tuple(mean[20, 40]) == (0, 1, 0, 0) and tuple(mean[0, 0]) == (1, 0, 1, 0)
    want8, want_mean = R.resolve(S, SPP)
    assert_bits_equal(mean, want_mean, "mean vs the restatement")
    _assert_bytes_close(b8, want8, "%d x %d, tone-mapped" % (w, h))
    assert (b8[..., 3] == 255).all() and b8[9, 3, 2] == 255 and len(np.unique(b8[..., :3])) > 100
    _assert_bytes_close(api.resolve(S, SPP, exposure=2.5)[0], R.resolve(S, SPP, exposure=2.5)[0], "%d x %d, exposure 2.5" % (w, h))
    lin8, lin_mean = api.resolve(S, SPP, tonemap=False, exposure=0.75)
    assert np.array_equal(lin8, R.resolve(S, SPP, tonemap=False, exposure=0.75)[0])      # no powf: bit-equal bytes
    assert tuple(lin8[9, 3]) == (0, 24, 255, 255)          # -0.5, 0.125 and 3e4 times 0.75: clamped below, 0.09375 * 255 + 0.5 = 24.4, clamped above
    assert_bits_equal(lin_mean, mean, "the mean does not depend on the display parameters")
    # the device form is the host form
    dS = torch.from_numpy(S).to("cuda:0")
    d8 = torch.zeros(h, w, 4, dtype=torch.uint8, device="cuda:0"); dM = torch.full((h, w, 4), 9.0, device="cuda:0")
    s = torch.cuda.Stream()
    api.resolve_device(w, h, dS.data_ptr(), SPP, d8.data_ptr(), dM.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d8.cpu().numpy(), b8)
    assert_bits_equal(dM.cpu().numpy(), mean, "device mean")
    d8.zero_()
    api.resolve_device(w, h, dS.data_ptr(), SPP, d8.data_ptr(), tonemap=False, exposure=0.75)    # no mean buffer
    torch.cuda.synchronize()
    assert np.array_equal(d8.cpu().numpy(), lin8)
    for kw in (dict(d_rgba8_ptr=dS.data_ptr(), d_mean_ptr=dM.data_ptr()), dict(d_rgba8_ptr=d8.data_ptr(), d_mean_ptr=dS.data_ptr()),
               dict(d_rgba8_ptr=dM.data_ptr() + 32, d_mean_ptr=dM.data_ptr())):
        with pytest.raises(api.PtError, match="alias"):
            api.resolve_device(w, h, dS.data_ptr(), SPP, **kw)
    assert_bits_equal(dS.cpu().numpy(), S, "the input is left as it was")


def test_resolve_with_the_tile_map_of_an_adaptive_frame(api, gpu_ready, scenes_by_size):
    torch = gpu_ready
    w, h = 61, 43
    gs = scenes_by_size[(w, h)]
    cam = _cams(api, "pinhole", w, h, 1)[0]
    for threshold in (0.05, 0.1, 0.2, 0.4, 0.02):
        col, tiles, _, _ = gs.render_adaptive(cam, w, h, DEPTH, 2, 16, 2, threshold)
        if np.unique(tiles).size >= 2:
            break
    print("adaptive 61 x 43, threshold %g: tile counts %s" % (threshold, dict(zip(*np.unique(tiles, return_counts=True)))))
    assert np.unique(tiles).size >= 2
    b8, mean = api.resolve(col, 0, tile_spp=tiles)          # the map overrides spp
    assert_bits_equal(mean, api.adaptive_mean(col, tiles), "mean vs adaptive_mean")
    want8, want_mean = R.resolve(col, 0, tiles)
    assert_bits_equal(mean, want_mean, "mean vs the restatement")
    _assert_bytes_close(b8, want8, "adaptive frame, tone-mapped")
    assert np.array_equal(api.resolve(col, 0, tile_spp=tiles, tonemap=False)[0], R.resolve(col, 0, tiles, tonemap=False)[0])
    assert not np.array_equal(mean, api.finalise(col, int(tiles.max())))      # the map, not one count, divided
    dS, dT = torch.from_numpy(col).to("cuda:0"), torch.from_numpy(tiles).to("cuda:0")
    d8 = torch.zeros(h, w, 4, dtype=torch.uint8, device="cuda:0"); dM = torch.zeros(h, w, 4, device="cuda:0")
    api.resolve_device(w, h, dS.data_ptr(), 0, d8.data_ptr(), dM.data_ptr(), d_tile_spp_ptr=dT.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d8.cpu().numpy(), b8)
    assert_bits_equal(dM.cpu().numpy(), mean, "device mean")


# ---- 2. the session is the chain -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", ["identity", "pinhole", "thin_lens"])
def test_session_equals_the_host_chain_after_every_frame(api, scenes_by_size, kind, w, h):
    gs = scenes_by_size[(w, h)]
    cams = _cams(api, kind, w, h, 4)
    seeds = [Q.SEED0 + t for t in range(4)]
    want = _host_chain(api, gs, cams, w, h, seeds)
    pv = api.Preview(gs, w, h, spp=SPP, batches=BATCHES, max_depth=DEPTH)
    for t, (cam, seed) in enumerate(zip(cams, seeds)):
        pv.frame(cam, seed)
        got = pv.read()
        _assert_frame(got, want[t], "%s %d x %d frame %d" % (kind, w, h, t))
        assert np.array_equal(got["rgba8"], api.resolve(want[t][3], 1)[0])
    assert pv.stats()["frames"] == 4
    pv.close()


@pytest.mark.parametrize("temporal,filter", [(1, 0), (0, 1), (0, 0)])
def test_session_modes_equal_their_chains(api, scenes_by_size, temporal, filter):
    w, h = 61, 43
    gs = scenes_by_size[(w, h)]
    cams = _cams(api, "pinhole", w, h, 3)
    seeds = [70 + t for t in range(3)]
    want = _host_chain(api, gs, cams, w, h, seeds, temporal, filter)
    pv = api.Preview(gs, w, h, spp=SPP, batches=BATCHES, max_depth=DEPTH, temporal=temporal, filter=filter)
    for t, (cam, seed) in enumerate(zip(cams, seeds)):
        got = pv.frame(cam, seed).read()
        assert ("hist" in got) == bool(temporal)
        _assert_frame(got, want[t], "temporal %d filter %d frame %d" % (temporal, filter, t))
        assert np.array_equal(got["rgba8"], api.resolve(want[t][3], 1 if temporal else SPP)[0])
    if not temporal:
        with pytest.raises(api.PtError, match="keeps no history"):
            pv.read(hist=True)
    pv.close()


# ---- 3. state ------------------------------------------------------------------------------------------------------------------------
def test_reset_failed_frames_and_stats(api, gpu_ready, scenes_by_size):
    torch = gpu_ready
    w, h = 64, 48
    gs = scenes_by_size[(w, h)]
    cams = _cams(api, "pinhole", w, h, 3)
    kw = dict(spp=SPP, batches=BATCHES, max_depth=DEPTH)
    with pytest.raises(api.PtError, match="batches 3 must divide spp 4"):
        api.Preview(gs, w, h, spp=4, batches=3, max_depth=DEPTH)
    with pytest.raises(api.PtError, match="exposure"):
        api.Preview(gs, w, h, exposure=0.0, **kw)
    clean, pv = api.Preview(gs, w, h, **kw), api.Preview(gs, w, h, **kw)
    with pytest.raises(api.PtError, match="no frame"):
        pv.read()
    assert pv.stats()["frames"] == 0
    first = clean.frame(cams[0], 90).read()
    pv.frame(cams[0], 90)
    before = pv.read()
    _assert_frame(before, (first["mean"], first["hist"], first["hist_len"], None), "two sessions, first frame")
    # a frame that fails leaves the session where it was
    with pytest.raises(api.PtError, match="camera is 61 x 43"):
        pv.frame(_cams(api, "pinhole", 61, 43, 2)[1], 91)
    after = pv.read()
    assert_bits_equal(after["hist"], before["hist"], "hist after a failed frame"); assert_bits_equal(after["hist_len"], before["hist_len"], "hist_len")
    assert pv.stats()["frames"] == 1
    second = clean.frame(cams[1], 91).read()
    got = pv.frame(cams[1], 91).read()
    _assert_frame(got, (second["mean"], second["hist"], second["hist_len"], None), "the next good frame")
    assert np.array_equal(got["rgba8"], second["rgba8"]) and (got["hist_len"] == 2).mean() > 0.3
    # reset: the next frame is a first frame
    pv.reset()
    with pytest.raises(api.PtError, match="no frame"):
        pv.read()
    again = pv.frame(cams[0], 90).read()
    _assert_frame(again, (first["mean"], first["hist"], first["hist_len"], None), "first frame after reset")
    assert np.array_equal(again["rgba8"], first["rgba8"]) and again["hist_len"].max() == 1
    # the device pointers hold what read() copies
    # the device pointers hold what read() copies: resolving the displayed mean once more (spp 1) changes nothing
    d8 = torch.zeros(h, w, 4, dtype=torch.uint8, device="cuda:0"); dM = torch.zeros(h, w, 4, device="cuda:0")
    assert pv.device_rgba8() and pv.device_mean()
    api.resolve_device(w, h, pv.device_mean(), 1, d8.data_ptr(), dM.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d8.cpu().numpy(), again["rgba8"])
    assert_bits_equal(dM.cpu().numpy(), again["mean"], "device mean")
    # a still camera builds history; the stage times are sane
    still = _cams(api, "identity", w, h, 4)
    pv.reset()
    for t, cam in enumerate(still):
        pv.frame(cam, 100 + t)
    assert pv.read()["hist_len"].mean() > 2.5
    st = pv.stats()
    assert st["frames"] == 7
    times = [st[k] for k in ("render_ms", "aov_ms", "accumulate_ms", "filter_ms", "resolve_ms", "total_ms")]
    print("stage times of a 64 x 48 frame (ms):", st)
    assert all(np.isfinite(v) and v >= 0 for v in times) and st["total_ms"] >= max(times[:5])
    pv.close(); clean.close()
    pv.close()                                             # idempotent


# ---- 4. full HD ----------------------------------------------------------------------------------------------------------------------
def test_full_hd_two_frames_equal_the_host_chain(api, gpu_ready, scene_dir):
    w, h = 1920, 1080
    gs = _scene(api, scene_dir, w, h)
    cams = [Q.camera(api, t, True, w, h) for t in (0, 1)]
    want = _host_chain(api, gs, cams, w, h, [60, 61])
    pv = api.Preview(gs, w, h, spp=SPP, batches=BATCHES, max_depth=DEPTH)
    for t in (0, 1):
        got = pv.frame(cams[t], 60 + t).read()
        _assert_frame(got, want[t], "full HD frame %d" % t)
    assert (got["hist_len"] == 2).mean() > 0.5
    b8, _ = api.resolve(want[1][3], 1)
    assert np.array_equal(got["rgba8"], b8)
    _assert_bytes_close(b8, R.display(want[1][0]), "full HD, tone-mapped")
    print("full HD frame, stage times (ms):", pv.stats())
    pv.close(); gs.close()
