"""The pt_preview session at a render scale against the chain of host calls it stands for: render_moments and render_aovs with
the low-res camera, render_aovs with the display camera, upsample, temporal_accumulate_cur, denoise_hist, finalise, bit for bit.
Every link has its own test against a restatement (test_upsample.py and the files test_preview.py names)."""
import numpy as np
import pytest

import preview_ref as R
import temporal_seq as Q
from test_preview import _assert_bytes_close, _assert_frame, _scene
from test_temporal import _cams
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SPP, BATCHES, DEPTH = 4, 2, 4
SIZES = [(64, 48), (63, 45)]


@pytest.fixture(scope="module")
def scenes_by_size(api, gpu_ready, scene_dir):
    return {(w, h): _scene(api, scene_dir, w, h) for w, h in SIZES}


def _host_chain(api, gs, cams, w, h, seeds, scales, temporal=1, filter=1):
    """What a session computes at the given scale of each frame, through the host API: per frame (mean, hist, hist_len, filtered)."""
    hist = ln = prev_n = prev_cam = None
    out = []
    it = {} if filter else {"iterations": 0}
    for cam, seed, s in zip(cams, seeds, scales):
        A, N = gs.render_aovs(cam, w, h, aov_spp=1, seed=seed)
        if s == 1:
            S, Qs = gs.render_moments(cam, w, h, SPP, SPP // BATCHES, DEPTH, seed=seed)
            assert temporal
            hist, ln = api.temporal_accumulate(cam, S, Qs, SPP, BATCHES, A, N, prev_cam, prev_n, hist, ln)
        else:
            lo = api.scaled_camera(cam, s)
            S, Qs = gs.render_moments(lo, w // s, h // s, SPP, SPP // BATCHES, DEPTH, seed=seed)
            Al, Nl = gs.render_aovs(lo, w // s, h // s, aov_spp=1, seed=seed)
            cur = api.upsample(s, S, Qs, SPP, BATCHES, Al, Nl, A, N)
            if temporal:
                hist, ln = api.temporal_accumulate_cur(cam, cur, N, prev_cam, prev_n, hist, ln)
        prev_n, prev_cam = N, cam
        filt = api.denoise_hist(hist if temporal else cur, A, N, **it)
        out.append((api.finalise(filt, 1), hist, ln, filt))
    return out


def _params(**kw):
    return dict(spp=SPP, batches=BATCHES, max_depth=DEPTH, **kw)


# ---- 1. the scaled session is the chain --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,s", [(64, 48, 2), (63, 45, 3)])
def test_scaled_session_equals_the_host_chain_after_every_frame(api, scenes_by_size, w, h, s):
    gs = scenes_by_size[(w, h)]
    cams = _cams(api, "pinhole", w, h, 4)
    seeds = [Q.SEED0 + t for t in range(4)]
    want = _host_chain(api, gs, cams, w, h, seeds, [s] * 4)
    pv = api.Preview(gs, w, h, **_params()).set_scale(s)
    lin = api.Preview(gs, w, h, **_params(tonemap=False)).set_scale(s)
    assert pv.scale == s
    for t, (cam, seed) in enumerate(zip(cams, seeds)):
        got = pv.frame(cam, seed).read()
        what = "%d x %d scale %d frame %d" % (w, h, s, t)
        _assert_frame(got, want[t], what)
        assert np.array_equal(got["rgba8"], api.resolve(want[t][3], 1)[0]), what
        _assert_bytes_close(got["rgba8"], R.display(want[t][0]), what + ", tone-mapped")            # powf: one code on at most 0.1 %
        flat = lin.frame(cam, seed).read()
        _assert_frame(flat, want[t], what + ", no tone map")
        assert np.array_equal(flat["rgba8"], R.display(want[t][0], tonemap=False)), what              # no powf: equal bytes
    assert (got["hist_len"] >= 2).mean() > 0.3 and pv.stats()["frames"] == 4
    st = pv.stats()
    print("stage times of a %d x %d frame at scale %d (ms):" % (w, h, s), st)
    assert all(np.isfinite(st[k]) and st[k] >= 0 for k in ("render_ms", "aov_ms", "accumulate_ms", "filter_ms", "resolve_ms", "total_ms"))
    pv.close(); lin.close()


@pytest.mark.parametrize("filter", [1, 0])
def test_scaled_session_without_history_equals_its_chain(api, scenes_by_size, filter):
    w, h, s = 64, 48, 4
    gs = scenes_by_size[(w, h)]
    cams = _cams(api, "pinhole", w, h, 2)
    want = _host_chain(api, gs, cams, w, h, [70, 71], [s, s], temporal=0, filter=filter)
    pv = api.Preview(gs, w, h, **_params(temporal=0, filter=filter)).set_scale(s)
    for t in range(2):
        got = pv.frame(cams[t], 70 + t).read()
        assert "hist" not in got
        _assert_frame(got, want[t], "temporal 0 filter %d frame %d" % (filter, t))
        assert np.array_equal(got["rgba8"], api.resolve(want[t][3], 1)[0])
    pv.close()


# ---- 2. the scale as session state -------------------------------------------------------------------------------------------------
def test_set_scale_one_changes_nothing(api, scenes_by_size):
    w, h = 64, 48
    gs = scenes_by_size[(w, h)]
    cams = _cams(api, "pinhole", w, h, 2)
    plain, one = api.Preview(gs, w, h, **_params()), api.Preview(gs, w, h, **_params())
    assert plain.scale == 1 and one.set_scale(1).scale == 1
    for t in range(2):
        a, b = plain.frame(cams[t], 80 + t).read(), one.frame(cams[t], 80 + t).read()
        _assert_frame(b, (a["mean"], a["hist"], a["hist_len"], None), "frame %d" % t)
        assert np.array_equal(a["rgba8"], b["rgba8"])
    plain.close(); one.close()


def test_scale_changes_carry_the_history(api, scenes_by_size):
    w, h = 64, 48
    gs = scenes_by_size[(w, h)]
    cams = _cams(api, "identity", w, h, 5)
    seeds = [100 + t for t in range(5)]
    scales = [2, 2, 2, 1, 4]
    want = _host_chain(api, gs, cams, w, h, seeds, scales)
    pv = api.Preview(gs, w, h, **_params())
    for t in range(5):
        got = pv.set_scale(scales[t]).frame(cams[t], seeds[t]).read()
        _assert_frame(got, want[t], "frame %d at scale %d" % (t, scales[t]))
        if t == 3:
            assert got["hist_len"].max() == 4           # three scaled frames and the full-resolution one: one history
    assert got["hist_len"].max() == 5 and pv.scale == 4
    pv.close()


def test_a_scale_that_does_not_divide_is_refused(api, scenes_by_size):
    w, h = 64, 48
    gs = scenes_by_size[(w, h)]
    cams = _cams(api, "pinhole", w, h, 2)
    clean, pv = api.Preview(gs, w, h, **_params()).set_scale(2), api.Preview(gs, w, h, **_params()).set_scale(2)
    for bad, msg in ((5, "scale 5 must divide the session's size 64 x 48"), (3, "scale 3 must divide"), (0, "scale 0 must be 1..8"), (9, "scale 9")):
        with pytest.raises(api.PtError, match=msg):
            pv.set_scale(bad)
        assert pv.scale == 2
    for t in range(2):
        a, b = clean.frame(cams[t], 90 + t).read(), pv.frame(cams[t], 90 + t).read()
        _assert_frame(b, (a["mean"], a["hist"], a["hist_len"], None), "frame %d" % t)
    clean.close(); pv.close()


def test_a_failed_scaled_frame_leaves_history_and_scale(api, scenes_by_size):
    w, h = 64, 48
    gs = scenes_by_size[(w, h)]
    cams = _cams(api, "pinhole", w, h, 2)
    clean, pv = api.Preview(gs, w, h, **_params()).set_scale(2), api.Preview(gs, w, h, **_params()).set_scale(2)
    clean.frame(cams[0], 90)
    before = pv.frame(cams[0], 90).read()
    for other in ((61, 43), (32, 24)):                    # a size the scale does not divide, and one it does
        with pytest.raises(api.PtError, match="camera is %d x %d" % other):
            pv.frame(_cams(api, "pinhole", other[0], other[1], 2)[1], 91)
    after = pv.read()
    assert_bits_equal(after["hist"], before["hist"], "hist after a failed frame"); assert_bits_equal(after["hist_len"], before["hist_len"], "hist_len")
    assert pv.scale == 2 and pv.stats()["frames"] == 1
    a, b = clean.frame(cams[1], 91).read(), pv.frame(cams[1], 91).read()
    _assert_frame(b, (a["mean"], a["hist"], a["hist_len"], None), "the next good frame")
    assert np.array_equal(a["rgba8"], b["rgba8"]) and (b["hist_len"] == 2).mean() > 0.3
    clean.close(); pv.close()


# ---- 3. full HD ----------------------------------------------------------------------------------------------------------------------
def test_full_hd_one_frame_at_scale_two_equals_the_host_chain(api, gpu_ready, scene_dir):
    w, h = 1920, 1080
    gs = _scene(api, scene_dir, w, h)
    cam = Q.camera(api, 1, True, w, h)
    want = _host_chain(api, gs, [cam], w, h, [60], [2])
    pv = api.Preview(gs, w, h, **_params()).set_scale(2)
    got = pv.frame(cam, 60).read()
    _assert_frame(got, want[0], "full HD at scale 2")
    assert np.array_equal(got["rgba8"], api.resolve(want[0][3], 1)[0])
    print("full HD frame at scale 2, stage times (ms):", pv.stats())
    pv.close(); gs.close()
