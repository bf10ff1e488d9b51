"""The pt_preview session with the responsive history on (pt_preview_set_respond), at 40 x 24 as tests/test_preview_motion.py: every
temporal frame with a history equals the chain of host calls with pt_temporal_accumulate_respond, bit for bit; first frames and
converging frames are the session without the option; turning the option off restores the base frames; a change of value does not
reset the session."""
import numpy as np
import pytest

import motion_cases as MC
from test_preview import _assert_frame
from test_temporal import _cams
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SPP, BATCHES, DEPTH = 4, 2, 4
W, H = MC.W, MC.H
BEFORE, AFTER = 3, 2
LIGHT = (20, 24, (0.3, 0.0, 0.0))


@pytest.fixture(scope="module")
def host(api, gpu_ready, scene_dir):
    return MC.cornell_host(api, scene_dir, "respond_pv")


def _params(**kw):
    return dict(spp=SPP, batches=BATCHES, max_depth=DEPTH, **kw)


def _same_frame(got, want, what):
    _assert_frame(got, (want["mean"], want["hist"], want["hist_len"], None), what)
    assert np.array_equal(got["rgba8"], want["rgba8"]), what + ": bytes"


def _chain_step(api, gs, state, cam, seed, centre, scale, changed, motion_frame, respond):
    """One frame through the host API, as include/pt_api.h states it (RESPOND): the accumulation of a frame with a history is
    pt_temporal_accumulate_respond with the arguments of the form the frame would have taken. state = (hist, hist_len, prev albedo,
    prev guide, prev camera). Returns the new state, (mean, hist, hist_len, filtered) and lambda (None on a first frame)."""
    hist, ln, prev_a, prev_n, prev_cam = state
    aovs = (lambda c, w, h: gs.render_aovs_centre(c, w, h, 0)) if centre else (lambda c, w, h: gs.render_aovs(c, w, h, aov_spp=1, seed=seed))
    mv = None
    rests = centre and not changed and prev_cam is not None and cam.tobytes() == prev_cam.tobytes()  # (a changed scene traces its guide again)
    if rests:
        A, N = prev_a, prev_n
    elif motion_frame and centre:
        A, N, mv = gs.render_motion(cam, W, H, guides=True)
    else:
        A, N = aovs(cam, W, H)
        if motion_frame:
            mv = gs.render_motion(cam, W, H)
    lam = None
    past = dict(camera_prev=prev_cam, prev_normal_depth=prev_n, hist=hist, hist_len=ln)
    if scale == 1:
        S, Qs = gs.render_moments(cam, W, H, SPP, SPP // BATCHES, DEPTH, seed=seed)
        if hist is None:
            hist, ln = api.temporal_accumulate(cam, S, Qs, SPP, BATCHES, A, N)
        else:
            hist, ln, lam = api.temporal_accumulate_respond(cam, N, S, Qs, SPP, BATCHES, A, motion=mv, **past, **respond)
    else:
        lo = api.scaled_camera(cam, scale)
        S, Qs = gs.render_moments(lo, W // scale, H // scale, SPP, SPP // BATCHES, DEPTH, seed=seed)
        Al, Nl = api.guide_subsample(scale, A, N) if centre else aovs(lo, W // scale, H // scale)
        cur = api.upsample(scale, S, Qs, SPP, BATCHES, Al, Nl, A, N)
        if hist is None:
            hist, ln = api.temporal_accumulate_cur(cam, cur, N)
        else:
            hist, ln, lam = api.temporal_accumulate_respond(cam, N, cur=cur, motion=mv, **past, **respond)
    filt = api.denoise_hist(hist, A, N)
    return (hist, ln, A, N, cam), (api.finalise(filt, 1), hist, ln, filt), lam


# ---- (a) a frame with a history is the chain of host calls -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,centre,scale,kind,motion,change", [
    ("normal", 0, 1, "pinhole", 0, None),                    # jittered guides, a moving camera
    ("scale 2", 0, 2, "pinhole", 0, None),                   # the cur form on pt_upsample's output
    ("motion", 1, 1, "pinhole", 1, "box"),                   # a motion frame: the _motion form's arguments
    ("motion, scale 2", 1, 2, "pinhole", 1, "box"),          # ... and the _cur_motion form's
    ("moved light", 0, 1, "identity", 0, "light"),           # keep_history 1 after a moved light: the case the option is for
    ("centre", 1, 1, "identity", 0, "light")])               # centre guides: a resting camera reuses its guide, the identity path
def test_frames_equal_the_chain_of_host_calls(api, host, name, centre, scale, kind, motion, change):
    cams = _cams(api, kind, W, H, BEFORE + AFTER)
    seeds = [70 + t for t in range(BEFORE + AFTER)]
    respond = dict(threshold=2.0, radius=2, power=2) if scale == 2 else api.respond_defaults()
    moves = {"box": [MC.moved_arrays(host)["points"], MC.moved_arrays(host, shift=(0.32, 0.0, 0.22))["points"]],
             "light": [MC.moved_arrays(host, *LIGHT)["points"], MC.moved_arrays(host, 20, 24, (0.45, 0.0, 0.0))["points"]]}
    sc = api.Scene.from_mesh(host)
    pv = api.Preview(sc, W, H, **_params()).set_scale(scale).set_guide_centre(centre).set_motion(motion).set_respond(**respond)
    assert pv.respond() == dict(api.respond_defaults(), **respond)
    state = (None,) * 5
    shortened = 0
    for t, (cam, seed) in enumerate(zip(cams, seeds)):
        changed = change is not None and t >= BEFORE
        if changed:
            sc.update_vertices(moves[change][t - BEFORE])
            pv.scene_changed(True)
        state, want, lam = _chain_step(api, sc, state, cam, seed, centre, scale, changed, bool(changed and motion), respond)
        got = pv.frame(cam, seed).read()
        what = "%s frame %d" % (name, t)
        _assert_frame(got, want, what)
        assert np.array_equal(got["rgba8"], api.resolve(want[3], 1)[0]), what
        assert (lam is None) == (t == 0)
        if changed:
            shortened += int((lam < 1).sum())
            st = pv.stats()
            assert np.isfinite(st["accumulate_ms"]) and st["accumulate_ms"] > 0
    print("%s: lambda < 1 on %d pixels of the frames after the change" % (name, shortened))
    if change == "light":
        assert shortened >= 20                               # the moved light is seen (a condition on the input)
    pv.close(); sc.close()


# ---- (b) frames the option leaves alone ----------------------------------------------------------------------------------------------------
def test_first_and_converging_frames_equal_the_session_without_the_option(api, host):
    """A resting camera with converge on: frame 0 is a first frame, the others are converging frames, which the option does not touch."""
    cam = _cams(api, "identity", W, H, 1)[0]
    sc = api.Scene.from_mesh(host)
    pvs = [api.Preview(sc, W, H, **_params()).set_guide_centre(1).set_converge(0.5, 2) for _ in range(2)]
    pvs[1].set_respond(threshold=1.5, radius=3, power=4)     # (a setting that shortens many pixels by chance wherever it runs)
    for t in range(4):
        off, on = (pv.frame(api.Camera.frombytes(cam.tobytes()), 90 + t).read() for pv in pvs)
        _same_frame(on, off, "frame %d" % t)
        assert pvs[0].last_live() == pvs[1].last_live()
    # ... and a temporal-0 session has no history stage at all
    flat = [api.Preview(sc, W, H, **_params(temporal=0)) for _ in range(2)]
    flat[1].set_respond()
    for t in range(2):
        a, b = (pv.frame(cam, 95 + t).read() for pv in flat)
        assert_bits_equal(b["mean"], a["mean"], "temporal 0, frame %d" % t)
    for pv in pvs + flat:
        pv.close()
    sc.close()


# ---- (c), (d) the switch ---------------------------------------------------------------------------------------------------------------------
def test_turning_the_option_off_restores_the_base_frames_and_no_change_of_value_resets(api, host):
    cams = _cams(api, "pinhole", W, H, 5)
    sc = api.Scene.from_mesh(host)
    pv = api.Preview(sc, W, H, **_params())
    ref = api.Preview(sc, W, H, **_params())
    assert pv.respond() is None
    for t in range(2):
        pv.frame(cams[t], 80 + t); ref.frame(cams[t], 80 + t)
    before = pv.read()
    pv.set_respond(threshold=1.5, radius=1, power=1)
    assert pv.respond() == {"radius": 1, "power": 1, "threshold": 1.5}
    for k in ("mean", "hist", "hist_len"):
        assert_bits_equal(pv.read()[k], before[k], k + " after set_respond")
    for bad, msg in ((dict(radius=4), "radius 4"), (dict(power=3), "power 3"), (dict(threshold=0.0), "threshold must be positive")):
        with pytest.raises(api.PtError, match=msg):
            pv.set_respond(**bad)
        assert pv.respond() == {"radius": 1, "power": 1, "threshold": 1.5}
    on = pv.frame(cams[2], 82).read()
    base = ref.frame(cams[2], 82).read()
    assert on["hist_len"].max() > 2                          # no reset: the third frame blends into two frames of history
    assert not np.array_equal(on["hist_len"], base["hist_len"])                # k = 1.5 shortens some pixels by chance
    pv.set_respond(threshold=6.0)                            # another value: still no reset
    pv.frame(cams[3], 83); ref.frame(cams[3], 83)
    assert pv.read()["hist_len"].max() > 3
    # off again: from the same history the frames are the base session's (the history is handed over through a fresh pair)
    pv.set_respond(False)
    assert pv.respond() is None
    pv2 = api.Preview(sc, W, H, **_params()); ref2 = api.Preview(sc, W, H, **_params())
    pv2.set_respond(threshold=float("inf"))                  # an infinite threshold is the base function: both sessions hold one history
    for t in range(3):
        pv2.frame(cams[t], 60 + t); ref2.frame(cams[t], 60 + t)
    _same_frame(pv2.read(), ref2.read(), "threshold inf")
    pv2.set_respond(threshold=1.5); pv2.set_respond(False)
    _same_frame(pv2.frame(cams[3], 63).read(), ref2.frame(cams[3], 63).read(), "the frame after the option was turned off")
    for p in (pv, ref, pv2, ref2):
        p.close()
    sc.close()
