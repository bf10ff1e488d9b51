"""The pt_preview session with motion on (pt_preview_set_motion), at 40 x 24 with 3 + 2 frames as tests/test_preview_update.py: the
frames after an announced vertex update equal the chain of host calls with pt_render_motion and pt_temporal_accumulate[_cur]_motion,
bit for bit; every other frame is the session without the option."""
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


@pytest.fixture(scope="module")
def host(api, gpu_ready, scene_dir):
    return MC.cornell_host(api, scene_dir, "motion_pv")


@pytest.fixture(scope="module")
def moves(host):
    """The tall box pushed aside, then pushed further: the points of the two updates."""
    return [MC.moved_arrays(host)["points"], MC.moved_arrays(host, shift=(0.32, 0.0, 0.22))["points"]]


def _params(**kw):
    return dict(spp=SPP, batches=BATCHES, max_depth=DEPTH, **kw)


def _same_frame(got, want, what):
    _assert_frame(got, (want["mean"], want["hist"], want["hist_len"], None), what)
    assert np.array_equal(got["rgba8"], want["rgba8"]), what + ": bytes"


def _chain_step(api, gs, state, cam, seed, centre, links, scale, motion_frame):
    """One frame through the host API, as include/pt_api.h states it (MOTION); state = (hist, hist_len, prev albedo, prev guide,
    prev camera). Returns the new state, (mean, hist, hist_len, filtered) and the number of feature-pass launches."""
    hist, ln, prev_a, prev_n, prev_cam = state

    def aovs(c, w, h):
        if centre:
            return gs.render_aovs_centre(c, w, h, links)
        return gs.render_aovs_chain(c, w, h, links, aov_spp=1, seed=seed) if links else gs.render_aovs(c, w, h, aov_spp=1, seed=seed)

    mv, passes = None, 0
    rests = centre and not motion_frame and prev_cam is not None and cam.tobytes() == prev_cam.tobytes()
    if rests:
        A, N = prev_a, prev_n
    elif motion_frame and centre and links == 0:
        A, N, mv = gs.render_motion(cam, W, H, guides=True)                  # one trace serves the guide and the motion
        passes += 1
    else:
        A, N = aovs(cam, W, H)
        passes += 1
        if motion_frame:
            mv = gs.render_motion(cam, W, H)
            passes += 1
    if scale == 1:
        S, Qs = gs.render_moments(cam, W, H, SPP, SPP // BATCHES, DEPTH, seed=seed)
        hist, ln = api.temporal_accumulate_motion(cam, S, Qs, SPP, BATCHES, A, N, prev_cam, prev_n, hist, ln, motion=mv)
    else:
        lo = api.scaled_camera(cam, scale)
        S, Qs = gs.render_moments(lo, W // scale, H // scale, SPP, SPP // BATCHES, DEPTH, seed=seed)
        if centre:
            Al, Nl = api.guide_subsample(scale, A, N)
        else:
            Al, Nl = aovs(lo, W // scale, H // scale)
            passes += 1
        cur = api.upsample(scale, S, Qs, SPP, BATCHES, Al, Nl, A, N)
        hist, ln = api.temporal_accumulate_cur_motion(cam, cur, N, prev_cam, prev_n, hist, ln, motion=mv)
    filt = api.denoise_hist(hist, A, N)
    return (hist, ln, A, N, cam), (api.finalise(filt, 1), hist, ln, filt), passes


# ---- (a) a motion frame is the chain of host calls ------------------------------------------------------------------------------------
@pytest.mark.parametrize("centre,links,scale,kind,rise", [
    (0, 0, 1, "pinhole", 2),       # jittered guides: the guide pass, then the motion pass
    (1, 0, 1, "identity", 1),      # centre guides: one fused pass; a camera that rests takes the identity path for its static pixels
    (1, 0, 1, "pinhole", 1),
    (1, 2, 1, "pinhole", 2),       # a guide chain: the chain pass, then the motion pass
    (0, 0, 2, "pinhole", 3),       # scale 2: the low-res guide, the display guide, the motion pass
    (1, 0, 2, "pinhole", 1),       # ... with centre guides the subsample is no pass
    (0, 2, 2, "pinhole", 3),       # scale 2 with a guide chain: the low-res chain, the display chain, the motion pass
    (1, 2, 2, "pinhole", 2)])      # ... with centre guides: the centre chain, the motion pass
def test_motion_frames_equal_the_chain_of_host_calls(api, host, moves, centre, links, scale, kind, rise):
    cams = _cams(api, kind, W, H, BEFORE + AFTER)
    seeds = [70 + t for t in range(BEFORE + AFTER)]
    sc = api.Scene.from_mesh(host)
    pv = api.Preview(sc, W, H, **_params()).set_scale(scale).set_guide_chain(links).set_guide_centre(centre).set_motion(1)
    assert pv.motion == 1
    state = (None,) * 5
    for t, (cam, seed) in enumerate(zip(cams, seeds)):
        changed = t >= BEFORE
        if changed:
            sc.update_vertices(moves[t - BEFORE])
            pv.scene_changed(True)
        state, want, passes = _chain_step(api, sc, state, cam, seed, centre, links, scale, changed)
        before = pv.guide_passes
        got = pv.frame(cam, seed).read()
        what = "centre %d links %d scale %d %s frame %d" % (centre, links, scale, kind, t)
        _assert_frame(got, want, what)
        assert np.array_equal(got["rgba8"], api.resolve(want[3], 1)[0]), what
        assert pv.guide_passes - before == passes, what
        if changed:
            assert passes == rise, what
            st = pv.stats()
            assert np.isfinite(st["aov_ms"]) and st["aov_ms"] > 0
    # the motion frames found history on the moved box's pixels (not with a guide chain: the box is glass, its chain guide is the
    # surface behind it, and motion through glass is out of scope)
    mv = sc.render_motion(cams[-1], W, H)
    moved = mv[..., 3] == 1
    assert moved.sum() >= 16 and (links > 0 or (got["hist_len"][moved] > 1).sum() >= 4)
    pv.close(); sc.close()


def test_motion_frames_differ_from_the_session_without_the_option(api, host, moves):
    """A still camera: without the option a moved pixel keeps history only where the old guide happens to agree."""
    cam = _cams(api, "identity", W, H, 1)[0]
    out = []
    for motion in (0, 1):
        sc = api.Scene.from_mesh(host)
        pv = api.Preview(sc, W, H, **_params()).set_guide_centre(1).set_motion(motion)
        for t in range(BEFORE):
            pv.frame(api.Camera.frombytes(cam.tobytes()), 40 + t)
        sc.update_vertices(moves[0])
        pv.scene_changed(True)
        out.append(pv.frame(api.Camera.frombytes(cam.tobytes()), 43).read())
        mv = sc.render_motion(cam, W, H)
        pv.close(); sc.close()
    moved = mv[..., 3] == 1
    off, on = out
    assert_bits_equal(on["hist"][~moved], off["hist"][~moved], "static pixels")
    assert_bits_equal(on["hist_len"][~moved], off["hist_len"][~moved], "static pixels' lengths")
    gained = moved & (on["hist_len"] > 1) & (off["hist_len"] == 1)
    print("moved %d, with history: motion on %d, off %d, gained %d" % (moved.sum(), (on["hist_len"][moved] > 1).sum(),
                                                                       (off["hist_len"][moved] > 1).sum(), gained.sum()))
    assert gained.sum() >= 4


# ---- (b) frames that are no motion frames ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["no_update", "keep_history_0", "unannounced"])
def test_other_frames_equal_the_session_without_the_option(api, host, moves, what):
    cams = _cams(api, "pinhole", W, H, BEFORE + AFTER)
    seeds = [50 + t for t in range(BEFORE + AFTER)]
    scs = [api.Scene.from_mesh(host) for _ in range(2)]
    pvs = [api.Preview(sc, W, H, **_params()).set_motion(on) for sc, on in zip(scs, (0, 1))]
    for t in range(BEFORE + AFTER):
        if t == BEFORE and what != "no_update":
            for sc, pv in zip(scs, pvs):
                sc.update_vertices(moves[0])
                if what == "keep_history_0":
                    pv.scene_changed(False)
        off, on = (pv.frame(cams[t], seeds[t]).read() for pv in pvs)
        _same_frame(on, off, "%s frame %d" % (what, t))
    assert pvs[0].guide_passes == pvs[1].guide_passes == BEFORE + AFTER       # no motion pass was launched
    # (a moving camera's lengths are bilinear means of its taps' lengths, so not whole numbers)
    assert on["hist_len"].max() > BEFORE if what == "no_update" else on["hist_len"].max() < AFTER + 0.01
    for pv in pvs:
        pv.close()
    for sc in scs:
        sc.close()


# ---- (c) a generation that jumped by two ----------------------------------------------------------------------------------------------
def test_two_updates_before_one_frame_take_the_path_without_motion(api, host, moves):
    cams = _cams(api, "pinhole", W, H, BEFORE + 1)
    scs = [api.Scene.from_mesh(host) for _ in range(2)]
    pvs = [api.Preview(sc, W, H, **_params()).set_motion(on) for sc, on in zip(scs, (0, 1))]
    for t in range(BEFORE):
        for pv in pvs:
            pv.frame(cams[t], 30 + t)
    for sc, pv in zip(scs, pvs):
        sc.update_vertices(moves[0]); sc.update_vertices(moves[1])
        assert sc.has_motion == 1                             # the motion spans one update only: not what the session's history saw
        pv.scene_changed(True)
    off, on = (pv.frame(cams[BEFORE], 33).read() for pv in pvs)
    _same_frame(on, off, "generation + 2")
    assert pvs[1].guide_passes == BEFORE + 1 and on["hist_len"].max() > 1     # keep_history 1: the history was kept
    for pv in pvs:
        pv.close()
    for sc in scs:
        sc.close()


# ---- (d) the switch ---------------------------------------------------------------------------------------------------------------------
def test_toggling_motion_does_not_reset_the_history(api, host):
    cams = _cams(api, "pinhole", W, H, 3)
    sc = api.Scene.from_mesh(host)
    pv = api.Preview(sc, W, H, **_params())
    ref = api.Preview(sc, W, H, **_params())
    assert pv.motion == 0
    for t in range(2):
        pv.frame(cams[t], 80 + t); ref.frame(cams[t], 80 + t)
    before = pv.read()
    assert before["hist_len"].max() == 2
    pv.set_motion(1)
    assert pv.motion == 1
    for k in ("mean", "hist", "hist_len"):
        assert_bits_equal(pv.read()[k], before[k], k + " after set_motion(1)")
    with pytest.raises(api.PtError, match="on 2 must be 0 or 1"):
        pv.set_motion(2)
    assert pv.motion == 1
    pv.set_motion(0); pv.set_motion(1)
    _same_frame(pv.frame(cams[2], 82).read(), ref.frame(cams[2], 82).read(), "the frame after the toggles")
    assert pv.read()["hist_len"].max() > 2
    pv.close(); ref.close(); sc.close()
