"""The pt_preview session with the motion-chain switch (pt_preview_set_motion_chain), on scene A of tests/motion_chain_cases.py at
64 x 40 with 3 + 2 frames as tests/test_preview_motion.py: with the switch on, the motion frames of a session with a guide chain
equal the chain of host calls with pt_render_motion_chain, bit for bit; with it off, or with guide chain 0, every frame is that of a
session that never heard of the switch."""
import numpy as np
import pytest

import motion_chain_cases as CC
from test_preview import _assert_frame
from test_temporal import _cams
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SPP, BATCHES, DEPTH = 4, 2, 4
W, H = CC.W, CC.H
BEFORE, AFTER = 3, 2
RESPOND = dict(threshold=1.5, radius=1, power=1)


@pytest.fixture(scope="module")
def host(api, gpu_ready, scene_dir):
    return CC.scene_a(api, scene_dir, "mchain_pv")


@pytest.fixture(scope="module")
def moves(host):
    """The box pushed aside, then pushed further: the points of the two updates."""
    return [CC.moved_box(host)["points"], CC.moved_box(host, shift=(0.32, 0.0, 0.22))["points"]]


def _params(**kw):
    return dict(spp=SPP, batches=BATCHES, max_depth=DEPTH, **kw)


def _same_frame(got, want, what):
    _assert_frame(got, (want["mean"], want["hist"], want["hist_len"], None), what)
    assert np.array_equal(got["rgba8"], want["rgba8"]), what + ": bytes"


def _chain_step(api, gs, state, cam, seed, centre, links, scale, motion_frame, respond):
    """One frame through the host API, as include/pt_api.h states it (MOTION CHAIN); state = (hist, hist_len, prev albedo, prev guide,
    prev camera). Returns the new state, (mean, hist, hist_len, filtered), the motion buffer and the number of feature-pass launches."""
    hist, ln, prev_a, prev_n, prev_cam = state

    def aovs(c, w, h):
        return gs.render_aovs_centre(c, w, h, links) if centre else gs.render_aovs_chain(c, w, h, links, aov_spp=1, seed=seed)

    mv, passes = None, 0
    rests = centre and not motion_frame and prev_cam is not None and cam.tobytes() == prev_cam.tobytes()
    if rests:
        A, N = prev_a, prev_n
    elif motion_frame and centre:
        A, N, mv = gs.render_motion_chain(cam, W, H, links, guides=True)     # one trace serves the chain guide and the motion
        passes += 1
    else:
        A, N = aovs(cam, W, H)
        passes += 1
        if motion_frame:
            mv = gs.render_motion_chain(cam, W, H, links)
            passes += 1
    past = dict(camera_prev=prev_cam, prev_normal_depth=prev_n, hist=hist, hist_len=ln)
    if scale == 1:
        S, Qs = gs.render_moments(cam, W, H, SPP, SPP // BATCHES, DEPTH, seed=seed)
        if respond and hist is not None:
            hist, ln, _ = api.temporal_accumulate_respond(cam, N, S, Qs, SPP, BATCHES, A, motion=mv, **past, **respond)
        else:
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
        if respond and hist is not None:
            hist, ln, _ = api.temporal_accumulate_respond(cam, N, cur=cur, motion=mv, **past, **respond)
        else:
            hist, ln = api.temporal_accumulate_cur_motion(cam, cur, N, prev_cam, prev_n, hist, ln, motion=mv)
    filt = api.denoise_hist(hist, A, N)
    return (hist, ln, A, N, cam), (api.finalise(filt, 1), hist, ln, filt), mv, passes


# ---- a motion frame with the switch on is the chain of host calls ----------------------------------------------------------------------
@pytest.mark.parametrize("centre,links,scale,kind,respond,rise", [
    (0, 2, 1, "pinhole", False, 2),      # jittered guides: the chain pass, then the motion-chain pass
    (1, 2, 1, "identity", False, 1),     # centre guides: ONE fused pass; a camera that rests
    (1, 2, 1, "pinhole", False, 1),
    (1, 8, 1, "pinhole", False, 1),
    (0, 8, 2, "pinhole", False, 3),      # scale 2: the low-res chain, the display chain, the motion-chain pass
    (1, 2, 2, "pinhole", False, 1),      # ... with centre guides the subsample is no pass
    (1, 8, 2, "identity", False, 1),
    (1, 2, 1, "pinhole", True, 1)])      # respond on: the same passes, the other accumulate call
def test_motion_frames_equal_the_chain_of_host_calls(api, host, moves, centre, links, scale, kind, respond, rise):
    cams = _cams(api, kind, W, H, BEFORE + AFTER)
    seeds = [70 + t for t in range(BEFORE + AFTER)]
    sc = api.Scene.from_mesh(host)
    pv = api.Preview(sc, W, H, **_params()).set_scale(scale).set_guide_chain(links).set_guide_centre(centre).set_motion(1).set_motion_chain(1)
    if respond:
        pv.set_respond(**RESPOND)
    assert pv.motion == 1 and pv.motion_chain == 1
    state = (None,) * 5
    for t, (cam, seed) in enumerate(zip(cams, seeds)):
        changed = t >= BEFORE
        if changed:
            sc.update_vertices(moves[t - BEFORE])
            pv.scene_changed(True)
        state, want, mv, passes = _chain_step(api, sc, state, cam, seed, centre, links, scale, changed, RESPOND if respond else None)
        before = pv.guide_passes
        got = pv.frame(cam, seed).read()
        what = "centre %d links %d scale %d %s respond %d frame %d" % (centre, links, scale, kind, respond, t)
        _assert_frame(got, want, what)
        assert np.array_equal(got["rgba8"], api.resolve(want[3], 1)[0]), what
        assert pv.guide_passes - before == passes, what
        if changed:
            assert passes == rise, what
            st = pv.stats()
            assert np.isfinite(st["aov_ms"]) and st["aov_ms"] > 0
    # the last motion frame saw the box through the mirror, and those pixels found history
    ln = sc.render_aovs_centre(cams[-1], W, H, links, links=True)[2]
    through = (ln >= 1) & (mv[..., 3] == 1)
    print("%d pixels through the mirror, %d of them with history" % (through.sum(), (got["hist_len"][through] > 1).sum()))
    assert through.sum() >= 12                               # oracle: 16 to 19 over these cameras
    if centre and kind == "identity":                        # (the CPU test's case: 12 rescued pixels by the oracle)
        assert (got["hist_len"][through] > 1).sum() >= 6
    pv.close(); sc.close()


def test_the_switch_changes_the_motion_frame_of_a_chain_session(api, host, moves):
    """A still camera, centre guides, chain 2: with the switch the pixels that show the box in the mirror gain history."""
    cam = _cams(api, "identity", W, H, 1)[0]
    out = []
    for chain in (0, 1):
        sc = api.Scene.from_mesh(host)
        pv = api.Preview(sc, W, H, **_params()).set_guide_chain(2).set_guide_centre(1).set_motion(1).set_motion_chain(chain)
        for t in range(BEFORE):
            pv.frame(api.Camera.frombytes(cam.tobytes()), 40 + t)
        sc.update_vertices(moves[0])
        pv.scene_changed(True)
        before = pv.guide_passes
        out.append(pv.frame(api.Camera.frombytes(cam.tobytes()), 43).read())
        assert pv.guide_passes - before == (1 if chain else 2)             # the fused pass counts as one
        _, _, mv, ln = sc.render_motion_chain(cam, W, H, 2, guides=True, links=True)
        pv.close(); sc.close()
    through = (ln >= 1) & (mv[..., 3] == 1)
    off, on = out
    assert_bits_equal(on["hist"][~through], off["hist"][~through], "every other pixel")
    assert_bits_equal(on["hist_len"][~through], off["hist_len"][~through], "every other pixel's length")
    gained = through & (on["hist_len"] > 1) & (off["hist_len"] == 1)
    print("through the mirror %d, with history: switch on %d, off %d, gained %d" % (through.sum(), (on["hist_len"][through] > 1).sum(),
                                                                                    (off["hist_len"][through] > 1).sum(), gained.sum()))
    assert gained.sum() >= 6                                 # the CPU test's rescued pixels: 12 by the oracle


# ---- the switch off, and guide chain 0 with the switch on -------------------------------------------------------------------------------
@pytest.mark.parametrize("centre,links,chain", [(1, 2, 0), (0, 2, 0), (1, 0, 1), (0, 0, 1)])
def test_switch_off_and_chain_0_equal_a_session_without_the_switch(api, host, moves, centre, links, chain):
    cams = _cams(api, "pinhole", W, H, BEFORE + AFTER)
    seeds = [50 + t for t in range(BEFORE + AFTER)]
    scs = [api.Scene.from_mesh(host) for _ in range(2)]
    pvs = [api.Preview(sc, W, H, **_params()).set_guide_chain(links).set_guide_centre(centre).set_motion(1) for sc in scs]
    pvs[1].set_motion_chain(1); pvs[1].set_motion_chain(chain)      # (set and, for the first two cases, cleared again: no reset either way)
    assert pvs[0].motion_chain == 0 and pvs[1].motion_chain == chain
    for t in range(BEFORE + AFTER):
        if t >= BEFORE:
            for sc, pv in zip(scs, pvs):
                sc.update_vertices(moves[t - BEFORE])
                pv.scene_changed(True)
        never, other = (pv.frame(cams[t], seeds[t]).read() for pv in pvs)
        _same_frame(other, never, "centre %d links %d chain %d frame %d" % (centre, links, chain, t))
    assert pvs[0].guide_passes == pvs[1].guide_passes
    assert never["hist_len"].max() > BEFORE                  # the history was kept through both updates
    for pv in pvs:
        pv.close()
    for sc in scs:
        sc.close()


def test_the_switch_does_not_reset_and_refuses_other_values(api, host):
    cams = _cams(api, "pinhole", W, H, 3)
    sc = api.Scene.from_mesh(host)
    pv = api.Preview(sc, W, H, **_params()).set_guide_chain(2)
    ref = api.Preview(sc, W, H, **_params()).set_guide_chain(2)
    assert pv.motion_chain == 0
    for t in range(2):
        pv.frame(cams[t], 80 + t); ref.frame(cams[t], 80 + t)
    before = pv.read()
    assert before["hist_len"].max() == 2
    pv.set_motion_chain(1)
    assert pv.motion_chain == 1 and pv.motion == 0           # (a switch of its own: it does not turn motion on)
    for k in ("mean", "hist", "hist_len"):
        assert_bits_equal(pv.read()[k], before[k], k + " after set_motion_chain(1)")
    with pytest.raises(api.PtError, match="on 2 must be 0 or 1"):
        pv.set_motion_chain(2)
    with pytest.raises(api.PtError, match="on 2 must be 0 or 1"):
        pv.set_motion(2)
    assert pv.motion_chain == 1
    _same_frame(pv.frame(cams[2], 82).read(), ref.frame(cams[2], 82).read(), "the frame after the switch")
    assert pv.read()["hist_len"].max() > 2
    pv.close(); ref.close(); sc.close()
