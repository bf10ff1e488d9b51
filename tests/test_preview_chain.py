"""The pt_preview session with a guide chain against the chain of host calls it stands for: test_preview.py's and
test_preview_scaled.py's chains with render_aovs_chain in place of render_aovs, bit for bit, on a glass + mirror Cornell box."""
import os

import numpy as np
import pytest

import temporal_seq as Q
from test_preview import _assert_frame
from test_temporal import _cams

pytestmark = pytest.mark.gpu

SPP, BATCHES, DEPTH = 4, 2, 4
W, H = 40, 24
LINKS = 8


@pytest.fixture(scope="module")
def scene(api, gpu_ready, scene_dir):
    from cudapathtracer_amd import scenes
    cfg = scenes.cornell(os.path.join(scene_dir, "pvchain"), width=W, height=H, name="pvchain", spp=SPP, max_depth=DEPTH, tall_material=5,
                         short_material=19)["config"]
    return api.Scene(api.HostScene(cfg))


def _params(**kw):
    return dict(spp=SPP, batches=BATCHES, max_depth=DEPTH, **kw)


def _host_chain(api, gs, cams, seeds, scale, links):
    """Per frame (mean, hist, hist_len, filtered) through the host API; links 0 takes render_aovs, as a session without a chain does."""
    def aovs(cam, w, h, seed):
        if links == 0:
            return gs.render_aovs(cam, w, h, aov_spp=1, seed=seed)
        return gs.render_aovs_chain(cam, w, h, links, aov_spp=1, seed=seed)

    hist = ln = prev_n = prev_cam = None
    out = []
    for cam, seed in zip(cams, seeds):
        A, N = aovs(cam, W, H, seed)
        if scale == 1:
            S, Qs = gs.render_moments(cam, W, H, SPP, SPP // BATCHES, DEPTH, seed=seed)
            hist, ln = api.temporal_accumulate(cam, S, Qs, SPP, BATCHES, A, N, prev_cam, prev_n, hist, ln)
        else:
            lo = api.scaled_camera(cam, scale)
            S, Qs = gs.render_moments(lo, W // scale, H // scale, SPP, SPP // BATCHES, DEPTH, seed=seed)
            Al, Nl = aovs(lo, W // scale, H // scale, seed)
            hist, ln = api.temporal_accumulate_cur(cam, api.upsample(scale, S, Qs, SPP, BATCHES, Al, Nl, A, N), N, prev_cam, prev_n, hist, ln)
        prev_n, prev_cam = N, cam
        filt = api.denoise_hist(hist, A, N)
        out.append((api.finalise(filt, 1), hist, ln, filt))
    return out


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("kind", ["pinhole", "identity"])
def test_chain_session_equals_the_host_chain_after_every_frame(api, scene, kind, scale):
    cams = _cams(api, kind, W, H, 3)
    seeds = [Q.SEED0 + t for t in range(3)]
    want = _host_chain(api, scene, cams, seeds, scale, LINKS)
    plain = _host_chain(api, scene, cams[:1], seeds[:1], scale, 0)
    assert not np.array_equal(want[0][1], plain[0][1])     # the scene has specular pixels: chain guides change the frame
    pv = api.Preview(scene, W, H, **_params()).set_scale(scale).set_guide_chain(LINKS)
    assert pv.guide_chain == LINKS
    for t, (cam, seed) in enumerate(zip(cams, seeds)):
        got = pv.frame(cam, seed).read()
        what = "%s scale %d frame %d" % (kind, scale, t)
        _assert_frame(got, want[t], what)
        assert np.array_equal(got["rgba8"], api.resolve(want[t][3], 1)[0]), what
    if kind == "identity":
        assert got["hist_len"].max() == 3
    pv.close()


def test_a_converging_frame_takes_the_chain_pass_too(api, scene):
    """A resting camera with converge on (test_converge.py's chain): select, moments on the live list, the CHAIN pass on the whole
    frame, the accumulation with the live map."""
    thr, mh = 0.05, 2
    cams = _cams(api, "identity", W, H, 4)
    seeds = [50 + t for t in range(4)]
    pv = api.Preview(scene, W, H, **_params()).set_guide_chain(LINKS).set_converge(thr, mh)
    hist = ln = prev_n = None
    converging = 0
    for t, (cam, seed) in enumerate(zip(cams, seeds)):
        pv.frame(cam, seed)
        A, N = scene.render_aovs_chain(cam, W, H, LINKS, aov_spp=1, seed=seed)
        if hist is None:
            S, Qs = scene.render_moments(cam, W, H, SPP, SPP // BATCHES, DEPTH, seed=seed)
            hist, ln = api.temporal_accumulate(cam, S, Qs, SPP, BATCHES, A, N, None, None, None, None)
        else:
            _, live, lst = api.temporal_select(hist, ln, thr, mh)
            S, Qs = scene.render_moments_tiles(cam, W, H, SPP, SPP // BATCHES, DEPTH, lst, seed=seed) if lst.size else (np.zeros((H, W, 4), np.float32),) * 2
            hist, ln = api.temporal_accumulate_live(cam, S, Qs, SPP, BATCHES, A, N, prev_n, hist, ln, live, camera_prev=cam)
            converging += 1
            assert pv.last_live()[0] == lst.size
        prev_n = N
        _assert_frame(pv.read(), (api.finalise(api.denoise_hist(hist, A, N), 1), hist, ln, None), "converging frame %d" % t)
    assert converging == 3
    pv.close()


def test_changing_the_chain_resets_the_history(api, scene):
    cams = _cams(api, "pinhole", W, H, 4)
    seeds = [70 + t for t in range(4)]
    pv = api.Preview(scene, W, H, **_params())
    assert pv.guide_chain == 0
    pv.set_guide_chain(LINKS)
    for t in range(2):
        pv.frame(cams[t], seeds[t])
    assert pv.read()["hist_len"].max() == 2
    pv.set_guide_chain(LINKS)                              # the current value: nothing changes
    assert pv.read()["hist_len"].max() == 2
    pv.set_guide_chain(0)
    with pytest.raises(api.PtError, match="no frame"):
        pv.read()
    fresh = api.Preview(scene, W, H, **_params())
    for t in (2, 3):
        got, want = pv.frame(cams[t], seeds[t]).read(), fresh.frame(cams[t], seeds[t]).read()
        _assert_frame(got, (want["mean"], want["hist"], want["hist_len"], None), "frame %d after set_guide_chain(0)" % t)
        assert np.array_equal(got["rgba8"], want["rgba8"])
    assert got["hist_len"].max() == 2
    for bad in (-1, 17):
        with pytest.raises(api.PtError, match="max_links %d must be 0..16" % bad):
            pv.set_guide_chain(bad)
        assert pv.guide_chain == 0
    pv.close(); fresh.close()


@pytest.mark.parametrize("scale", [1, 2])
def test_the_default_session_is_unchanged(api, scene, scale):
    """A session that never heard of the setter, and one told 0, are the first-hit chain of host calls."""
    cams = _cams(api, "pinhole", W, H, 3)
    seeds = [90 + t for t in range(3)]
    want = _host_chain(api, scene, cams, seeds, scale, 0)
    never, zero = api.Preview(scene, W, H, **_params()).set_scale(scale), api.Preview(scene, W, H, **_params()).set_scale(scale).set_guide_chain(0)
    for t in range(3):
        _assert_frame(never.frame(cams[t], seeds[t]).read(), want[t], "default session, scale %d frame %d" % (scale, t))
        _assert_frame(zero.frame(cams[t], seeds[t]).read(), want[t], "set_guide_chain(0), scale %d frame %d" % (scale, t))
    never.close(); zero.close()
