"""pt_render_adaptive on the GPU: the schedule replayed exactly (tests/adaptive_ref.py) against the CPU reference and against
pt_render's partial sums, through the production kernel instantiations in list mode, plus boundary and isolation cases."""
import os

import numpy as np
import pytest

import adaptive_ref as R
from conftest import golden_scene
from denoise_ref import denoise as denoise_ref
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SEED = 103033


def _frames(render):
    cache = {}

    def frame_at(n):
        if n not in cache:
            cache[n] = render(n)
        return cache[n]
    return frame_at


def _check(api, gs, cam, w, h, depth, integ, frame_at, mn, mx, c, want_rounds=3):
    """Pick a threshold from the replay, render adaptively, compare everything bit for bit. Returns the replay."""
    t = R.pick_threshold(frame_at, w, h, mn, mx, c, want_rounds)
    assert t is not None, "no threshold spreads the tiles over %d rounds" % want_rounds
    r = R.replay(frame_at, w, h, mn, mx, c, t)
    col, spp, err, st = gs.render_adaptive(cam, w, h, depth, mn, mx, c, t, integrator=integ)
    assert np.array_equal(spp, r["tile_spp"]), (np.unique(spp, return_counts=True), np.unique(r["tile_spp"], return_counts=True))
    assert np.unique(spp).size >= want_rounds
    assert_bits_equal(err, r["tile_err"], "tile_err")
    assert_bits_equal(col, r["colors"], "sums at each tile's count")
    at_max, px = R.stats(r["tile_spp"], w, h, r["ns"][-1])
    assert st == {"rounds": r["rounds"], "tiles_at_max": at_max, "pixel_samples": px}
    assert gs.queue_stalls() == 0
    return r


# ---- 1. exact replay against the CPU reference ------------------------------------------------------------------------------
def _cornell_cfg(scene_dir, name, w, h, **kw):
    from cudapathtracer_amd import scenes
    return scenes.cornell(os.path.join(scene_dir, name), width=w, height=h, spp=4, max_depth=8, name=name, **kw)["config"]


@pytest.mark.parametrize("case", ["cornell", "mixed", "textured_naive", "thin_lens"])
def test_replay_against_the_cpu_reference(api, oracle, gpu_ready, scene_dir, case):
    integ, depth = 0, 8
    if case == "mixed":
        cfg = _cornell_cfg(scene_dir, "ad_mixed", 64, 48, tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4])
    elif case == "textured_naive":
        cfg, integ, depth = golden_scene("textured32", "scenes_tex"), 2, 5
    else:
        cfg = _cornell_cfg(scene_dir, "ad_cornell", 64, 48)
    hs = api.HostScene(cfg)
    gs, osc = api.Scene(hs), oracle.OracleScene(cfg)
    cam = hs.camera()
    w, h = cam.w, cam.h
    if case == "thin_lens":
        cam = api.Camera.NotPinhole((0.15, -0.1, 1.2), w, h, (3.0, -8.0, 2.0), 55.0, 0.08, 2.2)
    camb = np.frombuffer(cam.tobytes(), np.uint8).copy()
    frame_at = _frames(lambda n: osc.render(camera=camb, width=w, height=h, spp=n, max_depth=depth, integrator=integ, threads=16)[0])
    _check(api, gs, cam, w, h, depth, integ, frame_at, 4, 16, 2)
    gs.close()


# ---- 2. the production instantiations in list mode, against pt_render -------------------------------------------------------
def _pt_frames(gs, cam, w, h, depth, integ):
    return _frames(lambda n: gs.render(cam, w, h, n, depth, integrator=integ)[0])


def test_headline_cornell_1080p(api, gpu_ready, scene_dir):
    """C2: the pair form of FLAT with tens of thousands of tiles in the first rounds and thousands later."""
    hs = api.HostScene(_cornell_cfg(scene_dir, "ad_c2", 1920, 1080))
    gs = api.Scene(hs)
    cam = hs.camera()
    _check(api, gs, cam, 1920, 1080, 8, 0, _pt_frames(gs, cam, 1920, 1080, 8, 0), 8, 32, 4)
    assert gs.flags()["flat_pair"]                                      # (the flags describe the last launch: the adaptive one)
    gs.close()


@pytest.fixture(scope="module")
def blobs(api, gpu_ready, scene_dir):
    from cudapathtracer_amd import scenes
    plain = scenes.blob_in_box(os.path.join(scene_dir, "ad_blob"), 160, 128, 4, 8, name="ad_blob")["config"]
    glass = scenes.blob_in_box(os.path.join(scene_dir, "ad_glass"), 160, 128, 4, 8, material=5, name="ad_glass")["config"]
    return api.HostScene(plain), api.HostScene(glass)


@pytest.mark.parametrize("which,options,flags", [("plain", {"waves_hbm": 2}, ("simple", "hbm_kernel")), ("plain", {}, ("simple",)),
                                                 ("glass", {}, ("lean",))])
def test_blob_tiles_in_list_mode(api, blobs, which, options, flags):
    """320 tiles of the 82 k blob: the 8-wave SIMPLE kernel (forced), the kernel its tile count picks, and the glass blob (LEAN)."""
    hs = blobs[0 if which == "plain" else 1]
    gs = api.Scene(hs, options=options)
    cam = hs.camera()
    _check(api, gs, cam, 160, 128, 8, 0, _pt_frames(gs, cam, 160, 128, 8, 0), 4, 16, 2)
    assert all(gs.flags()[f] for f in flags), gs.flags()
    gs.close()


@pytest.mark.parametrize("case", ["naive", "slices"])
def test_naive_integrator_and_tiles_that_change_hands(api, gpu_ready, scene_dir, case):
    cfg = _cornell_cfg(scene_dir, "ad_m128", 128, 96, tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4])
    hs = api.HostScene(cfg)
    opts = {"slice_iters": 16, "sched_mask": 3} if case == "slices" else {}
    gs = api.Scene(hs, options=opts)
    cam = hs.camera()
    integ = 2 if case == "naive" else 0
    _check(api, gs, cam, 128, 96, 8, integ, _pt_frames(gs, cam, 128, 96, 8, integ), 4, 16, 2)
    if case == "slices":
        # 8 samples per launch, so waves yield tiles; tiles stop before the last round, so it lists fewer tiles than the frame has
        r = _check(api, gs, cam, 128, 96, 8, integ, _pt_frames(gs, cam, 128, 96, 8, integ), 16, 48, 8, want_rounds=2)
        assert (r["tile_spp"] < r["ns"][-1]).any()                       # some tiles stopped before the last round
        assert gs.tile_handovers() > 0                                  # in the last launch: a tile of a partial list changed hands
        # threshold 0 keeps every tile listed
        col, _, _, _ = gs.render_adaptive(cam, 128, 96, 8, 0, 16, 8, 0.0, integrator=integ)
        assert gs.tile_handovers() > 0 and gs.queue_stalls() == 0
        assert_bits_equal(col, gs.render(cam, 128, 96, 16, 8)[0], "threshold 0 with time slices")
    gs.close()


# ---- 3. boundaries and isolation ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell64(api, gpu_ready, scene_dir):
    hs = api.HostScene(_cornell_cfg(scene_dir, "ad_c64", 64, 48))
    return hs, hs.camera()


def test_queue_words_of_both_launches_of_a_round_are_checked(api, cornell64):
    """The second launch of a round re-initialises the tile queue, so the first launch's words are saved before it: with a wait
    bound of zero every launch's waiters give up at once (a stall, counted: the frame is complete), and with time slices of
    four iterations on top a tile yielded to a queue nobody waits on may stay unfinished in EITHER launch of a round. That is
    reported (-4), never returned as a tile with fewer samples than its tile_spp says."""
    hs, cam = cornell64
    ref, _ = api.Scene(hs).render(cam, 64, 48, 16, 8)
    sc = api.Scene(hs, options={"queue_timeout_ms": 0})
    col, spp, _, st = sc.render_adaptive(cam, 64, 48, 8, 0, 16, 2, 0.0)
    assert_bits_equal(col, ref, "waiters gave up at once")
    assert st["rounds"] == 4 and (spp == 16).all()
    assert sc.queue_stalls() > st["rounds"], (sc.queue_stalls(), st)     # the first launches' stalls are counted too
    sc.close()
    outcomes = set()
    for opts in ({"queue_timeout_ms": 0, "slice_iters": 4, "sched_mask": 3}, {"queue_timeout_ms": 0, "slice_iters": 4, "sched_mask": 3, "onchip": 0, "waves_hbm": 2}):
        sc = api.Scene(hs, options=opts)
        try:
            col, spp, _, _ = sc.render_adaptive(cam, 64, 48, 8, 0, 16, 2, 0.0)
            assert_bits_equal(col, ref, "complete although the waiters had left, %s" % opts)
            assert (spp == 16).all()
            outcomes.add("complete")
        except api.PtError as e:
            assert "incomplete" in str(e) and "tiles finished" in str(e), e
            outcomes.add("incomplete")
        sc.close()
    assert outcomes


def test_threshold_zero_is_pt_render_at_max_spp(api, cornell64):
    hs, cam = cornell64
    gs = api.Scene(hs)
    col, spp, err, st = gs.render_adaptive(cam, 64, 48, 8, 0, 12, 3, 0.0)
    ref, _ = gs.render(cam, 64, 48, 12, 8)
    assert_bits_equal(col, ref, "threshold 0")
    assert (spp == 12).all() and st == {"rounds": 2, "tiles_at_max": 48, "pixel_samples": 12 * 64 * 48}
    assert np.isfinite(err).all()
    gs.close()


def test_huge_threshold_stops_every_tile_at_the_first_round_past_min_spp(api, cornell64):
    hs, cam = cornell64
    gs = api.Scene(hs)
    col, spp, err, st = gs.render_adaptive(cam, 64, 48, 8, 5, 16, 2, float("inf"))
    ref, _ = gs.render(cam, 64, 48, 8, 8)
    assert_bits_equal(col, ref, "threshold inf")
    assert (spp == 8).all() and st["rounds"] == 2
    col, spp, _, st = gs.render_adaptive(cam, 64, 48, 8, 0, 16, 2, 1e30)
    assert (spp == 4).all() and st["rounds"] == 1
    assert_bits_equal(col, gs.render(cam, 64, 48, 4, 8)[0], "first round")
    gs.close()


def test_pt_render_after_an_adaptive_render_is_unchanged(api, cornell64):
    hs, cam = cornell64
    gs = api.Scene(hs)
    before, _ = gs.render(cam, 64, 48, 6, 8)
    gs.render_adaptive(cam, 64, 48, 8, 2, 10, 2, 0.05)
    after, _ = gs.render(cam, 64, 48, 6, 8)
    assert_bits_equal(after, before, "pt_render after pt_render_adaptive")
    gs.close()


def test_host_and_device_forms_agree(api, cornell64):
    import torch
    hs, cam = cornell64
    gs = api.Scene(hs)
    col, spp, err, st = gs.render_adaptive(cam, 64, 48, 8, 2, 16, 2, 0.05)
    dcol = torch.full((48, 64, 4), 9.0, device="cuda:0")                  # the call writes the sums, it does not add
    dspp = torch.zeros((6, 8), dtype=torch.int32, device="cuda:0")
    derr = torch.zeros((6, 8), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    st2 = gs.render_adaptive_device(cam, 64, 48, 8, 2, 16, 2, 0.05, dcol.data_ptr(), dspp.data_ptr(), derr.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert_bits_equal(dcol.cpu().numpy(), col, "device form")
    assert np.array_equal(dspp.cpu().numpy(), spp) and st2 == st
    assert_bits_equal(derr.cpu().numpy(), err, "device form tile_err")
    dspp.zero_()
    gs.render_adaptive_device(cam, 64, 48, 8, 2, 16, 2, 0.05, dcol.data_ptr(), dspp.data_ptr(), None)    # no error buffer
    assert np.array_equal(dspp.cpu().numpy(), spp)
    gs.close()


def test_wavefront_variant_is_refused_and_outputs_stay(api, cornell64):
    hs, cam = cornell64
    gs = api.Scene(hs).set_variant("wavefront")
    col = np.full((48, 64, 4), 7.0, np.float32)
    spp = np.full((6, 8), 3, np.int32)
    err = np.full((6, 8), 5.0, np.float32)
    p = api.adaptive_params(2, 8, 2, 0.1)
    import ctypes
    rc = api.lib().pt_render_adaptive(gs.h, ctypes.byref(cam), 64, 48, 8, 0, 1, SEED, ctypes.byref(p), api._p(col), api._p(spp), api._p(err), None)
    assert rc == -1 and "wavefront" in api.lib().pt_last_error().decode()
    assert (col == 7.0).all() and (spp == 3).all() and (err == 5.0).all()
    with pytest.raises(api.PtError):
        gs.render_adaptive(cam, 64, 48, 8, 2, 8, 2, 0.1)
    gs.close()


def test_denoising_an_adaptive_frame(api, cornell64):
    hs, cam = cornell64
    gs = api.Scene(hs)
    t = R.pick_threshold(_pt_frames(gs, cam, 64, 48, 8, 0), 64, 48, 2, 16, 2, 2)
    assert t is not None
    col, spp, _, _ = gs.render_adaptive(cam, 64, 48, 8, 2, 16, 2, t)
    assert np.unique(spp).size >= 2
    mean = api.adaptive_mean(col, spp)
    A, N = gs.render_aovs(cam, 64, 48, aov_spp=2)
    got = api.denoise(mean, 1, A, N)
    want, skip, L = denoise_ref(mean, 1, A, N)
    assert_bits_equal(got[skip], mean[skip], "pass-through pixels")
    np.testing.assert_allclose(got[~skip][:, :3], want[~skip][:, :3], rtol=1e-3, atol=1e-6 * L)
    gs.close()
