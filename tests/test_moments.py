"""pt_render_moments on the GPU: S is pt_render's frame and Q the float32 replay (tests/denoise_var_ref.py) over the partial
sums, of the library and of the CPU reference, through the production kernel instantiations; both variants, options, the device
form and isolation from the rest of the scene's state."""
import os

import numpy as np
import pytest

from conftest import golden_scene
from denoise_var_ref import moments_from_partial_sums
from util import assert_bits_equal

pytestmark = pytest.mark.gpu


def _check(gs, cam, w, h, spp, c, depth, integ, partial_at, what):
    """render_moments against render(spp) and against the replay over partial_at(j c), j = 1..B. Returns (S, Q)."""
    B = spp // c
    S, Q = gs.render_moments(cam, w, h, spp, c, depth, integrator=integ)
    sums = [partial_at(j * c) for j in range(1, B + 1)]
    assert_bits_equal(S, sums[-1], what + ": S")
    want = moments_from_partial_sums(sums)
    assert_bits_equal(Q, want, what + ": Q")
    assert np.all(Q[..., 3] == B)
    assert gs.queue_stalls() == 0
    return S, Q


def _golden(api, name, sub="scenes", options=None):
    cfg = golden_scene(name, sub)
    hs = api.HostScene(cfg)
    return cfg, hs, api.Scene(hs, options=options), hs.camera()


# ---- 1. against pt_render's partial sums, through the production kernels ------------------------------------------------------
@pytest.mark.parametrize("case", ["cornell32", "mixed32", "textured32_naive"])
def test_moments_against_pt_render_and_the_cpu_reference(api, oracle, gpu_ready, case):
    integ, depth = 0, 6
    if case == "textured32_naive":
        cfg, hs, gs, cam = _golden(api, "textured32", "scenes_tex")
        integ, depth = 2, 5
    else:
        cfg, hs, gs, cam = _golden(api, case)
    w, h = hs.info["width"], hs.info["height"]
    S, Q = _check(gs, cam, w, h, 12, 3, depth, integ, lambda n: gs.render(cam, w, h, n, depth, integrator=integ)[0], case)
    if case == "cornell32":
        assert gs.flags()["flat_pair"], gs.flags()                       # the FLAT pair kernel (the flags describe the last launch)
    if case == "mixed32":
        assert not gs.flags()["simple"], gs.flags()                      # the general bounce
    assert (Q[..., :3] > 0).mean() > 0.05
    if case != "textured32_naive":
        # ... and the same replay over the CPU reference's partial sums: the buffer is tied to the reference, not only to the library
        osc = oracle.OracleScene(cfg)
        sums = [osc.render(spp=j * 3, max_depth=depth, integrator=integ, threads=16)[0] for j in range(1, 5)]
        assert_bits_equal(S, sums[-1], case + ": S vs the CPU reference")
        assert_bits_equal(Q, moments_from_partial_sums(sums), case + ": Q vs the CPU reference")
    gs.close()


def test_moments_on_a_scene_in_hbm(api, gpu_ready, scene_dir):
    from cudapathtracer_amd import scenes
    cfg = scenes.blob_in_box(os.path.join(scene_dir, "mo_blob"), 160, 128, 4, 8, name="mo_blob")["config"]
    hs = api.HostScene(cfg)
    gs = api.Scene(hs, options={"waves_hbm": 2})                         # the kernel for scenes in HBM whatever the tile count
    cam = hs.camera()
    _check(gs, cam, 160, 128, 8, 2, 8, 0, lambda n: gs.render(cam, 160, 128, n, 8)[0], "blob")
    assert gs.flags()["hbm_kernel"] and not gs.flags()["onchip"], gs.flags()
    gs.close()


def _cornell(api, scene_dir, name, w, h, **kw):
    from cudapathtracer_amd import scenes
    hs = api.HostScene(scenes.cornell(os.path.join(scene_dir, name), width=w, height=h, spp=4, max_depth=8, name=name, **kw)["config"])
    return hs, hs.camera()


def test_frame_size_not_a_multiple_of_the_tile(api, gpu_ready, scene_dir):
    hs, cam = _cornell(api, scene_dir, "mo_70x41", 70, 41)
    gs = api.Scene(hs)
    _check(gs, cam, 70, 41, 8, 2, 8, 0, lambda n: gs.render(cam, 70, 41, n, 8)[0], "70 x 41")
    gs.close()


def test_full_hd_cornell(api, gpu_ready, scene_dir):
    hs, cam = _cornell(api, scene_dir, "mo_hd", 1920, 1080)
    gs = api.Scene(hs)
    _check(gs, cam, 1920, 1080, 4, 2, 8, 0, lambda n: gs.render(cam, 1920, 1080, n, 8)[0], "1920 x 1080")
    gs.close()


# ---- 2. batch sizes, variants, options, the device form, isolation --------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed96(api, gpu_ready, scene_dir):
    return _cornell(api, scene_dir, "mo_m96", 96, 64, tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4])


def test_batch_sizes_give_the_same_sum_and_different_squares(api, mixed96):
    hs, cam = mixed96
    gs = api.Scene(hs)
    got = {c: gs.render_moments(cam, 96, 64, 16, c, 8) for c in (2, 4, 8)}
    for c in (4, 8):
        assert_bits_equal(got[c][0], got[2][0], "S at batch_spp %d" % c)
        assert not np.array_equal(got[c][1][..., :3], got[2][1][..., :3])
    assert not np.array_equal(got[4][1][..., :3], got[8][1][..., :3])
    assert [float(got[c][1][0, 0, 3]) for c in (2, 4, 8)] == [8.0, 4.0, 2.0]
    gs.close()


@pytest.mark.parametrize("case", ["wavefront", "slices", "not_persistent"])
def test_variants_and_options_give_the_same_moments(api, mixed96, case):
    hs, cam = mixed96
    ref = api.Scene(hs)
    S0, Q0 = ref.render_moments(cam, 96, 64, 24, 8, 8)
    ref.close()
    opts = {"slices": {"slice_iters": 16, "sched_mask": 3}, "not_persistent": {"persistent": 0}}.get(case, {})
    gs = api.Scene(hs, options=opts)
    if case == "wavefront":
        gs.set_variant("wavefront")
    S, Q = gs.render_moments(cam, 96, 64, 24, 8, 8)
    assert_bits_equal(S, S0, case + ": S")
    assert_bits_equal(Q, Q0, case + ": Q")
    if case == "slices":
        assert gs.tile_handovers() > 0                                   # 8 samples per launch: tiles changed hands within the last batch
    assert gs.queue_stalls() == 0
    gs.close()


def test_device_form_is_the_host_form(api, gpu_ready, mixed96):
    torch = gpu_ready
    hs, cam = mixed96
    gs = api.Scene(hs)
    S0, Q0 = gs.render_moments(cam, 96, 64, 16, 4, 8)
    dS = torch.full((64, 96, 4), 3.0, device="cuda:0"); dQ = torch.full((64, 96, 4), 5.0, device="cuda:0")     # the call writes, it does not add
    gs.render_moments_device(cam, 96, 64, 16, 4, 8, dS.data_ptr(), dQ.data_ptr())
    assert_bits_equal(dS.cpu().numpy(), S0, "device form: S")
    assert_bits_equal(dQ.cpu().numpy(), Q0, "device form: Q")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dS.fill_(1.0); dQ.fill_(1.0)
        gs.render_moments_device(cam, 96, 64, 16, 4, 8, dS.data_ptr(), dQ.data_ptr(), stream=side.cuda_stream)
    assert_bits_equal(dS.cpu().numpy(), S0, "device form on a stream: S")
    assert_bits_equal(dQ.cpu().numpy(), Q0, "device form on a stream: Q")
    gs.close()


def test_counters_and_a_later_render_are_untouched(api, mixed96):
    hs, cam = mixed96
    fresh = api.Scene(hs)
    want, _ = fresh.render(cam, 96, 64, 6, 8)
    fresh.close()
    gs = api.Scene(hs)
    gs.render(cam, 96, 64, 2, 8, counters=True)                          # something in the counters
    before = gs.counters()
    assert sum(before.values()) > 0
    gs.render_moments(cam, 96, 64, 16, 4, 8)
    assert gs.counters() == before
    got, _ = gs.render(cam, 96, 64, 6, 8)                                # re-seeds: the streams the moments render left do not matter
    assert_bits_equal(got, want, "pt_render after pt_render_moments")
    gs.close()
