"""Centre feature buffers (pt_render_aovs_centre) on the GPU: the ray against the CPU oracle's camera_ray of cam0, the buffers
against the oracle's hits along those rays (tests/aov_chain_ref.py for the chain), against the library's own jittered entry points
handed cam0, and the subsample identity that makes a scaled frame's low-res guide a strided copy."""
import os

import numpy as np
import pytest

import aov_chain_ref as R
from conftest import golden_scene
from denoise_ref import aovs_from_hits
from test_aov import _blob, _oracle_hits, _pair
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SEEDS = (103033, 7)


def _cam0(api, cam):
    """The camera with antiAliasJitterDist = 0 and aperture = 0, everything else unchanged."""
    c = api.Camera.frombytes(cam.tobytes())
    c.antiAliasJitterDist = 0.0
    c.aperture = 0.0
    return c


def _thin_lens(api, w=40, h=24):
    return api.Camera.NotPinhole((0.15, -0.1, 1.2), w, h, (3.0, -8.0, 2.0), 55.0, 0.08, 2.2)


def _case(api, oracle, scene_dir, which):
    cfg = _blob(scene_dir) if which == "blob3" else golden_scene("cornell32" if which == "thin_lens" else which)
    gs, hs, osc = _pair(api, oracle, cfg)
    cam = _thin_lens(api) if which == "thin_lens" else hs.camera()
    return gs, osc, cam, cam.w, cam.h


# ---- 1. the ray ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pinhole", "thin_lens"])
def test_centre_rays_are_the_oracles_camera_ray_of_cam0(api, oracle, gpu_ready, kind):
    w, h = 40, 24
    cam = _thin_lens(api) if kind == "thin_lens" else api.make_camera(True, (0.1, -0.2, 1.1), (4.0, -6.0, 1.0), 50.0, w, h)
    assert cam.antiAliasJitterDist != 0 and (kind == "pinhole" or cam.aperture > 0)
    cam0 = _cam0(api, cam)
    xy = np.array([(x, y) for y in range(h) for x in range(w)], np.int32)
    got = api.probe_centre_rays(cam, xy)
    assert np.isfinite(got).all()
    for seed in SEEDS:
        assert_bits_equal(got, R.camera_rays(oracle, cam0, w, h, seed), "%s, seed %d: oracle camera_ray(cam0)" % (kind, seed))
        assert_bits_equal(got, api.probe_camera_rays(cam0, xy, seed), "%s, seed %d: pt_probe_camera_rays(cam0)" % (kind, seed))
    assert_bits_equal(got, api.probe_centre_rays(cam0, xy), "cam0 itself")
    assert not np.array_equal(got, api.probe_camera_rays(cam, xy, SEEDS[0]))       # the jittered rays are other rays


# ---- 2. the buffers against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cornell32", "mixed32", "thin_lens", "blob3"])
def test_first_hit_buffers_are_bit_exact_against_the_oracle(api, oracle, gpu_ready, scene_dir, which):
    gs, osc, cam, w, h = _case(api, oracle, scene_dir, which)
    alb, nd = gs.render_aovs_centre(cam, w, h)
    valid, _, a, n, t, _ = _oracle_hits(oracle, osc, _cam0(api, cam), w, h, SEEDS[0])
    ra, rn = aovs_from_hits([(valid, a, n, t)], 1)
    assert valid.any()
    assert_bits_equal(alb.reshape(-1, 4), ra, "albedo + coverage")
    assert_bits_equal(nd.reshape(-1, 4), rn, "normal + depth")
    assert set(np.unique(alb[..., 3]).tolist()) <= {0.0, 1.0}


@pytest.fixture(scope="module")
def mixed(api, oracle, gpu_ready, scene_dir):
    gs, osc, cam, w, h = _case(api, oracle, scene_dir, "mixed32")
    return gs, osc, cam, w, h, R.Materials(osc)


@pytest.mark.parametrize("max_links", [1, 4, 16])
def test_chain_buffers_are_bit_exact_against_the_reference(api, oracle, mixed, max_links):
    gs, osc, cam, w, h, mats = mixed
    ra, rn, rl, per_k = R.chain_aovs(oracle, osc, _cam0(api, cam), w, h, 1, max_links, SEEDS[1], mats)
    alb, nd, ln = gs.render_aovs_centre(cam, w, h, max_links, links=True)
    assert_bits_equal(alb.reshape(-1, 4), ra, "albedo + coverage")
    assert_bits_equal(nd.reshape(-1, 4), rn, "normal + depth")
    assert_bits_equal(ln.reshape(-1), rl, "links")
    assert rl.max() >= 1 and rl.max() <= max_links          # the scene has chains, and the cap holds
    a2, n2 = gs.render_aovs_centre(cam, w, h, max_links)    # without the links buffer: the same eight floats
    assert_bits_equal(a2, alb, "albedo, links NULL"); assert_bits_equal(n2, nd, "normal + depth, links NULL")


# ---- 3. against the library's own jittered entry points handed cam0 --------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (37, 21), (130, 9)])
def test_equals_the_jittered_entry_points_with_cam0(api, gpu_ready, w, h):
    """Ragged sizes: one pixel, one full tile, partial tiles in both axes, more tiles than one workgroup's waves in a row."""
    gs = api.Scene(api.HostScene(golden_scene("mixed32")))
    cam = api.Camera.NotPinhole((0.05, -0.1, 1.0), w, h, (2.0, -5.0, 0.0), 60.0, 0.05, 2.0)
    cam0 = _cam0(api, cam)
    for links in (0, 4):
        got = gs.render_aovs_centre(cam, w, h, links, links=True)
        for seed in SEEDS:
            want = gs.render_aovs_chain(cam0, w, h, links, aov_spp=1, seed=seed, links=True)
            for g, x, what in zip(got, want, ("albedo", "normal + depth", "links")):
                assert_bits_equal(g, x, "%d x %d, max_links %d, seed %d: %s" % (w, h, links, seed, what))
    first = gs.render_aovs_centre(cam, w, h)
    for seed in SEEDS:
        want = gs.render_aovs(cam0, w, h, aov_spp=1, seed=seed)
        assert_bits_equal(first[0], want[0], "first hit, albedo"); assert_bits_equal(first[1], want[1], "first hit, normal + depth")
    if w * h > 64:
        assert first[0][..., 3].any()
    gs.close()


def test_jitter_and_aperture_play_no_part(api, mixed):
    gs, _, cam, w, h, _ = mixed
    other = api.Camera.frombytes(cam.tobytes())
    other.antiAliasJitterDist = 3.5
    other.aperture = 0.3
    for links in (0, 4):
        a = gs.render_aovs_centre(cam, w, h, links, links=True)
        b = gs.render_aovs_centre(other, w, h, links, links=True)
        for x, y in zip(a, b):
            assert_bits_equal(x, y, "max_links %d" % links)


def test_device_form_matches_host_form(api, gpu_ready, mixed):
    torch = gpu_ready
    gs, _, cam, w, h, _ = mixed
    for links in (0, 4):
        a = torch.full((h, w, 4), 7.0, device="cuda:0"); n = torch.full((h, w, 4), 7.0, device="cuda:0"); l = torch.full((h, w), 7.0, device="cuda:0")
        s = torch.cuda.Stream()
        gs.render_aovs_centre_device(cam, w, h, links, a.data_ptr(), n.data_ptr(), l.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        ha, hn, hl = gs.render_aovs_centre(cam, w, h, links, links=True)
        assert_bits_equal(a.cpu().numpy(), ha, "albedo"); assert_bits_equal(n.cpu().numpy(), hn, "normal + depth")
        assert_bits_equal(l.cpu().numpy(), hl, "links")


# ---- 4. the scene's state ------------------------------------------------------------------------------------------------------------
def test_a_centre_pass_leaves_the_render_untouched(api, gpu_ready):
    torch = gpu_ready
    hs = api.HostScene(golden_scene("cornell32"))
    gs = api.Scene(hs)
    cam = hs.camera()
    w, h = cam.w, cam.h
    before_img = gs.render(cam, w, h, 2, 4, counters=True)[0].copy()
    before = gs.counters()
    assert before["rays_closest"] > 0
    for links in (0, 4):
        gs.render_aovs_centre(cam, w, h, links)
    assert gs.counters() == before
    seen = []

    def progress(done):
        c0 = gs.counters()
        a, _ = gs.render_aovs_centre(cam, w, h, 4 if done % 4 else 0)
        seen.append((done, c0 == gs.counters(), float(a[..., 3].sum())))
        return 0

    prog = torch.zeros(h, w, 4, device="cuda:0")
    gs.launch_progressive(0, 4, cam, 8, True, w, h, prog.data_ptr(), 2, progress=progress)
    one = torch.zeros(h, w, 4, device="cuda:0")
    gs.launch_unidirectional(4, cam, 8, True, w, h, one.data_ptr())
    assert [d for d, _, _ in seen] == [2, 4, 6, 8]
    assert all(same for _, same, _ in seen) and gs.counters() == before
    assert all(cov > 0 for _, _, cov in seen)
    assert_bits_equal(prog.cpu().numpy(), one.cpu().numpy(), "progressive with centre passes vs one-shot")
    assert_bits_equal(gs.render(cam, w, h, 2, 4, counters=True)[0], before_img, "the same render after the passes")


# ---- 5. the subsample identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4])
def test_the_scaled_cameras_guide_is_a_subsample(api, gpu_ready, s):
    torch = gpu_ready
    w, h = 48, 24
    gs = api.Scene(api.HostScene(golden_scene("mixed32")))
    cam = api.Camera.NotPinhole((0.05, -0.1, 1.0), w, h, (2.0, -5.0, 0.0), 60.0, 0.05, 2.0)
    lo = api.scaled_camera(cam, s)
    for links in (0, 4):
        A, N = gs.render_aovs_centre(cam, w, h, links)
        Al, Nl = gs.render_aovs_centre(lo, w // s, h // s, links)
        gA, gN = api.guide_subsample(s, A, N)
        assert gA.shape == (h // s, w // s, 4) and Al[..., 3].any()
        assert_bits_equal(gA, Al, "scale %d, max_links %d: albedo" % (s, links)); assert_bits_equal(gN, Nl, "normal + depth")
        assert_bits_equal(gA, np.ascontiguousarray(A[::s, ::s]), "numpy [::s, ::s]"); assert_bits_equal(gN, np.ascontiguousarray(N[::s, ::s]), "numpy")
        dA, dN = torch.from_numpy(A).to("cuda:0"), torch.from_numpy(N).to("cuda:0")
        oA = torch.full((h // s, w // s, 4), 9.0, device="cuda:0"); oN = torch.full((h // s, w // s, 4), 9.0, device="cuda:0")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        api.guide_subsample_device(w, h, s, dA.data_ptr(), dN.data_ptr(), oA.data_ptr(), oN.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        assert_bits_equal(oA.cpu().numpy(), gA, "device form, albedo"); assert_bits_equal(oN.cpu().numpy(), gN, "device form, normal + depth")
        assert_bits_equal(dA.cpu().numpy(), A, "the input is left as it was")
    gs.close()


# ---- 6. more tiles than resident waves, on a scene that spills ------------------------------------------------------------------------
def test_a_waves_second_tile_on_a_scene_that_spills(api, gpu_ready, scene_dir):
    """Every size above is a few tiles, so no wave there takes a second one. Here the frame has more tiles than the widest launch of
    the feature kernels has waves (8 per SIMD, 4 SIMDs per CU), on a tree deep enough to use the spill area: the kernels' stack and
    spill slice must serve a wave's second tile as they served its first. The four AOV kernels are tied to each other through
    cam0, the motion kernel to the centre pass, and the centre pass to pt_probe_trace_closest, which shares none of their set-up."""
    from cudapathtracer_amd import scenes
    from test_scene_update import _moved
    num_cu = gpu_ready.cuda.get_device_properties(0).multi_processor_count
    w = 1021                                                 # 128 tile columns, the last one partial
    h = (num_cu * 8 * 4 // 128 + 1) * 8 + 3                  # ... and one tile row more than the waves cover, then a partial one
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    assert tiles > num_cu * 8 * 4
    hs = api.HostScene(scenes.blob_in_box(os.path.join(scene_dir, "aov_trip_blob"), w, h, 2, 5, subdiv=4, name="aov_trip_blob")["config"])
    assert hs.info["n_tris"] == 20 * 4 ** 4 + 12             # the shell's 12 triangles, then the blob's
    sc = api.Scene.from_mesh(hs)
    assert not sc.flags()["onchip"]                          # a scene in HBM, with a spill area
    sc.update_vertices(_moved(hs, "displace")["points"])
    assert sc.has_motion == 1 and not sc.flags()["onchip"]
    cam = api.Camera.frombytes(hs.camera().tobytes())
    cam.antiAliasJitterDist = 1.0
    cam.aperture = 0.05
    cam0 = _cam0(api, cam)
    seed = SEEDS[0]
    # (a) the centre kernels equal the jittered kernels handed cam0
    for links in (0, 4):
        got = sc.render_aovs_centre(cam, w, h, links, links=True)
        want = sc.render_aovs_chain(cam0, w, h, links, aov_spp=1, seed=seed, links=True)
        for g, x, what in zip(got, want, ("albedo", "normal + depth", "links")):
            assert_bits_equal(g, x, "%d x %d, max_links %d: %s" % (w, h, links, what))
    first = sc.render_aovs_centre(cam, w, h)
    want = sc.render_aovs(cam0, w, h, aov_spp=1, seed=seed)
    assert_bits_equal(first[0], want[0], "first hit, albedo"); assert_bits_equal(first[1], want[1], "first hit, normal + depth")
    # (b) the motion kernel's guides are the centre pass, and the motion is the same without them
    A, N, mv = sc.render_motion(cam, w, h, guides=True)
    assert_bits_equal(A, first[0], "motion: albedo"); assert_bits_equal(N, first[1], "motion: normal_depth")
    assert_bits_equal(sc.render_motion(cam, w, h), mv, "motion without the guide outputs")
    assert (mv[-16:, :, 3] == 1).any()
    # (c) coverage and depth against the probe, over the first and the last 16 rows (the last ones are second tiles)
    rows = list(range(16)) + list(range(h - 16, h))
    xy = np.array([(x, y) for y in rows for x in range(w)], np.int32)
    gi, gf, _ = sc.trace_closest(api.probe_centre_rays(cam, xy))
    valid, t = (gi[:, 0] == 1).reshape(32, w), gf[:, 0].reshape(32, w)
    cov, depth = first[0][rows, :, 3], first[1][rows, :, 3]
    assert_bits_equal(cov, valid.astype(np.float32), "coverage")
    assert_bits_equal(depth, np.where(valid, t, np.float32(0.0)).astype(np.float32), "depth")
    # (d) ... and the last rows are not empty, nor all blob
    shell = valid & (gi[:, 1].reshape(32, w) < 12)
    assert valid[16:].any() and ((~valid[16:]).any() or shell[16:].any())
    sc.close()
