"""Radiance queries (pt_query_radiance) on the GPU, bit for bit on every ray: the centre rays of cam0 against the CPU oracle's render
and the library's own, in the host and the device form; the rays of two cameras shuffled into one call with their streams in the pad
word; sub-ranges; a max_t at and just past the first hit; guard words; a frame with more tiles than resident waves on a scene that
spills; edited scenes against fresh ones; and that a call moves nothing else of the scene. tests/radiance_cases.py has the input."""
import os

import numpy as np
import pytest

import motion_cases as MC
import query_cases as QC
import radiance_cases as RC
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SEED = 103033


@pytest.fixture(scope="module")
def cases(api, oracle, gpu_ready, scene_dir):
    """Per case: the GPU scene, cam0, its centre rays as records, and per (integrator, use_mis) the oracle's render as [N, 4] rows,
    computed once and never written to."""
    out = {}
    for name in RC.CASES:
        hs = RC.host(api, scene_dir, name)
        cam0 = RC.cam0(api, hs, name)
        osc = oracle.OracleScene(arrays=RC.arrays(hs))
        cb = np.frombuffer(cam0.tobytes(), np.uint8).copy()
        want = {}
        for integ, mis in RC.SETTINGS[name]:
            img = osc.render(camera=cb, width=RC.W, height=RC.H, spp=RC.SPP, max_depth=RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED)[0]
            want[(integ, mis)] = RC.as_rays(img)
            want[(integ, mis)].setflags(write=False)
        out[name] = {"hs": hs, "sc": api.Scene(hs), "cam0": cam0, "osc": osc, "recs": RC.centre_records(api, cam0), "want": want}
    yield out
    for c in out.values():
        c["sc"].close()


def _query(c, recs, integ, mis, **kw):
    return c["sc"].query_radiance(recs, RC.SPP, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED, **kw)


# ---- 1. the centre rays are the camera's render, the oracle's and the library's ------------------------------------------------------------
@pytest.mark.parametrize("name", RC.CASES)
def test_centre_rays_are_the_oracles_render(api, gpu_ready, cases, name):
    c = cases[name]
    lib_rays = c["sc"].query_camera_rays(c["cam0"], RC.W, RC.H)             # pt_query_camera_rays_device(cam0, w, h, 999999)
    assert np.array_equal(lib_rays.cpu().numpy().view(np.uint32), c["recs"].view(np.uint32))
    for (integ, mis), want in c["want"].items():
        what = "%s, integrator %d, mis %d" % (name, integ, mis)
        assert np.isfinite(want).all() and (want[:, :3] > 0).any() and not want[:, 3].any(), what
        host = _query(c, c["recs"], integ, mis)
        assert isinstance(host, np.ndarray) and host.shape == (RC.N, 4)
        assert_bits_equal(host, want, what + ": host form against the oracle")
        dev = _query(c, lib_rays, integ, mis)
        assert dev.is_cuda and dev.shape == (RC.N, 4)
        assert_bits_equal(dev.cpu().numpy(), want, what + ": device form against the oracle")
        img, _ = c["sc"].render(c["cam0"], RC.W, RC.H, RC.SPP, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED)
        assert_bits_equal(host, RC.as_rays(img), what + ": against Scene.render into zeros")
    # the call writes, it does not add: a second call into the same tensor's place gives the same bits (numpy out is fresh each time;
    # the device buffer here is pre-filled)
    torch = gpu_ready
    integ, mis = RC.SETTINGS[name][0]
    buf = torch.full((RC.N, 4), 3.5, device="cuda:0")
    L = api.lib()
    assert L.pt_query_radiance_device(c["sc"].h, RC.N, lib_rays.data_ptr(), RC.SPP, RC.DEPTH, integ, int(mis), SEED, 0, buf.data_ptr(), 0,
                                      torch.cuda.current_stream().cuda_stream or None) == 0, L.pt_last_error()
    assert_bits_equal(buf.cpu().numpy(), c["want"][(integ, mis)], name + ": into a buffer that held 3.5")


# ---- 2. a ray is its own: two cameras' rays shuffled into one call ----------------------------------------------------------------------
def test_shuffled_rays_of_two_cameras_with_their_streams_in_the_pad_word(api, gpu_ready, cases):
    """Neighbouring lanes hold paths of unrelated length, some inside the box, some missing everything; each ray draws from the
    stream its pad word names, whatever its place in the buffer."""
    a, b = cases["cornell"], cases["cornell_outside"]
    recs = np.concatenate([a["recs"], b["recs"]], 0)
    recs[:, 7].view(np.uint32)[:] = np.concatenate([np.arange(RC.N), np.arange(RC.N)]).astype(np.uint32)
    perm = np.random.default_rng(5).permutation(2 * RC.N)
    shuffled = np.ascontiguousarray(recs[perm])
    for integ, mis in RC.SETTINGS["cornell_outside"]:
        got = np.empty((2 * RC.N, 4), np.float32)
        got[perm] = _query(a, shuffled, integ, mis, stream_pad=True)
        assert_bits_equal(got[:RC.N], a["want"][(integ, mis)], "cornell's half, integrator %d" % integ)
        assert_bits_equal(got[RC.N:], b["want"][(integ, mis)], "cornell_outside's half, integrator %d" % integ)
        dev = _query(a, gpu_ready.from_numpy(shuffled).to("cuda:0"), integ, mis, stream_pad=True).cpu().numpy()
        assert_bits_equal(dev, got[perm], "the device form, integrator %d" % integ)
    # first_stream adds to the pad word, in uint32 arithmetic: pad - 7 (wrapping below 0) with first_stream = 7
    recs2 = a["recs"].copy()
    recs2[:, 7].view(np.uint32)[:] = (np.arange(RC.N, dtype=np.int64) - 7).astype(np.uint32)
    assert_bits_equal(_query(a, recs2, 0, True, first_stream=7, stream_pad=True), a["want"][(0, True)], "pad - 7 + first_stream 7")
    # without the flag the pad word is not read
    assert_bits_equal(_query(a, recs2, 0, True), a["want"][(0, True)], "pad ignored without the flag")


# ---- 3. sub-ranges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "textured"])
def test_sub_ranges_with_first_stream(api, gpu_ready, cases, name):
    c = cases[name]
    for integ, mis in RC.SETTINGS[name][:2]:
        for k, m in ((0, 1), (1, 63), (63, 2), (64, 64), (65, 895)):
            got = _query(c, np.ascontiguousarray(c["recs"][k:k + m]), integ, mis, first_stream=k)
            assert_bits_equal(got, c["want"][(integ, mis)][k:k + m], "%s, integrator %d, rays %d..%d" % (name, integ, k, k + m))


# ---- 4. a max_t of the ray's own on the first segment -------------------------------------------------------------------------------------
def test_max_t_at_and_just_past_the_first_hit(api, gpu_ready, cases):
    """max_t = the oracle's first-hit t: the hit is not below it, nothing else is: the first segment misses, and every sample is the
    miss path's value, which is what a ray aimed out of the scene gets. The next float after t: test 1's value. Rays the oracle
    misses keep 999999. Later segments are not limited: with max_t just past the first hit the whole path is the camera's."""
    c = cases["cornell"]
    r6 = c["recs"][:, [0, 1, 2, 4, 5, 6]]
    oi, of, _ = c["osc"].trace_closest(r6)
    hit = oi[:, 0] == 1
    assert hit.sum() == 897                                       # (the other 63 centre rays leave through the open front)
    t = of[:, 0].astype(np.float32)
    away = QC.records(np.tile(np.array([(0.0, 50.0, 0.0, 0.0, 1.0, 0.0)], np.float32), (RC.N, 1)))
    for integ, mis in RC.SETTINGS["cornell"]:
        want = c["want"][(integ, mis)]
        missed = _query(c, away, integ, mis)
        assert not missed.view(np.uint32).any()                   # (0 + 0) + 0 ...: the miss path adds beta * the black sky
        at = QC.records(r6, np.where(hit, t, QC.MAX_T).astype(np.float32))
        assert_bits_equal(_query(c, at, integ, mis), np.where(hit[:, None], missed, want), "max_t = t, integrator %d" % integ)
        past = QC.records(r6, np.where(hit, np.nextafter(t, np.float32(np.inf)), QC.MAX_T).astype(np.float32))
        assert_bits_equal(_query(c, past, integ, mis), want, "max_t = nextafter(t), integrator %d" % integ)
        mixed = past.copy(); mixed[::2] = at[::2]
        cut = hit.copy(); cut[1::2] = False
        got = _query(c, gpu_ready.from_numpy(mixed).to("cuda:0"), integ, mis).cpu().numpy()
        assert_bits_equal(got, np.where(cut[:, None], missed, want), "max_t alternating within a wave, integrator %d" % integ)


# ---- 5. nothing past entry n - 1 is written ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, RC.CROP])
def test_no_stray_writes(api, gpu_ready, cases, n):
    torch = gpu_ready
    c = cases["textured"]
    L = api.lib()
    recs = torch.from_numpy(c["recs"]).to("cuda:0")
    GUARD, PAD = 0x5a5a5a5a, 16
    stream = torch.cuda.current_stream().cuda_stream or None
    for integ, mis in RC.SETTINGS["textured"]:
        buf = torch.full((n + PAD, 4), GUARD, dtype=torch.int32, device="cuda:0")
        assert L.pt_query_radiance_device(c["sc"].h, n, recs.data_ptr(), RC.SPP, RC.DEPTH, integ, int(mis), SEED, 0, buf.data_ptr(), 0, stream) == 0, L.pt_last_error()
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[n:] == GUARD).all()
        assert_bits_equal(got[:n].view(np.float32), c["want"][(integ, mis)][:n], "n = %d, integrator %d" % (n, integ))


# ---- 6. more tiles than resident waves, on a scene that spills -----------------------------------------------------------------------------
def test_a_waves_second_tile_on_a_scene_that_spills(api, gpu_ready, scene_dir):
    """test_query.py's blob: 5 132 triangles, in HBM, with a spill area, at 1021 x 523 or more: more tiles of 64 rays than the widest
    launch has waves, so every wave takes a second tile with its stacks as the first left them."""
    from cudapathtracer_amd import scenes
    num_cu = gpu_ready.cuda.get_device_properties(0).multi_processor_count
    w = 1021
    h = (num_cu * 8 * 4 // 128 + 1) * 8 + 3
    hs = api.HostScene(scenes.blob_in_box(os.path.join(scene_dir, "radiance_blob"), w, h, 2, 5, subdiv=4, name="radiance_blob")["config"])
    assert hs.info["n_tris"] == 20 * 4 ** 4 + 12
    sc = api.Scene.from_mesh(hs)
    assert not sc.flags()["onchip"]
    cam0 = api.Camera.frombytes(MC.cam0_bytes(hs.camera()).tobytes())
    n = w * h
    assert (n + 63) // 64 > num_cu * 8 * 4
    rays = sc.query_camera_rays(cam0, w, h)
    for integ in (0, 2):
        want, _ = sc.render(cam0, w, h, 1, 4, integrator=integ, seed=SEED)
        got = sc.query_radiance(rays, 1, 4, integrator=integ, seed=SEED).cpu().numpy()
        assert (want[..., :3] > 0).any()
        assert_bits_equal(got, want.reshape(n, 4), "the blob at %d x %d, integrator %d" % (w, h, integ))
    sc.close()


# ---- 7. after edits ------------------------------------------------------------------------------------------------------------------------
def test_an_edited_scene_answers_as_a_fresh_one(api, gpu_ready, scene_dir):
    """The plain diffuse box (the SIMPLE kernel) with its white row made a mirror (LEAN), then its tall box moved: after each edit the
    scene answers as a fresh scene of the edited arrays, and as it did before once the edit is undone."""
    from cudapathtracer_amd import scenes
    cfg = scenes.cornell(os.path.join(scene_dir, "radiance_edit"), width=RC.W, height=RC.H, name="radiance_edit", spp=4, max_depth=4)["config"]
    hs = api.HostScene(cfg)
    leaf = hs.info["leaf_size"]
    cam0 = api.Camera.frombytes(MC.cam0_bytes(hs.camera()).tobytes())
    sc = api.Scene.from_mesh(hs)
    recs = RC.centre_records(api, cam0)

    def answers(s):
        return [s.query_radiance(recs, RC.SPP, RC.DEPTH, integrator=i, use_mis=m, seed=SEED) for i, m in ((0, True), (2, True), (0, False))]

    def same(a, b, what):
        for x, y, k in zip(a, b, ("MIS", "naive", "without MIS")):
            assert_bits_equal(x, y, what + ", " + k)

    def klass(s):
        s.render(cam0, RC.W, RC.H, 1, 2)
        f = s.flags()
        return "simple" if f["simple"] else "lean" if f["lean"] else "generic"

    assert klass(sc) == "simple"
    before = answers(sc)
    img, _ = sc.render(cam0, RC.W, RC.H, RC.SPP, RC.DEPTH, seed=SEED)
    assert_bits_equal(before[0], RC.as_rays(img), "the SIMPLE kernel against Scene.render")
    a = {k: hs.array(k) for k in MC.GEOMETRY}
    mats = a["materials"].copy().reshape(-1, 176)
    mats[2] = mats[19]                                        # the white walls and boxes become mirrors
    mirrored = dict(a, materials=mats.reshape(-1))
    sc.update_materials(mirrored["materials"])
    fresh = api.Scene.from_mesh(mirrored, max_leaf_size=leaf)
    got = answers(sc)
    same(got, answers(fresh), "after update_materials")
    assert klass(sc) == "lean" and klass(fresh) == "lean"
    assert not np.array_equal(got[0].view(np.uint32), before[0].view(np.uint32))
    fresh.close()
    moved = dict(mirrored, points=MC.moved_arrays(hs)["points"])
    sc.update_vertices(moved["points"])
    fresh = api.Scene.from_mesh(moved, max_leaf_size=leaf)
    got2 = answers(sc)
    same(got2, answers(fresh), "after update_vertices")
    assert not np.array_equal(got2[0].view(np.uint32), got[0].view(np.uint32))
    fresh.close()
    sc.update_vertices(a["points"])
    sc.update_materials(a["materials"])
    same(answers(sc), before, "with both edits undone")
    assert klass(sc) == "simple"
    sc.close()


# ---- 8. nothing else moves -----------------------------------------------------------------------------------------------------------------
def test_a_query_moves_nothing_else(api, gpu_ready, cases):
    torch = gpu_ready
    c = cases["glass_mirror"]
    sc = c["sc"]
    integ, mis = 0, True
    img0, _ = sc.render(c["cam0"], RC.W, RC.H, RC.SPP, RC.DEPTH, seed=SEED)
    sc.render(c["cam0"], RC.W, RC.H, 1, 3, counters=True)                       # something in the counters
    cnt0 = sc.counters()
    assert cnt0["rays_closest"] > 0
    host = _query(c, c["recs"], integ, mis)
    assert sc.counters() == cnt0
    img1, _ = sc.render(c["cam0"], RC.W, RC.H, RC.SPP, RC.DEPTH, seed=SEED)
    assert_bits_equal(img1, img0, "a render after the query against one before it")
    # torch in, torch out, on a stream of its own, the input made by torch
    d = torch.from_numpy(c["recs"]).to("cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d2 = d.clone()
        t = sc.query_radiance(d2, RC.SPP, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED)
    side.synchronize()
    assert isinstance(t, torch.Tensor) and t.device == d.device and t.dtype == torch.float32 and t.shape == (RC.N, 4)
    assert_bits_equal(t.cpu().numpy(), host, "a stream of its own")
    with pytest.raises(api.PtError, match="contiguous"):
        sc.query_radiance(d[:, :6], RC.SPP, RC.DEPTH)
    empty = sc.query_radiance(d[:0], RC.SPP, RC.DEPTH)
    assert empty.shape == (0, 4) and empty.is_cuda
    # a panorama from the middle of the scene: a smoke check of rays.py's buffers, not parity
    from cudapathtracer_amd import rays
    pts = np.ascontiguousarray(c["hs"].array("points")).view(np.float32).reshape(-1, 4)[:, :3]
    pano = sc.query_radiance(rays.panorama_rays(tuple(0.5 * (pts.min(0) + pts.max(0))), 64, 32), 2, 4)
    assert pano.shape == (64 * 32, 4) and np.isfinite(pano).all() and (pano[:, :3] > 0).any() and not pano[:, 3].any()
    ortho = sc.query_radiance(rays.orthographic_rays((0.0, 0.0, 3.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 1.0, 1.0, 16, 16, device="cuda:0"), 2, 4)
    assert ortho.is_cuda and bool(torch.isfinite(ortho).all())


# ---- 9. every instantiation is reached -----------------------------------------------------------------------------------------------------
def test_the_material_class_options_pick_the_kernel_and_change_no_bit(api, gpu_ready, cases, scene_dir):
    """"lean" 0 on the Cornell case (a LEAN scene) gives the generic kernel; on a plain diffuse box (a SIMPLE scene) "simple" 0 gives the
    LEAN kernel and both at 0 the generic one. With test 1 (LEAN and, on the textured case, generic) and test 7 (SIMPLE) every one of
    the six kernels has run against the oracle or the render; the bits are the same whichever runs."""
    from cudapathtracer_amd import scenes
    c = cases["cornell"]
    sc = api.Scene(c["hs"], options={"lean": 0})
    for (integ, mis), want in c["want"].items():
        got = sc.query_radiance(c["recs"], RC.SPP, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED)
        assert_bits_equal(got, want, "cornell with lean = 0, integrator %d, mis %d" % (integ, mis))
    sc.close()
    hs = api.HostScene(scenes.cornell(os.path.join(scene_dir, "radiance_plain"), width=RC.W, height=RC.H, name="radiance_plain", spp=4, max_depth=4)["config"])
    cam0 = api.Camera.frombytes(MC.cam0_bytes(hs.camera()).tobytes())
    recs = RC.centre_records(api, cam0)
    plain = api.Scene(hs)
    for integ, mis in ((0, True), (2, True), (0, False)):
        img, _ = plain.render(cam0, RC.W, RC.H, RC.SPP, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED)
        want = RC.as_rays(img)
        assert_bits_equal(plain.query_radiance(recs, RC.SPP, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED), want, "the SIMPLE kernel, integrator %d" % integ)
        for options in ({"simple": 0}, {"simple": 0, "lean": 0}):
            s = api.Scene(hs, options=options)
            got = s.query_radiance(recs, RC.SPP, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED)
            assert_bits_equal(got, want, "the plain box with %r, integrator %d, mis %d" % (options, integ, mis))
            s.close()
    plain.close()
