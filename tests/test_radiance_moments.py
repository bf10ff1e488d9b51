"""Radiance queries with their variance (pt_query_radiance_moments) on the GPU, bit for bit on every ray: S and Q of cam0's centre rays
against pt_query_radiance, the CPU oracle's partial renders and pt_render_moments, in the host and the device form; two cameras' rays
shuffled into one call; sub-ranges; guard words behind both outputs; a max_t at and just past the first hit alternating within a wave;
a frame with more tiles than resident waves on a scene that spills; the other kernels by option; an edited scene; and that a call
moves nothing else of the scene. tests/radiance_cases.py has the input."""
import os

import numpy as np
import pytest

import motion_cases as MC
import query_cases as QC
import radiance_cases as RC
from denoise_var_ref import moments_from_partial_sums
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SEED = 103033
BATCH_SPPS = (1, 2)                   # B = 4 and B = 2


@pytest.fixture(scope="module")
def cases(api, oracle, gpu_ready, scene_dir):
    """Per case: the GPU scene, cam0, its centre rays as records, and per (integrator, use_mis) the oracle's render(spp = 1 .. SPP) as
    [N, 4] rows and from them Q per batch size, computed once and never written to."""
    out = {}
    for name in RC.CASES:
        hs = RC.host(api, scene_dir, name, prefix="radmom_")
        cam0 = RC.cam0(api, hs, name)
        osc = oracle.OracleScene(arrays=RC.arrays(hs))
        cb = np.frombuffer(cam0.tobytes(), np.uint8).copy()
        want = {}
        for integ, mis in RC.SETTINGS[name]:
            part = [None] + [RC.as_rays(osc.render(camera=cb, width=RC.W, height=RC.H, spp=k, max_depth=RC.DEPTH, integrator=integ, use_mis=mis,
                                                   seed=SEED)[0]) for k in range(1, RC.SPP + 1)]
            w = {"S": part[RC.SPP]}
            for c in BATCH_SPPS:
                w[c] = moments_from_partial_sums([part[j * c] for j in range(1, RC.SPP // c + 1)])
            for v in w.values():
                v.setflags(write=False)
            want[(integ, mis)] = w
        out[name] = {"hs": hs, "sc": api.Scene(hs), "cam0": cam0, "osc": osc, "recs": RC.centre_records(api, cam0), "want": want}
    yield out
    for c in out.values():
        c["sc"].close()


def _query(c, recs, integ, mis, batch_spp, **kw):
    return c["sc"].query_radiance_moments(recs, RC.SPP, batch_spp, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED, **kw)


def _same(got, S, Q, what):
    assert_bits_equal(np.asarray(got[0]), S, what + ": S")
    assert_bits_equal(np.asarray(got[1]), Q, what + ": Q")


def _np(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


# ---- 1. the centre rays are the camera's moments: the oracle's and the library's --------------------------------------------------------
@pytest.mark.parametrize("name", RC.CASES)
def test_centre_rays_are_the_cameras_moments(api, gpu_ready, cases, name):
    torch = gpu_ready
    c = cases[name]
    sc, L = c["sc"], api.lib()
    lib_rays = sc.query_camera_rays(c["cam0"], RC.W, RC.H)
    stream = torch.cuda.current_stream().cuda_stream or None
    for (integ, mis), want in c["want"].items():
        plain = sc.query_radiance(c["recs"], RC.SPP, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED)
        assert_bits_equal(plain, want["S"], "%s: query_radiance against the oracle" % name)
        for bs in BATCH_SPPS:
            B = RC.SPP // bs
            what = "%s, integrator %d, mis %d, batch_spp %d" % (name, integ, mis, bs)
            S, Q = _query(c, c["recs"], integ, mis, bs)
            assert isinstance(S, np.ndarray) and S.shape == (RC.N, 4) and Q.shape == (RC.N, 4)
            assert (Q[:, 3] == B).all() and not S[:, 3].view(np.uint32).any(), what
            assert (Q[:, :3] > 0).any(), what
            assert_bits_equal(S, plain, what + ": S against query_radiance")
            _same((S, Q), want["S"], want[bs], what + ": host form against the oracle")
            dS, dQ = _query(c, lib_rays, integ, mis, bs)
            assert dS.is_cuda and dQ.is_cuda and dS.shape == (RC.N, 4) and dQ.shape == (RC.N, 4)
            _same(_np((dS, dQ)), want["S"], want[bs], what + ": device form against the oracle")
            rS, rQ = sc.render_moments(c["cam0"], RC.W, RC.H, RC.SPP, bs, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED)
            _same((S, Q), RC.as_rays(rS), RC.as_rays(rQ), what + ": against render_moments")
            # the call writes, it does not add: into buffers that held other values
            b0 = torch.full((RC.N, 4), 3.5, device="cuda:0")
            b1 = torch.full((RC.N, 4), -2.25, device="cuda:0")
            assert L.pt_query_radiance_moments_device(sc.h, RC.N, lib_rays.data_ptr(), RC.SPP, bs, RC.DEPTH, integ, int(mis), SEED, 0, b0.data_ptr(),
                                                      b1.data_ptr(), 0, stream) == 0, L.pt_last_error()
            _same(_np((b0, b1)), want["S"], want[bs], what + ": into pre-filled buffers")


# ---- 2. a ray is its own: two cameras' rays shuffled into one call ----------------------------------------------------------------------
def test_shuffled_rays_of_two_cameras_with_their_streams_in_the_pad_word(api, gpu_ready, cases):
    a, b = cases["cornell"], cases["cornell_outside"]
    recs = np.concatenate([a["recs"], b["recs"]], 0)
    recs[:, 7].view(np.uint32)[:] = np.concatenate([np.arange(RC.N), np.arange(RC.N)]).astype(np.uint32)
    perm = np.random.default_rng(5).permutation(2 * RC.N)
    shuffled = np.ascontiguousarray(recs[perm])
    for integ, mis in RC.SETTINGS["cornell_outside"]:
        for bs in BATCH_SPPS:
            what = "integrator %d, batch_spp %d" % (integ, bs)
            S, Q = _query(a, shuffled, integ, mis, bs, stream_pad=True)
            gS, gQ = np.empty_like(S), np.empty_like(Q)
            gS[perm], gQ[perm] = S, Q
            _same((gS[:RC.N], gQ[:RC.N]), a["want"][(integ, mis)]["S"], a["want"][(integ, mis)][bs], "cornell's half, " + what)
            _same((gS[RC.N:], gQ[RC.N:]), b["want"][(integ, mis)]["S"], b["want"][(integ, mis)][bs], "cornell_outside's half, " + what)
            dev = _np(_query(a, gpu_ready.from_numpy(shuffled).to("cuda:0"), integ, mis, bs, stream_pad=True))
            _same(dev, S, Q, "the device form, " + what)


# ---- 3. sub-ranges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "textured"])
def test_sub_ranges_with_first_stream(api, gpu_ready, cases, name):
    c = cases[name]
    for integ, mis in RC.SETTINGS[name][:2]:
        want = c["want"][(integ, mis)]
        for k, m in ((0, 1), (1, 63), (63, 2), (64, 64), (65, 895)):
            got = _query(c, np.ascontiguousarray(c["recs"][k:k + m]), integ, mis, 2, first_stream=k)
            _same(got, want["S"][k:k + m], want[2][k:k + m], "%s, integrator %d, rays %d..%d" % (name, integ, k, k + m))


# ---- 4. nothing past entry n - 1 is written, in either output ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, RC.CROP])
def test_no_stray_writes(api, gpu_ready, cases, n):
    torch = gpu_ready
    c = cases["textured"]
    L = api.lib()
    recs = torch.from_numpy(c["recs"]).to("cuda:0")
    GUARD, PAD = 0x5a5a5a5a, 16
    stream = torch.cuda.current_stream().cuda_stream or None
    for integ, mis in RC.SETTINGS["textured"]:
        want = c["want"][(integ, mis)]
        b0 = torch.full((n + PAD, 4), GUARD, dtype=torch.int32, device="cuda:0")
        b1 = torch.full((n + PAD, 4), GUARD, dtype=torch.int32, device="cuda:0")
        assert L.pt_query_radiance_moments_device(c["sc"].h, n, recs.data_ptr(), RC.SPP, 1, RC.DEPTH, integ, int(mis), SEED, 0, b0.data_ptr(), b1.data_ptr(), 0,
                                                  stream) == 0, L.pt_last_error()
        torch.cuda.synchronize()
        g0, g1 = b0.cpu().numpy(), b1.cpu().numpy()
        assert (g0[n:] == GUARD).all() and (g1[n:] == GUARD).all()
        _same((g0[:n].view(np.float32), g1[:n].view(np.float32)), want["S"][:n], want[1][:n], "n = %d, integrator %d" % (n, integ))


# ---- 5. a max_t of the ray's own on the first segment -------------------------------------------------------------------------------------
def test_max_t_alternating_within_a_wave(api, gpu_ready, cases):
    """Even rays get max_t = the oracle's first-hit t (the hit is not below it: every sample is the miss path's, S = 0 and Q.rgb = 0
    exactly), odd rays the next float (the camera's values); rays the oracle misses keep 999999."""
    c = cases["cornell"]
    r6 = c["recs"][:, [0, 1, 2, 4, 5, 6]]
    oi, of, _ = c["osc"].trace_closest(r6)
    hit = oi[:, 0] == 1
    assert hit.sum() == 897
    t = of[:, 0].astype(np.float32)
    at = QC.records(r6, np.where(hit, t, QC.MAX_T).astype(np.float32))
    mixed = QC.records(r6, np.where(hit, np.nextafter(t, np.float32(np.inf)), QC.MAX_T).astype(np.float32))
    mixed[::2] = at[::2]
    cut = hit.copy(); cut[1::2] = False
    assert cut.sum() > 400 and (hit & ~cut).sum() > 400
    for integ, mis in RC.SETTINGS["cornell"]:
        want = c["want"][(integ, mis)]
        for bs in BATCH_SPPS:
            zS = np.zeros((RC.N, 4), np.float32)
            zQ = np.zeros((RC.N, 4), np.float32); zQ[:, 3] = RC.SPP // bs
            S, Q = _np(_query(c, gpu_ready.from_numpy(mixed).to("cuda:0"), integ, mis, bs))
            assert not S[cut].view(np.uint32).any() and not Q[cut, :3].view(np.uint32).any()
            _same((S, Q), np.where(cut[:, None], zS, want["S"]), np.where(cut[:, None], zQ, want[bs]), "integrator %d, batch_spp %d" % (integ, bs))


# ---- 6. more tiles than resident waves, on a scene that spills -----------------------------------------------------------------------------
def test_a_waves_second_tile_on_a_scene_that_spills(api, gpu_ready, scene_dir):
    """test_radiance.py's blob: 5 132 triangles, in HBM, with a spill area, at 1021 x 523 or more: more tiles of 64 rays than the
    widest launch has waves, so every wave takes a second tile with its stacks and its bookkeeping words as the first left them."""
    from cudapathtracer_amd import scenes
    num_cu = gpu_ready.cuda.get_device_properties(0).multi_processor_count
    w = 1021
    h = (num_cu * 8 * 4 // 128 + 1) * 8 + 3
    hs = api.HostScene(scenes.blob_in_box(os.path.join(scene_dir, "radmom_blob"), w, h, 2, 5, subdiv=4, name="radmom_blob")["config"])
    assert hs.info["n_tris"] == 20 * 4 ** 4 + 12
    sc = api.Scene.from_mesh(hs)
    assert not sc.flags()["onchip"]
    cam0 = api.Camera.frombytes(MC.cam0_bytes(hs.camera()).tobytes())
    n = w * h
    assert (n + 63) // 64 > num_cu * 8 * 4
    rays = sc.query_camera_rays(cam0, w, h)
    for integ in (0, 2):
        wS, wQ = sc.render_moments(cam0, w, h, 2, 1, 4, integrator=integ, seed=SEED)
        assert (wS[..., :3] > 0).any() and (wQ[..., 3] == 2).all()
        _same(_np(sc.query_radiance_moments(rays, 2, 1, 4, integrator=integ, seed=SEED)), wS.reshape(n, 4), wQ.reshape(n, 4),
              "the blob at %d x %d, integrator %d" % (w, h, integ))
    sc.close()


# ---- 7. every instantiation is reached -----------------------------------------------------------------------------------------------------
def test_the_material_class_options_pick_the_kernel_and_change_no_bit(api, gpu_ready, cases, scene_dir):
    """"lean" 0 on the Cornell case (a LEAN scene) gives the generic kernel; on a plain diffuse box (a SIMPLE scene) "simple" 0 gives the
    LEAN kernel and both at 0 the generic one. With test 1 (LEAN and, on the textured case, generic) every one of the six kernels has
    run against the oracle or render_moments; the bits are the same whichever runs."""
    from cudapathtracer_amd import scenes
    c = cases["cornell"]
    sc = api.Scene(c["hs"], options={"lean": 0})
    for (integ, mis), want in c["want"].items():
        got = sc.query_radiance_moments(c["recs"], RC.SPP, 2, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED)
        _same(got, want["S"], want[2], "cornell with lean = 0, integrator %d, mis %d" % (integ, mis))
    sc.close()
    hs = api.HostScene(scenes.cornell(os.path.join(scene_dir, "radmom_plain"), width=RC.W, height=RC.H, name="radmom_plain", spp=4, max_depth=4)["config"])
    cam0 = api.Camera.frombytes(MC.cam0_bytes(hs.camera()).tobytes())
    recs = RC.centre_records(api, cam0)
    plain = api.Scene(hs)
    for integ, mis in ((0, True), (2, True), (0, False)):
        for bs in BATCH_SPPS:
            wS, wQ = plain.render_moments(cam0, RC.W, RC.H, RC.SPP, bs, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED)
            wS, wQ = RC.as_rays(wS), RC.as_rays(wQ)
            _same(plain.query_radiance_moments(recs, RC.SPP, bs, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED), wS, wQ,
                  "the SIMPLE kernel, integrator %d, batch_spp %d" % (integ, bs))
            for options in ({"simple": 0}, {"simple": 0, "lean": 0}):
                s = api.Scene(hs, options=options)
                _same(s.query_radiance_moments(recs, RC.SPP, bs, RC.DEPTH, integrator=integ, use_mis=mis, seed=SEED), wS, wQ,
                      "the plain box with %r, integrator %d, mis %d, batch_spp %d" % (options, integ, mis, bs))
                s.close()
    plain.close()


# ---- 8. after an edit ----------------------------------------------------------------------------------------------------------------------
def test_an_edited_scene_answers_as_a_fresh_one(api, gpu_ready, scene_dir):
    """The plain diffuse box (SIMPLE) with its white row made a mirror (LEAN) by update_materials answers as a fresh scene of the
    edited arrays."""
    from cudapathtracer_amd import scenes
    cfg = scenes.cornell(os.path.join(scene_dir, "radmom_edit"), width=RC.W, height=RC.H, name="radmom_edit", spp=4, max_depth=4)["config"]
    hs = api.HostScene(cfg)
    cam0 = api.Camera.frombytes(MC.cam0_bytes(hs.camera()).tobytes())
    sc = api.Scene.from_mesh(hs)
    recs = RC.centre_records(api, cam0)

    def answers(s):
        return [s.query_radiance_moments(recs, RC.SPP, 2, RC.DEPTH, integrator=i, use_mis=m, seed=SEED) for i, m in ((0, True), (2, True))]

    before = answers(sc)
    a = {k: hs.array(k) for k in MC.GEOMETRY}
    mats = a["materials"].copy().reshape(-1, 176)
    mats[2] = mats[19]                                        # the white walls and boxes become mirrors
    mirrored = dict(a, materials=mats.reshape(-1))
    sc.update_materials(mirrored["materials"])
    fresh = api.Scene.from_mesh(mirrored, max_leaf_size=hs.info["leaf_size"])
    got, want = answers(sc), answers(fresh)
    for g, w, b, k in zip(got, want, before, ("MIS", "naive")):
        _same(g, w[0], w[1], "after update_materials, " + k)
        assert not np.array_equal(g[1].view(np.uint32), b[1].view(np.uint32))
    fresh.close()
    sc.close()


# ---- 9. nothing else moves -----------------------------------------------------------------------------------------------------------------
def test_a_query_moves_nothing_else(api, gpu_ready, cases):
    c = cases["glass_mirror"]
    sc = c["sc"]
    img0, _ = sc.render(c["cam0"], RC.W, RC.H, RC.SPP, RC.DEPTH, seed=SEED)
    plain0 = sc.query_radiance(c["recs"], RC.SPP, RC.DEPTH, seed=SEED)
    sc.render(c["cam0"], RC.W, RC.H, 1, 3, counters=True)                       # something in the counters
    cnt0 = sc.counters()
    assert cnt0["rays_closest"] > 0
    S, Q = _query(c, c["recs"], 0, True, 2)
    assert sc.counters() == cnt0
    img1, _ = sc.render(c["cam0"], RC.W, RC.H, RC.SPP, RC.DEPTH, seed=SEED)
    assert_bits_equal(img1, img0, "a render after the query against one before it")
    assert_bits_equal(sc.query_radiance(c["recs"], RC.SPP, RC.DEPTH, seed=SEED), plain0, "a query_radiance after the query against one before it")
    _same(_query(c, c["recs"], 0, True, 2), S, Q, "the same call again")
    empty = sc.query_radiance_moments(gpu_ready.from_numpy(c["recs"]).to("cuda:0")[:0], RC.SPP, 2, RC.DEPTH)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 4) and empty[0].is_cuda
