"""SH queries (pt_query_sh, pt_query_sh_rays_device) on the GPU, bit for bit. The tie is to calls that are checked against the oracle:
a lane's one sample is pt_query_radiance on the ray pt_query_sh_rays_device emits for it, the local direction is
pt_probe_bsdf_sample's for a diffuse material, the map onto the sphere, the nine terms and the products are tests/sh_ref.py's
restatement of the header's arithmetic, and the sums are its adjacent-pair tree (tests/irradiance_ref.py's).

Scenes: test_query_irradiance.py's. The plain diffuse Cornell box (the SIMPLE kernels), tests/radiance_cases.py's Cornell box with a
glass and a mirror box (LEAN; generic with "lean" 0) and the blob in the box, which lies in HBM and spills. Probes: five each, four
inside the scene (in the plain box the first hangs 0.05 under the emitter) and one far above it."""
import os

import numpy as np
import pytest

import irradiance_ref as IR
import motion_cases as MC
import radiance_cases as RC
import sh_ref as SR
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SEED = 103033
N = 5
DEPTH = 4
SETTINGS = ((0, True), (0, False), (2, True))
PAD = 2                                                        # api.QUERY_STREAM_PAD
FAR = 5000.0                                                   # the last probe hangs this many scene sizes above the scene: at 3e-9 of its sphere
                                                               # the scene is not met by the few thousand directions drawn here
INSIDE = ((0.3, 0.6, 0.4), (0.7, 0.3, 0.6), (0.5, 0.8, 0.5), (0.25, 0.25, 0.7))      # fractions of the scene's bounding box


def _probes(hs, sc, under_emitter):
    from cudapathtracer_amd import rays as R
    pts = np.ascontiguousarray(hs.array("points")).view(np.float32).reshape(-1, 4)[:, :3]
    lo, hi = pts.min(0), pts.max(0)
    mid = 0.5 * (lo + hi)
    p = np.concatenate([lo + np.array(INSIDE, np.float32) * (hi - lo), [(mid[0], hi[1] + FAR * (hi - lo).max(), mid[2])]], 0).astype(np.float32)
    if under_emitter:
        gx, gz = np.meshgrid(np.linspace(lo[0], hi[0], 13)[1:-1], np.linspace(lo[2], hi[2], 13)[1:-1])
        up = R.irradiance_records(np.stack([gx.ravel(), np.full(gx.size, 0.5 * (lo[1] + hi[1])), gz.ravel()], 1), np.tile([(0.0, 1.0, 0.0)], (gx.size, 1)))
        surf = sc.query_closest(up, surfaces=True)[1]
        lit = np.flatnonzero(surf["light"] >= 0)
        assert len(lit) >= 1
        p[0] = (surf["px"][lit[0]], surf["py"][lit[0]] - np.float32(0.05), surf["pz"][lit[0]])
    recs = R.sh_records(p)
    recs[:, 4:7] = (7.0, -3.0, np.nan)                         # the direction words are not read
    recs.setflags(write=False)
    return recs


@pytest.fixture(scope="module")
def cases(api, gpu_ready, scene_dir):
    from cudapathtracer_amd import scenes
    out = {}
    plain = api.HostScene(scenes.cornell(os.path.join(scene_dir, "sh_plain"), width=RC.W, height=RC.H, name="sh_plain", spp=4, max_depth=4)["config"])
    mixed = RC.host(api, scene_dir, "cornell", prefix="sh_")
    blob = api.HostScene(scenes.blob_in_box(os.path.join(scene_dir, "sh_blob"), RC.W, RC.H, 2, 5, subdiv=4, name="sh_blob")["config"])
    for name, hs, make in (("simple", plain, api.Scene.from_mesh), ("mixed", mixed, api.Scene), ("hbm", blob, api.Scene.from_mesh)):
        sc = make(hs)
        cam0 = api.Camera.frombytes(MC.cam0_bytes(hs.camera()).tobytes())
        sc.render(cam0, RC.W, RC.H, 1, 2)
        out[name] = {"hs": hs, "sc": sc, "cam0": cam0, "recs": _probes(hs, sc, name == "simple"), "flags": sc.flags()}
    assert out["simple"]["flags"]["simple"] and out["mixed"]["flags"]["lean"] and not out["hbm"]["flags"]["onchip"]
    yield out
    for c in out.values():
        c["sc"].close()


def _lane_terms(sc, rays, depth, integ, mis, first_stream=0):
    """[m, 9, 3]: pt_query_radiance's one sample on each emitted ray, times the nine terms at the ray's direction."""
    li = sc.query_radiance(rays, 1, depth, integrator=integ, use_mis=mis, seed=SEED, first_stream=first_stream, stream_pad=True)
    return SR.terms(li, rays[:, 4:7])


# ---- 1. one sample per stream: the emitted rays through pt_query_radiance, the projection, then the tree ------------------------------------
@pytest.mark.parametrize("name", ["simple", "mixed", "hbm"])
def test_one_sample_per_stream_is_query_radiance_on_the_emitted_rays(api, gpu_ready, cases, name):
    """L = 128 is the smallest record with a second stage, L = 256 the smallest whose second stage has an order."""
    c = cases[name]
    sc, recs = c["sc"], c["recs"]
    lit, tells_lanes, tells_waves = 0, False, False
    for lanes, first in ((1, 0), (4, 7), (64, 0), (128, 3), (256, 0)):
        rays = sc.query_sh_rays(recs, lanes, seed=SEED, first_stream=first)
        assert rays.shape == (N * lanes, 8) and np.array_equal(rays[:, 7].view(np.uint32), np.arange(N * lanes, dtype=np.uint32))
        for integ, mis in SETTINGS:
            what = "%s, %d lanes, integrator %d, mis %d" % (name, lanes, integ, mis)
            a = SR.lane_sum([_lane_terms(sc, rays, DEPTH, integ, mis, first)]).reshape(N, lanes, 9, 3)      # 0 + t_0: a -0 term sums to +0
            want = SR.coeffs(a)
            got = sc.query_sh(recs, lanes, 1, DEPTH, integrator=integ, use_mis=mis, seed=SEED, first_stream=first)
            assert got.shape == (N, 9, 4)
            assert_bits_equal(got, want, what)
            assert np.isfinite(got).all() and not got[..., 3].any()
            lit += int((got[:, 0, :3] > 0).any(1).sum())
            assert not got[N - 1].view(np.uint32).any(), what + ": the far probe"
            if lanes == 256:
                # the orders this comparison can tell apart on its own data: the lanes one after the other, and the tree within
                # each wave with the four waves one after the other
                tells_lanes |= not np.array_equal(SR.left_to_right(a), want[..., :3])
                waves = IR.tree(a.reshape(N * 4, 64, 9, 3)).reshape(N, 4, 9, 3)
                tells_waves |= not np.array_equal(SR.left_to_right(waves), want[..., :3])
    print(name, "lit results", lit, "tells lanes", tells_lanes, "tells waves", tells_waves)
    assert lit > 0 and tells_lanes and tells_waves


# ---- 2. the emitted ray --------------------------------------------------------------------------------------------------------------------------
def test_the_emitted_ray_is_the_headers_map_on_cosine_sample_fs_direction(api, gpu_ready, cases):
    """The local direction from pt_probe_bsdf_sample on the plain box's white Lambert row (its first two draws on the same stream), the
    map restated in numpy; o is p bit for bit, and max_t and the pad word are passed on."""
    from cudapathtracer_amd import rays as R
    c = cases["simple"]
    sc = c["sc"]
    pts = np.concatenate([np.random.default_rng(2).uniform(-2, 2, (20, 3)).astype(np.float32), c["recs"][:, 0:3], [(0.0, -0.0, 1e-30)]], 0).astype(np.float32)
    recs = R.sh_records(pts, 7.5)
    for lanes, first in ((4, 11), (128, 5)):
        m = len(recs) * lanes
        rays = sc.query_sh_rays(recs, lanes, seed=SEED, first_stream=first)
        probe = sc.bsdf_sample(np.full(m, 2, np.int32), np.tile(np.array([(0, 0, 1)], np.float32), (m, 1)), np.zeros(m, np.int32),
                               (first + np.arange(m)).astype(np.uint32), seed=SEED)
        assert (probe[:, 7] == 2).all()                               # a diffuse bounce spends two draws: the sample's direction is made of two
        local = probe[:, 0:3]
        assert (local[:, 2] > 0).all() and len(np.unique(local.view(np.uint32), axis=0)) == m
        d = SR.sphere_map(local)
        assert_bits_equal(rays[:, 4:7], d, "d against the restatement, %d lanes" % lanes)
        assert_bits_equal(rays[:, 0:3], np.repeat(pts, lanes, 0), "o is p, %d lanes" % lanes)
        assert (rays[:, 3] == 7.5).all() and np.array_equal(rays[:, 7].view(np.uint32), np.arange(m, dtype=np.uint32))
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 4 * 2.0 ** -23
        assert (d[:, 2] < 0).any() and (d[:, 2] > 0).any()                # both hemispheres
        # PT_QUERY_STREAM_PAD: lane l of a record with pad word p is stream first + p * L + l, and carries p * L + l
        padded = recs.copy()
        padded[:, 7].view(np.uint32)[:] = 5 + np.arange(len(recs), dtype=np.uint32)
        shifted = sc.query_sh_rays(padded, lanes, seed=SEED, first_stream=first + 1000 - 5 * lanes, flags=PAD)
        again = sc.query_sh_rays(recs, lanes, seed=SEED, first_stream=first + 1000)
        assert_bits_equal(shifted[:, :7], again[:, :7], "pad = 5 + i with first_stream - 5 L, %d lanes" % lanes)
        assert np.array_equal(shifted[:, 7].view(np.uint32), 5 * lanes + np.arange(m, dtype=np.uint32))
    # the device form, and draw offsets of zero, change nothing
    torch = gpu_ready
    dev = sc.query_sh_rays(torch.from_numpy(recs).to("cuda:0"), lanes, seed=SEED, first_stream=first, draw_offset=np.zeros(m, np.uint32))
    assert dev.is_cuda
    assert_bits_equal(dev.cpu().numpy(), rays, "torch in, torch out")


# ---- 3. several samples per stream -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 4])
def test_the_stream_runs_on_through_a_lanes_samples(api, gpu_ready, cases, lanes):
    """Integrator 2 at max_depth 1 on the plain box: Li is the first hit's emission and reads no random number, and a sample spends
    its two direction draws and, on a hit, the bounce's two (cosine_sample_f: pt_probe_bsdf_sample counts them). So sample j of a lane
    is the ray emitted at the lane's current draw offset, wherever pt_query_radiance's own stream stands."""
    c = cases["simple"]
    sc, recs = c["sc"], c["recs"]
    m = N * lanes
    offs = np.zeros(m, np.uint32)
    ts, hits_seen, lit_later = [], 0, 0
    for j in range(3):
        rays = sc.query_sh_rays(recs, lanes, seed=SEED, draw_offset=offs)
        hit = sc.query_closest(rays)["tri"] >= 0
        li = sc.query_radiance(rays, 1, 1, integrator=2, seed=SEED, stream_pad=True)
        ts.append(SR.terms(li, rays[:, 4:7]))
        offs = IR.advance(offs, hit)
        hits_seen += int(hit.sum())
        lit_later += int((li[:, :3] > 0).any(1).sum()) if j else 0
    assert hits_seen > 0 and offs.max() == 12 and offs[(N - 1) * lanes:].max() == 6         # lanes that hit, and the far probe's that missed
    want = SR.coeffs(SR.lane_sum(ts).reshape(N, lanes, 9, 3))
    print("lanes", lanes, "probes that see the emitter:", int((want[:, 0, :3] > 0).any(1).sum()), "lit after the first sample:", lit_later)
    assert (want[:, 0, :3] > 0).any() and lit_later > 0
    got = sc.query_sh(recs, lanes, 3, 1, integrator=2, seed=SEED)
    assert_bits_equal(got, want, "three samples a lane")


# ---- 4. a record is its own ------------------------------------------------------------------------------------------------------------------
def test_a_records_result_depends_on_nothing_around_it(api, gpu_ready, cases):
    c = cases["mixed"]
    sc = c["sc"]
    recs = c["recs"].copy()
    recs[:, 7].view(np.uint32)[:] = np.arange(N, dtype=np.uint32)
    spp_lane = 2
    for lanes in (4, 128):
        for integ, mis in SETTINGS:
            what = "%d lanes, integrator %d, mis %d" % (lanes, integ, mis)
            q = lambda r, **kw: sc.query_sh(r, lanes, spp_lane, DEPTH, integrator=integ, use_mis=mis, seed=SEED, **kw)
            base = q(recs)
            assert (base[:, 0, :3] > 0).any()
            assert_bits_equal(q(recs, flags=PAD), base, what + ": pad = i")
            perm = np.random.default_rng(9).permutation(N)
            assert_bits_equal(q(np.ascontiguousarray(recs[perm]), flags=PAD), base[perm], what + ": permuted")
            for i in (0, 3):
                assert_bits_equal(q(np.ascontiguousarray(recs[i:i + 1]), flags=PAD), base[i:i + 1], what + ": record %d alone" % i)
                assert_bits_equal(q(np.ascontiguousarray(recs[i:i + 1]), first_stream=i * lanes), base[i:i + 1], what + ": record %d alone by first_stream" % i)
            moved = recs.copy()
            moved[:, 4:7] = (0.0, 1.0, 0.0)
            assert_bits_equal(q(moved), base, what + ": other direction words")


def test_the_material_class_options_change_no_bit(api, gpu_ready, cases):
    """The plain box with "simple" 0 (the LEAN kernel), "lean" 0 (still SIMPLE) and both (the generic kernel); the mixed box with
    "lean" 0 (generic): every one of the six kernels has then run, on the same bits."""
    for name, option_sets in (("simple", ({"simple": 0}, {"lean": 0}, {"simple": 0, "lean": 0})), ("mixed", ({"lean": 0},))):
        c = cases[name]
        q = lambda s, integ, mis: s.query_sh(c["recs"], 8, 2, DEPTH, integrator=integ, use_mis=mis, seed=SEED)
        want = {st: q(c["sc"], *st) for st in SETTINGS}
        for options in option_sets:
            s = api.Scene(c["hs"], options=options)
            for st in SETTINGS:
                assert_bits_equal(q(s, *st), want[st], "%s with %r, integrator %d, mis %d" % ((name, options) + st))
            s.close()


# ---- 5. the device form ----------------------------------------------------------------------------------------------------------------------
def test_the_device_form_is_the_host_form_and_writes_nothing_past_its_buffers(api, gpu_ready, cases):
    torch = gpu_ready
    c = cases["mixed"]
    sc, recs = c["sc"], c["recs"]
    d = torch.from_numpy(recs.copy()).to("cuda:0")
    L = api.lib()
    GUARD, TAIL = 0x5a5a5a5a, 16
    for lanes in (1, 64, 128):
        host = sc.query_sh(recs, lanes, 2, DEPTH, seed=SEED)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            t = sc.query_sh(d.clone(), lanes, 2, DEPTH, seed=SEED)
        side.synchronize()
        assert isinstance(t, torch.Tensor) and t.device == d.device and t.shape == (N, 9, 4)
        assert_bits_equal(t.cpu().numpy(), host, "torch in, torch out, %d lanes" % lanes)
        # the call writes, it does not add, and nothing past coefficient 9 n - 1 or past the workspace: the buffers pre-filled
        stream = torch.cuda.current_stream().cuda_stream or None
        for n in (1, N):
            tiles = n * (lanes // 64) if lanes > 64 else 0
            assert L.pt_query_sh_workspace_bytes(n, lanes) == tiles * 9 * 16
            bc = torch.full((9 * n + TAIL, 4), GUARD, dtype=torch.int32, device="cuda:0")
            bw = torch.full((9 * tiles + TAIL, 4), GUARD, dtype=torch.int32, device="cuda:0")
            assert L.pt_query_sh_device(sc.h, n, d.data_ptr(), lanes, 2, DEPTH, 0, 1, SEED, 0, bc.data_ptr(), bw.data_ptr(), 0, stream) == 0, L.pt_last_error()
            torch.cuda.synchronize()
            gc, gw = bc.cpu().numpy(), bw.cpu().numpy()
            assert (gc[9 * n:] == GUARD).all() and (gw[9 * tiles:] == GUARD).all(), (n, lanes)
            assert_bits_equal(gc[:9 * n].view(np.float32).reshape(n, 9, 4), host[:n], "n = %d, %d lanes" % (n, lanes))
            if lanes <= 64:                                           # and without a workspace
                bc.fill_(GUARD)
                assert L.pt_query_sh_device(sc.h, n, d.data_ptr(), lanes, 2, DEPTH, 0, 1, SEED, 0, bc.data_ptr(), None, 0, stream) == 0, L.pt_last_error()
                torch.cuda.synchronize()
                assert_bits_equal(bc.cpu().numpy()[:9 * n].view(np.float32).reshape(n, 9, 4), host[:n], "n = %d, %d lanes, NULL workspace" % (n, lanes))
    empty = sc.query_sh(d[:0], 128, 2, DEPTH)
    assert empty.shape == (0, 9, 4) and empty.is_cuda


# ---- 6. nothing to see ---------------------------------------------------------------------------------------------------------------------------
def test_the_far_probe_and_max_t_zero_give_exact_zeros(api, gpu_ready, cases):
    from cudapathtracer_amd import rays as R
    for name in ("simple", "hbm"):
        c = cases[name]
        sc = c["sc"]
        away = R.sh_records(np.tile(c["recs"][N - 1:, 0:3], (3, 1)))
        blind = R.sh_records(c["recs"][:4, 0:3], 0.0)
        for integ, mis in SETTINGS:
            for lanes in (64, 256):
                z = sc.query_sh(away, lanes, 3, DEPTH, integrator=integ, use_mis=mis, seed=SEED)
                assert z.shape == (3, 9, 4) and not z.view(np.uint32).any(), (name, integ, mis, lanes)
                z = sc.query_sh(blind, lanes, 3, DEPTH, integrator=integ, use_mis=mis, seed=SEED)
                assert z.shape == (4, 9, 4) and not z.view(np.uint32).any(), (name, integ, mis, lanes, "max_t = 0")
        assert (sc.query_sh(c["recs"], 64, 3, DEPTH, seed=SEED)[:4, 0, :3] > 0).any()


# ---- 7. the scene around the call ----------------------------------------------------------------------------------------------------------------
def test_an_edited_scene_answers_as_a_fresh_one(api, gpu_ready, cases):
    c = cases["simple"]
    hs = c["hs"]
    sc = api.Scene.from_mesh(hs)
    q = lambda s: [s.query_sh(c["recs"], lanes, 2, DEPTH, integrator=i, use_mis=m, seed=SEED) for i, m in SETTINGS for lanes in (4, 128)]
    before = q(sc)
    for x, y in zip(before, q(c["sc"])):
        assert_bits_equal(x, y, "two scenes of the same arrays")
    a = {k: hs.array(k) for k in MC.GEOMETRY}
    mats = a["materials"].copy().reshape(-1, 176)
    mats[2] = mats[19]                                        # the white walls and boxes become mirrors
    mirrored = dict(a, materials=mats.reshape(-1))
    sc.update_materials(mirrored["materials"])
    fresh = api.Scene.from_mesh(mirrored, max_leaf_size=hs.info["leaf_size"])
    got = q(sc)
    for x, y in zip(got, q(fresh)):
        assert_bits_equal(x, y, "after update_materials")
    assert not np.array_equal(got[0].view(np.uint32), before[0].view(np.uint32))
    fresh.close()
    sc.close()


def test_a_query_moves_nothing_else(api, gpu_ready, cases):
    from cudapathtracer_amd import rays as R
    c = cases["mixed"]
    sc, recs = c["sc"], c["recs"]
    surface = R.irradiance_records(recs[:4, 0:3], np.tile([(0.0, 1.0, 0.0)], (4, 1)))
    img0, _ = sc.render(c["cam0"], RC.W, RC.H, 2, DEPTH, seed=SEED)
    irr0 = sc.query_irradiance(surface, 4, 2, DEPTH, seed=SEED)
    sc.render(c["cam0"], RC.W, RC.H, 1, 3, counters=True)                       # something in the counters
    cnt0 = sc.counters()
    assert cnt0["rays_closest"] > 0
    for lanes in (4, 128):
        sc.query_sh(recs, lanes, 2, DEPTH, seed=SEED)
        sc.query_sh_rays(recs, lanes, seed=SEED)
    assert sc.counters() == cnt0
    img1, _ = sc.render(c["cam0"], RC.W, RC.H, 2, DEPTH, seed=SEED)
    assert_bits_equal(img1, img0, "a render after the query against one before it")
    assert_bits_equal(sc.query_irradiance(surface, 4, 2, DEPTH, seed=SEED), irr0, "an irradiance query after the query against one before it")
