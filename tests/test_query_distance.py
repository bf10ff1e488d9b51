"""Distance probes (pt_query_distance, pt_query_distance_rays_device) on the GPU, bit for bit. The tie is to a call that is checked
against the oracle: a lane's one sample is pt_query_closest (with surfaces) on the ray pt_query_distance_rays_device emits for it;
the emitted direction is tests/distance_ref.py's restatement of the header's map on pt_probe_rng's uniforms; the sums are its
sequential sums.

Scenes: test_query_sh.py's three at their small sizes: the plain diffuse Cornell box, tests/radiance_cases.py's Cornell box with a
glass and a mirror box, and the blob in the box, which lies in HBM and spills. Probes: six each: four inside the scene, one far above
it, and one inside a closed object (the tall box, the blob), found as the midpoint of the entry and exit hits of a ray through it.
The fourth probe sees no further than a quarter of the scene's size."""
import os

import numpy as np
import pytest

import distance_ref as DR
import motion_cases as MC
import radiance_cases as RC
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SEED = 103033
N = 6
PAD, CENTRE = 2, 4                                             # api.QUERY_STREAM_PAD, api.QUERY_TEXEL_CENTRE
FAR = 5000.0                                                   # the fifth probe hangs this many scene sizes above the scene
INSIDE = ((0.3, 0.6, 0.4), (0.7, 0.3, 0.6), (0.5, 0.8, 0.5), (0.25, 0.25, 0.7))      # fractions of the scene's bounding box
SHORT = 3                                                      # the record with the small max_t (the fourth probe stands in the open in all three scenes)
FAR_I, IN_OBJECT = 4, 5


def _bounds(hs):
    pts = np.ascontiguousarray(hs.array("points")).view(np.float32).reshape(-1, 4)[:, :3]
    return pts.min(0), pts.max(0)


def _inside_object(sc, lo, hi, through):
    """The midpoint of the entry and the exit hit of a ray along +x from the left wall through `through`, a point of the object."""
    from cudapathtracer_amd import rays as R
    d = np.array([(1.0, 0.0, 0.0)], np.float32)
    o = np.array([(lo[0] + 0.01, through[1], through[2])], np.float32)
    h1, s1 = sc.query_closest(R.irradiance_records(o, d), surfaces=True)
    assert h1["tri"][0] >= 0 and s1["backface"][0] == 0
    entry = np.array([(s1["px"][0], s1["py"][0], s1["pz"][0])], np.float32)
    h2, s2 = sc.query_closest(R.irradiance_records(entry + np.float32(1e-3) * d, d), surfaces=True)
    assert h2["tri"][0] >= 0 and s2["backface"][0] == 1                       # the exit is seen from behind: the object is closed
    leave = np.array([(s2["px"][0], s2["py"][0], s2["pz"][0])], np.float32)
    assert entry[0, 0] < through[0] < leave[0, 0]
    return (0.5 * (entry + leave))[0]


def _probes(hs, sc, through):
    from cudapathtracer_amd import rays as R
    lo, hi = _bounds(hs)
    size = float((hi - lo).max())
    mid = 0.5 * (lo + hi)
    p = np.concatenate([lo + np.array(INSIDE, np.float32) * (hi - lo), [(mid[0], hi[1] + FAR * size, mid[2])],
                        [_inside_object(sc, lo, hi, through)]], 0).astype(np.float32)
    recs = R.distance_records(p, 4.0 * size)
    recs[SHORT, 3] = 0.25 * size
    recs[:, 4:7] = (7.0, -3.0, np.nan)                         # the direction words are not read
    recs.setflags(write=False)
    return recs


@pytest.fixture(scope="module")
def cases(api, gpu_ready, scene_dir):
    from cudapathtracer_amd import scenes
    out = {}
    plain = api.HostScene(scenes.cornell(os.path.join(scene_dir, "dist_plain"), width=RC.W, height=RC.H, name="dist_plain", spp=4, max_depth=4)["config"])
    mixed = RC.host(api, scene_dir, "cornell", prefix="dist_")
    blob = api.HostScene(scenes.blob_in_box(os.path.join(scene_dir, "dist_blob"), RC.W, RC.H, 2, 5, subdiv=4, name="dist_blob")["config"])
    for name, hs, make in (("simple", plain, api.Scene.from_mesh), ("mixed", mixed, api.Scene), ("hbm", blob, api.Scene.from_mesh)):
        sc = make(hs)
        cam0 = api.Camera.frombytes(MC.cam0_bytes(hs.camera()).tobytes())
        sc.render(cam0, RC.W, RC.H, 1, 2)
        lo, hi = _bounds(hs)
        zc = 0.5 * (lo[2] + hi[2])
        through = (0.0, -0.25, zc) if name == "hbm" else (-0.6 if RC.W / RC.H > 1.2 else -0.42, -0.5, zc - 0.35)      # scenes.py: the blob's centre, the tall box's axis
        out[name] = {"hs": hs, "sc": sc, "cam0": cam0, "recs": _probes(hs, sc, through), "flags": sc.flags()}
    assert out["simple"]["flags"]["simple"] and out["mixed"]["flags"]["lean"] and not out["hbm"]["flags"]["onchip"]
    yield out
    for c in out.values():
        c["sc"].close()


def _by_closest(sc, rays):
    """[m, 4]: the texel a single sample on each emitted ray gives, through pt_query_closest with surfaces."""
    hits, surf = sc.query_closest(rays, surfaces=True)
    return DR.texel_sums([DR.from_closest(hits, surf, rays[:, 3])])


# ---- 1. one sample per lane: the emitted rays through pt_query_closest ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["simple", "mixed", "hbm"])
def test_one_sample_per_lane_is_query_closest_on_the_emitted_rays(api, gpu_ready, cases, name):
    """Five records at R = 4 are 80 lanes, a full tile shared by four records and a ragged one; six are 96. At R = 8 a record is a
    tile, at R = 16 four."""
    c = cases[name]
    sc, recs = c["sc"], c["recs"]
    for res, first, n in ((4, 7, 5), (4, 7, N), (8, 0, N), (16, 3, N)):
        what = "%s, res %d, %d records" % (name, res, n)
        r = np.ascontiguousarray(recs[:n])
        rays = sc.query_distance_rays(r, res, seed=SEED, first_stream=first)
        assert rays.shape == (n * res * res, 8) and np.array_equal(rays[:, 7].view(np.uint32), np.arange(n * res * res, dtype=np.uint32))
        want = _by_closest(sc, rays).reshape(n, res, res, 4)
        got = sc.query_distance(r, res, 1, seed=SEED, first_stream=first)
        assert got.shape == (n, res, res, 4) and got.dtype == np.float32
        assert_bits_equal(got, want, what)
        if n < N:
            continue
        # what this data holds: hits, misses, and hits that a small max_t turns into misses at max_t
        hit = got[..., 2] == 1
        assert hit[:4].any() and not hit[FAR_I].any(), what
        assert (got[FAR_I, ..., 0] == recs[FAR_I, 3]).all()
        far_reach = rays[SHORT * res * res:(SHORT + 1) * res * res].copy()
        far_reach[:, 3] = recs[0, 3]
        t = sc.query_closest(far_reach)
        clamped = (t["tri"] >= 0) & (t["t"] > recs[SHORT, 3])
        assert clamped.any() and not hit[SHORT].reshape(-1)[clamped].any(), what
        assert (got[SHORT].reshape(-1, 4)[clamped, 0] == recs[SHORT, 3]).all() and hit[SHORT].any(), what
        # the probe inside the object sees surfaces from behind; a probe in the open sees them from the front
        assert hit[IN_OBJECT].all() and (got[IN_OBJECT, ..., 3] > 0).any(), what
        assert ((got[:4, ..., 3] == 0) & hit[:4]).any(), what
        assert (got[..., 3] <= got[..., 2]).all()
        print(what, "hits", int(hit.sum()), "clamped", int(clamped.sum()), "from behind", int(got[..., 3].sum()))


# ---- 2. the emitted ray ------------------------------------------------------------------------------------------------------------------------------
def test_the_emitted_ray_is_the_headers_map_on_the_streams_first_two_uniforms(api, gpu_ready, cases):
    from cudapathtracer_amd import rays as R
    c = cases["simple"]
    sc = c["sc"]
    pts = np.concatenate([np.random.default_rng(2).uniform(-2, 2, (20, 3)).astype(np.float32), c["recs"][:, 0:3], [(0.0, -0.0, 1e-30)]], 0).astype(np.float32)
    recs = R.distance_records(pts, 7.5)
    for res, first in ((4, 11), (16, 5)):
        L = res * res
        m = len(recs) * L
        rays = sc.query_distance_rays(recs, res, seed=SEED, first_stream=first)
        u = api.probe_rng((first + np.arange(m)).astype(np.uint32), 2, seed=SEED)[2]
        tx, ty = DR.texel_of_lane(np.arange(m) % L, res)
        d = DR.oct_map(tx, ty, u[:, 0], u[:, 1], res)
        assert_bits_equal(rays[:, 4:7], d, "d against the restatement, res %d" % res)
        assert_bits_equal(rays[:, 0:3], np.repeat(pts, L, 0), "o is p, res %d" % res)
        assert np.signbit(rays[-L:, 1]).all() and (rays[-L:, 2] == np.float32(1e-30)).all()
        assert (rays[:, 3] == 7.5).all() and np.array_equal(rays[:, 7].view(np.uint32), np.arange(m, dtype=np.uint32))
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 4 * 2.0 ** -23
        assert (d[:, 2] < 0).any() and (d[:, 2] > 0).any()                # both sides of the fold
        # PT_QUERY_STREAM_PAD: lane l of a record with pad word p is stream first + p * L + l, and carries p * L + l
        perm = np.random.default_rng(4).permutation(len(recs)).astype(np.uint32)
        padded = recs.copy()
        padded[:, 7].view(np.uint32)[:] = 5 + perm
        shifted = sc.query_distance_rays(padded, res, seed=SEED, first_stream=first + 1000 - 5 * L, flags=PAD)
        again = sc.query_distance_rays(recs, res, seed=SEED, first_stream=first + 1000).reshape(len(recs), L, 8)
        lanes = (perm[:, None] * L + np.arange(L, dtype=np.uint32)[None, :]).reshape(-1)
        moved = np.concatenate([np.repeat(pts, L, 0), np.full((m, 1), 7.5, np.float32), again[perm][:, :, 4:7].reshape(m, 3)], 1)
        assert_bits_equal(shifted[:, :7], moved, "pad = 5 + perm(i) with first_stream - 5 L, res %d" % res)
        assert np.array_equal(shifted[:, 7].view(np.uint32), 5 * L + lanes)
    # the device form, and draw offsets of zero, change nothing
    torch = gpu_ready
    dev = sc.query_distance_rays(torch.from_numpy(recs).to("cuda:0"), res, seed=SEED, first_stream=first, draw_offset=np.zeros(m, np.uint32))
    assert dev.is_cuda
    assert_bits_equal(dev.cpu().numpy(), rays, "torch in, torch out")


# ---- 3. centre mode ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["simple", "hbm"])
def test_centre_mode_reads_no_stream_and_is_query_closest_on_the_texel_centres(api, gpu_ready, cases, name):
    c = cases[name]
    sc = c["sc"]
    for res, n in ((4, N), (8, N), (16, N), (32, 1)):
        what = "%s, res %d" % (name, res)
        L = res * res
        recs = np.ascontiguousarray(c["recs"][:n]) if n > 1 else np.ascontiguousarray(c["recs"][2:3])
        rays = sc.query_distance_rays(recs, res, seed=SEED, first_stream=9, flags=CENTRE)
        tx, ty = DR.texel_of_lane(np.arange(n * L) % L, res)
        assert_bits_equal(rays[:, 4:7], DR.oct_map(tx, ty, np.float32(0.5), np.float32(0.5), res), what + ": d is the map at the centre")
        assert_bits_equal(rays[:, 0:3], np.repeat(recs[:, 0:3], L, 0), what)
        assert np.array_equal(rays[:, 7].view(np.uint32), np.arange(n * L, dtype=np.uint32)) and np.array_equal(rays[:, 3], np.repeat(recs[:, 3], L))
        other = sc.query_distance_rays(recs, res, seed=7, first_stream=0xfffffff0, flags=CENTRE | PAD, draw_offset=np.full(n * L, 3, np.uint32))
        assert_bits_equal(other, rays, what + ": another seed, first_stream, pad flag and draw offset")
        got = sc.query_distance(recs, res, 1, seed=SEED, first_stream=9, flags=CENTRE)
        assert_bits_equal(got, _by_closest(sc, rays).reshape(n, res, res, 4), what + ": the identity")
        assert_bits_equal(sc.query_distance(recs, res, 1, seed=7, first_stream=0xfffffff0, flags=CENTRE), got, what + ": another seed and first_stream")
        assert (got[..., 2] == 1).any()
        jittered = sc.query_distance(recs, res, 1, seed=SEED, first_stream=9)
        assert not np.array_equal(jittered.view(np.uint32), got.view(np.uint32))


# ---- 4. several samples per lane -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [4, 16])
def test_the_stream_runs_on_through_a_lanes_samples(api, gpu_ready, cases, res):
    """The trace draws nothing: sample j of a lane is the ray emitted at draw offset 2 j."""
    told = False
    for name in ("simple", "hbm"):
        c = cases[name]
        sc, recs = c["sc"], c["recs"]
        m = N * res * res
        samples = []
        for j in range(3):
            rays = sc.query_distance_rays(recs, res, seed=SEED, first_stream=2, draw_offset=np.full(m, 2 * j, np.uint32))
            hits, surf = sc.query_closest(rays, surfaces=True)
            samples.append(DR.from_closest(hits, surf, rays[:, 3]))
        want = DR.texel_sums(samples)
        got = sc.query_distance(recs, res, 3, seed=SEED, first_stream=2)
        assert_bits_equal(got, want.reshape(N, res, res, 4), "%s, res %d: three samples a lane" % (name, res))
        assert (want[:, 2] == 3).any() and ((want[:, 2] > 0) & (want[:, 2] < 3)).any()
        told |= not np.array_equal(DR.texel_sums(samples[::-1])[:, :2], want[:, :2])            # the order of the sums shows on this data
    assert told


# ---- 5. a record is its own ------------------------------------------------------------------------------------------------------------------------------
def test_a_records_map_depends_on_nothing_around_it(api, gpu_ready, cases):
    c = cases["mixed"]
    sc = c["sc"]
    recs = c["recs"].copy()
    recs[:, 7].view(np.uint32)[:] = np.arange(N, dtype=np.uint32)
    for res in (4, 16):
        L = res * res
        what = "res %d" % res
        q = lambda r, **kw: sc.query_distance(r, res, 2, seed=SEED, **kw)
        base = q(recs)
        assert (base[..., 2] > 0).any()
        assert_bits_equal(q(recs, flags=PAD), base, what + ": pad = i")
        perm = np.random.default_rng(9).permutation(N)
        assert_bits_equal(q(np.ascontiguousarray(recs[perm]), flags=PAD), base[perm], what + ": permuted")
        for i in (0, 3, 5):
            assert_bits_equal(q(np.ascontiguousarray(recs[i:i + 1]), flags=PAD), base[i:i + 1], what + ": record %d alone" % i)
            assert_bits_equal(q(np.ascontiguousarray(recs[i:i + 1]), first_stream=i * L), base[i:i + 1], what + ": record %d alone by first_stream" % i)
        assert_bits_equal(q(np.ascontiguousarray(recs[2:]), first_stream=2 * L), base[2:], what + ": the tail, shifted by first_stream")
        shifted = recs.copy()
        shifted[:, 7].view(np.uint32)[:] += 3
        assert_bits_equal(q(shifted, flags=PAD, first_stream=0xffffffff - 3 * L + 1), base, what + ": pad = i + 3 with first_stream = -3 L (it wraps)")
        moved = recs.copy()
        moved[:, 4:7] = (0.0, 1.0, 0.0)
        assert_bits_equal(q(moved), base, what + ": other direction words")


def test_the_material_class_options_change_no_bit(api, gpu_ready, cases):
    for name, option_sets in (("simple", ({"simple": 0}, {"lean": 0}, {"simple": 0, "lean": 0})), ("mixed", ({"lean": 0},))):
        c = cases[name]
        q = lambda s: [s.query_distance(c["recs"], 8, 2, seed=SEED), s.query_distance(c["recs"], 4, 1, flags=CENTRE)]
        want = q(c["sc"])
        for options in option_sets:
            s = api.Scene(c["hs"], options=options)
            for x, y in zip(q(s), want):
                assert_bits_equal(x, y, "%s with %r" % (name, options))
            s.close()


# ---- 6. the device form --------------------------------------------------------------------------------------------------------------------------------
def test_the_device_form_is_the_host_form_and_writes_nothing_past_its_maps(api, gpu_ready, cases):
    torch = gpu_ready
    c = cases["mixed"]
    sc, recs = c["sc"], c["recs"]
    d = torch.from_numpy(recs.copy()).to("cuda:0")
    L = api.lib()
    GUARD, TAIL = 0x5a5a5a5a, 16
    for res in (4, 8, 16):
        host = sc.query_distance(recs, res, 2, seed=SEED)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            t = sc.query_distance(d.clone(), res, 2, seed=SEED)
        side.synchronize()
        assert isinstance(t, torch.Tensor) and t.device == d.device and t.shape == (N, res, res, 4)
        assert_bits_equal(t.cpu().numpy(), host, "torch in, torch out, res %d" % res)
        stream = torch.cuda.current_stream().cuda_stream or None
        for n in (1, 5):
            for flags, spp in ((0, 2), (CENTRE, 1)):
                want = host[:n] if not flags else sc.query_distance(np.ascontiguousarray(recs[:n]), res, 1, flags=CENTRE)
                buf = torch.full((n * res * res + TAIL, 4), GUARD, dtype=torch.int32, device="cuda:0")
                assert L.pt_query_distance_device(sc.h, n, d.data_ptr(), res, spp, SEED, 0, buf.data_ptr(), flags, stream) == 0, L.pt_last_error()
                torch.cuda.synchronize()
                g = buf.cpu().numpy()
                assert (g[n * res * res:] == GUARD).all(), (n, res, flags)
                assert_bits_equal(g[:n * res * res].view(np.float32).reshape(n, res, res, 4), want, "n = %d, res %d, flags %d" % (n, res, flags))
    empty = sc.query_distance(d[:0], 8)
    assert empty.shape == (0, 8, 8, 4) and empty.is_cuda


# ---- 7. nothing to see -----------------------------------------------------------------------------------------------------------------------------------
def test_the_far_probe_sums_max_t_and_max_t_zero_gives_exact_zeros(api, gpu_ready, cases):
    from cudapathtracer_amd import rays as R
    F = np.float32
    for name in ("simple", "hbm"):
        c = cases[name]
        sc = c["sc"]
        reach = F(c["recs"][FAR_I, 3]) * F(1.1)                              # a value whose triple sum rounds
        away = R.distance_records(np.tile(c["recs"][FAR_I:FAR_I + 1, 0:3], (3, 1)), reach)
        blind = R.distance_records(c["recs"][:4, 0:3], 0.0)
        a = (F(0.0) + reach + reach) + reach
        b = ((F(0.0) + reach * reach) + reach * reach) + reach * reach
        for res in (4, 16):
            z = sc.query_distance(away, res, 3, seed=SEED)
            assert z.shape == (3, res, res, 4) and (z[..., 0] == a).all() and (z[..., 1] == b).all() and not z[..., 2:].view(np.uint32).any(), (name, res)
            z = sc.query_distance(blind, res, 3, seed=SEED)
            assert z.shape == (4, res, res, 4) and not z.view(np.uint32).any(), (name, res, "max_t = 0")
            z = sc.query_distance(blind, res, 1, flags=CENTRE)
            assert not z.view(np.uint32).any(), (name, res, "max_t = 0, centre")


# ---- 8. the scene around the call ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["simple", "mixed", "hbm"])
def test_an_edited_scene_answers_as_a_fresh_one(api, gpu_ready, cases, name):
    c = cases[name]
    hs = c["hs"]
    leaf = hs.info["leaf_size"]
    from_mesh = name != "mixed"
    everything = {k: hs.array(k) for k in MC.GEOMETRY + ("bvh", "indices")}
    a = {k: everything[k] for k in MC.GEOMETRY}

    def make(arrays):
        if from_mesh:
            return api.Scene.from_mesh(arrays, max_leaf_size=leaf), None
        desc, keep = api._desc_from_arrays(dict(everything, **arrays))
        return api.Scene(desc=desc), keep

    sc = api.Scene.from_mesh(hs) if from_mesh else api.Scene(hs)
    q = lambda s: [s.query_distance(c["recs"], 8, 2, seed=SEED), s.query_distance(c["recs"], 16, 1, flags=CENTRE), s.query_distance(c["recs"], 4, 1, seed=SEED)]
    before = q(sc)
    for x, y in zip(before, q(c["sc"])):
        assert_bits_equal(x, y, "two scenes of the same arrays")
    if from_mesh:
        moved = dict(a, points=a["points"].copy())
        first = 24 if name == "hbm" else 48                                 # the blob, which is the scene's last vertices; the second box
        moved["points"].view(np.float32).reshape(-1, 4)[first:, :3] += np.array((0.1, 0.05, -0.1), np.float32)
        sc.update_vertices(moved["points"])
        fresh, _ = make(moved)
        got = q(sc)
        for x, y in zip(got, q(fresh)):
            assert_bits_equal(x, y, name + ": after update_vertices")
        assert not np.array_equal(got[0].view(np.uint32), before[0].view(np.uint32))
        fresh.close()
        a = moved
    mats = a["materials"].copy().reshape(-1, 176)
    mats[2] = mats[19]                                                      # the white row becomes a mirror
    mirrored = dict(a, materials=mats.reshape(-1))
    sc.update_materials(mirrored["materials"])
    fresh, keep = make(mirrored)
    for x, y in zip(q(sc), q(fresh)):
        assert_bits_equal(x, y, name + ": after update_materials")
    fresh.close()
    sc.close()


def test_a_query_moves_nothing_else(api, gpu_ready, cases):
    c = cases["mixed"]
    sc, recs = c["sc"], c["recs"]
    img0, _ = sc.render(c["cam0"], RC.W, RC.H, 2, 4, seed=SEED)
    sh0 = sc.query_sh(recs, 4, 2, 4, seed=SEED)
    sc.render(c["cam0"], RC.W, RC.H, 1, 3, counters=True)                       # something in the counters
    cnt0 = sc.counters()
    assert cnt0["rays_closest"] > 0
    for res in (4, 16):
        sc.query_distance(recs, res, 2, seed=SEED)
        sc.query_distance(recs, res, 1, flags=CENTRE)
        sc.query_distance_rays(recs, res, seed=SEED)
    assert sc.counters() == cnt0
    img1, _ = sc.render(c["cam0"], RC.W, RC.H, 2, 4, seed=SEED)
    assert_bits_equal(img1, img0, "a render after the query against one before it")
    assert_bits_equal(sc.query_sh(recs, 4, 2, 4, seed=SEED), sh0, "an SH query after the query against one before it")
