"""Guide queries (pt_query_guides) on the GPU, bit for bit on every ray: the centre rays of a camera against pt_render_aovs_centre in
the host and the device form; rays that are no camera's against the numpy restatement of the chain on the oracle's hits; a max_t at
and just past the first hit; two cameras' rays shuffled; guard words behind all three outputs; edited scenes against fresh ones; and
the composition the calls exist for: moments + guides + the variance-guided filter on a camera's rays and on a panorama.
tests/radiance_cases.py and tests/query_cases.py have the input."""
import os

import numpy as np
import pytest

import aov_chain_ref as CR
import motion_cases as MC
import query_cases as QC
import radiance_cases as RC
from denoise_ref import aovs_from_hits
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SEED = 103033
LINKS = (0, 1, 4)


@pytest.fixture(scope="module")
def cases(api, oracle, gpu_ready, scene_dir):
    """Per case: the GPU scene, cam0, its centre rays as records, the oracle scene, and per max_links the camera's centre pass as
    [N, 4], [N, 4] and [N] rows, computed once and never written to."""
    out = {}
    for name in RC.CASES:
        hs = RC.host(api, scene_dir, name, prefix="qguides_")
        cam0 = RC.cam0(api, hs, name)
        sc = api.Scene(hs)
        want = {}
        for m in LINKS:
            a, nd, ln = sc.render_aovs_centre(cam0, RC.W, RC.H, m, links=True)
            want[m] = (RC.as_rays(a), RC.as_rays(nd), np.ascontiguousarray(ln).reshape(RC.N))
            for v in want[m]:
                v.setflags(write=False)
        out[name] = {"hs": hs, "sc": sc, "cam0": cam0, "osc": oracle.OracleScene(arrays=RC.arrays(hs)), "recs": RC.centre_records(api, cam0),
                     "want": want}
    yield out
    for c in out.values():
        c["sc"].close()


def _same(got, want, what):
    for g, w, k in zip(got, want, ("albedo", "normal_depth", "links")):
        g = g.cpu().numpy() if hasattr(g, "is_cuda") else g
        assert_bits_equal(g, w, what + ": " + k)


# ---- 1. the centre rays are the camera's centre pass ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.CASES)
def test_centre_rays_are_the_cameras_centre_pass(api, gpu_ready, cases, name):
    c = cases[name]
    lib_rays = c["sc"].query_camera_rays(c["cam0"], RC.W, RC.H)
    for m in LINKS:
        want = c["want"][m]
        assert (want[0][:, 3] == 1).any() and (m == 0 or name == "textured" or (want[2] > 0).any())
        host = c["sc"].query_guides(c["recs"], m, links=True)
        assert all(isinstance(v, np.ndarray) for v in host) and host[0].shape == (RC.N, 4) and host[1].shape == (RC.N, 4) and host[2].shape == (RC.N,)
        _same(host, want, "%s, max_links %d, host form" % (name, m))
        dev = c["sc"].query_guides(lib_rays, m, links=True)
        assert all(v.is_cuda for v in dev) and dev[2].shape == (RC.N,)
        _same(dev, want, "%s, max_links %d, device form" % (name, m))
        two = c["sc"].query_guides(c["recs"], m)
        assert len(two) == 2
        _same(two, want[:2], "%s, max_links %d, without links" % (name, m))


# ---- 2. rays that are no camera's, against the restated chain on the oracle's hits ---------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "glass_mirror"])
def test_arbitrary_rays_against_the_restated_chain(api, oracle, gpu_ready, cases, name):
    c = cases[name]
    rays = QC.ray_set(oracle, c["cam0"], RC.arrays(c["hs"]), name)
    mats = CR.Materials(c["osc"])
    r = CR.chain_rays(c["osc"], mats, rays, 4)
    k = CR.classes([r])
    print(name, k)
    assert k["one_link"] >= 1 and k["two_or_more"] >= 1 and k["miss"] >= 1 and k["diffuse_first"] >= 1, k
    recs = QC.records(rays)
    for m in LINKS:
        r = CR.chain_rays(c["osc"], mats, rays, m)
        a, nd = aovs_from_hits([(r["valid"], r["albedo"], r["normal"], r["depth"])], 1)         # chain_aovs' one sample
        ln = np.where(r["valid"], r["links"], 0).astype(np.float32)
        _same(c["sc"].query_guides(recs, m, links=True), (a, nd, ln), "%s, max_links %d, host form" % (name, m))
        _same(c["sc"].query_guides(gpu_ready.from_numpy(recs).to("cuda:0"), m, links=True), (a, nd, ln), "%s, max_links %d, device form" % (name, m))


# ---- 3. a max_t of the ray's own on the first segment --------------------------------------------------------------------------------------
def test_max_t_at_and_just_past_the_first_hit(api, gpu_ready, cases):
    """max_t = the oracle's first-hit t: the hit is not below it, the ray hits nothing: eight zeros and links 0, whatever lies behind.
    The next float after t: test 1's value (the links are not limited by it). Both alternating within a wave."""
    c = cases["cornell"]
    r6 = c["recs"][:, [0, 1, 2, 4, 5, 6]]
    oi, of, _ = c["osc"].trace_closest(r6)
    hit = oi[:, 0] == 1
    assert hit.sum() == 897
    t = of[:, 0].astype(np.float32)
    at = QC.records(r6, np.where(hit, t, QC.MAX_T).astype(np.float32))
    past = QC.records(r6, np.where(hit, np.nextafter(t, np.float32(np.inf)), QC.MAX_T).astype(np.float32))
    mixed = past.copy(); mixed[::2] = at[::2]
    cut = hit.copy(); cut[1::2] = False
    for m in LINKS:
        want = c["want"][m]
        zero = tuple(np.zeros_like(v) for v in want)
        assert not want[0][~hit].view(np.uint32).any()
        _same(c["sc"].query_guides(at, m, links=True), tuple(np.where(hit.reshape((-1,) + (1,) * (v.ndim - 1)), z, v) for v, z in zip(want, zero)),
              "max_t = t, max_links %d" % m)
        _same(c["sc"].query_guides(past, m, links=True), want, "max_t = nextafter(t), max_links %d" % m)
        got = c["sc"].query_guides(gpu_ready.from_numpy(mixed).to("cuda:0"), m, links=True)
        _same(got, tuple(np.where(cut.reshape((-1,) + (1,) * (v.ndim - 1)), z, v) for v, z in zip(want, zero)), "alternating, max_links %d" % m)


# ---- 4. a ray is its own: two cameras' rays shuffled into one call -------------------------------------------------------------------------
def test_shuffled_rays_of_two_cameras(api, gpu_ready, cases):
    a, b = cases["cornell"], cases["cornell_outside"]            # one scene, two cameras
    recs = np.concatenate([a["recs"], b["recs"]], 0)
    perm = np.random.default_rng(5).permutation(2 * RC.N)
    shuffled = np.ascontiguousarray(recs[perm])
    for m in LINKS:
        got = a["sc"].query_guides(shuffled, m, links=True)
        back = tuple(np.empty_like(g) for g in got)
        for dst, g in zip(back, got):
            dst[perm] = g
        _same(tuple(v[:RC.N] for v in back), a["want"][m], "cornell's half, max_links %d" % m)
        _same(tuple(v[RC.N:] for v in back), b["want"][m], "cornell_outside's half, max_links %d" % m)
        _same(a["sc"].query_guides(gpu_ready.from_numpy(shuffled).to("cuda:0"), m, links=True), got, "the device form, max_links %d" % m)


# ---- 5. nothing past entry n - 1 is written, in any output ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, RC.CROP])
def test_no_stray_writes(api, gpu_ready, cases, n):
    torch = gpu_ready
    c = cases["glass_mirror"]
    L = api.lib()
    recs = torch.from_numpy(c["recs"]).to("cuda:0")
    GUARD, PAD = 0x5a5a5a5a, 16
    stream = torch.cuda.current_stream().cuda_stream or None
    for m in LINKS:
        want = c["want"][m]
        for with_links in (True, False):
            ba = torch.full((n + PAD, 4), GUARD, dtype=torch.int32, device="cuda:0")
            bn = torch.full((n + PAD, 4), GUARD, dtype=torch.int32, device="cuda:0")
            bl = torch.full((n + PAD,), GUARD, dtype=torch.int32, device="cuda:0")
            assert L.pt_query_guides_device(c["sc"].h, n, recs.data_ptr(), m, ba.data_ptr(), bn.data_ptr(), bl.data_ptr() if with_links else None, 0,
                                            stream) == 0, L.pt_last_error()
            torch.cuda.synchronize()
            ga, gn, gl = ba.cpu().numpy(), bn.cpu().numpy(), bl.cpu().numpy()
            assert (ga[n:] == GUARD).all() and (gn[n:] == GUARD).all() and (gl[n if with_links else 0:] == GUARD).all()
            _same((ga[:n].view(np.float32), gn[:n].view(np.float32)), (want[0][:n], want[1][:n]), "n = %d, max_links %d" % (n, m))
            if with_links:
                assert_bits_equal(gl[:n].view(np.float32), want[2][:n], "n = %d, max_links %d: links" % (n, m))


# ---- 6. after edits ------------------------------------------------------------------------------------------------------------------------
def test_an_edited_scene_answers_as_a_fresh_one(api, gpu_ready, scene_dir):
    """ids_cases' Cornell box (glass tall box, mirror short box) with its tall box moved by update_vertices, then its white row made
    a mirror by update_materials: after each edit the scene answers as a fresh scene of the edited arrays."""
    hs = MC.cornell_host(api, scene_dir, "qguides_edit")
    leaf = hs.info["leaf_size"]
    cam0 = api.Camera.frombytes(MC.cam0_bytes(hs.camera()).tobytes())
    sc = api.Scene.from_mesh(hs)
    recs = RC.centre_records(api, cam0)

    def answers(s):
        return [s.query_guides(recs, m, links=True) for m in LINKS]

    def same(a, b, what):
        for x, y, m in zip(a, b, LINKS):
            _same(x, y, what + ", max_links %d" % m)

    before = answers(sc)
    moved = MC.moved_arrays(hs)
    sc.update_vertices(moved["points"])
    fresh = api.Scene.from_mesh(moved, max_leaf_size=leaf)
    got = answers(sc)
    same(got, answers(fresh), "after update_vertices")
    assert not np.array_equal(got[2][1].view(np.uint32), before[2][1].view(np.uint32))
    fresh.close()
    mats = moved["materials"].copy().reshape(-1, 176)
    mats[2] = mats[19]                                        # the white walls become mirrors
    mirrored = dict(moved, materials=mats.reshape(-1))
    sc.update_materials(mirrored["materials"])
    fresh = api.Scene.from_mesh(mirrored, max_leaf_size=leaf)
    got2 = answers(sc)
    same(got2, answers(fresh), "after update_materials")
    assert not np.array_equal(got2[2][0].view(np.uint32), got[2][0].view(np.uint32))
    fresh.close()
    sc.close()


# ---- 7. composition ------------------------------------------------------------------------------------------------------------------------
def test_the_queries_feed_the_variance_guided_filter_as_the_camera_passes_do(api, gpu_ready, cases):
    c = cases["cornell"]
    sc, cam0 = c["sc"], c["cam0"]
    img = lambda v: v.reshape(RC.H, RC.W, 4)
    S, Q = sc.query_radiance_moments(c["recs"], 4, 2, RC.DEPTH, seed=SEED)
    A, N = sc.query_guides(c["recs"], 4)
    got = api.denoise_var(img(S), img(Q), 4, 2, img(A), img(N))
    rS, rQ = sc.render_moments(cam0, RC.W, RC.H, 4, 2, RC.DEPTH, seed=SEED)
    rA, rN = sc.render_aovs_centre(cam0, RC.W, RC.H, 4)
    want = api.denoise_var(rS, rQ, 4, 2, rA, rN)
    assert np.isfinite(want).all() and not np.array_equal(want.view(np.uint32), rS.view(np.uint32))        # (the filter did something)
    assert_bits_equal(got, want, "denoise_var on the queries' outputs against the camera passes'")


def test_a_panorama_through_the_device_pipeline(api, gpu_ready, cases):
    """64 x 32 equirectangular rays from the middle of the Cornell box: moments -> guides -> denoise_var_device on tensors equals the
    host calls chained, is finite, and passes every ray of coverage 0 (those that leave through the open front) through unchanged."""
    torch = gpu_ready
    from cudapathtracer_amd import rays
    c = cases["cornell"]
    sc = c["sc"]
    w, h, spp, bs = 64, 32, 4, 2
    pts = np.ascontiguousarray(c["hs"].array("points")).view(np.float32).reshape(-1, 4)[:, :3]
    pano = rays.panorama_rays(tuple(0.5 * (pts.min(0) + pts.max(0))), w, h)
    S, Q = sc.query_radiance_moments(pano, spp, bs, RC.DEPTH, seed=SEED)
    A, N = sc.query_guides(pano, 4)
    want = api.denoise_var(S.reshape(h, w, 4), Q.reshape(h, w, 4), spp, spp // bs, A.reshape(h, w, 4), N.reshape(h, w, 4))
    d = torch.from_numpy(pano).to("cuda:0")
    dS, dQ = sc.query_radiance_moments(d, spp, bs, RC.DEPTH, seed=SEED)
    dA, dN = sc.query_guides(d, 4)
    ws = torch.zeros(api.denoise_var_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    out = torch.full((h, w, 4), 9.0, device="cuda:0")
    api.denoise_var_device(w, h, dS.data_ptr(), dQ.data_ptr(), spp, spp // bs, dA.data_ptr(), dN.data_ptr(), ws.data_ptr(), out.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert_bits_equal(got, want, "the device pipeline against the host calls chained")
    assert np.isfinite(got).all() and (got[..., :3] > 0).any()
    miss = A[:, 3] == 0
    assert 0 < miss.sum() < w * h
    assert_bits_equal(got.reshape(-1, 4)[miss], S[miss], "rays of coverage 0 pass through")
