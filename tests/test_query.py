"""Ray queries (pt_query_closest, pt_query_shadow, pt_query_camera_rays_device) on the GPU, bit for bit: against the CPU oracle's
trace_closest and trace_shadow on the ray sets of tests/query_cases.py (tests/test_query_cases_cpu.py keeps them honest; no ray is
left out of a comparison here), against the library's own passes and probes on a frame with more rays than resident lanes on a
scene that spills, a reordered call against the unordered one, an edited scene against a fresh one, and torch tensors against numpy."""
import os

import numpy as np
import pytest

import query_cases as QC
from util import assert_bits_equal, random_rays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(api, oracle, gpu_ready, scene_dir):
    """Per scene: the GPU scene, the oracle's closest hits at MAX_T and shadow throughputs at shadow_max_t, computed once."""
    out = {}
    for name in QC.SCENES:
        hs = QC.host(api, scene_dir, name)
        a = QC.arrays(hs)
        osc = oracle.OracleScene(arrays=a)
        rays = QC.ray_set(oracle, QC.camera(api, hs, name), a, name)
        oi, of, _ = osc.trace_closest(rays)
        max_t = QC.shadow_max_t(oi, of)
        thr, _ = osc.trace_shadow(rays, max_t)
        out[name] = {"hs": hs, "sc": api.Scene(hs), "rays": rays, "oi": oi, "of": of, "shadow_max_t": max_t, "thr": thr,
                     "lights": QC.lights_of_triangles(a)}
    yield out
    for c in out.values():
        c["sc"].close()


@pytest.fixture(scope="module")
def blob(api, gpu_ready, scene_dir):
    """The blob of tests/test_aov_centre.py's second-tile test: 5 132 triangles, in HBM, with a spill area, at its 1021 x h frame."""
    from cudapathtracer_amd import scenes
    num_cu = gpu_ready.cuda.get_device_properties(0).multi_processor_count
    w = 1021
    h = (num_cu * 8 * 4 // 128 + 1) * 8 + 3
    hs = api.HostScene(scenes.blob_in_box(os.path.join(scene_dir, "query_blob"), w, h, 2, 5, subdiv=4, name="query_blob")["config"])
    assert hs.info["n_tris"] == 20 * 4 ** 4 + 12
    sc = api.Scene.from_mesh(hs)
    assert not sc.flags()["onchip"]
    yield {"hs": hs, "sc": sc, "w": w, "h": h, "num_cu": num_cu}
    sc.close()


def _want_hits(oi, of, found=None):
    """The RAY_HIT_DTYPE records of the oracle's hits where `found` (default: where the oracle hit), a miss elsewhere."""
    from cudapathtracer_amd import api
    found = (oi[:, 0] == 1) if found is None else found
    want = np.zeros(len(oi), api.RAY_HIT_DTYPE)
    want["t"], want["u"], want["v"] = (np.where(found, of[:, k], np.float32(0.0)).astype(np.float32) for k in range(3))
    want["tri"] = np.where(found, oi[:, 1], -1)
    return want


def _want_surfaces(oi, of, lights, found=None):
    from cudapathtracer_amd import api
    found = (oi[:, 0] == 1) if found is None else found
    want = np.zeros(len(oi), api.RAY_SURFACE_DTYPE)
    for k, f in enumerate(("px", "py", "pz", "nx", "ny", "nz", "uvx", "uvy")):
        want[f] = np.where(found, of[:, 3 + k], np.float32(0.0))
    want["material"] = np.where(found, oi[:, 2], -1)
    want["light"] = np.where(found, lights[np.maximum(oi[:, 1], 0)], -1)
    want["backface"] = np.where(found, (oi[:, 3] != 0).astype(np.int32), 0)
    return want


def _same_records(got, want, what):
    """Structured records equal in every byte (so -0 differs from +0), reported per field."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    for f in got.dtype.names:
        g, x = np.ascontiguousarray(got[f]).view(np.uint32), np.ascontiguousarray(want[f]).view(np.uint32)
        bad = np.flatnonzero(g != x)
        assert bad.size == 0, "%s: field %s differs in %d of %d rays, first %d: %r vs %r" % (what, f, bad.size, len(g), bad[0], got[f][bad[0]], want[f][bad[0]])


def _numpy_hits(api, t):
    return t.cpu().numpy().view(api.RAY_HIT_DTYPE).reshape(-1)


def _numpy_surfaces(api, t):
    return t.cpu().numpy().view(api.RAY_SURFACE_DTYPE).reshape(-1)


# ---- 1. closest against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QC.SCENES)
def test_closest_is_the_oracles_in_both_forms(api, gpu_ready, cases, name):
    c = cases[name]
    recs = QC.records(c["rays"])
    want_h, want_s = _want_hits(c["oi"], c["of"]), _want_surfaces(c["oi"], c["of"], c["lights"])
    assert (want_s["light"] >= 0).any() and (want_s["backface"] == 1).any() and (want_h["tri"] < 0).any()
    hits, surf = c["sc"].query_closest(recs, surfaces=True)
    _same_records(hits, want_h, name + ", host form: hits"); _same_records(surf, want_s, name + ", host form: surfaces")
    _same_records(c["sc"].query_closest(recs), want_h, name + ", host form, hits only")
    d = gpu_ready.from_numpy(recs).to("cuda:0")
    th, ts = c["sc"].query_closest(d, surfaces=True)
    assert th.is_cuda and ts.is_cuda and th.shape == (QC.N, 4) and ts.shape == (QC.N, 12)
    _same_records(_numpy_hits(api, th), want_h, name + ", device form: hits"); _same_records(_numpy_surfaces(api, ts), want_s, name + ", device form: surfaces")
    _same_records(_numpy_hits(api, c["sc"].query_closest(d)), want_h, name + ", device form, hits only")


# ---- 2. a max_t of each ray's own ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QC.SCENES)
def test_max_t_at_and_just_past_the_hit(api, gpu_ready, cases, name):
    """max_t = the oracle's t exactly: the hit is not below it, and nothing else is (t is the smallest): a miss. The next float after
    t: the hit. Rays the oracle misses keep MAX_T and miss. (MAX_T itself is test 1.)"""
    c = cases[name]
    hit = c["oi"][:, 0] == 1
    t = c["of"][:, 0].astype(np.float32)
    none = np.zeros(QC.N, bool)
    at = QC.records(c["rays"], np.where(hit, t, QC.MAX_T).astype(np.float32))
    hits, surf = c["sc"].query_closest(at, surfaces=True)
    _same_records(hits, _want_hits(c["oi"], c["of"], none), name + ": max_t = t"); _same_records(surf, _want_surfaces(c["oi"], c["of"], c["lights"], none), name + ": max_t = t")
    past = QC.records(c["rays"], np.where(hit, np.nextafter(t, np.float32(np.inf)), QC.MAX_T).astype(np.float32))
    th, ts = c["sc"].query_closest(gpu_ready.from_numpy(past).to("cuda:0"), surfaces=True)
    _same_records(_numpy_hits(api, th), _want_hits(c["oi"], c["of"]), name + ": max_t = nextafter(t)")
    _same_records(_numpy_surfaces(api, ts), _want_surfaces(c["oi"], c["of"], c["lights"]), name + ": max_t = nextafter(t)")
    # every second ray at t, the others past it: the lanes of one wave differ
    mixed = past.copy(); mixed[::2] = at[::2]
    found = hit.copy(); found[::2] = False
    _same_records(c["sc"].query_closest(mixed), _want_hits(c["oi"], c["of"], found), name + ": max_t alternating")


# ---- 3. shadow against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QC.SCENES)
def test_shadow_is_the_oracles_in_both_forms(api, gpu_ready, cases, name):
    c = cases[name]
    recs = QC.records(c["rays"], c["shadow_max_t"])
    want = np.concatenate([c["thr"], np.zeros((QC.N, 1), np.float32)], 1)
    if name == "textured":
        assert ((c["thr"] > 0) & (c["thr"] < 1)).all(1).sum() >= 5
    assert_bits_equal(c["sc"].query_shadow(recs), want, name + ", host form: throughput")
    got = c["sc"].query_shadow(gpu_ready.from_numpy(recs).to("cuda:0"))
    assert got.is_cuda and got.shape == (QC.N, 4)
    assert_bits_equal(got.cpu().numpy(), want, name + ", device form: throughput")
    # ... and pt_probe_trace_shadow's three floats
    probe, _ = c["sc"].trace_shadow(c["rays"], c["shadow_max_t"])
    assert_bits_equal(got.cpu().numpy()[:, :3], probe, name + ": the probe")


# ---- 4. nothing past entry n - 1 is written ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 997])
def test_no_stray_writes(api, gpu_ready, cases, n):
    torch = gpu_ready
    c = cases["textured"]
    sc, L = c["sc"], api.lib()
    recs = torch.from_numpy(QC.records(c["rays"], c["shadow_max_t"])).to("cuda:0")
    full_h, full_s = sc.query_closest(recs, surfaces=True)
    full_t = sc.query_shadow(recs)
    GUARD, PAD = 0x5a5a5a5a, 16
    stream = torch.cuda.current_stream().cuda_stream or None
    for flags in (0, api.QUERY_REORDER):
        # one allocation: hits, then surfaces, then throughput, each with PAD guard records behind its n entries
        buf = torch.full(((n + PAD) * (4 + 12 + 4),), GUARD, dtype=torch.int32, device="cuda:0")
        h, s, t = buf[:(n + PAD) * 4].view(-1, 4), buf[(n + PAD) * 4:(n + PAD) * 16].view(-1, 12), buf[(n + PAD) * 16:].view(-1, 4)
        assert L.pt_query_closest_device(sc.h, n, recs.data_ptr(), h.data_ptr(), None, flags, stream) == 0, L.pt_last_error()
        torch.cuda.synchronize()
        assert torch.equal(h[:n], full_h[:n].view(torch.int32)) and bool((h[n:] == GUARD).all())
        assert bool((s == GUARD).all()) and bool((t == GUARD).all())          # surfaces NULL: nothing of a surface buffer is touched
        h.fill_(GUARD)
        assert L.pt_query_closest_device(sc.h, n, recs.data_ptr(), h.data_ptr(), s.data_ptr(), flags, stream) == 0, L.pt_last_error()
        torch.cuda.synchronize()
        assert torch.equal(h[:n], full_h[:n].view(torch.int32)) and bool((h[n:] == GUARD).all())
        assert torch.equal(s[:n], full_s[:n].view(torch.int32)) and bool((s[n:] == GUARD).all()) and bool((t == GUARD).all())
        assert L.pt_query_shadow_device(sc.h, n, recs.data_ptr(), t.data_ptr(), flags, stream) == 0, L.pt_last_error()
        torch.cuda.synchronize()
        assert torch.equal(t[:n], full_t[:n].view(torch.int32)) and bool((t[n:] == GUARD).all())
        assert bool((h[n:] == GUARD).all()) and bool((s[n:] == GUARD).all())


# ---- 5. camera rays ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(40, 24), (13, 11), (1, 1)])
def test_camera_rays_are_the_centre_rays(api, gpu_ready, w, h):
    cam = api.make_camera(True, (0.3, -0.2, 2.9), (4.0, -11.0, 2.0), 52.0, w, h)
    want = api.probe_centre_rays(cam, np.array([(x, y) for y in range(h) for x in range(w)], np.int32))
    for max_t in (QC.MAX_T, np.float32(2.5)):
        out = gpu_ready.full((w * h + 4, 8), 7.0, device="cuda:0")
        got = api.query_camera_rays(cam, w, h, float(max_t), out=out).cpu().numpy()
        assert_bits_equal(got[:w * h, 0:3], want[:, 0:3], "origins"); assert_bits_equal(got[:w * h, 4:7], want[:, 3:6], "directions")
        assert (got[:w * h, 3] == max_t).all() and not got[:w * h, 7].view(np.uint32).any() and (got[w * h:] == 7.0).all()
    fresh = api.Scene.query_camera_rays(None, cam, w, h)                # a tensor of its own, max_t = MAX_T
    assert fresh.is_cuda and fresh.shape == (w * h, 8)
    fresh = fresh.cpu().numpy()
    assert_bits_equal(fresh[:, [0, 1, 2, 4, 5, 6]], want, "a fresh tensor"); assert (fresh[:, 3] == QC.MAX_T).all() and not fresh[:, 7].any()


# ---- 6. more rays than resident lanes, on a scene that spills ---------------------------------------------------------------------------
def test_a_waves_second_tile_on_a_scene_that_spills(api, gpu_ready, blob):
    sc, w, h = blob["sc"], blob["w"], blob["h"]
    cam = blob["hs"].camera()
    n = w * h
    assert (n + 63) // 64 > blob["num_cu"] * 8 * 4           # more tiles than the widest launch has waves
    rays = sc.query_camera_rays(cam, w, h)
    hits = _numpy_hits(api, sc.query_closest(rays))
    ids = sc.render_ids(cam, w, h).reshape(n, 4)
    depth = sc.render_aovs_centre(cam, w, h)[1].reshape(n, 4)[:, 3]
    assert np.array_equal(hits["tri"], ids[:, 0])
    assert_bits_equal(hits["t"], depth, "t against the centre pass's depth")
    assert (hits["tri"][-1024:] >= 0).any() and (hits["tri"] < 0).any()
    # the first and the last 1 024 rays against the probe, surfaces included
    th, ts = sc.query_closest(rays, surfaces=True)
    surf = _numpy_surfaces(api, ts)
    _same_records(_numpy_hits(api, th), hits, "hits with and without surfaces")
    r6 = rays.cpu().numpy()[:, [0, 1, 2, 4, 5, 6]]
    for sl in (slice(0, 1024), slice(n - 1024, n)):
        gi, gf, _ = sc.trace_closest(r6[sl])
        _same_records(hits[sl], _want_hits(gi, gf), "the probe: hits")
        want = _want_surfaces(gi, gf, np.full(blob["hs"].info["n_tris"], -1, np.int32))
        want["light"] = surf["light"][sl]                   # (the probe reports no light word: the ID pass is its reference)
        _same_records(surf[sl], want, "the probe: surfaces")
    assert np.array_equal(surf["light"], ids[:, 2]) and np.array_equal(surf["material"], ids[:, 1]) and np.array_equal(surf["backface"], ids[:, 3] & 1)


# ---- 7. reorder -------------------------------------------------------------------------------------------------------------------------
def _reorder_equals_unordered(api, torch, sc, recs, what):
    d = torch.from_numpy(np.ascontiguousarray(recs, np.float32)).to("cuda:0")
    h0, s0 = sc.query_closest(d, surfaces=True)
    h1, s1 = sc.query_closest(d, surfaces=True, reorder=True)
    assert torch.equal(h0.view(torch.int32), h1.view(torch.int32)) and torch.equal(s0.view(torch.int32), s1.view(torch.int32)), what + ": closest with surfaces"
    assert torch.equal(h0.view(torch.int32), sc.query_closest(d, reorder=True).view(torch.int32)), what + ": closest, hits only"
    assert torch.equal(sc.query_shadow(d).view(torch.int32), sc.query_shadow(d, reorder=True).view(torch.int32)), what + ": shadow"
    # ... and the host form takes the flag too
    _same_records(sc.query_closest(recs, reorder=True), _numpy_hits(api, h0), what + ": host form")
    return h0


def test_reorder_changes_no_bit(api, gpu_ready, cases, blob):
    c = cases["cornell"]
    recs = QC.records(c["rays"], c["shadow_max_t"])
    h = _reorder_equals_unordered(api, gpu_ready, c["sc"], recs, "cornell")
    assert bool((h.view(gpu_ready.int32)[:, 3] >= 0).any())
    for n in (1, 64, 65):
        _reorder_equals_unordered(api, gpu_ready, c["sc"], recs[300:300 + n], "cornell, n = %d" % n)
    _reorder_equals_unordered(api, gpu_ready, c["sc"], np.tile(recs[260], (300, 1)), "300 identical rays")
    # origins outside the bounds, huge, and not finite: the keys clamp, or are 0
    odd = recs[250:450].copy()
    odd[0::5, 0] = 1e30; odd[1::5, 1] = -np.inf; odd[2::5, 2] = np.nan; odd[3::5, 0:3] *= 40.0
    _reorder_equals_unordered(api, gpu_ready, c["sc"], odd, "origins outside, huge and not finite")
    # the blob: incoherent rays in its box, more than one workgroup of them, some max_t short
    rays = random_rays(np.random.default_rng(11), 4099)
    max_t = np.where(np.arange(4099) % 3 == 0, np.float32(0.7), QC.MAX_T).astype(np.float32)
    h = _reorder_equals_unordered(api, gpu_ready, blob["sc"], QC.records(rays, max_t), "blob")
    tri = h.view(gpu_ready.int32)[:, 3]
    assert bool((tri >= 12).any()) and bool((tri < 0).any())         # the blob itself, and misses


# ---- 8. after edits ---------------------------------------------------------------------------------------------------------------------
def test_an_edited_scene_answers_as_a_fresh_one(api, gpu_ready, cases, scene_dir):
    c = cases["textured"]
    hs = c["hs"]
    leaf = hs.info["leaf_size"]
    recs = QC.records(c["rays"], c["shadow_max_t"])
    recs_far = QC.records(c["rays"])
    sc = api.Scene.from_mesh(hs)

    def answers(s):
        return s.query_closest(recs_far, surfaces=True) + (s.query_shadow(recs), s.query_shadow(recs, reorder=True))

    def same(a, b, what):
        _same_records(a[0], b[0], what + ": hits"); _same_records(a[1], b[1], what + ": surfaces")
        assert_bits_equal(a[2], b[2], what + ": shadow"); assert_bits_equal(a[3], b[3], what + ": shadow, reordered")

    before = answers(sc)
    a = QC.arrays(hs)
    geometry = {k: a[k] for k in a if k not in ("bvh", "indices")}
    moved = dict(geometry, points=a["points"].copy())
    moved["points"].view(np.float32).reshape(-1, 4)[-8:, :3] += np.array((0.2, -0.25, 0.1), np.float32)      # the two canopy quads
    sc.update_vertices(moved["points"])
    fresh = api.Scene.from_mesh(moved, max_leaf_size=leaf)
    got = answers(sc)
    same(got, answers(fresh), "after update_vertices")
    assert not np.array_equal(got[0]["t"].view(np.uint32), before[0]["t"].view(np.uint32))
    fresh.close()
    # the leaf rows 13 and 16 become row 2's diffuse white: the canopy now blocks what it attenuated
    mats = a["materials"].copy().reshape(-1, 176)
    mats[13] = mats[2]; mats[16] = mats[2]
    edited = dict(moved, materials=mats.reshape(-1))
    sc.update_materials(edited["materials"])
    fresh = api.Scene.from_mesh(edited, max_leaf_size=leaf)
    got2 = answers(sc)
    same(got2, answers(fresh), "after update_materials")
    frac = lambda t: int(((t[:, :3] > 0) & (t[:, :3] < 1)).all(1).sum())
    assert frac(before[2]) >= 1 and frac(got2[2]) == 0
    fresh.close(); sc.close()


# ---- 9. torch tensors in, torch tensors out ---------------------------------------------------------------------------------------------
def test_torch_input_on_a_stream_of_its_own(api, gpu_ready, cases):
    torch = gpu_ready
    c = cases["glass_mirror"]
    recs = QC.records(c["rays"], c["shadow_max_t"])
    hits, surf = c["sc"].query_closest(recs, surfaces=True)
    thr = c["sc"].query_shadow(recs)
    assert isinstance(hits, np.ndarray) and isinstance(surf, np.ndarray) and isinstance(thr, np.ndarray)
    d = torch.from_numpy(recs).to("cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        th, ts = c["sc"].query_closest(d, surfaces=True, reorder=True)
        tt = c["sc"].query_shadow(d)
    side.synchronize()
    for t in (th, ts, tt):
        assert isinstance(t, torch.Tensor) and t.device == d.device and t.dtype == torch.float32
    _same_records(_numpy_hits(api, th), hits, "hits"); _same_records(_numpy_surfaces(api, ts), surf, "surfaces")
    assert_bits_equal(tt.cpu().numpy(), thr, "throughput")
    with pytest.raises(api.PtError, match="contiguous"):
        c["sc"].query_closest(d[:, :6])
    with pytest.raises(api.PtError, match="contiguous"):
        c["sc"].query_shadow(d.cpu())
    empty = c["sc"].query_closest(d[:0])
    assert empty.shape == (0, 4) and empty.is_cuda
