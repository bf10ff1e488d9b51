"""Probe-grid lookups on the device (pt_grid_pack, pt_grid_irradiance), bit for bit against tests/grid_ref.py's f32
restatement of the header's arithmetic: seeded grids of every shape of cell (one probe, a row, a slab, a volume), every map size, with
and without maps, at record counts around a wave, on points chosen for the lookup's edges."""
import os

import numpy as np
import pytest

import grid_ref as GR
import motion_cases as MC
import radiance_cases as RC
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

F = np.float32
SH_SAMPLES = 80
JUNK = np.array([0x7fc12345], np.uint32).view(F)[0]               # a NaN with a payload, for the words the lookup does not read


def _grid(counts, res, map_samples, seed, flat=None):
    """A seeded grid whose lo corner has a zero and a negative coordinate: (lo, hi, sums [n, 9, 4], maps [n, R, R, 4] or None)."""
    rng = np.random.default_rng(seed)
    n = counts[0] * counts[1] * counts[2]
    lo, hi = (0.0, -1.5, 0.25), (2.0, 0.75, 1.75)
    sums = np.zeros((n, 9, 4), F)
    sums[:, 0, :3] = rng.uniform(3.0, 9.0, (n, 3))
    sums[:, 1:, :3] = rng.uniform(-2.0, 2.0, (n, 8, 3))
    sums[..., 3] = rng.uniform(-1.0, 1.0, (n, 9))                  # the fourth word of a sum is not read
    maps = None
    if res:
        maps = np.zeros((n, res, res, 4), F)
        mean = np.full((n, res, res), flat) if flat is not None else rng.uniform(0.3, 2.5, (n, res, res))
        var = 0.0 if flat is not None else rng.uniform(0.0, 0.4, (n, res, res))
        maps[..., 0], maps[..., 1] = mean * map_samples, (mean * mean + var) * map_samples
        maps[..., 2:] = rng.uniform(0.0, map_samples, (n, res, res, 2))
    return lo, hi, sums, maps


def _probe_at(lo, hi, counts, i):
    return np.array([lo[a] + (hi[a] - lo[a]) / (counts[a] - 1) * i[a] if counts[a] > 1 else lo[a] for a in range(3)], np.float64)


def _records(lo, hi, counts, m, seed):
    """m records: the edge cases first (as many as fit), seeded points in and around the grid after them."""
    from cudapathtracer_amd import rays
    rng = np.random.default_rng(seed)
    lo64, hi64 = np.array(lo), np.array(hi)
    cell = np.array([(hi[a] - lo[a]) / (counts[a] - 1) if counts[a] > 1 else 1.0 for a in range(3)])
    last = tuple(c - 1 for c in counts)
    p0, p1 = _probe_at(lo, hi, counts, (0, 0, 0)), _probe_at(lo, hi, counts, last)
    eps = 1e-4
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),                         # the axes
            (0.6, 0.8, 0.0), (-0.6, 0.8, -0.0), (0.8, -0.6, 0.0), (-1, -1, 0.0),                        # the fold z == 0
            (eps, eps, -1), (-eps, eps, -1), (eps, -eps, -1), (-eps, -eps, -1),                         # the square's corners: every gutter corner
            (-1, 0.02, eps), (-1, -0.02, -eps), (1, 0.02, eps), (1, -0.02, -eps),                       # the gutter's columns
            (0.02, -1, eps), (-0.02, -1, -eps), (0.02, 1, eps), (-0.02, 1, -eps)]                       # and rows
    pts = [p0, p1, 0.5 * (p0 + p1)]                                                                     # on a probe (dist == 0), mid-grid
    pts += [p0 + 0.37 * np.array(d, np.float64) for d in dirs]
    pts += [p1 + 0.21 * np.array(d, np.float64) for d in dirs[:10]]
    pts.append(np.array([-0.0, p0[1] + 0.5, p0[2]]))                                                    # signed zeros: v = (-0, 0.5, +0) from the probe at x = 0
    pts.append(np.array([-0.0, p0[1], p0[2] - 0.5]))
    for a in range(3):
        e = np.eye(3)[a]
        pts += [lo64 + 0.5 * cell * (1 - e), lo64 - 0.3 * cell * e, hi64 + 0.3 * cell * e, lo64 - 1e6 * cell * e, hi64 + 1e6 * cell * e]      # a cell face, outside every face, far away
    pts += [lo64.copy(), hi64.copy(), lo64 - 1e6 * cell, hi64 + 1e6 * cell]
    pts = np.array(pts)[:m]
    more = rng.uniform(lo64 - cell, hi64 + cell, (m - len(pts), 3))
    p = np.concatenate([pts, more], 0).astype(F)
    nrm = rng.standard_normal((m, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F)
    nrm[::7] = np.eye(3, dtype=F)[np.arange(len(nrm[::7])) % 3] * F(-1.0)                               # axis normals, with negative zeros beside them
    rec = rays.irradiance_records(p, nrm)
    rec[:, 3] = rng.uniform(-5.0, 5.0, m)
    rec[::2, 3] = JUNK
    rec[:, 7] = JUNK
    return rec


def _pack_ref(sums, maps, map_samples):
    return GR.pack(SH_SAMPLES, sums, maps, map_samples)


def _desc(api, lo, hi, counts, res, map_samples, power):
    return api.grid_desc(lo, hi, counts, SH_SAMPLES, res, map_samples, power)


# (counts, res, power, map_samples): every shape of cell with and without maps, every R (32 with one cell), powers 1, 3, 8, samples 1 and 16
GRIDS = [((1, 1, 1), 0, 3, 1), ((1, 1, 1), 8, 3, 16), ((2, 1, 1), 0, 1, 1), ((2, 1, 1), 4, 1, 1), ((1, 3, 2), 0, 3, 1), ((1, 3, 2), 16, 8, 16),
         ((3, 3, 3), 0, 3, 1), ((3, 3, 3), 4, 3, 16), ((3, 3, 3), 8, 1, 1), ((3, 3, 3), 16, 3, 1), ((3, 3, 3), 8, 8, 16), ((2, 2, 2), 32, 3, 1)]


@pytest.mark.parametrize("counts,res,power,map_samples", GRIDS)
def test_the_lookup_is_the_restatement_bit_for_bit(api, gpu_ready, counts, res, power, map_samples):
    from cudapathtracer_amd import rays
    lo, hi, sums, maps = _grid(counts, res, map_samples, 7)
    d = _desc(api, lo, hi, counts, res, map_samples, power)
    packed = api.grid_pack(d, sums, maps)
    coeff, tex = _pack_ref(sums, maps, map_samples)
    assert_bits_equal(packed, GR.packed_words(coeff, tex), "the packed buffer")
    seen_gutter = set()
    for m in (1, 63, 64, 65, 130):
        rec = _records(lo, hi, counts, m, 100 + m)
        want, _ = GR.lookup(lo, hi, counts, coeff, tex, power, rec)
        got = api.grid_irradiance(packed, d, rec)
        assert got.shape == (m, 4) and got.dtype == F
        assert_bits_equal(got, want, "counts %s, res %d, power %d, m %d" % (counts, res, power, m))
        assert np.isfinite(got[:min(m, 60)]).all()
        if res and m == 130:
            # the edge cases are in the data: dist == 0, both sides of the fold, and every gutter column, row and corner
            p0 = _probe_at(lo, hi, counts, (0, 0, 0)).astype(F)
            v = rec[:, 0:3] - p0[None, :]
            assert (np.abs(v).sum(1) == 0).any() and (v[:, 2] == 0).sum() >= 4 and np.signbit(v[:, 0][v[:, 0] == 0]).any()
            uv = rays.oct_encode(np.where((np.abs(v).sum(1) > 0)[:, None], v, F(1)))
            gx, gy = np.floor(uv[:, 0] * F(res) + F(0.5)), np.floor(uv[:, 1] * F(res) + F(0.5))
            inner = lambda g: (g >= 1) & (g <= res - 1)
            for ex, ey in ((0, None), (res, None), (None, 0), (None, res), (0, 0), (0, res), (res, 0), (res, res)):
                if ((inner(gx) if ex is None else gx == ex) & (inner(gy) if ey is None else gy == ey)).any():
                    seen_gutter.add((ex, ey))
            assert len(seen_gutter) == 8, seen_gutter
    if not res:
        assert np.abs(got[:, 3] - 1.0).max() <= 4 * 2.0 ** -23                      # without maps W is the trilinear weights' sum


def test_bad_records_give_exact_zeros_and_junk_words_are_not_read(api, gpu_ready):
    counts, res = (3, 3, 3), 8
    lo, hi, sums, maps = _grid(counts, res, 4, 9)
    for r, mp in ((res, maps), (0, None)):
        d = _desc(api, lo, hi, counts, r, 4, 3)
        packed = api.grid_pack(d, sums, mp)
        rec = _records(lo, hi, counts, 130, 5)
        clean = api.grid_irradiance(packed, d, rec)
        other = rec.copy()
        other[:, 3], other[:, 7] = 3.0, 0.0
        assert_bits_equal(api.grid_irradiance(packed, d, other), clean, "max_t and pad are not read")
        bad = rec.copy()
        where = {3: (0, np.nan), 64: (1, np.inf), 65: (2, -np.inf), 66: (4, np.nan), 100: (5, np.inf), 129: (6, -np.inf)}
        for i, (col, v) in where.items():
            bad[i, col] = v
        got = api.grid_irradiance(packed, d, bad)
        idx = sorted(where)
        assert not got[idx].view(np.uint32).any()
        keep = np.setdiff1d(np.arange(130), idx)
        assert_bits_equal(got[keep], clean[keep], "the neighbours of a bad record")
        assert clean[idx].any(1).all()


def test_blind_probes_take_the_fallback_and_flat_maps_are_a_step(api, gpu_ready):
    """Flat maps whose every texel ends at 0.4, with no variance but what the f32 mean square leaves (var = m2 - mean * mean is some
    1e-9 or clamps to 0): a point further than that from all eight probes is seen by none, its weights vanish and the plain trilinear
    mix answers; a point on a probe has that probe's light alone."""
    counts, res, ms = (3, 3, 3), 4, 16
    lo, hi, sums, maps = _grid(counts, res, ms, 3, flat=0.4)
    d = _desc(api, lo, hi, counts, res, ms, 3)
    d0 = _desc(api, lo, hi, counts, 0, ms, 3)
    packed, plain_packed = api.grid_pack(d, sums, maps), api.grid_pack(d0, sums)
    rec = _records(lo, hi, counts, 130, 21)
    coeff, tex = _pack_ref(sums, maps, ms)
    want, fallback = GR.lookup(lo, hi, counts, coeff, tex, 3, rec)
    got = api.grid_irradiance(packed, d, rec)
    assert_bits_equal(got, want, "flat maps")
    assert fallback.sum() >= 20 and (~fallback).sum() >= 10
    plain = api.grid_irradiance(plain_packed, d0, rec)
    assert_bits_equal(got[fallback, :3], plain[fallback, :3], "the fallback arm is the plain mix")
    assert (got[fallback, 3] < 1e-12).all()                                         # blind: ratio^3 of a variance of 1e-9 at the most
    near = np.abs(rec[:, 0:3] - _probe_at(lo, hi, counts, (0, 0, 0)).astype(F)).max(1) == 0
    assert near.any() and not fallback[near].any() and (got[near, 3] == 1).all()    # on the probe: it alone, at full weight


def test_the_pack_writes_its_buffer_and_nothing_else(api, gpu_ready):
    """The packed arrays against rays._sh_convolved and rays.oct_border in f32, device and host form, into pre-filled buffers with
    guard words behind them."""
    torch = gpu_ready
    from cudapathtracer_amd import rays
    L = api.lib()
    GUARD, TAIL = 0x5a5a5a5a, 16
    stream = torch.cuda.current_stream().cuda_stream or None
    for counts, res, ms in (((2, 1, 1), 4, 1), ((3, 3, 3), 8, 16), ((1, 3, 2), 16, 3), ((2, 2, 2), 32, 1), ((3, 3, 3), 0, 1)):
        lo, hi, sums, maps = _grid(counts, res, ms, 13)
        n = len(sums)
        d = _desc(api, lo, hi, counts, res, ms, 3)
        words = api.grid_packed_bytes(d) // 4
        assert words == GR.packed_bytes(counts, res) // 4
        e = rays._sh_convolved(sums, SH_SAMPLES)
        assert e.dtype == F
        want = np.zeros((n, 9, 4), F)
        want[..., :3] = e
        want = [want.ravel()]
        if res:
            b = (rays.oct_border(maps[..., :2]) / F(ms)).astype(F)
            assert b.shape == (n, res + 2, res + 2, 2)
            want.append(b.ravel())
        want = np.concatenate(want)
        ds, dm = torch.from_numpy(sums).to("cuda:0"), torch.from_numpy(maps).to("cuda:0") if res else None
        buf = torch.full((words + TAIL,), GUARD, dtype=torch.int32, device="cuda:0")
        assert L.pt_grid_pack_device(d, ds.data_ptr(), dm.data_ptr() if res else None, buf.data_ptr(), stream) == 0, L.pt_last_error()
        torch.cuda.synchronize()
        g = buf.cpu().numpy()
        assert (g[words:] == GUARD).all(), (counts, res)
        assert_bits_equal(g[:words].view(F), want, "device pack %s res %d" % (counts, res))
        host = np.full(words + TAIL, GUARD, np.uint32)
        assert L.pt_grid_pack(d, sums.ctypes.data, maps.ctypes.data if res else None, host.ctypes.data) == 0, L.pt_last_error()
        assert (host[words:] == GUARD).all()
        assert_bits_equal(host[:words].view(F), want, "host pack %s res %d" % (counts, res))
        t = api.grid_pack(d, ds, dm)
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.shape == (words,)
        assert_bits_equal(t.cpu().numpy(), want, "torch in, torch out")


def test_the_device_form_is_the_host_form_on_a_stream_of_its_own(api, gpu_ready):
    torch = gpu_ready
    L = api.lib()
    GUARD, TAIL = 0x5a5a5a5a, 16
    for counts, res in (((3, 3, 3), 8), ((1, 3, 2), 0)):
        lo, hi, sums, maps = _grid(counts, res, 2, 17)
        d = _desc(api, lo, hi, counts, res, 2, 3)
        packed = api.grid_pack(d, sums, maps)
        rec = _records(lo, hi, counts, 130, 31)
        host = api.grid_irradiance(packed, d, rec)
        dp, dr = torch.from_numpy(packed).to("cuda:0"), torch.from_numpy(rec).to("cuda:0")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            t = api.grid_irradiance(dp, d, dr)
        side.synchronize()
        assert isinstance(t, torch.Tensor) and t.device == dr.device and t.shape == (130, 4)
        assert_bits_equal(t.cpu().numpy(), host, "torch in, torch out")
        for m in (1, 65):
            buf = torch.full((m + TAIL, 4), GUARD, dtype=torch.int32, device="cuda:0")
            assert L.pt_grid_irradiance_device(d, dp.data_ptr(), m, dr.data_ptr(), buf.data_ptr(), side.cuda_stream) == 0, L.pt_last_error()
            side.synchronize()
            g = buf.cpu().numpy()
            assert (g[m:] == GUARD).all()
            assert_bits_equal(g[:m].view(F), host[:m], "m = %d into a pre-filled buffer" % m)
        out = np.full((130 + TAIL, 4), GUARD, np.uint32)
        assert L.pt_grid_irradiance(d, packed.ctypes.data, 130, rec.ctypes.data, out.ctypes.data) == 0, L.pt_last_error()
        assert (out[130:] == GUARD).all()
        assert api.grid_irradiance(dp, d, dr[:0]).shape == (0, 4)
        # a record's output depends on the record alone: the records permuted give the outputs permuted
        perm = np.random.default_rng(1).permutation(130)
        assert_bits_equal(api.grid_irradiance(packed, d, np.ascontiguousarray(rec[perm])), host[perm], "permuted records")


def test_a_baked_probe_grid_shades_surfaces_and_moves_nothing_else(api, gpu_ready, scene_dir):
    """End to end on the Cornell box: a 2 x 2 x 2 ProbeGrid at 64 lanes x 1 sample and R = 4, ProbeGrid.shade of 130 of
    query_closest's surfaces against the restatement over the same query outputs; the scene's counters, a later render and a later
    query_distance are what they were."""
    torch = gpu_ready
    from cudapathtracer_amd import rays, scenes
    hs = api.HostScene(scenes.cornell(os.path.join(scene_dir, "grid_plain"), width=RC.W, height=RC.H, name="grid_plain", spp=4, max_depth=4)["config"])
    sc = api.Scene.from_mesh(hs)
    cam0 = api.Camera.frombytes(MC.cam0_bytes(hs.camera()).tobytes())
    pts = np.ascontiguousarray(hs.array("points")).view(np.float32).reshape(-1, 4)[:, :3]
    lo, hi = pts.min(0), pts.max(0)
    glo, ghi = lo + 0.2 * (hi - lo), hi - 0.2 * (hi - lo)
    img0, _ = sc.render(cam0, RC.W, RC.H, 2, 4)
    probe = rays.sh_grid(glo, ghi, (2, 2, 2), 1.0)
    dist0 = sc.query_distance(probe, 4, 2)
    sc.render(cam0, RC.W, RC.H, 1, 3, counters=True)
    cnt0 = sc.counters()
    surf = sc.query_closest(sc.query_camera_rays(cam0, RC.W, RC.H).cpu().numpy(), surfaces=True)[1]
    pick = np.linspace(0, len(surf) - 1, 130).astype(np.int64)
    surf = np.ascontiguousarray(surf[pick])
    assert (surf["material"] >= 0).sum() >= 100
    grid = api.ProbeGrid(sc, glo, ghi, (2, 2, 2), res=4).bake(64, 1, 4, map_spp=1)
    got = grid.shade(surf)
    assert got.shape == (130, 4)
    assert_bits_equal(grid.sums, sc.query_sh(rays.sh_grid(glo, ghi, (2, 2, 2)), 64, 1, 4), "the bake's SH sums")
    assert_bits_equal(grid.maps, sc.query_distance(rays.sh_grid(glo, ghi, (2, 2, 2), grid.max_t), 4, 1), "the bake's maps")
    assert grid.max_t == pytest.approx(1.5 * float(np.linalg.norm((ghi - glo).astype(np.float64))))
    coeff, tex = GR.pack(64, grid.sums, grid.maps, 1)
    lo32, hi32 = [float(F(v)) for v in glo], [float(F(v)) for v in ghi]
    want, _ = GR.lookup(lo32, hi32, (2, 2, 2), coeff, tex, 3, rays.records_from_surfaces(surf))
    assert_bits_equal(got, want, "ProbeGrid.shade against the restatement")
    assert got[:, :3].max() > 0
    hit, words = surf["material"] >= 0, surf.view(F).reshape(-1, 12)
    assert_bits_equal(grid.irradiance(words[hit, 0:3], words[hit, 4:7]), got[hit], "irradiance(points, normals)")
    on_device = api.ProbeGrid(sc, glo, ghi, (2, 2, 2), res=4, device=True).bake(64, 1, 4, map_spp=1)
    t = on_device.shade(torch.from_numpy(surf.view(F).reshape(-1, 12).copy()).to("cuda:0"))
    assert t.is_cuda
    assert_bits_equal(t.cpu().numpy(), got, "the device ProbeGrid")
    assert sc.counters() == cnt0
    img1, _ = sc.render(cam0, RC.W, RC.H, 2, 4)
    assert_bits_equal(img1, img0, "a render after the lookups against one before them")
    assert_bits_equal(sc.query_distance(probe, 4, 2), dist0, "a distance query after the lookups against one before them")
    sc.close()
