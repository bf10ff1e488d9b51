"""Live probe grids on the device (pt_grid_classify, pt_grid_update, pt_grid_irradiance_states), bit for bit against
tests/grid_live_ref.py's f32 restatement: tests/test_grid.py's seeded grids and edge records under every pattern of dead probes, in
one cell (the wave-uniform path) and across cells (the lane path); updates through lists of every kind; classification at every map
size; and api.ProbeGrid's update and classify end to end on the Cornell box."""
import os

import numpy as np
import pytest

import grid_live_ref as GL
import grid_ref as GR
import motion_cases as MC
import radiance_cases as RC
import test_grid as TG
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

F = np.float32
SH_SAMPLES = TG.SH_SAMPLES
GUARD, TAIL = 0x5a5a5a5a, 16


def _patterns(n):
    """State words for n probes: none dead, one, every second, all; live words carry junk in their high bits, dead ones too."""
    none, one, alt, every = (np.full(n, 0xfffffffe, np.uint32) for _ in range(4))
    none[::2] = 0
    one[n // 2] = 3
    alt[::2] = 0x80000001
    every[:] = 1
    every[::3] = 0xffffffff
    return {"none": none, "one": one, "alternate": alt, "all": every}


@pytest.mark.parametrize("power", [1, 3])
@pytest.mark.parametrize("res", [0, 4, 8])
@pytest.mark.parametrize("counts", [(1, 1, 1), (2, 1, 1), (1, 3, 2), (3, 3, 3)])
def test_the_masked_lookup_is_the_restatement_bit_for_bit(api, gpu_ready, counts, res, power):
    ms = 16 if res == 8 else 1
    lo, hi, sums, maps = TG._grid(counts, res, ms, 7)
    n = len(sums)
    d = TG._desc(api, lo, hi, counts, res, ms, power)
    packed = api.grid_pack(d, sums, maps)
    coeff, tex = GR.pack(SH_SAMPLES, sums, maps, ms)
    for name, st in _patterns(n).items():
        for m in (1, 63, 64, 65, 130):
            rec = TG._records(lo, hi, counts, m, 100 + m)
            want, arm, _ = GL.lookup(lo, hi, counts, coeff, tex, power, rec, st)
            got = api.grid_irradiance(packed, d, rec, states=st)
            assert got.shape == (m, 4) and got.dtype == F
            assert_bits_equal(got, want, "counts %s, res %d, power %d, states %s, m %d" % (counts, res, power, name, m))
            if name == "none":
                assert_bits_equal(got, api.grid_irradiance(packed, d, rec), "no probe dead: pt_grid_irradiance's output")
            if name == "all":
                assert not got.view(np.uint32).any()


def _one_cell_records(lo, hi, counts, cell, m, seed):
    """m records strictly inside cell `cell` of the grid, the first ones a hair from its corners and faces, with test_grid's junk in
    the words not read. (The points on a probe and on a face itself are among test_grid's records.)"""
    from cudapathtracer_amd import rays
    rng = np.random.default_rng(seed)
    step = np.array([(hi[a] - lo[a]) / (counts[a] - 1) for a in range(3)])
    c0 = np.array(lo) + step * np.array(cell)
    u = rng.uniform(0.02, 0.98, (m, 3))
    u[:8] = [[0.999 if (c >> a) & 1 else 0.001 for a in range(3)] for c in range(8)]
    for i in range(6):
        u[8 + i, i % 3] = 0.999 if i // 3 else 0.001
    p = (c0 + u * step).astype(F)
    nrm = rng.standard_normal((m, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F)
    rec = rays.irradiance_records(p, nrm)
    rec[:, 3], rec[:, 7] = TG.JUNK, TG.JUNK
    return rec


@pytest.mark.parametrize("res", [0, 4])
def test_both_paths_give_a_record_the_same_bits_and_every_arm_is_reached(api, gpu_ready, res):
    """256 records of one cell first (four whole waves whose lanes share the cell: the path with the states in SGPRs), test_grid's
    edge records after them (waves that mix cells: the lane path); then all of them permuted, so that every wave mixes cells. Each
    record's output has the same bits in both orders and is the restatement's. The maps are flat, so far points see no probe: with
    maps the data reaches every arm of the lookup's end."""
    counts, ms = (3, 3, 3), 16
    lo, hi, sums, maps = TG._grid(counts, res, ms, 3, flat=0.4)
    d = TG._desc(api, lo, hi, counts, res, ms, 3)
    packed = api.grid_pack(d, sums, maps)
    coeff, tex = GR.pack(SH_SAMPLES, sums, maps, ms)
    rec = np.concatenate([_one_cell_records(lo, hi, counts, (1, 1, 0), 256, 5), TG._records(lo, hi, counts, 130, 21)], 0)
    rec[300, 0], rec[17, 6] = np.nan, np.inf
    low = np.floor((rec[:256, 0:3] - np.array(lo, F)) / (np.array(hi, F) - np.array(lo, F)) * F(2))
    assert (low[np.isfinite(low).all(1)] == np.array([1, 1, 0], F)).all()       # (record 17 is the bad one)
    perm = np.random.default_rng(2).permutation(len(rec))
    seen = set()
    for name, st in _patterns(27).items():
        want, arm, _ = GL.lookup(lo, hi, counts, coeff, tex, 3, rec, st)
        got = api.grid_irradiance(packed, d, rec, states=st)
        assert_bits_equal(got, want, "res %d, states %s: cell by cell" % (res, name))
        mixed = api.grid_irradiance(packed, d, np.ascontiguousarray(rec[perm]), states=st)
        assert_bits_equal(mixed, got[perm], "res %d, states %s: permuted across cells" % (res, name))
        seen |= set(np.unique(arm))
    want_arms = {GL.ARM_PLAIN, GL.ARM_DIVIDED, GL.ARM_DEAD, GL.ARM_BAD} | ({GL.ARM_WEIGHTED} if res else set())
    assert seen == want_arms, seen


def test_the_device_form_is_the_host_form_on_a_stream_of_its_own(api, gpu_ready):
    torch = gpu_ready
    L = api.lib()
    for counts, res in (((3, 3, 3), 8), ((1, 3, 2), 0)):
        lo, hi, sums, maps = TG._grid(counts, res, 2, 17)
        d = TG._desc(api, lo, hi, counts, res, 2, 3)
        packed = api.grid_pack(d, sums, maps)
        st = _patterns(len(sums))["alternate"]
        rec = TG._records(lo, hi, counts, 130, 31)
        host = api.grid_irradiance(packed, d, rec, states=st)
        dp, dr = torch.from_numpy(packed).to("cuda:0"), torch.from_numpy(rec).to("cuda:0")
        ds = torch.from_numpy(st.view(np.int32)).to("cuda:0")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            t = api.grid_irradiance(dp, d, dr, states=ds)
        side.synchronize()
        assert isinstance(t, torch.Tensor) and t.device == dr.device and t.shape == (130, 4)
        assert_bits_equal(t.cpu().numpy(), host, "torch in, torch out")
        for m in (1, 65):
            buf = torch.full((m + TAIL, 4), GUARD, dtype=torch.int32, device="cuda:0")
            assert L.pt_grid_irradiance_states_device(d, dp.data_ptr(), ds.data_ptr(), m, dr.data_ptr(), buf.data_ptr(), side.cuda_stream) == 0, L.pt_last_error()
            side.synchronize()
            g = buf.cpu().numpy()
            assert (g[m:] == GUARD).all()
            assert_bits_equal(g[:m].view(F), host[:m], "m = %d into a pre-filled buffer" % m)
        out = np.full((130 + TAIL, 4), GUARD, np.uint32)
        assert L.pt_grid_irradiance_states(d, packed.ctypes.data, st.ctypes.data, 130, rec.ctypes.data, out.ctypes.data) == 0, L.pt_last_error()
        assert (out[130:] == GUARD).all()
        assert_bits_equal(out[:130].view(F), host, "the host form into a pre-filled buffer")
        assert api.grid_irradiance(dp, d, dr[:0], states=ds).shape == (0, 4)


# ---- update -------------------------------------------------------------------------------------------------------------------------
def _fresh(sums, maps, seed):
    rng = np.random.default_rng(seed)
    s = (sums * rng.uniform(0.5, 1.5, sums.shape)).astype(F)
    return s, (None if maps is None else (maps * rng.uniform(0.5, 1.5, maps.shape)).astype(F))


def _lists(n):
    """(name, indices or None, rows of fresh data): one probe, all but one permuted, all permuted, the identity without a list, and a
    list with an index of -1 and one of n, which touch nothing."""
    rng = np.random.default_rng(n)
    out = [("one", np.array([n - 1], np.int32)), ("all permuted", rng.permutation(n).astype(np.int32)), ("identity", None)]
    if n > 1:
        out.append(("all but one", rng.permutation(n)[:n - 1].astype(np.int32)))
    if n > 2:
        skip = rng.permutation(n)[:3].astype(np.int32)
        skip[0], skip[2] = -1, n
        out.append(("out of range", skip))
    return out


@pytest.mark.parametrize("counts,res", [((1, 3, 2), 0), ((3, 3, 3), 4), ((1, 3, 2), 8), ((1, 1, 1), 32), ((2, 1, 1), 4)])
def test_the_update_is_the_restatement_and_touches_nothing_else(api, gpu_ready, counts, res):
    torch = gpu_ready
    L = api.lib()
    ms_old, ms_new, sh_new = 4, 3, 48
    lo, hi, sums, maps = TG._grid(counts, res, ms_old, 13)
    n = len(sums)
    d_old = TG._desc(api, lo, hi, counts, res, ms_old, 3)
    d_new = api.grid_desc(lo, hi, counts, sh_new, res, ms_new, 3)
    base = api.grid_pack(d_old, sums, maps)
    coeff, tex = GR.pack(SH_SAMPLES, sums, maps, ms_old)
    words = len(base)
    fs, fm = _fresh(sums, maps, 5)
    # h = 0 over all probes: pt_grid_pack's buffer of the fresh sums, whatever was there
    junk = np.full(words, np.nan, F)
    assert api.grid_update(junk, d_new, fs, fm, 0.0) is junk
    assert_bits_equal(junk, api.grid_pack(d_new, fs, fm), "h = 0 over all probes against the pack")
    for name, idx in _lists(n):
        k = n if idx is None else len(idx)
        rs, rm = np.ascontiguousarray(fs[:k]), (None if fm is None else np.ascontiguousarray(fm[:k]))
        for h in (0.0, 0.5, 0.96875):
            wc, wt = GL.update(coeff, tex, sh_new, rs, rm, ms_new, h, idx)
            want = GR.packed_words(wc, wt)
            host = np.concatenate([np.full(TAIL, GUARD, np.uint32).view(F), base, np.full(TAIL, GUARD, np.uint32).view(F)])
            inner = host[TAIL:TAIL + words]
            assert L.pt_grid_update(d_new, k, None if idx is None else idx.ctypes.data, rs.ctypes.data, None if rm is None else rm.ctypes.data, h,
                                    inner.ctypes.data) == 0, L.pt_last_error()
            assert (host.view(np.uint32)[:TAIL] == GUARD).all() and (host.view(np.uint32)[TAIL + words:] == GUARD).all()
            assert_bits_equal(inner, want, "host update, %s, h %g" % (name, h))
            touched = np.arange(n) if idx is None else idx[(idx >= 0) & (idx < n)]
            rest = np.setdiff1d(np.arange(n), touched)
            assert_bits_equal(inner[:n * 36].reshape(n, 36)[rest], base[:n * 36].reshape(n, 36)[rest], "unlisted probes' coefficients")
            if res:
                assert_bits_equal(inner[n * 36:].reshape(n, -1)[rest], base[n * 36:].reshape(n, -1)[rest], "unlisted probes' maps")
            if h == 0.5:
                dev = torch.from_numpy(host.copy()).to("cuda:0")
                t = dev[TAIL:TAIL + words]
                t.copy_(torch.from_numpy(base).to("cuda:0"))
                args = [torch.from_numpy(a).to("cuda:0") if a is not None else None for a in (rs, rm, idx)]
                assert api.grid_update(t, d_new, args[0], args[1], h, args[2]) is t
                torch.cuda.synchronize()
                g = dev.cpu().numpy()
                assert (g.view(np.uint32)[:TAIL] == GUARD).all() and (g.view(np.uint32)[TAIL + words:] == GUARD).all()
                assert_bits_equal(g[TAIL:TAIL + words], want, "device update, %s" % name)


# ---- classify -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("res", [4, 8, 16, 32])
def test_classify_is_the_restatement_and_writes_its_own_words(api, gpu_ready, res, n):
    torch = gpu_ready
    rng = np.random.default_rng(res + n)
    spp = 4
    maps = np.zeros((n, res, res, 4), F)
    maps[..., :2] = rng.uniform(0.0, 5.0, (n, res, res, 2))                     # the moments are not read
    hits = rng.integers(0, spp + 1, (n, res, res))
    maps[..., 2] = hits
    maps[..., 3] = np.minimum(hits, rng.integers(0, spp + 1, (n, res, res)) * (rng.uniform(0, 1, (n, 1, 1)) < 0.5))
    maps[0, ..., 2], maps[0, ..., 3] = 4, 0
    maps[0, 0, :4, 3] = res * res / 4                                           # probe 0: Ks = res^2 = 0.25 Hs, the tie
    if n > 1:
        maps[1, ..., 2:] = 0                                                    # probe 1 hits nothing
        maps[2, ..., 2], maps[2, ..., 3] = 1, 1
        maps[2, res - 1, res - 1, 2] = np.nan                                   # probe 2: a NaN count
        maps[3, ..., 2], maps[3, ..., 3] = 4, 0
        maps[3, 0, :4, 3] = res * res / 4
        maps[3, res - 1, res - 1, 3] += 1                                       # probe 3: one past the tie
    d = api.grid_desc((0, 0, 0), (1, 1, 1), (n, 1, 1), 64, res, spp, 3)
    want = GL.classify(maps, 0.25, n)
    assert want[0] == 0 and (n == 1 or list(want[1:4]) == [GL.IDLE, 0, GL.INSIDE])
    got = api.grid_classify(d, maps)
    assert got.dtype == np.uint32 and np.array_equal(got, want), (got, want)
    for bf in (0.0, 0.5, 1.0):
        assert np.array_equal(api.grid_classify(d, maps, bf), GL.classify(maps, bf, n))
    t = api.grid_classify(d, torch.from_numpy(maps).to("cuda:0"))
    assert t.is_cuda and t.dtype == torch.int32 and np.array_equal(t.cpu().numpy().view(np.uint32), want)
    if n > 1:
        # a list: its probes' words alone, rows out of range none; guard words round the states
        idx = np.array([3, -1, 0, n, 1], np.int32)
        rows = np.ascontiguousarray(maps[[3, 2, 0, 4, 1]])
        before = np.full(n + 2 * TAIL, GUARD, np.uint32)
        inner = before[TAIL:TAIL + n]
        inner[:] = 0xabcd0000
        assert api.grid_classify(d, rows, 0.25, idx, inner) is inner
        assert np.array_equal(inner, GL.classify(rows, 0.25, n, idx, np.full(n, 0xabcd0000, np.uint32)))
        assert list(inner) == [0, GL.IDLE, 0xabcd0000, GL.INSIDE, 0xabcd0000]
        assert (before[:TAIL] == GUARD).all() and (before[TAIL + n:] == GUARD).all()
        dev = torch.from_numpy(np.full(n + 2 * TAIL, GUARD, np.uint32).view(np.int32)).to("cuda:0")
        ts = dev[TAIL:TAIL + n]
        ts.fill_(7)
        api.grid_classify(d, torch.from_numpy(rows).to("cuda:0"), 0.25, torch.from_numpy(idx).to("cuda:0"), ts)
        g = dev.cpu().numpy().view(np.uint32)
        assert list(g[TAIL:TAIL + n]) == [0, GL.IDLE, 7, GL.INSIDE, 7] and (g[:TAIL] == GUARD).all() and (g[TAIL + n:] == GUARD).all()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_a_live_probe_grid_on_the_cornell_box(api, gpu_ready, scene_dir):
    """A 2 x 2 x 2 ProbeGrid at 64 lanes x 1 sample and R = 4, and a row of two probes whose first lies inside the tall box: a subset
    update with the bake's seed and no hysteresis changes no bit; a blended update with another seed, classify() and shade() with
    states are the restatement over the same query outputs; the device grid is the host grid; the scene's counters, a later render
    and a later query_distance are what they were."""
    torch = gpu_ready
    from cudapathtracer_amd import rays, scenes
    hs = api.HostScene(scenes.cornell(os.path.join(scene_dir, "grid_live"), width=RC.W, height=RC.H, name="grid_live", spp=4, max_depth=4)["config"])
    sc = api.Scene.from_mesh(hs)
    cam0 = api.Camera.frombytes(MC.cam0_bytes(hs.camera()).tobytes())
    pts = np.ascontiguousarray(hs.array("points")).view(np.float32).reshape(-1, 4)[:, :3]
    lo, hi = pts.min(0), pts.max(0)
    glo, ghi = lo + 0.2 * (hi - lo), hi - 0.2 * (hi - lo)
    counts = (2, 2, 2)
    img0, _ = sc.render(cam0, RC.W, RC.H, 2, 4)
    probe = rays.sh_grid(glo, ghi, counts, 1.0)
    dist0 = sc.query_distance(probe, 4, 2)
    sc.render(cam0, RC.W, RC.H, 1, 3, counters=True)
    cnt0 = sc.counters()
    surf = sc.query_closest(sc.query_camera_rays(cam0, RC.W, RC.H).cpu().numpy(), surfaces=True)[1]
    surf = np.ascontiguousarray(surf[np.linspace(0, len(surf) - 1, 130).astype(np.int64)])
    lo32, hi32 = [float(F(v)) for v in glo], [float(F(v)) for v in ghi]

    grid = api.ProbeGrid(sc, glo, ghi, counts, res=4).bake(64, 1, 4, map_spp=1)
    assert grid.states is None
    baked = grid.packed.copy()
    # the listed probes get the full bake's streams: same seed, no hysteresis, the same bits
    assert grid.update(64, 1, 4, map_spp=1, hysteresis=0.0, probes=[1, 6]) is grid
    assert_bits_equal(grid.packed, baked, "a subset re-bake with the bake's seed")
    # another seed, blended: the restatement over the same query outputs
    sums0, maps0 = grid.sums.copy(), grid.maps.copy()
    grid.update(64, 1, 4, map_spp=1, hysteresis=0.5, seed=api.SEED + 1)
    sums1 = sc.query_sh(rays.sh_grid(glo, ghi, counts), 64, 1, 4, seed=api.SEED + 1)
    maps1 = sc.query_distance(rays.sh_grid(glo, ghi, counts, grid.max_t), 4, 1, seed=api.SEED + 1)
    assert (sums1 != sums0).any() and (maps1 != maps0).any()
    assert_bits_equal(grid.sums, sums1, "the kept sums are the fresh ones")
    assert_bits_equal(grid.maps, maps1, "the kept maps are the fresh ones")
    coeff, tex = GL.update(*GR.pack(64, sums0, maps0, 1), 64, sums1, maps1, 1, 0.5)
    assert_bits_equal(grid.packed, GR.packed_words(coeff, tex), "a blended update against the restatement")
    assert grid.classify() is grid
    assert np.array_equal(grid.states, GL.classify(maps1, 0.25, 8))
    got = grid.shade(surf)
    want, _, _ = GL.lookup(lo32, hi32, counts, coeff, tex, 3, rays.records_from_surfaces(surf), grid.states)
    assert_bits_equal(got, want, "ProbeGrid.shade with states against the restatement")
    assert got[:, :3].max() > 0

    # a probe inside the tall box next to one in the open room
    A = RC.W / RC.H
    zc = scenes._FRONT_Z - 1.25
    inside = (-(0.42 if A <= 1.2 else 0.6), -0.4, zc - 0.35)
    row = api.ProbeGrid(sc, inside, (0.2, 0.0, 0.0), (2, 1, 1), res=4).bake(64, 1, 4, map_spp=2).classify()
    assert_bits_equal(row.maps, sc.query_distance(rays.sh_grid(inside, (0.2, 0.0, 0.0), (2, 1, 1), row.max_t), 4, 2), "the row's maps")
    assert np.array_equal(row.states, GL.classify(row.maps, 0.25, 2))
    assert row.states[0] & api.PROBE_INSIDE and not row.states[1] & api.PROBE_INSIDE, row.states
    c2, t2 = GR.pack(64, row.sums, row.maps, 2)
    in32, hi2 = [float(F(v)) for v in inside], [float(F(0.2)), 0.0, 0.0]
    rec = rays.records_from_surfaces(surf)
    got_row = row.lookup(rec)
    want_row, arm, _ = GL.lookup(in32, hi2, (2, 1, 1), c2, t2, 3, rec, row.states)
    assert_bits_equal(got_row, want_row, "the row with its dead probe against the restatement")
    unmasked, _ = GR.lookup(in32, hi2, (2, 1, 1), c2, t2, 3, rec)
    assert (got_row != unmasked).any()                                          # the probe in the box lit something before
    # states survive an update of the listed probes and are classified again from the fresh maps
    row.update(64, 1, 4, map_spp=2, hysteresis=0.5, probes=[0], seed=api.SEED + 2, skip_idle=True)
    assert row.states[0] & api.PROBE_INSIDE and np.array_equal(row.states, GL.classify(row.maps, 0.25, 2))
    assert row.bake(64, 1, 4, map_spp=2).states is None

    # the device grid is the host grid, step by step
    dev = api.ProbeGrid(sc, glo, ghi, counts, res=4, device=True).bake(64, 1, 4, map_spp=1)
    assert_bits_equal(dev.packed.cpu().numpy(), baked, "the device bake")
    dev.update(64, 1, 4, map_spp=1, hysteresis=0.0, probes=[1, 6])
    assert_bits_equal(dev.packed.cpu().numpy(), baked, "the device subset re-bake")
    dev.update(64, 1, 4, map_spp=1, hysteresis=0.5, seed=api.SEED + 1).classify()
    assert_bits_equal(dev.packed.cpu().numpy(), grid.packed, "the device blended update")
    assert np.array_equal(dev.states.cpu().numpy().view(np.uint32), grid.states)
    t = dev.shade(torch.from_numpy(surf.view(F).reshape(-1, 12).copy()).to("cuda:0"))
    assert t.is_cuda
    assert_bits_equal(t.cpu().numpy(), got, "the device ProbeGrid with states")

    assert sc.counters() == cnt0
    img1, _ = sc.render(cam0, RC.W, RC.H, 2, 4)
    assert_bits_equal(img1, img0, "a render after the updates against one before them")
    assert_bits_equal(sc.query_distance(probe, 4, 2), dist0, "a distance query after the updates against one before them")
    sc.close()
