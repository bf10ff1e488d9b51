"""Probe relocation on the device (pt_grid_relocate, pt_grid_irradiance_offsets), bit for bit against
tests/grid_relocate_ref.py's f32 restatement: tests/test_grid.py's seeded grids and edge records with offsets of every kind and every
pattern of dead probes, in one cell (the wave-uniform path) and across cells (the lane path); relocation at every map size through
lists of every kind; and api.ProbeGrid.relocate round by round on the Cornell box. Offsets are compared by value: +0 and -0 are equal."""
import os

import numpy as np
import pytest

import grid_live_ref as GL
import grid_ref as GR
import grid_relocate_ref as RR
import motion_cases as MC
import radiance_cases as RC
import test_grid as TG
import test_grid_live as TLV
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

F = np.float32
SH_SAMPLES = TG.SH_SAMPLES
GUARD, TAIL = 0x5a5a5a5a, 16


def _box(lo, hi, counts):
    """max_offset per axis: 0.45 of the axis' step, on an axis with one probe 0.45 of the smallest step of the others (0.3 with none)."""
    steps = [(hi[a] - lo[a]) / (counts[a] - 1) if counts[a] > 1 else None for a in range(3)]
    have = [s for s in steps if s is not None]
    return np.array([0.45 * (s if s is not None else (min(have) if have else 0.3 / 0.45)) for s in steps], F)


def _offset_kinds(lo, hi, counts, seed):
    """Offsets [n, 4] per kind: zero (+0 and -0 mixed), one probe moved, every probe at a corner of the clamp's box. Word 3 is junk."""
    n = counts[0] * counts[1] * counts[2]
    rng = np.random.default_rng(seed)
    box = _box(lo, hi, counts)
    zero, one, clamp = (np.zeros((n, 4), F) for _ in range(3))
    zero[::2, :3] = -0.0
    one[n // 2, :3] = rng.uniform(-1, 1, 3) * box
    clamp[:, :3] = np.where(rng.uniform(0, 1, (n, 3)) < 0.5, -box, box)
    for o in (zero, one, clamp):
        o[:, 3] = TG.JUNK
    return {"zero": zero, "one": one, "clamp": clamp}


def _state_kinds(n):
    p = TLV._patterns(n)
    return {"null": None, "one": p["one"], "alternate": p["alternate"]}


@pytest.mark.parametrize("power", [1, 3])
@pytest.mark.parametrize("counts,res", [(c, r) for c in ((1, 1, 1), (2, 1, 1), (1, 3, 2), (3, 3, 3)) for r in (4, 8, 16)] + [((2, 2, 2), 32)])
def test_the_offsets_lookup_is_the_restatement_bit_for_bit(api, gpu_ready, counts, res, power):
    ms = 16 if res == 8 else 1
    lo, hi, sums, maps = TG._grid(counts, res, ms, 7)
    n = len(sums)
    d = TG._desc(api, lo, hi, counts, res, ms, power)
    packed = api.grid_pack(d, sums, maps)
    coeff, tex = GR.pack(SH_SAMPLES, sums, maps, ms)
    assert RR.fma_of_the_grid_is_never_minus_zero(lo, hi, counts)
    recs = {m: TG._records(lo, hi, counts, m, 100 + m) for m in (1, 63, 64, 65, 130)}
    differs = False
    for oname, off in _offset_kinds(lo, hi, counts, 11).items():
        for sname, st in _state_kinds(n).items():
            for m, rec in recs.items():
                want, _, _ = RR.lookup(lo, hi, counts, coeff, tex, power, rec, off, st)
                got = api.grid_irradiance(packed, d, rec, states=st, offsets=off)
                assert got.shape == (m, 4) and got.dtype == F
                assert_bits_equal(got, want, "counts %s, res %d, power %d, offsets %s, states %s, m %d" % (counts, res, power, oname, sname, m))
                older = api.grid_irradiance(packed, d, rec, states=st)
                if oname == "zero":
                    assert_bits_equal(got, older, "zero offsets, states %s: the older lookup's output" % sname)
                elif oname == "clamp":
                    differs |= bool((got != older).any())
    assert differs                                                              # the offsets reach the result


def test_both_paths_give_a_record_the_same_bits_with_offsets(api, gpu_ready):
    """tests/test_grid_live.py's two orders: 256 records of one cell first (whole waves whose lanes share the cell: offsets and state
    words by scalar loads), test_grid's edge records after them (the lane path); then all permuted. Each record's output has the same
    bits in both orders and is the restatement's. The maps are flat, so far points see no probe: every arm of the end is reached."""
    counts, ms, res = (3, 3, 3), 16, 4
    lo, hi, sums, maps = TG._grid(counts, res, ms, 3, flat=0.4)
    d = TG._desc(api, lo, hi, counts, res, ms, 3)
    packed = api.grid_pack(d, sums, maps)
    coeff, tex = GR.pack(SH_SAMPLES, sums, maps, ms)
    rec = np.concatenate([TLV._one_cell_records(lo, hi, counts, (1, 1, 0), 256, 5), TG._records(lo, hi, counts, 130, 21)], 0)
    rec[300, 0], rec[17, 6] = np.nan, np.inf
    perm = np.random.default_rng(2).permutation(len(rec))
    off = _offset_kinds(lo, hi, counts, 4)["clamp"]
    seen = set()
    states = dict(TLV._patterns(27), null=None)
    for name, st in states.items():
        want, arm, _ = RR.lookup(lo, hi, counts, coeff, tex, 3, rec, off, st)
        got = api.grid_irradiance(packed, d, rec, states=st, offsets=off)
        assert_bits_equal(got, want, "states %s: cell by cell" % name)
        mixed = api.grid_irradiance(packed, d, np.ascontiguousarray(rec[perm]), states=st, offsets=off)
        assert_bits_equal(mixed, got[perm], "states %s: permuted across cells" % name)
        seen |= set(np.unique(arm))
    assert seen == {GL.ARM_WEIGHTED, GL.ARM_PLAIN, GL.ARM_DIVIDED, GL.ARM_DEAD, GL.ARM_BAD}, seen


def test_the_device_lookup_is_the_host_lookup_on_a_stream_of_its_own(api, gpu_ready):
    torch = gpu_ready
    L = api.lib()
    counts, res = (3, 3, 3), 8
    lo, hi, sums, maps = TG._grid(counts, res, 2, 17)
    d = TG._desc(api, lo, hi, counts, res, 2, 3)
    packed = api.grid_pack(d, sums, maps)
    off = _offset_kinds(lo, hi, counts, 9)["clamp"]
    rec = TG._records(lo, hi, counts, 130, 31)
    dp, dr, do = (torch.from_numpy(a).to("cuda:0") for a in (packed, rec, off))
    side = torch.cuda.Stream()
    for st in (TLV._patterns(27)["alternate"], None):
        host = api.grid_irradiance(packed, d, rec, states=st, offsets=off)
        ds = None if st is None else torch.from_numpy(st.view(np.int32)).to("cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            t = api.grid_irradiance(dp, d, dr, states=ds, offsets=do)
        side.synchronize()
        assert isinstance(t, torch.Tensor) and t.device == dr.device and t.shape == (130, 4)
        assert_bits_equal(t.cpu().numpy(), host, "torch in, torch out")
        for m in (1, 65):
            buf = torch.full((m + TAIL, 4), GUARD, dtype=torch.int32, device="cuda:0")
            assert L.pt_grid_irradiance_offsets_device(d, dp.data_ptr(), None if ds is None else ds.data_ptr(), do.data_ptr(), m, dr.data_ptr(), buf.data_ptr(),
                                                       side.cuda_stream) == 0, L.pt_last_error()
            side.synchronize()
            g = buf.cpu().numpy()
            assert (g[m:] == GUARD).all()
            assert_bits_equal(g[:m].view(F), host[:m], "m = %d into a pre-filled buffer" % m)
        out = np.full((130 + TAIL, 4), GUARD, np.uint32)
        assert L.pt_grid_irradiance_offsets(d, packed.ctypes.data, None if st is None else st.ctypes.data, off.ctypes.data, 130, rec.ctypes.data,
                                            out.ctypes.data) == 0, L.pt_last_error()
        assert (out[130:] == GUARD).all()
        assert_bits_equal(out[:130].view(F), host, "the host form into a pre-filled buffer")
        assert api.grid_irradiance(dp, d, dr[:0], states=ds, offsets=do).shape == (0, 4)


# ---- relocate -------------------------------------------------------------------------------------------------------------------------
SPP, N_PROBES, MIN_DIST = 4, 7, 0.25
BOX = np.array([0.375, 0.25, 0.5], F)


def _relocate_maps(res):
    """Seven probes' maps, seeded, means in [0.05, 2): 0 inside with back texels tied at l and l + 1 (across lanes); 1 a near front
    texel tied with the texel a lane's stride on (l + 64; at R < 16 the next row); 2 nothing near; 3 inside without a back majority
    anywhere; 4 NaN and negative means nearest; 5, 6 seeded hit counts."""
    rng = np.random.default_rng(res)
    n, t = N_PROBES, res * res
    maps = np.zeros((n, t, 4), F)
    mean = rng.uniform(0.3, 2.0, (n, t))
    maps[..., 2] = SPP
    maps[0, :, 3] = SPP
    a = int(rng.integers(1, t - 1))
    mean[0, a], mean[0, a + 1] = 0.125, 0.125
    stride = 64 if t > 64 else res
    b = int(rng.integers(0, t - stride))
    mean[1, b + stride], mean[1, b] = 0.0625, 0.0625
    maps[1, (b + 2) % t, 3], mean[1, (b + 2) % t] = SPP, 0.03125                # a nearer back texel in a probe that is not inside: not looked at
    maps[3, :, 2], maps[3, :, 3] = 4, 2
    mean[4, 3], mean[4, 5], mean[4, t - 1] = np.nan, -0.25, 0.1875
    hits = rng.integers(0, SPP + 1, (2, t))
    maps[5:, :, 2] = hits
    maps[5:, :, 3] = np.minimum(hits, rng.integers(0, SPP + 1, (2, t)))
    mean[5:] = rng.uniform(0.05, 0.6, (2, t))
    maps[..., 0], maps[..., 1] = mean * SPP, mean * mean * SPP
    return maps.reshape(n, res, res, 4), a, b


def _same(a, b):
    """Offsets by value: +0 and -0 are equal, and no written offset is a NaN."""
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("res", [4, 8, 16, 32])
def test_relocate_is_the_restatement_and_writes_its_own_rows(api, gpu_ready, res):
    torch = gpu_ready
    n = N_PROBES
    maps, a, b = _relocate_maps(res)
    d = api.grid_desc((0, 0, 0), (1, 1, 1), (n, 1, 1), 64, res, SPP, 3)
    rng = np.random.default_rng(7)
    old = np.zeros((n, 4), F)
    old[:, :3] = rng.uniform(-0.2, 0.2, (n, 3))
    old[:, 3] = 5.0
    old[2, 0], old[6, 1] = 3.0, np.nan                                         # outside the box, and a NaN: both end inside it
    want = RR.relocate(maps, SPP, 0.25, MIN_DIST, BOX, old)
    assert RR.chosen_texel(maps[0], SPP, 0.25)[:2] == (True, a) and RR.chosen_texel(maps[1], SPP, 0.25)[:2] == (False, b)
    assert RR.chosen_texel(maps[4], SPP, 0.25)[:2] == (False, res * res - 1)
    assert list(want[:5, 3]) == [RR.PUSHED_OUT, RR.PUSHED_OFF, RR.KEPT, RR.KEPT, RR.PUSHED_OFF]
    assert np.isfinite(want).all() and (np.abs(want[:, :3]) <= BOX).all() and want[2, 0] == BOX[0]
    got = api.grid_relocate(d, maps, old.copy(), 0.25, MIN_DIST, BOX)
    assert got.dtype == F and _same(got, want), (got, want)
    zeros = api.grid_relocate(d, maps, None, 0.25, MIN_DIST, BOX)
    assert _same(zeros, RR.relocate(maps, SPP, 0.25, MIN_DIST, BOX, np.zeros((n, 4), F)))
    for bf, md in ((0.0, 0.0), (1.0, 0.5)):
        assert _same(api.grid_relocate(d, maps, old.copy(), bf, md, BOX), RR.relocate(maps, SPP, bf, md, BOX, old))
    t = api.grid_relocate(d, torch.from_numpy(maps).to("cuda:0"), torch.from_numpy(old).to("cuda:0"), 0.25, MIN_DIST, BOX)
    assert t.is_cuda and t.dtype == torch.float32 and _same(t.cpu().numpy(), want)
    # lists: k = 1, n - 1 and n, permuted, and rows out of range, which touch nothing; guard words on both sides of the offsets
    perm = rng.permutation(n).astype(np.int32)
    skip = perm[:5].copy()
    skip[1], skip[3] = -1, n
    for idx in (np.array([n - 1], np.int32), perm[:n - 1], perm, skip, None):
        rows = maps if idx is None else np.ascontiguousarray(maps[np.clip(idx, 0, n - 1)])
        wanted = RR.relocate(rows, SPP, 0.25, MIN_DIST, BOX, old, idx)
        touched = np.arange(n) if idx is None else idx[(idx >= 0) & (idx < n)]
        rest = np.setdiff1d(np.arange(n), touched)
        host = np.concatenate([np.full(TAIL, GUARD, np.uint32).view(F), old.ravel(), np.full(TAIL, GUARD, np.uint32).view(F)])
        inner = host[TAIL:TAIL + 4 * n].reshape(n, 4)
        assert api.grid_relocate(d, rows, inner, 0.25, MIN_DIST, BOX, idx) is inner
        assert (host.view(np.uint32)[:TAIL] == GUARD).all() and (host.view(np.uint32)[TAIL + 4 * n:] == GUARD).all()
        assert _same(inner[touched], wanted[touched]), (idx, inner, wanted)
        assert_bits_equal(inner[rest], old[rest], "unlisted probes' offsets")
        dev = torch.from_numpy(np.concatenate([np.full(TAIL, GUARD, np.uint32).view(F), old.ravel(), np.full(TAIL, GUARD, np.uint32).view(F)])).to("cuda:0")
        ti = dev[TAIL:TAIL + 4 * n].view(n, 4)
        api.grid_relocate(d, torch.from_numpy(rows).to("cuda:0"), ti, 0.25, MIN_DIST, BOX, None if idx is None else torch.from_numpy(idx).to("cuda:0"))
        g = dev.cpu().numpy()
        assert (g.view(np.uint32)[:TAIL] == GUARD).all() and (g.view(np.uint32)[TAIL + 4 * n:] == GUARD).all()
        gi = g[TAIL:TAIL + 4 * n].reshape(n, 4)
        assert _same(gi[touched], wanted[touched])
        assert_bits_equal(gi[rest], old[rest], "unlisted probes' offsets, device form")


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_a_relocated_probe_grid_on_the_cornell_box(api, gpu_ready, scene_dir):
    """tests/test_grid_live.py's row of two probes whose first lies inside the tall box, at 64 lanes x 1 sample and R = 4, min_dist and
    max_offset given: every round of ProbeGrid.relocate is the restatement over the grid's kept maps, the moved probes' fresh maps are
    pt_query_distance's at grid position + offset, the packed buffer is the pack of the kept sums and maps, the states are the
    classification of the kept maps; the device grid is the host grid at every step; shade() with offsets and states is the
    restatement; the scene's counters, a later render and a later query_distance are what they were."""
    torch = gpu_ready
    from cudapathtracer_amd import rays, scenes
    hs = api.HostScene(scenes.cornell(os.path.join(scene_dir, "grid_reloc"), width=RC.W, height=RC.H, name="grid_reloc", spp=4, max_depth=4)["config"])
    sc = api.Scene.from_mesh(hs)
    cam0 = api.Camera.frombytes(MC.cam0_bytes(hs.camera()).tobytes())
    img0, _ = sc.render(cam0, RC.W, RC.H, 2, 4)
    A = RC.W / RC.H
    zc = scenes._FRONT_Z - 1.25
    inside, hi, counts = (-(0.42 if A <= 1.2 else 0.6), -0.4, zc - 0.35), (0.2, 0.0, 0.0), (2, 1, 1)
    probe = rays.sh_grid(inside, hi, counts, 1.0)
    dist0 = sc.query_distance(probe, 4, 2)
    sc.render(cam0, RC.W, RC.H, 1, 3, counters=True)
    cnt0 = sc.counters()
    surf = sc.query_closest(sc.query_camera_rays(cam0, RC.W, RC.H).cpu().numpy(), surfaces=True)[1]
    surf = np.ascontiguousarray(surf[np.linspace(0, len(surf) - 1, 130).astype(np.int64)])
    step = 0.2 - inside[0]
    min_dist, box = 0.2 * step, [0.45 * step] * 3
    in32, hi32 = [float(F(v)) for v in inside], [float(F(0.2)), 0.0, 0.0]

    row = api.ProbeGrid(sc, inside, hi, counts, res=4).bake(64, 1, 4, map_spp=2).classify()
    dev = api.ProbeGrid(sc, inside, hi, counts, res=4, device=True).bake(64, 1, 4, map_spp=2).classify()
    assert row.offsets is None and row.states[0] & api.PROBE_INSIDE and not row.states[1] & api.PROBE_INSIDE
    off = np.zeros((2, 4), F)
    history = [(list(row.states), off.tolist())]
    rounds = 0
    for r in range(4):
        want = RR.relocate(row.maps, 2, 0.25, min_dist, box, off)
        moved = np.flatnonzero((want[:, :3] != off[:, :3]).any(1)).astype(np.int32)
        maps_before = row.maps.copy()
        assert row.relocate(64, 1, 4, map_spp=2, min_dist=min_dist, max_offset=box, iterations=1) is row and row.relocate_rounds == 1
        dev.relocate(64, 1, 4, map_spp=2, min_dist=min_dist, max_offset=box, iterations=1)
        rounds += 1
        assert _same(row.offsets, want), (r, row.offsets, want)
        assert _same(dev.offsets.cpu().numpy(), row.offsets)
        if r == 0:
            assert want[0, 3] == RR.PUSHED_OUT and want[0, :3].any()
        if len(moved):
            rec = np.ascontiguousarray(rays.sh_grid(inside, hi, counts, row.max_t, offsets=want)[moved])
            assert np.array_equal(rec[:, :3], (rays.sh_grid(inside, hi, counts)[:, :3] + want[:, :3])[moved])
            rec.view(np.int32)[:, 7] = moved
            assert_bits_equal(row.maps[moved], sc.query_distance(rec, 4, 2, flags=api.QUERY_STREAM_PAD), "round %d: the moved probes' fresh maps" % r)
        rest = np.setdiff1d(np.arange(2), moved)
        assert_bits_equal(row.maps[rest], maps_before[rest], "round %d: the other probes' maps" % r)
        assert_bits_equal(row.packed, GR.packed_words(*GR.pack(64, row.sums, row.maps, 2)), "round %d: the packed buffer" % r)
        assert np.array_equal(row.states, GL.classify(row.maps, 0.25, 2))
        assert_bits_equal(dev.packed.cpu().numpy(), row.packed, "round %d: the device grid's buffer" % r)
        assert np.array_equal(dev.states.cpu().numpy().view(np.uint32), row.states)
        off = want
        history.append((list(row.states), off.tolist()))
        assert not row.states[0] & api.PROBE_INSIDE                             # as measured: out of the box after round one
        if not len(moved):
            break
    print("states and offsets per round:", history)
    # the loop in one call: the same rounds, the same grid
    whole = api.ProbeGrid(sc, inside, hi, counts, res=4).bake(64, 1, 4, map_spp=2).classify()
    assert whole.relocate(64, 1, 4, map_spp=2, min_dist=min_dist, max_offset=box) is whole
    assert whole.relocate_rounds == rounds and _same(whole.offsets, row.offsets)
    assert_bits_equal(whole.packed, row.packed, "relocate() in one call")
    assert np.array_equal(whole.states, row.states)
    # the lookups pass the offsets and the states
    rec = rays.records_from_surfaces(surf)
    got = row.shade(surf)
    want, _, _ = RR.lookup(in32, hi32, counts, *GR.pack(64, row.sums, row.maps, 2), 3, rec, row.offsets, row.states)
    assert_bits_equal(got, want, "ProbeGrid.shade with offsets and states against the restatement")
    assert got[:, :3].max() > 0
    t = dev.shade(torch.from_numpy(surf.view(F).reshape(-1, 12).copy()).to("cuda:0"))
    assert t.is_cuda
    assert_bits_equal(t.cpu().numpy(), got, "the device ProbeGrid with offsets and states")
    assert row.bake(64, 1, 4, map_spp=2).offsets is None

    assert sc.counters() == cnt0
    img1, _ = sc.render(cam0, RC.W, RC.H, 2, 4)
    assert_bits_equal(img1, img0, "a render after the relocation against one before it")
    assert_bits_equal(sc.query_distance(probe, 4, 2), dist0, "a distance query after the relocation against one before it")
    sc.close()
