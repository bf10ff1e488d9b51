"""What probe relocation costs and what it changes, in one run.

    python tools/grid_relocate_time.py [--scene cornell|mixed|blob --w 1920 --h 1080 --reps 5 --warmup 1 --parent-lib PATH]
    python tools/grid_relocate_time.py --resources    (no device needed: compiles pt_grid_relocate.hip and pt_grid.hip and prints the kernels' registers, scratch and LDS)

tools/grid_live_time.py's method: HIP events around each call, the median of --reps after --warmup, the grids baked at few samples (64
lanes x 1 a probe, 8 a texel). On the w x h surface points of cam0's centre rays, for an 8^3 and a 16^3 grid with R = 8:
  lookup    pt_grid_irradiance_offsets_device with the scene's states and zero offsets next to pt_grid_irradiance_states_device on
            the same inputs in the same run, and without states next to pt_grid_irradiance_device, the device forms called as they
            are into one output buffer; with --parent-lib each of the four next to the same call into another build of the library
            (the parent commit's: parent_<form>_ms), the two builds alternating, and <form>_over_parent;
            then the lookup with the relocated grid's offsets and states, next to the states lookup with those states
  relocate  pt_grid_relocate_device of all n probes next to pt_grid_classify_device
  rounds    api.ProbeGrid.relocate round by round (wall clock with a device synchronisation: a round is queries, an update and a
            classification of the probes that moved): the probes moved, the codes, the probes PROBE_INSIDE before and after
  leak      tools/grid_live_time.py's leak table with a column for the relocated grid
With --no-leak the leak table is left out. Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

MAP_SPP = 8
ROUNDS = 4


def relocate_kernel_resources():
    """kernel_resources.kernel_resources of pt_grid_relocate.hip's kernel and of the offsets lookup's two instantiations
    (pt_grid.hip's grid_lookup_kernel<1, STATES, 1>) under the names reloc, reloc_lookup_states and reloc_lookup_none."""
    from grid_time import lookup_kernel_resources
    from kernel_resources import kernel_resources
    out = {name[:-len("_kernel")]: r for name, r in kernel_resources("pt_grid_relocate", r"(reloc\w*?_kernel)").items()}
    out.update(lookup_kernel_resources({"111": "reloc_lookup_states", "101": "reloc_lookup_none"}, {}))
    return out


def relocate_rounds(grid, api, lanes, spp_lane, max_depth, map_spp, sync=None):
    """ProbeGrid.relocate one round at a time, at most ROUNDS: per round its wall-clock ms, the probes whose offset changed, the
    codes' counts and the PROBE_INSIDE probes after it."""
    import numpy as np
    host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else v
    rows = []
    for _ in range(ROUNDS):
        before = np.zeros((grid.counts[0] * grid.counts[1] * grid.counts[2], 4), np.float32) if grid.offsets is None else host(grid.offsets).copy()
        if sync:
            sync()
        t0 = time.perf_counter()
        grid.relocate(lanes, spp_lane, max_depth, map_spp=map_spp, iterations=1)
        if sync:
            sync()
        ms = (time.perf_counter() - t0) * 1e3
        off, st = host(grid.offsets), host(grid.states).view(np.uint32)
        moved = int((off[:, :3] != before[:, :3]).any(1).sum())
        rows.append({"ms": round(ms, 3), "moved": moved, "codes": [int((off[:, 3] == c).sum()) for c in (0, 1, 2)],
                     "inside": int((st & api.PROBE_INSIDE != 0).sum())})
        if not moved:
            break
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scene", choices=("cornell", "mixed", "blob"), default="cornell")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-leak", action="store_true", help="time the library's calls only: no leak table")
    ap.add_argument("--parent-lib", help="another build of libptamd.so whose four lookup forms are timed in the same run")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps({"resources": relocate_kernel_resources()}))
        return
    import numpy as np
    import torch
    from cudapathtracer_amd import api, rays as R, scenes
    if not torch.cuda.is_available():
        raise SystemExit("grid_relocate_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h = a.w, a.h
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    gen = scenes.blob_in_box if a.scene == "blob" else scenes.cornell
    kw = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4]) if a.scene == "mixed" else {}
    hs = api.HostScene(gen(tempfile.mkdtemp(), width=w, height=h, spp=1, max_depth=8, name="grt", **kw)["config"])
    sc = api.Scene(hs)
    cam0 = api.Camera.frombytes(hs.camera().tobytes())
    cam0.antiAliasJitterDist = 0.0
    cam0.aperture = 0.0
    parent = None
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        for fn in ("pt_grid_irradiance_device", "pt_grid_irradiance_states_device", "pt_grid_irradiance_offsets_device"):
            getattr(parent, fn).argtypes = getattr(api.lib(), fn).argtypes

    def events(run):
        ms = []
        for _ in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); run(); e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return med(ms[a.warmup:])

    pts = np.ascontiguousarray(hs.array("points")).view(np.float32).reshape(-1, 4)[:, :3]
    lo, hi = pts.min(0), pts.max(0)
    inset = 0.02 * (hi - lo)
    glo, ghi = lo + inset, hi - inset
    surf = sc.query_closest(sc.query_camera_rays(cam0, w, h), surfaces=True)[1]
    recs = R.records_from_surfaces(surf)
    res = {"scene": a.scene, "n_tris": hs.info["n_tris"], "w": w, "h": h, "points": w * h, "reps": a.reps, "warmup": a.warmup}

    for side in (8, 16):
        counts = (side, side, side)
        n = side ** 3
        g = api.ProbeGrid(sc, glo, ghi, counts, res=8, device=True).bake(64, 1, 4, map_spp=MAP_SPP).classify()
        zero = torch.zeros((n, 4), dtype=torch.float32, device=recs.device)
        st0 = g.states.clone()
        row = {"inside_before": int((st0.cpu().numpy().view(np.uint32) & api.PROBE_INSIDE != 0).sum())}
        # the lookups alternate, so that a drift of the device's clock falls on all of them; each is the library's device form called
        # as it is, into one output buffer: at a tenth of a millisecond a wrapper's checks and its allocation would show
        out = torch.empty((w * h, 4), dtype=torch.float32, device=recs.device)
        L, dref, m = api.lib(), C.byref(g.desc), w * h
        ptr = lambda t: t.data_ptr()
        forms = {"plain": lambda B: B.pt_grid_irradiance_device(dref, ptr(g.packed), m, ptr(recs), ptr(out), None),
                 "states": lambda B: B.pt_grid_irradiance_states_device(dref, ptr(g.packed), ptr(st0), m, ptr(recs), ptr(out), None),
                 "offsets_zero": lambda B: B.pt_grid_irradiance_offsets_device(dref, ptr(g.packed), ptr(st0), ptr(zero), m, ptr(recs), ptr(out), None),
                 "offsets_zero_no_states": lambda B: B.pt_grid_irradiance_offsets_device(dref, ptr(g.packed), None, ptr(zero), m, ptr(recs), ptr(out), None)}
        builds = {"": L} if parent is None else {"": L, "parent_": parent}
        names = {pre + k + "_ms": (lambda run=run, B=B: run(B)) for k, run in forms.items() for pre, B in builds.items()}
        took = {k: [] for k in names}
        for _ in range(3):
            for k, run in names.items():
                took[k].append(events(run))
        row.update({k: med(v) for k, v in took.items()})
        row["offsets_over_states"] = round(row["offsets_zero_ms"] / row["states_ms"], 3)
        row["offsets_over_plain_no_states"] = round(row["offsets_zero_no_states_ms"] / row["plain_ms"], 3)
        assert torch.equal(api.grid_irradiance(g.packed, g.desc, recs, st0, zero), api.grid_irradiance(g.packed, g.desc, recs, st0))
        assert torch.equal(api.grid_irradiance(g.packed, g.desc, recs, None, zero), api.grid_irradiance(g.packed, g.desc, recs))
        if parent is not None:
            for k, (st, off) in {"plain": (None, None), "states": (st0, None), "offsets_zero": (st0, zero), "offsets_zero_no_states": (None, zero)}.items():
                row[k + "_over_parent"] = round(row[k + "_ms"] / row["parent_" + k + "_ms"], 3)
                names["parent_" + k + "_ms"]()
                torch.cuda.synchronize()
                assert torch.equal(out, api.grid_irradiance(g.packed, g.desc, recs, st, off)), k
        row["classify_ms"] = events(lambda: api.grid_classify(g.desc, g.maps))
        scratch = torch.zeros((n, 4), dtype=torch.float32, device=recs.device)
        row["relocate_ms"] = events(lambda: api.grid_relocate(g.desc, g.maps, scratch.zero_()))
        row["rounds"] = relocate_rounds(g, api, 64, 1, 4, MAP_SPP, torch.cuda.synchronize)
        row["inside_after"] = row["rounds"][-1]["inside"]
        row["offsets_scene_ms"] = events(lambda: L.pt_grid_irradiance_offsets_device(dref, ptr(g.packed), ptr(g.states), ptr(g.offsets), m, ptr(recs), ptr(out), None))
        row["states_scene_relocated_ms"] = events(lambda: L.pt_grid_irradiance_states_device(dref, ptr(g.packed), ptr(g.states), m, ptr(recs), ptr(out), None))
        res["grid_%d_res_8" % side] = row
        del g
        torch.cuda.empty_cache()

    # the leak table of tools/grid_live_time.py, with a column for the relocated grid
    gx, gz = np.meshgrid(np.linspace(lo[0], hi[0], 13)[1:-1], np.linspace(lo[2], hi[2], 13)[1:-1])
    up = np.tile([(0.0, 1.0, 0.0)], (gx.size, 1))
    s = sc.query_closest(R.irradiance_records(np.stack([gx.ravel(), np.full(gx.size, lo[1] + 0.9 * (hi[1] - lo[1])), gz.ravel()], 1), up), surfaces=True)[1]
    lit = s["light"] >= 0
    if lit.any() and not a.no_leak:
        light = np.array([s["px"][lit].mean(), s["py"][lit].mean(), s["pz"][lit].mean()])
        fx, fz = np.meshgrid(np.linspace(lo[0], hi[0], 34)[1:-1], np.linspace(lo[2], hi[2], 34)[1:-1])
        floor = np.stack([fx.ravel(), np.full(fx.size, lo[1] + 1e-4), fz.ravel()], 1).astype(np.float32)
        to = light[None, :] - floor
        dist = np.linalg.norm(to, axis=1)
        sh = R.irradiance_records(floor, to / dist[:, None])
        sh[:, 3] = dist - 1e-2
        blocked = ~sc.query_shadow(sh)[:, :3].any(1)
        clear = sc.query_closest(R.irradiance_records(floor, np.tile([(0.0, 1.0, 0.0)], (len(floor), 1))))["t"] > 0.05
        p = floor[blocked & clear]
        nrm = np.tile(np.array([(0.0, 1.0, 0.0)], np.float32), (len(p), 1))
        c, lanes, spl, ms = (8, 8, 8), 256, 16, 16
        cell = float(np.linalg.norm((ghi - glo) / 7.0))
        g = api.ProbeGrid(sc, glo, ghi, c, res=8, max_t=1.5 * cell).bake(lanes, spl, 8, map_spp=ms)
        rnd = lambda v: [round(float(x), 4) for x in v.mean(0)] if len(v) else None
        leak = {"points": int(len(p)), "with_maps": rnd(g.irradiance(p, nrm)[:, :3].astype(np.float64))}
        g.classify()
        leak["inside"] = int((g.states & api.PROBE_INSIDE != 0).sum())
        leak["with_maps_states"] = rnd(g.irradiance(p, nrm)[:, :3].astype(np.float64))
        leak["rounds"] = relocate_rounds(g, api, lanes, spl, 8, ms)
        leak["inside_relocated"] = int((g.states & api.PROBE_INSIDE != 0).sum())
        leak["with_maps_states_relocated"] = rnd(g.irradiance(p, nrm)[:, :3].astype(np.float64))
        leak["float64_with_maps_states_relocated"] = rnd(R.grid_irradiance(glo, ghi, c, g.sums.astype(np.float64), lanes * spl, p, nrm, g.maps.astype(np.float64), ms,
                                                                           states=g.states, offsets=g.offsets.astype(np.float64)))
        res["leak"] = leak
    sc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
