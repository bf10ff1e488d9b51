"""What keeping a probe grid live costs, in one run.

    python tools/grid_live_time.py [--scene cornell|mixed|blob --w 1920 --h 1080 --reps 5 --warmup 1]
    python tools/grid_live_time.py --resources    (no device needed: compiles pt_grid_live.hip and pt_grid.hip and prints the kernels' registers, scratch and LDS)

tools/grid_time.py's method: HIP events around each call, the median of --reps after --warmup, the grids baked at few samples (64
lanes x 1 a probe, 8 a texel). On the w x h surface points of cam0's centre rays, for an 8^3 and a 16^3 grid with R = 0 and R = 8:
  mask      pt_grid_irradiance_states_device with every state 0 next to pt_grid_irradiance_device in the same run: what the mask
            costs; the same lookup with the states pt_grid_classify gives the scene (R = 8), and with every second probe dead
  update    pt_grid_update_device of n / 8 probes (every eighth, through a list) and of all n (no list), next to pt_grid_pack_device
  classify  pt_grid_classify_device of all n probes (R = 8)
  leak      tools/grid_time.py's leak table through api.ProbeGrid without and with the states of classify(), next to
            rays.grid_irradiance(states=...) in float64 on the same query outputs
With --no-leak the leak table is left out. Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

MAP_SPP = 8


def live_kernel_resources():
    """kernel_resources.kernel_resources of pt_grid_live.hip's two kernels and of the states lookup's two instantiations
    (pt_grid.hip's grid_lookup_kernel<MAPS, 1, 0>) under the names live_classify, live_update, live_lookup_maps and live_lookup_plain."""
    from grid_time import lookup_kernel_resources
    from kernel_resources import kernel_resources
    out = {name[:-len("_kernel")]: r for name, r in kernel_resources("pt_grid_live", r"(live_\w+?_kernel)").items()}
    out.update(lookup_kernel_resources({"110": "live_lookup_maps", "010": "live_lookup_plain"}, {}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scene", choices=("cornell", "mixed", "blob"), default="cornell")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-leak", action="store_true", help="time the library's calls only: no leak table")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps({"resources": live_kernel_resources()}))
        return
    import numpy as np
    import torch
    from cudapathtracer_amd import api, rays as R, scenes
    if not torch.cuda.is_available():
        raise SystemExit("grid_live_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h = a.w, a.h
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    gen = scenes.blob_in_box if a.scene == "blob" else scenes.cornell
    kw = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4]) if a.scene == "mixed" else {}
    hs = api.HostScene(gen(tempfile.mkdtemp(), width=w, height=h, spp=1, max_depth=8, name="glt", **kw)["config"])
    sc = api.Scene(hs)
    cam0 = api.Camera.frombytes(hs.camera().tobytes())
    cam0.antiAliasJitterDist = 0.0
    cam0.aperture = 0.0

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
        for r in (0, 8):
            g = api.ProbeGrid(sc, glo, ghi, counts, res=r, device=True).bake(64, 1, 4, map_spp=MAP_SPP)
            zero = torch.zeros(n, dtype=torch.int32, device=recs.device)
            second = (torch.arange(n, device=recs.device) % 2).to(torch.int32)
            row = {"lookup_ms": events(lambda: api.grid_irradiance(g.packed, g.desc, recs)),
                   "states_zero_ms": events(lambda: api.grid_irradiance(g.packed, g.desc, recs, zero)),
                   "second_dead_ms": events(lambda: api.grid_irradiance(g.packed, g.desc, recs, second))}
            row["mask_over_lookup"] = round(row["states_zero_ms"] / row["lookup_ms"], 3)
            assert torch.equal(api.grid_irradiance(g.packed, g.desc, recs, zero), api.grid_irradiance(g.packed, g.desc, recs))
            eighth = torch.arange(0, n, 8, dtype=torch.int32, device=recs.device)
            at = eighth.long()
            some_maps = g.maps[at].contiguous() if r else None
            some_sums = g.sums[at].contiguous()
            row["pack_ms"] = events(lambda: api.grid_pack(g.desc, g.sums, g.maps))
            row["update_all_ms"] = events(lambda: api.grid_update(g.packed, g.desc, g.sums, g.maps, 0.9))
            row["update_eighth_ms"] = events(lambda: api.grid_update(g.packed, g.desc, some_sums, some_maps, 0.9, eighth))
            if r:
                row["classify_ms"] = events(lambda: api.grid_classify(g.desc, g.maps))
                g.classify()
                st = g.states.cpu().numpy()
                row["inside"], row["idle"] = int((st & api.PROBE_INSIDE != 0).sum()), int((st & api.PROBE_IDLE != 0).sum())
                row["scene_states_ms"] = events(lambda: g.lookup(recs))
            res["grid_%d_res_%d" % (side, r)] = row
            del g
            torch.cuda.empty_cache()

    # the leak table of tools/grid_time.py, through ProbeGrid without and with the states classify() finds
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
        plain = api.ProbeGrid(sc, glo, ghi, c, res=0).bake(lanes, spl, 8)
        sums, maps = g.sums.astype(np.float64), g.maps.astype(np.float64)
        rnd = lambda v: [round(float(x), 4) for x in v.mean(0)] if len(v) else None
        leak = {"points": int(len(p)), "with_maps": rnd(g.irradiance(p, nrm)[:, :3].astype(np.float64)),
                "without_maps": rnd(plain.irradiance(p, nrm)[:, :3].astype(np.float64))}
        g.classify()
        plain.states = g.states
        leak["inside"], leak["idle"] = int((g.states & api.PROBE_INSIDE != 0).sum()), int((g.states & api.PROBE_IDLE != 0).sum())
        leak["with_maps_states"] = rnd(g.irradiance(p, nrm)[:, :3].astype(np.float64))
        leak["without_maps_states"] = rnd(plain.irradiance(p, nrm)[:, :3].astype(np.float64))
        leak["float64_with_maps_states"] = rnd(R.grid_irradiance(glo, ghi, c, sums, lanes * spl, p, nrm, maps, ms, states=g.states))
        leak["float64_without_maps_states"] = rnd(R.grid_irradiance(glo, ghi, c, sums, lanes * spl, p, nrm, states=g.states))
        res["leak"] = leak
    sc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
