"""What a probe-grid lookup costs next to the route it replaces, in one run.

    python tools/grid_time.py [--scene cornell|mixed|blob --w 1920 --h 1080 --reps 5 --warmup 1]
    python tools/grid_time.py --resources    (no device needed: compiles pt_grid.hip and prints its kernels' registers, scratch and LDS)

HIP events around each call, the median of --reps after --warmup (as tools/distance_time.py takes them):
  pack      pt_grid_pack_device for an 8^3 and a 16^3 grid at R = 8 and 16 and without maps, next to the torch route to the same
            arrays (rays._sh_convolved, rays.oct_border, a division)
  lookup    pt_grid_irradiance_device on the w x h surface points of cam0's centre rays (pt_query_closest's surfaces through
            rays.records_from_surfaces; cam0 is the scene's camera without jitter and aperture) for each of those grids, with and
            without maps; next to it rays.grid_irradiance on the same device tensors, the route the call replaces; the largest
            difference between the two over the largest value, which shows it is rounding; and the time of the bytes the call must
            move, (32 + 16) m, at the 6.3 TB/s of HBM bandwidth a kernel can reach on this device: the floor
  leak      tools/distance_time.py's table (c) through api.ProbeGrid next to the Python lookup on the same query outputs
The grids are baked at few samples (64 lanes x 1 a probe, 8 a texel): the tables time the lookup, not the bake. With --no-route the
torch route and the leak table are left out.
`cornell` is the plain box, `mixed` bench.py --full's mixed Cornell box, `blob` the 82 k blob in the box.
Prints one JSON line."""
import argparse
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

HBM_BYTES_PER_S = 6.3e12
MAP_SPP = 8                          # samples a texel of the timed grids' maps: enough for every texel to have a variance


def grid_kernel_resources():
    """kernel_resources.kernel_resources of pt_grid.hip's pack kernel and of the plain lookup's two instantiations
    (grid_lookup_kernel<MAPS, 0, 0>) under the names grid_pack, grid_irradiance_maps and grid_irradiance_plain."""
    return lookup_kernel_resources({"100": "grid_irradiance_maps", "000": "grid_irradiance_plain"}, {"grid_pack_kernel": "grid_pack"})


def lookup_kernel_resources(forms, others):
    """kernel_resources.kernel_resources of pt_grid.hip's kernels under the names asked for: `forms` names instantiations of
    grid_lookup_kernel<MAPS, STATES, OFFSETS> by their three template arguments as digits, `others` the kernels that are no
    templates."""
    from kernel_resources import kernel_resources
    out = {}
    for name, r in kernel_resources("pt_grid", r"(grid_\w+?_kernel)").items():
        t = re.search(r"grid_lookup_kernelILb(\d)ELb(\d)ELb(\d)E", name)
        key = forms.get("".join(t.groups())) if t else others.get(name)
        if key:
            out[key] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scene", choices=("cornell", "mixed", "blob"), default="cornell")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-route", action="store_true", help="time the library's calls only: no torch route, no leak table")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps({"resources": grid_kernel_resources()}))
        return
    import numpy as np
    import torch
    from cudapathtracer_amd import api, rays as R, scenes
    if not torch.cuda.is_available():
        raise SystemExit("grid_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h = a.w, a.h
    m = w * h
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    gen = scenes.blob_in_box if a.scene == "blob" else scenes.cornell
    kw = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4]) if a.scene == "mixed" else {}
    hs = api.HostScene(gen(tempfile.mkdtemp(), width=w, height=h, spp=1, max_depth=8, name="gt", **kw)["config"])
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
    hit = surf.view(torch.int32)[:, 8] >= 0
    floor_ms = round(48.0 * m / HBM_BYTES_PER_S * 1e3, 4)
    res = {"scene": a.scene, "n_tris": hs.info["n_tris"], "w": w, "h": h, "points": m, "hit": int(hit.sum()), "reps": a.reps, "warmup": a.warmup,
           "floor_ms": floor_ms}
    p3, n3 = recs[:, 0:3].contiguous(), recs[:, 4:7].contiguous()

    for side in (8, 16):
        counts = (side, side, side)
        for r in (0, 8, 16):
            g = api.ProbeGrid(sc, glo, ghi, counts, res=r, device=True).bake(64, 1, 4, map_spp=MAP_SPP)
            row = {"packed_mb": round(api.grid_packed_bytes(g.desc) / 1e6, 3)}
            row["pack_ms"] = events(lambda: api.grid_pack(g.desc, g.sums, g.maps))

            def torch_pack():
                e = R._sh_convolved(g.sums, 64)
                return (e, R.oct_border(g.maps[..., :2]) / MAP_SPP) if r else (e, None)
            route = lambda: R.grid_irradiance(glo, ghi, counts, g.sums, 64, p3, n3, g.maps, MAP_SPP if r else None)
            row["lookup_ms"] = events(lambda: g.lookup(recs))
            row["lookup_over_floor"] = round(row["lookup_ms"] / floor_ms, 2)
            res["grid_%d_res_%d" % (side, r)] = row
            if a.no_route:
                continue
            row["pack_torch_ms"] = events(torch_pack)
            row["route_ms"] = events(route)
            row["route_over_lookup"] = round(row["route_ms"] / row["lookup_ms"], 2)
            got, want = g.lookup(recs)[:, :3], route()
            diff = (got - want).abs().max(1).values / want.abs().max()
            row["max_diff_over_max"] = float(diff.max())
            row["share_above_1e-5"] = float((diff > 1e-5).float().mean())
            del g, got, want
            torch.cuda.empty_cache()

    # the leak table of tools/distance_time.py (c), through ProbeGrid and through the Python lookup on the same query outputs
    gx, gz = np.meshgrid(np.linspace(lo[0], hi[0], 13)[1:-1], np.linspace(lo[2], hi[2], 13)[1:-1])
    up = np.tile([(0.0, 1.0, 0.0)], (gx.size, 1))
    s = sc.query_closest(R.irradiance_records(np.stack([gx.ravel(), np.full(gx.size, lo[1] + 0.9 * (hi[1] - lo[1])), gz.ravel()], 1), up), surfaces=True)[1]
    lit = s["light"] >= 0
    if lit.any() and not a.no_route:
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
        with_maps = api.ProbeGrid(sc, glo, ghi, c, res=8, max_t=1.5 * cell).bake(lanes, spl, 8, map_spp=ms)
        without = api.ProbeGrid(sc, glo, ghi, c, res=0).bake(lanes, spl, 8)
        sums, maps = with_maps.sums.astype(np.float64), with_maps.maps.astype(np.float64)
        rnd = lambda v: [round(float(x), 4) for x in v.mean(0)] if len(v) else None
        res["leak"] = {"points": int(len(p)),
                       "probe_grid_without_maps": rnd(without.irradiance(p, nrm)[:, :3].astype(np.float64)),
                       "probe_grid_with_maps": rnd(with_maps.irradiance(p, nrm)[:, :3].astype(np.float64)),
                       "grid_irradiance_without_maps": rnd(R.grid_irradiance(glo, ghi, c, sums, lanes * spl, p, nrm)),
                       "grid_irradiance_with_maps": rnd(R.grid_irradiance(glo, ghi, c, sums, lanes * spl, p, nrm, maps, ms))}
    sc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
