"""What a distance-probe query costs next to the route a probe baker had before it, in one run.

    python tools/distance_time.py [--scene cornell|mixed|blob --records 1024 --spp 4 --reps 5 --warmup 1]
    python tools/distance_time.py --resources    (no device needed: compiles pt_distance.hip and prints its kernels' registers, scratch and LDS)

HIP events around each call, the median of --reps after --warmup (as tools/sh_time.py takes them):
  (a) res_8, res_16, jittered and centre   pt_query_distance_device on --records probes (a regular grid in the middle half of the
                                           scene's bounding box, max_t = the box's diagonal), jittered at --spp samples a texel
      route                                the device part of the route without the call: per sample pt_query_distance_rays_device's
                                           rays (a baker draws and uploads them, 32 bytes each, which costs more), then
                                           pt_query_closest_device with surfaces, then a torch reduce to the four sums
  (b) grid_spp_1, grid_spp_4               a 16 x 16 x 16 grid at res 8
  (c) leak                                 printed, not asserted: an 8 x 8 x 8 grid of SH and distance probes over the scene, and floor
                                           points in the occluder's shadow (a shadow ray to the emitter's centre is blocked):
                                           rays.grid_irradiance there without and with the maps, next to pt_query_irradiance at the
                                           same points, each the mean over the points
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


def distance_kernel_resources():
    """kernel_resources.kernel_resources of pt_distance.hip's two trace kernels under the names distance_jittered and distance_centre."""
    from kernel_resources import kernel_resources
    out = {}
    for name, r in kernel_resources("pt_distance", r"(distance_kernel)").items():
        out["distance_centre" if re.search(r"distance_kernelILb(\d)E", name).group(1) == "1" else "distance_jittered"] = r
    return out


def declared_waves():
    """{kernel name as above: the waves per SIMD pt_feature_host.h launches it at}."""
    src = open(os.path.join(ROOT, "cudapathtracer_amd", "csrc", "pt_feature_host.h")).read()
    return {"distance_jittered": int(re.search(r"constexpr int kDistanceWavesPerSimd = (\d);", src).group(1)),
            "distance_centre": int(re.search(r"constexpr int kDistanceCentreWavesPerSimd = (\d);", src).group(1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scene", choices=("cornell", "mixed", "blob"), default="cornell")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps({"resources": distance_kernel_resources(), "waves_per_simd": declared_waves()}))
        return
    import numpy as np
    import torch
    from cudapathtracer_amd import api, rays as R, scenes
    if not torch.cuda.is_available():
        raise SystemExit("distance_time.py needs a HIP device")
    torch.cuda.set_device(0)
    n, spp = a.records, a.spp
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    gen = scenes.blob_in_box if a.scene == "blob" else scenes.cornell
    kw = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4]) if a.scene == "mixed" else {}
    hs = api.HostScene(gen(tempfile.mkdtemp(), width=32, height=32, spp=1, max_depth=8, name="dt", **kw)["config"])
    sc = api.Scene(hs)

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
    mid, half, diag = 0.5 * (lo + hi), 0.25 * (hi - lo), float(np.linalg.norm(hi - lo))
    side = max(1, round(n ** (1.0 / 3.0)))
    grid = R.sh_grid(mid - half, mid + half, (side, side, side), max_t=diag, device="cuda:0")
    recs = grid[torch.arange(n, device=grid.device) % grid.shape[0]].contiguous()
    res = {"scene": a.scene, "n_tris": hs.info["n_tris"], "records": n, "spp": spp, "reps": a.reps, "warmup": a.warmup}

    def route(r, samples, flags):
        m = n * r * r
        acc = torch.zeros((m, 4), device=recs.device)
        for j in range(samples):
            off = torch.full((m,), 2 * j, dtype=torch.int32, device=recs.device) if j else None
            rays = sc.query_distance_rays(recs, r, draw_offset=off, flags=flags)
            hits, surf = sc.query_closest(rays, surfaces=True)
            hit = hits.view(torch.int32)[:, 3] >= 0
            d = torch.where(hit, hits[:, 0], rays[:, 3])
            back = hit & (surf.view(torch.int32)[:, 10] != 0)
            acc = acc + torch.stack([d, d * d, hit.float(), back.float()], 1)
        return acc.view(n, r, r, 4)

    for r in (8, 16):
        for mode, flags, samples in (("jittered", 0, spp), ("centre", api.QUERY_TEXEL_CENTRE, 1)):
            row = {"samples_a_texel": samples}
            row["query_ms"] = events(lambda: sc.query_distance(recs, r, samples, flags=flags))
            row["route_ms"] = events(lambda: route(r, samples, flags))
            row["route_over_query"] = round(row["route_ms"] / row["query_ms"], 3)
            row["mrays_per_s"] = round(n * r * r * samples / row["query_ms"] / 1e3, 1)
            got, want = sc.query_distance(recs, r, samples, flags=flags), route(r, samples, flags)
            row["same_bits"] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
            res["res_%d_%s" % (r, mode)] = row
    grid16 = R.sh_grid(mid - half, mid + half, (16, 16, 16), max_t=diag, device="cuda:0")
    for s in (1, 4):
        res["grid_spp_%d_ms" % s] = events(lambda: sc.query_distance(grid16, 8, s))

    # (c) floor points the emitter's centre does not see, and the probes around them
    gx, gz = np.meshgrid(np.linspace(lo[0], hi[0], 13)[1:-1], np.linspace(lo[2], hi[2], 13)[1:-1])
    up = np.tile([(0.0, 1.0, 0.0)], (gx.size, 1))
    surf = sc.query_closest(R.irradiance_records(np.stack([gx.ravel(), np.full(gx.size, lo[1] + 0.9 * (hi[1] - lo[1])), gz.ravel()], 1), up), surfaces=True)[1]
    lit = surf["light"] >= 0
    if lit.any():
        light = np.array([surf["px"][lit].mean(), surf["py"][lit].mean(), surf["pz"][lit].mean()])
        fx, fz = np.meshgrid(np.linspace(lo[0], hi[0], 34)[1:-1], np.linspace(lo[2], hi[2], 34)[1:-1])
        floor = np.stack([fx.ravel(), np.full(fx.size, lo[1] + 1e-4), fz.ravel()], 1).astype(np.float32)      # (below the boxes' bottoms, 1 mm up)
        to = light[None, :] - floor
        dist = np.linalg.norm(to, axis=1)
        sh = R.irradiance_records(floor, to / dist[:, None])
        sh[:, 3] = dist - 1e-2
        blocked = ~sc.query_shadow(sh)[:, :3].any(1)
        clear = sc.query_closest(R.irradiance_records(floor, np.tile([(0.0, 1.0, 0.0)], (len(floor), 1))))["t"] > 0.05      # not under the occluder itself
        p = floor[blocked & clear]
        nrm = np.tile(np.array([(0.0, 1.0, 0.0)], np.float32), (len(p), 1))
        c, lanes, spl, ms = (8, 8, 8), 256, 16, 16
        inset = 0.02 * (hi - lo)
        glo, ghi = lo + inset, hi - inset
        cell = float(np.linalg.norm((ghi - glo) / 7.0))
        sums = sc.query_sh(R.sh_grid(glo, ghi, c), lanes, spl, 8).astype(np.float64)
        maps = sc.query_distance(R.sh_grid(glo, ghi, c, max_t=1.5 * cell), 8, ms).astype(np.float64)
        plain = R.grid_irradiance(glo, ghi, c, sums, lanes * spl, p, nrm)
        seen = R.grid_irradiance(glo, ghi, c, sums, lanes * spl, p, nrm, maps, ms)
        truth = np.pi * sc.query_irradiance(R.irradiance_records(p, nrm), 64, 64, 8)[:, :3] / 4096.0
        rnd = lambda v: [round(float(x), 4) for x in v.mean(0)] if len(v) else None
        res["leak"] = {"points": int(len(p)), "grid_irradiance_without_maps": rnd(plain), "grid_irradiance_with_maps": rnd(seen),
                       "query_irradiance": rnd(truth)}
    sc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
