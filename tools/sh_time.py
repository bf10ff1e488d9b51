"""What an SH query costs next to the routes a probe baker had before it, in one run.

    python tools/sh_time.py [--scene cornell|mixed|blob --records 1024 --samples 1024 --depth 8 --reps 5 --warmup 1]
    python tools/sh_time.py --resources    (no device needed: compiles pt_sh.hip and prints its kernels' registers, scratch and LDS)

HIP events around each call, the median of --reps after --warmup (as tools/irradiance_time.py takes them), for both integrators:
  (a) lanes_64, lanes_256, lanes_1024   pt_query_sh_device on --records probes at --samples samples each, spp_lane = samples / lanes.
                                        The probes are a regular grid in the middle half of the scene's bounding box
      rays_route                        the route without the call, its device part only: pt_query_sh_rays_device's records * samples
                                        rays (a baker draws and uploads them, 32 bytes each, which is not timed) through
                                        pt_query_radiance_device at spp = 1 with PT_QUERY_STREAM_PAD, and a torch projection and sum
      irradiance_lanes_64               §26 (a)'s yardstick: pt_query_irradiance_device on as many records at 64 lanes, facing up
  (b) grid_lanes_8, _64, _256           a 16 x 16 x 16 grid at 256 samples a probe
  (c) one_sample_sh, _irradiance        the same number of lanes with one sample each at 64 lanes a record through sh_kernel (3 waves
                                        per SIMD) and through irradiance_kernel (the class's 4 to 6)
  (d) floor_check                       (--scene cornell) rays.sh_irradiance of a probe 1 mm above the floor's centre at the floor's
                                        normal, next to pt_query_irradiance there at the same sample count: printed, not asserted
`cornell` is the plain box (the SIMPLE kernel), `mixed` bench.py --full's mixed Cornell box (LEAN), `blob` the 82 k blob in the box.
Prints one JSON line."""
import argparse
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def sh_kernel_resources():
    """kernel_resources.kernel_resources of pt_sh.hip's six walk kernels under the names sh_<mis|naive>_<simple|lean|generic>."""
    from kernel_resources import kernel_resources
    out = {}
    for name, r in kernel_resources("pt_sh", r"(sh_kernel)").items():
        m = re.search(r"sh_kernelILi(\d)ELb(\d)ELb(\d)E", name)
        out["sh_%s_%s" % ("naive" if m.group(1) == "2" else "mis", "simple" if m.group(2) == "1" else "lean" if m.group(3) == "1" else "generic")] = r
    return out


def declared_waves():
    """{kernel name as above: the waves per SIMD pt_feature_host.h launches it at}: sh_waves_per_simd is the smaller of
    radiance_waves_per_simd, whose line tools/radiance_time.py reads, and the cap its own line names."""
    import radiance_time
    src = open(os.path.join(ROOT, "cudapathtracer_amd", "csrc", "pt_feature_host.h")).read()
    m = re.search(r"sh_waves_per_simd\(int integrator, bool simple, bool lean\) \{ return std::min\(radiance_waves_per_simd\(integrator, simple, lean\), (\d)\); \}", src)
    return {k.replace("radiance", "sh"): min(v, int(m.group(1))) for k, v in radiance_time.declared_waves().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scene", choices=("cornell", "mixed", "blob"), default="cornell")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps({"resources": sh_kernel_resources(), "waves_per_simd": declared_waves()}))
        return
    import numpy as np
    import torch
    from cudapathtracer_amd import api, rays as R, scenes
    if not torch.cuda.is_available():
        raise SystemExit("sh_time.py needs a HIP device")
    if a.samples % 1024 or a.samples < 1024:
        raise SystemExit("--samples must be a multiple of 1024")
    torch.cuda.set_device(0)
    n, spp, depth = a.records, a.samples, a.depth
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    gen = scenes.blob_in_box if a.scene == "blob" else scenes.cornell
    kw = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4]) if a.scene == "mixed" else {}
    hs = api.HostScene(gen(tempfile.mkdtemp(), width=32, height=32, spp=1, max_depth=depth, name="st", **kw)["config"])
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
    mid, half = 0.5 * (lo + hi), 0.25 * (hi - lo)
    side = max(1, round(n ** (1.0 / 3.0)))
    grid = R.sh_grid(mid - half, mid + half, (side, side, side), device="cuda:0")
    recs = grid[torch.arange(n, device=grid.device) % grid.shape[0]].contiguous()
    up = recs.clone()
    up[:, 5] = 1.0                                                          # the yardstick's records: the same points, facing +y
    res = {"scene": a.scene, "n_tris": hs.info["n_tris"], "records": n, "samples": spp, "depth": depth, "reps": a.reps, "warmup": a.warmup}
    # (a)'s route: samples / 1024 copies of every probe, copy j of probe i with pad = i * copies + j, emitted on 1024 lanes
    copies = spp // 1024
    wide = recs.repeat_interleave(copies, 0).contiguous()
    wide.view(torch.int32)[:, 7] = torch.arange(n * copies, device=wide.device, dtype=torch.int32)
    emitted = sc.query_sh_rays(wide, 1024, flags=api.QUERY_STREAM_PAD)
    basis = R.sh_basis(emitted[:, 4:7])                                     # [n * spp, 9]
    # (b)'s grid and (c)'s lanes
    grid16 = R.sh_grid(mid - half, mid + half, (16, 16, 16), device="cuda:0")
    one = recs[torch.arange(max(1, n * spp // 64), device=recs.device) % n].contiguous()
    one_up = one.clone()
    one_up[:, 5] = 1.0
    for integ, name in ((api.UNIDIRECTIONAL, "mis"), (api.NAIVE_UNIDIRECTIONAL, "naive")):
        row = {}
        for lanes in (64, 256, 1024):
            row["lanes_%d_ms" % lanes] = events(lambda: sc.query_sh(recs, lanes, spp // lanes, depth, integrator=integ))

        def route():
            li = sc.query_radiance(emitted, 1, depth, integrator=integ, stream_pad=True)[:, :3]
            return (li[:, None, :] * basis[:, :, None]).view(n, spp, 9, 3).sum(1)

        row["rays_route_ms"] = events(route)
        row["irradiance_lanes_64_ms"] = events(lambda: sc.query_irradiance(up, 64, spp // 64, depth, integrator=integ))
        for lanes in (64, 256, 1024):
            row["route_over_lanes_%d" % lanes] = round(row["rays_route_ms"] / row["lanes_%d_ms" % lanes], 3)
        row["route_over_irradiance_lanes_64"] = round(row["rays_route_ms"] / row["irradiance_lanes_64_ms"], 3)
        row["msamples_per_s_lanes_1024"] = round(n * spp / row["lanes_1024_ms"] / 1e3, 1)
        # the same light either way: band 0 of both estimates, averaged over the probes, agrees to sampling noise
        got = sc.query_sh(recs, 1024, spp // 1024, depth, integrator=integ)[:, 0, :3].mean().item() / spp
        row["mean_band0_lanes_1024"], row["mean_band0_route"] = round(got, 5), round(route()[:, 0].mean().item() / spp, 5)
        for lanes in (8, 64, 256):
            row["grid_lanes_%d_ms" % lanes] = events(lambda: sc.query_sh(grid16, lanes, 256 // lanes, depth, integrator=integ))
        row["one_sample_sh_ms"] = events(lambda: sc.query_sh(one, 64, 1, depth, integrator=integ))
        row["one_sample_irradiance_ms"] = events(lambda: sc.query_irradiance(one_up, 64, 1, depth, integrator=integ))
        row["one_sample_sh_over_irradiance"] = round(row["one_sample_sh_ms"] / row["one_sample_irradiance_ms"], 3)
        res[name] = row
    if a.scene == "cornell":
        p = np.array([[mid[0], lo[1] + 0.001, mid[2]]], np.float32)
        up1 = np.array([[0.0, 1.0, 0.0]], np.float32)
        sums = sc.query_sh(R.sh_records(p), 1024, spp // 1024 * 16, depth)
        irr = sc.query_irradiance(R.irradiance_records(p, up1), 64, spp // 64 * 16, depth)
        res["floor_check"] = {"samples": spp * 16, "sh_irradiance": [round(float(v), 4) for v in R.sh_irradiance(sums, spp * 16, up1)[0, 0]],
                              "query_irradiance": [round(float(v), 4) for v in np.pi * irr[0, :3] / (spp * 16)]}
    sc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
