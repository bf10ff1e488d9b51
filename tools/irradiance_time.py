"""What an irradiance query costs next to the route a baker had before it, in one run.

    python tools/irradiance_time.py [--scene cornell|mixed|blob --records 1024 --samples 1024 --depth 8 --reps 5 --warmup 1]
    python tools/irradiance_time.py --resources    (no device needed: compiles pt_irradiance.hip and prints its kernels' registers, scratch and LDS)

HIP events around each call, the median of --reps after --warmup (as tools/radiance_time.py takes them), for both integrators:
  lanes_1, lanes_8, lanes_64    pt_query_irradiance_device on --records records at --samples samples each, spp_lane = samples / lanes.
                                The records are the surfaces under the centre rays of a 32 x 32 frame of the scene's camera
  rays_route                    the route without the call, its device part only: the records * samples rays (here made by
                                pt_query_irradiance_rays_device, every ray on a stream of its own; a baker draws and uploads them,
                                32 bytes each, which is not timed) through pt_query_radiance_device at spp = 1 with
                                PT_QUERY_STREAM_PAD, and a torch sum over each record's rows
  lightmap                      (--scene cornell) a 256 x 256 lightmap of the floor: the records from pt_query_closest on an orthographic
                                sensor just above it, 64 samples a texel on 8 lanes with moments, pt_query_guides on the same rays,
                                and pt_denoise_var_device on the pair
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


def irradiance_kernel_resources():
    """kernel_resources.kernel_resources of pt_irradiance.hip's six walk kernels under the names
    irradiance_<mis|naive>_<simple|lean|generic>."""
    from kernel_resources import kernel_resources
    out = {}
    for name, r in kernel_resources("pt_irradiance", r"(irradiance_kernel)").items():
        m = re.search(r"irradiance_kernelILi(\d)ELb(\d)ELb(\d)E", name)
        out["irradiance_%s_%s" % ("naive" if m.group(1) == "2" else "mis", "simple" if m.group(2) == "1" else "lean" if m.group(3) == "1" else "generic")] = r
    return out


def declared_waves():
    """{kernel name as above: the waves per SIMD pt_feature_host.h launches it at}: irradiance_waves_per_simd hands on
    radiance_waves_per_simd, whose line tools/radiance_time.py reads."""
    import radiance_time
    src = open(os.path.join(ROOT, "cudapathtracer_amd", "csrc", "pt_feature_host.h")).read()
    assert re.search(r"irradiance_waves_per_simd\(int integrator, bool simple, bool lean\) \{ return radiance_waves_per_simd\(integrator, simple, lean\); \}", src)
    return {k.replace("radiance", "irradiance"): v for k, v in radiance_time.declared_waves().items()}


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
        print(json.dumps({"resources": irradiance_kernel_resources(), "waves_per_simd": declared_waves()}))
        return
    import numpy as np
    import torch
    from cudapathtracer_amd import api, rays as R, scenes
    if not torch.cuda.is_available():
        raise SystemExit("irradiance_time.py needs a HIP device")
    if a.samples % 64 or a.samples < 64:
        raise SystemExit("--samples must be a multiple of 64")
    torch.cuda.set_device(0)
    n, spp, depth = a.records, a.samples, a.depth
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    gen = scenes.blob_in_box if a.scene == "blob" else scenes.cornell
    kw = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4]) if a.scene == "mixed" else {}
    hs = api.HostScene(gen(tempfile.mkdtemp(), width=32, height=32, spp=1, max_depth=depth, name="it", **kw)["config"])
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

    # the records: the surfaces the camera sees, cycled up to n
    _, surf = sc.query_closest(sc.query_camera_rays(cam0, 32, 32), surfaces=True)
    seen = R.records_from_surfaces(surf)
    seen = seen[seen[:, 3] > 0]
    recs = seen[torch.arange(n, device=seen.device) % seen.shape[0]].contiguous()
    # the route without the call: spp / 64 copies of every record, copy j of record i with pad = i * (spp / 64) + j, emitted on 64 lanes
    copies = spp // 64
    wide = recs.repeat_interleave(copies, 0).contiguous()
    wide.view(torch.int32)[:, 7] = torch.arange(n * copies, device=wide.device, dtype=torch.int32)
    emitted = sc.query_irradiance_rays(wide, 64, flags=api.QUERY_STREAM_PAD)
    res = {"scene": a.scene, "n_tris": hs.info["n_tris"], "records": n, "samples": spp, "depth": depth, "reps": a.reps, "warmup": a.warmup,
           "distinct_records": int(seen.shape[0])}
    for integ, name in ((api.UNIDIRECTIONAL, "mis"), (api.NAIVE_UNIDIRECTIONAL, "naive")):
        row = {}
        for lanes in (1, 8, 64):
            row["lanes_%d_ms" % lanes] = events(lambda: sc.query_irradiance(recs, lanes, spp // lanes, depth, integrator=integ))
        route = lambda: sc.query_radiance(emitted, 1, depth, integrator=integ, stream_pad=True).view(n, spp, 4).sum(1)
        row["rays_route_ms"] = events(route)
        row["route_over_lanes_64"] = round(row["rays_route_ms"] / row["lanes_64_ms"], 3)
        row["lanes_1_over_lanes_64"] = round(row["lanes_1_ms"] / row["lanes_64_ms"], 3)
        row["lanes_8_over_lanes_64"] = round(row["lanes_8_ms"] / row["lanes_64_ms"], 3)
        row["msamples_per_s_lanes_64"] = round(n * spp / row["lanes_64_ms"] / 1e3, 1)
        # the same light either way: the means of the two estimates over all records agree to sampling noise
        got = sc.query_irradiance(recs, 64, spp // 64, depth, integrator=integ)[:, :3].mean().item() / spp
        row["mean_li_lanes_64"], row["mean_li_route"] = round(got, 5), round(route()[:, :3].mean().item() / spp, 5)
        res[name] = row
    if a.scene == "cornell":
        w = h = 256
        pts = np.ascontiguousarray(hs.array("points")).view(np.float32).reshape(-1, 4)[:, :3]
        lo, hi = pts.min(0), pts.max(0)
        down = R.orthographic_rays((0.5 * (lo[0] + hi[0]), lo[1] + 0.02, 0.5 * (lo[2] + hi[2])), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0),
                                   float(hi[0] - lo[0]), float(hi[2] - lo[2]), w, h, device="cuda:0")
        lanes, spp_lane = 8, 8
        work = torch.empty(api.denoise_var_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
        out = torch.empty(w * h, 4, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        box = {}

        def lightmap():
            _, sf = sc.query_closest(down, surfaces=True)
            texels = R.records_from_surfaces(sf)
            s, q = sc.query_irradiance(texels, lanes, spp_lane, depth, moments=True)
            alb, nd = sc.query_guides(down)
            api.denoise_var_device(w, h, s.data_ptr(), q.data_ptr(), lanes * spp_lane, lanes, alb.data_ptr(), nd.data_ptr(), work.data_ptr(),
                                   out.data_ptr(), stream=stream)
            box["s"], box["texels"] = s, texels

        row = {"w": w, "h": h, "lanes": lanes, "spp_lane": spp_lane, "total_ms": events(lightmap)}
        row["irradiance_ms"] = events(lambda: sc.query_irradiance(box["texels"], lanes, spp_lane, depth, moments=True))
        row["texels_on_a_surface"] = int((box["texels"][:, 3] > 0).sum().item())
        raw, den = box["s"][:, :3] / (lanes * spp_lane), out[:, :3] / (lanes * spp_lane)
        row["mean_raw"], row["mean_denoised"] = round(raw.mean().item(), 5), round(den.mean().item(), 5)
        # the filter's effect: the mean absolute difference between horizontally neighbouring texels, before and after
        grid = lambda t: t.view(h, w, 3)
        row["neighbour_diff_raw"] = round((grid(raw)[:, 1:] - grid(raw)[:, :-1]).abs().mean().item(), 5)
        row["neighbour_diff_denoised"] = round((grid(den)[:, 1:] - grid(den)[:, :-1]).abs().mean().item(), 5)
        res["lightmap"] = row
    sc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
