"""What a radiance query costs next to the render it reproduces, in one run.

    python tools/radiance_time.py [--scene cornell|mixed|blob --w 1920 --h 1080 --spp 16 --depth 8 --reps 7 --warmup 2]
    python tools/radiance_time.py --resources      (no device needed: compiles pt_radiance.hip and prints its kernels' registers, scratch and LDS)

HIP events around each call, the median of --reps after --warmup (as tools/query_time.py takes them), for both integrators:
  render        pt_render_tiles_device's kernel (pt_last_kernel_ms) for cam0, the scene's camera without jitter and aperture
  centre        pt_query_radiance_device on cam0's centre rays, streams 0 .. w*h - 1: the same image, bit for bit (checked here)
  shuffled      the same rays in a random order, each with its stream in its pad word (PT_QUERY_STREAM_PAD): the same paths, but a
                wave's lanes hold rays from all over the frame
  panorama      a 2048 x 1024 equirectangular panorama from the middle of the box (cudapathtracer_amd/rays.py)
`cornell` is the plain box (the SIMPLE kernel), `mixed` bench.py --full's mixed Cornell box (LEAN), `blob` the 82 k blob in the box.
The library holds each kernel at one waves-per-SIMD setting (pt_feature_host.h: radiance_waves_per_simd); --resources shows what
that setting compiled to. Prints one JSON line."""
import argparse
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def radiance_kernel_resources():
    """kernel_resources.kernel_resources of pt_radiance.hip's six kernels under the names radiance_<mis|naive>_<simple|lean|generic>."""
    from kernel_resources import kernel_resources
    out = {}
    for name, r in kernel_resources("pt_radiance", r"(radiance_kernel)").items():
        m = re.search(r"radiance_kernelILi(\d)ELb(\d)ELb(\d)E", name)
        out["radiance_%s_%s" % ("naive" if m.group(1) == "2" else "mis", "simple" if m.group(2) == "1" else "lean" if m.group(3) == "1" else "generic")] = r
    return out


def declared_waves():
    """{kernel name as above: the waves per SIMD pt_feature_host.h launches it at}, read from radiance_waves_per_simd's line."""
    src = open(os.path.join(ROOT, "cudapathtracer_amd", "csrc", "pt_feature_host.h")).read()
    m = re.search(r"radiance_waves_per_simd\(int integrator, bool simple, bool lean\) \{ return simple \? (\d) : lean \? (\d) : (\d); \}", src)
    s, l, g = (int(v) for v in m.groups())
    return {"radiance_%s_%s" % (i, k): v for i in ("naive", "mis") for k, v in (("simple", s), ("lean", l), ("generic", g))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scene", choices=("cornell", "mixed", "blob"), default="cornell")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps({"resources": radiance_kernel_resources(), "waves_per_simd": declared_waves()}))
        return
    import numpy as np
    import torch
    from cudapathtracer_amd import api, rays as R, scenes
    if not torch.cuda.is_available():
        raise SystemExit("radiance_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h, spp, depth = a.w, a.h, a.spp, a.depth
    n = w * h
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    gen = scenes.blob_in_box if a.scene == "blob" else scenes.cornell
    kw = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4]) if a.scene == "mixed" else {}
    hs = api.HostScene(gen(tempfile.mkdtemp(), width=w, height=h, spp=spp, max_depth=depth, name="rt", **kw)["config"])
    sc = api.Scene(hs)
    cam0 = api.Camera.frombytes(hs.camera().tobytes())
    cam0.antiAliasJitterDist = 0.0
    cam0.aperture = 0.0
    stream = torch.cuda.current_stream().cuda_stream

    def events(run):
        ms = []
        for _ in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); run(); e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return med(ms[a.warmup:])

    centre = sc.query_camera_rays(cam0, w, h)
    g = torch.Generator(device="cuda:0"); g.manual_seed(7)
    order = torch.randperm(n, generator=g, device="cuda:0")
    shuffled = centre[order].contiguous()
    shuffled.view(torch.int32)[:, 7] = order.to(torch.int32)
    pts = np.ascontiguousarray(hs.array("points")).view(np.float32).reshape(-1, 4)[:, :3]
    pano = R.panorama_rays(tuple(0.5 * (pts.min(0) + pts.max(0))), 2048, 1024, device="cuda:0")
    from cudapathtracer_amd import distributed as D
    tiles = torch.zeros(D.padded_tile_count(w, h, 1), 64, 4, device="cuda:0")
    frame = torch.zeros(h, w, 4, device="cuda:0")
    res = {"w": w, "h": h, "scene": a.scene, "n_tris": hs.info["n_tris"], "rays": n, "spp": spp, "depth": depth, "reps": a.reps, "warmup": a.warmup}
    for integ, name in ((api.UNIDIRECTIONAL, "mis"), (api.NAIVE_UNIDIRECTIONAL, "naive")):
        row = {}
        ms = []
        for _ in range(a.warmup + a.reps):
            tiles.zero_()
            sc.render_tiles_device(cam0, w, h, spp, depth, tiles.data_ptr(), integrator=integ, stream=stream)
            torch.cuda.synchronize()
            ms.append(sc.last_kernel_ms())
        row["render_kernel_ms"] = med(ms[a.warmup:])
        row["render_flags"] = [k for k, v in sc.flags().items() if v]
        row["centre_ms"] = events(lambda: sc.query_radiance(centre, spp, depth, integrator=integ))
        row["shuffled_ms"] = events(lambda: sc.query_radiance(shuffled, spp, depth, integrator=integ, stream_pad=True))
        row["panorama_ms"] = events(lambda: sc.query_radiance(pano, spp, depth, integrator=integ))
        row["centre_over_render"] = round(row["centre_ms"] / row["render_kernel_ms"], 3)
        row["shuffled_over_centre"] = round(row["shuffled_ms"] / row["centre_ms"], 3)
        row["panorama_mrays"] = round(2048 * 1024 * spp / row["panorama_ms"] / 1e3, 1)       # camera rays x samples per second
        # the three images are one image
        got = sc.query_radiance(centre, spp, depth, integrator=integ)
        back = torch.empty_like(got)
        back[order] = sc.query_radiance(shuffled, spp, depth, integrator=integ, stream_pad=True)
        tiles.zero_()
        sc.render_tiles_device(cam0, w, h, spp, depth, tiles.data_ptr(), integrator=integ, stream=stream)
        D.assemble_device([tiles], w, h, 1, frame, stream)
        torch.cuda.synchronize()
        row["centre_is_render"] = bool(torch.equal(got.view(torch.int32)[:, :3], frame.reshape(n, 4).view(torch.int32)[:, :3]))
        row["shuffled_is_centre"] = bool(torch.equal(got.view(torch.int32), back.view(torch.int32)))
        res[name] = row
    sc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
