"""What a denoisable image made of a caller's own rays costs, stage by stage.

    python tools/query_image_time.py [--scene cornell|mixed|blob --w 1920 --h 1080 --spp 16 --batches 4 --depth 8 --reps 7 --warmup 2]
    python tools/query_image_time.py --resources      (no device needed: compiles the two new units and prints their kernels' numbers)

HIP events around each call, the median of --reps after --warmup (as tools/radiance_time.py takes them):
  (a) moments     query_radiance_moments next to query_radiance on the same cam0 centre rays, both integrators: the cost of Q. The
                  tool checks that S is query_radiance's output and (S, Q) render_moments' pair, bit for bit
  (b) guides      query_guides at max_links 0 and 4 next to render_aovs_centre_device on the same camera, checked bit for bit
  (c) panorama    2048 x 1024 from the middle of the scene's bounds (cudapathtracer_amd/rays.py): moments, guides (4 links) and
                  denoise_var_device, each stage's ms, and the mean squared error of the raw and of the filtered mean against a
                  query of --long-spp samples per ray (a figure, not a check)
`cornell` is the plain box (the SIMPLE kernels), `mixed` bench.py --full's mixed Cornell box (LEAN), `blob` the 82 k blob in the box.
Prints one JSON line."""
import argparse
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def radiance_moments_kernel_resources():
    """kernel_resources.kernel_resources of pt_radiance_moments.hip's six kernels under the names
    radiance_moments_<mis|naive>_<simple|lean|generic>."""
    from kernel_resources import kernel_resources
    out = {}
    for name, r in kernel_resources("pt_radiance_moments", r"(radiance_moments_kernel)").items():
        m = re.search(r"radiance_moments_kernelILi(\d)ELb(\d)ELb(\d)E", name)
        out["radiance_moments_%s_%s" % ("naive" if m.group(1) == "2" else "mis", "simple" if m.group(2) == "1" else "lean" if m.group(3) == "1" else "generic")] = r
    return out


def guides_kernel_resources():
    """The same of pt_query_guides.hip's two kernels, under their own names."""
    from kernel_resources import kernel_resources
    return kernel_resources("pt_query_guides", r"(query_guides\w*?_kernel)")


def declared_waves():
    """{kernel name as above: the waves per SIMD pt_feature_host.h launches it at}, read from radiance_moments_waves_per_simd's line
    and the two constants of the guides kernels."""
    src = open(os.path.join(ROOT, "cudapathtracer_amd", "csrc", "pt_feature_host.h")).read()
    m = re.search(r"radiance_moments_waves_per_simd\(int integrator, bool simple, bool lean\) \{ return simple \? (\d) : lean \? (\d) : (\d); \}", src)
    s, l, g = (int(v) for v in m.groups())
    out = {"radiance_moments_%s_%s" % (i, k): v for i in ("naive", "mis") for k, v in (("simple", s), ("lean", l), ("generic", g))}
    out["query_guides_kernel"] = int(re.search(r"kQueryGuidesWavesPerSimd = (\d);", src).group(1))
    out["query_guides_chain_kernel"] = int(re.search(r"kQueryGuidesChainWavesPerSimd = (\d);", src).group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--long-spp", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scene", choices=("cornell", "mixed", "blob"), default="cornell")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps({"resources": dict(radiance_moments_kernel_resources(), **guides_kernel_resources()), "waves_per_simd": declared_waves()}))
        return
    import numpy as np
    import torch
    from cudapathtracer_amd import api, rays as R, scenes
    if not torch.cuda.is_available():
        raise SystemExit("query_image_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h, spp, depth = a.w, a.h, a.spp, a.depth
    c = spp // a.batches
    n = w * h
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    gen = scenes.blob_in_box if a.scene == "blob" else scenes.cornell
    kw = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4]) if a.scene == "mixed" else {}
    hs = api.HostScene(gen(tempfile.mkdtemp(), width=w, height=h, spp=spp, max_depth=depth, name="qit", **kw)["config"])
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

    bits = lambda t: t.view(torch.int32)
    centre = sc.query_camera_rays(cam0, w, h)
    res = {"w": w, "h": h, "scene": a.scene, "n_tris": hs.info["n_tris"], "rays": n, "spp": spp, "batches": a.batches, "depth": depth,
           "reps": a.reps, "warmup": a.warmup}
    # (a) the cost of Q
    dS, dQ = torch.zeros(h, w, 4, device="cuda:0"), torch.zeros(h, w, 4, device="cuda:0")
    for integ, name in ((api.UNIDIRECTIONAL, "mis"), (api.NAIVE_UNIDIRECTIONAL, "naive")):
        row = {}
        row["radiance_ms"] = events(lambda: sc.query_radiance(centre, spp, depth, integrator=integ))
        row["moments_ms"] = events(lambda: sc.query_radiance_moments(centre, spp, c, depth, integrator=integ))
        row["moments_over_radiance"] = round(row["moments_ms"] / row["radiance_ms"], 3)
        S, Q = sc.query_radiance_moments(centre, spp, c, depth, integrator=integ)
        row["s_is_radiance"] = bool(torch.equal(bits(S), bits(sc.query_radiance(centre, spp, depth, integrator=integ))))
        sc.render_moments_device(cam0, w, h, spp, c, depth, dS.data_ptr(), dQ.data_ptr(), integrator=integ, stream=stream)
        torch.cuda.synchronize()
        row["is_render_moments"] = bool(torch.equal(bits(S)[:, :3], bits(dS).reshape(n, 4)[:, :3]) and torch.equal(bits(Q), bits(dQ).reshape(n, 4)))
        res[name] = row
    # (b) the guides next to the camera's centre pass
    A, N, L = torch.zeros(n, 4, device="cuda:0"), torch.zeros(n, 4, device="cuda:0"), torch.zeros(n, device="cuda:0")
    for links in (0, 4):
        row = {}
        row["render_aovs_centre_ms"] = events(lambda: sc.render_aovs_centre_device(cam0, w, h, links, A.data_ptr(), N.data_ptr(), L.data_ptr() if links else 0, stream))
        row["query_guides_ms"] = events(lambda: sc.query_guides(centre, links, links=links > 0))
        row["query_over_render"] = round(row["query_guides_ms"] / row["render_aovs_centre_ms"], 3)
        sc.render_aovs_centre_device(cam0, w, h, links, A.data_ptr(), N.data_ptr(), L.data_ptr(), stream)
        qa, qn, ql = sc.query_guides(centre, links, links=True)
        torch.cuda.synchronize()
        row["is_render_aovs_centre"] = bool(torch.equal(bits(qa), bits(A)) and torch.equal(bits(qn), bits(N)) and torch.equal(bits(ql), bits(L)))
        res["guides_links_%d" % links] = row
    # (c) a panorama, stage by stage
    pw, ph = 2048, 1024
    pts = np.ascontiguousarray(hs.array("points")).view(np.float32).reshape(-1, 4)[:, :3]
    pano = R.panorama_rays(tuple(0.5 * (pts.min(0) + pts.max(0))), pw, ph, device="cuda:0")
    ws = torch.zeros(api.denoise_var_workspace_bytes(pw, ph), dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(ph, pw, 4, device="cuda:0")
    keep = {}
    row = {"w": pw, "h": ph}
    row["moments_ms"] = events(lambda: keep.__setitem__("sq", sc.query_radiance_moments(pano, spp, c, depth)))
    row["guides_ms"] = events(lambda: keep.__setitem__("an", sc.query_guides(pano, 4)))
    (S, Q), (ga, gn) = keep["sq"], keep["an"]
    row["denoise_var_ms"] = events(lambda: api.denoise_var_device(pw, ph, S.data_ptr(), Q.data_ptr(), spp, a.batches, ga.data_ptr(), gn.data_ptr(),
                                                                  ws.data_ptr(), out.data_ptr(), stream=stream))
    row["total_ms"] = round(row["moments_ms"] + row["guides_ms"] + row["denoise_var_ms"], 4)
    long = sc.query_radiance(pano, a.long_spp, depth, seed=api.SEED + 1)[:, :3].double() / a.long_spp
    torch.cuda.synchronize()
    row["long_spp"] = a.long_spp
    raw, filt = S[:, :3].double() / spp, out.reshape(-1, 4)[:, :3].double() / spp                    # (the filter returns a sum)
    ok = torch.isfinite(long).all(1) & torch.isfinite(raw).all(1) & torch.isfinite(filt).all(1)      # (the path's arithmetic has no NaN guard)
    row["non_finite_rays"] = int((~ok).sum())
    row["mse_raw"] = float(((raw[ok] - long[ok]) ** 2).mean())
    row["mse_filtered"] = float(((filt[ok] - long[ok]) ** 2).mean())
    res["panorama"] = row
    sc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
