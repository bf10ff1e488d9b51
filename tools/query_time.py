"""What a ray query costs, in one run.

    python tools/query_time.py [--w 1920 --h 1080 --reps 20 --warmup 3 --scene cornell|mixed|blob --parts coherent,incoherent,probe]
    python tools/query_time.py --resources      (no device needed: compiles pt_query.hip and prints its kernels' registers, scratch and LDS)

HIP events around each call, median of --reps after --warmup, and Mray/s for the w*h rays.
(a) coherent: the centre rays, made by pt_query_camera_rays_device. pt_query_closest_device (hits only, and with surfaces) and
    pt_query_shadow_device next to pt_render_aovs_centre_device and pt_render_ids_device, which trace the same rays.
(b) incoherent: origins = the centre pass's hit points + normal * EPS, directions cosine-distributed about the normal (torch ops, a
    generator with a fixed seed; a pixel without a hit gets its centre ray), max_t = a tenth of the scene's diagonal. Closest and
    shadow, unordered next to PT_QUERY_REORDER, and next to the same rays sorted into the key order beforehand ("presorted": the trace
    kernel alone on that order); *_keys_sort_ms = reordered - presorted: the key kernel, the sort and the gather through the order.
    These rays come pixel by pixel, so their origins are already neighbours; "shuffled" is the same set in a random order, again
    unordered next to PT_QUERY_REORDER.
(c) probe: Scene.trace_closest (the old host path: allocations, copies, the counting traversal) on the incoherent rays, wall clock.
`cornell` is the plain box, `mixed` bench.py --full's mixed Cornell box, `blob` the 82 k blob in the box. Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

EPS = 1e-4


def query_kernel_resources():
    """kernel_resources.kernel_resources of pt_query.hip's kernels under short names: query_closest_kernel (hits only),
    query_closest_surface_kernel (the SURFACE instantiation), query_shadow_kernel, query_camera_rays_kernel, query_keys_kernel."""
    from kernel_resources import kernel_resources
    out = {}
    for name, r in kernel_resources("pt_query", r"(query\w*?_kernel)").items():
        if "query_closest_kernel" in name:
            name = "query_closest_surface_kernel" if "ILb1E" in name else "query_closest_kernel"
        out[name] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scene", choices=("cornell", "mixed", "blob"), default="cornell")
    ap.add_argument("--parts", default="coherent,incoherent,probe")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps(query_kernel_resources()))
        return
    import numpy as np
    import torch
    from cudapathtracer_amd import api, scenes
    if not torch.cuda.is_available():
        raise SystemExit("query_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h, parts = a.w, a.h, a.parts.split(",")
    n = w * h
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    mrays = lambda ms: round(n / ms / 1e3, 1)
    gen = scenes.blob_in_box if a.scene == "blob" else scenes.cornell
    kw = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4]) if a.scene == "mixed" else {}
    hs = api.HostScene(gen(tempfile.mkdtemp(), width=w, height=h, spp=4, max_depth=8, name="qt", **kw)["config"])
    sc = api.Scene(hs)
    cam = hs.camera()
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

    def timed(row, name, run):
        row[name + "_ms"] = events(run)
        row[name + "_mrays"] = mrays(row[name + "_ms"])

    res = {"w": w, "h": h, "scene": a.scene, "n_tris": hs.info["n_tris"], "rays": n, "reps": a.reps, "warmup": a.warmup}
    A, N = torch.empty(h, w, 4, device="cuda:0"), torch.empty(h, w, 4, device="cuda:0")
    ids = torch.empty(h, w, 4, dtype=torch.int32, device="cuda:0")
    rays = sc.query_camera_rays(cam, w, h)
    if "coherent" in parts:
        row = {}
        timed(row, "camera_rays", lambda: api.query_camera_rays(cam, w, h, out=rays))
        timed(row, "aovs_centre", lambda: sc.render_aovs_centre_device(cam, w, h, 0, A.data_ptr(), N.data_ptr(), stream=stream))
        timed(row, "ids", lambda: sc.render_ids_device(cam, w, h, 0, ids.data_ptr(), stream=stream))
        timed(row, "closest", lambda: sc.query_closest(rays))
        timed(row, "closest_surfaces", lambda: sc.query_closest(rays, surfaces=True))
        timed(row, "shadow", lambda: sc.query_shadow(rays))
        row["closest_over_centre"] = round(row["closest_ms"] / row["aovs_centre_ms"], 3)
        row["closest_surfaces_over_centre"] = round(row["closest_surfaces_ms"] / row["aovs_centre_ms"], 3)
        res["coherent"] = row
    if "incoherent" in parts or "probe" in parts:
        sc.render_aovs_centre_device(cam, w, h, 0, A.data_ptr(), N.data_ptr(), stream=stream)
        hits = sc.query_closest(rays)
        g = torch.Generator(device="cuda:0"); g.manual_seed(7)
        u = torch.rand(n, 2, generator=g, device="cuda:0")
        nrm = N.reshape(n, 4)[:, :3]
        valid = hits.view(torch.int32)[:, 3] >= 0
        # a frame about the normal, then Malley's cosine-distributed direction in it
        up = torch.where(nrm[:, :1].abs() < 0.9, torch.tensor([1.0, 0.0, 0.0], device="cuda:0"), torch.tensor([0.0, 1.0, 0.0], device="cuda:0"))
        tx = torch.nn.functional.normalize(torch.linalg.cross(up.expand(n, 3), nrm), dim=1)
        ty = torch.linalg.cross(nrm, tx)
        r, phi = u[:, :1].sqrt(), 2.0 * np.pi * u[:, 1:]
        d = tx * (r * phi.cos()) + ty * (r * phi.sin()) + nrm * (1.0 - u[:, :1]).clamp_min(0.0).sqrt()
        o = rays[:, 0:3] + rays[:, 4:7] * hits[:, :1] + nrm * EPS
        pts = np.ascontiguousarray(hs.array("points")).view(np.float32).reshape(-1, 4)[:, :3]
        diag = float(np.linalg.norm(pts.max(0) - pts.min(0)))
        inc = rays.clone()
        inc[valid, 0:3] = o[valid]
        inc[valid, 4:7] = d[valid]
        inc_shadow = inc.clone()
        inc_shadow[:, 3] = 0.1 * diag
        torch.cuda.synchronize()
        res["incoherent_rays"] = {"secondary_share": round(float(valid.float().mean().item()), 4), "shadow_max_t": round(0.1 * diag, 4)}
    if "incoherent" in parts:
        row = {}
        timed(row, "closest", lambda: sc.query_closest(inc))
        timed(row, "closest_reorder", lambda: sc.query_closest(inc, reorder=True))
        timed(row, "shadow", lambda: sc.query_shadow(inc_shadow))
        timed(row, "shadow_reorder", lambda: sc.query_shadow(inc_shadow, reorder=True))
        # the key kernel + the sort (+ the gather through perm) separately: the same rays put into the library's key order by torch
        # beforehand (the key restated here: octant << 27 | Morton code of the origin's 9-bit cells in the scene's bounds) and traced
        # unordered are the trace kernel alone on that order; what a reordered call takes beyond it is the ordering itself
        lo, ext = torch.tensor(pts.min(0), device="cuda:0"), torch.tensor(pts.max(0) - pts.min(0), device="cuda:0")
        cell = ((inc[:, 0:3] - lo) / ext * 512.0).clamp(0.0, 511.0).to(torch.int64)
        key = ((inc[:, 4] < 0).long() | ((inc[:, 5] < 0).long() << 1) | ((inc[:, 6] < 0).long() << 2)) << 27
        for b in range(9):
            for c in range(3):
                key |= ((cell[:, c] >> b) & 1) << (3 * b + c)
        order = torch.argsort(key, stable=True)
        pre, pre_shadow = inc[order].contiguous(), inc_shadow[order].contiguous()
        timed(row, "closest_presorted", lambda: sc.query_closest(pre))
        timed(row, "shadow_presorted", lambda: sc.query_shadow(pre_shadow))
        row["closest_keys_sort_ms"] = round(row["closest_reorder_ms"] - row["closest_presorted_ms"], 4)
        row["shadow_keys_sort_ms"] = round(row["shadow_reorder_ms"] - row["shadow_presorted_ms"], 4)
        # the same rays in a random order: what a caller's buffer looks like when its rays do not come pixel by pixel
        shuffle = torch.randperm(n, generator=g, device="cuda:0")
        shuf, shuf_shadow = inc[shuffle].contiguous(), inc_shadow[shuffle].contiguous()
        timed(row, "closest_shuffled", lambda: sc.query_closest(shuf))
        timed(row, "closest_shuffled_reorder", lambda: sc.query_closest(shuf, reorder=True))
        timed(row, "shadow_shuffled", lambda: sc.query_shadow(shuf_shadow))
        timed(row, "shadow_shuffled_reorder", lambda: sc.query_shadow(shuf_shadow, reorder=True))
        row["closest_shuffled_reorder_over_unordered"] = round(row["closest_shuffled_reorder_ms"] / row["closest_shuffled_ms"], 3)
        row["shadow_shuffled_reorder_over_unordered"] = round(row["shadow_shuffled_reorder_ms"] / row["shadow_shuffled_ms"], 3)
        row["closest_reorder_over_unordered"] =round(row["closest_reorder_ms"] / row["closest_ms"], 3)
        row["shadow_reorder_over_unordered"] = round(row["shadow_reorder_ms"] / row["shadow_ms"], 3)
        res["incoherent"] = row
    if "probe" in parts:
        host = inc.cpu().numpy()[:, [0, 1, 2, 4, 5, 6]].copy()
        ms = []
        for _ in range(2):
            t0 = time.perf_counter(); sc.trace_closest(host)
            ms.append(1e3 * (time.perf_counter() - t0))
        res["probe"] = {"trace_closest_wall_ms": round(min(ms), 3), "trace_closest_mrays": mrays(min(ms))}
        t0 = time.perf_counter(); sc.query_closest(inc.cpu().numpy())
        res["probe"]["query_closest_host_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    sc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
