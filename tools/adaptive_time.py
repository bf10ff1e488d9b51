"""Time to equal error: adaptive sampling (pt_render_adaptive) against uniform sample counts on bench.py's 1080p frames.

    python tools/adaptive_time.py [--workloads c2,mixed] [--ref-spp 8192] [--uniform 64,128,256,512,1024]
                                  [--max-spp 1024,4096] [--thresholds 0.3,0.15,0.08,0.04] [--min-spp 16] [--chunk 8] [--reps 2]
                                  [--out FILE.jsonl]
    python tools/adaptive_time.py --denoise [--workloads ..] [--ref-spp ..] [--max-spp ..] [--thresholds ..] [--min-spp ..] [--chunk ..]

Error is relMSE = mean((x - r)^2 / (r^2 + 0.01)) over the rgb values of the pixels where both are finite, x the frame's per-pixel
mean and r a uniform ref-spp frame rendered with another seed. Time is the host clock around each blocking call (host forms, so
both include one frame download), after a warm-up, with the configurations interleaved over `reps` passes; the best pass counts.
One JSON line per configuration, then one summary line per workload: the uniform frame at the largest count, the fastest adaptive
configuration that reaches its relMSE, and the ratio of their times. The per-round bookkeeping kernels (adaptive_*_kernel,
queue_init_list_kernel) are timed by a separate `rocprofv3 --kernel-trace --stats` run of --profile-one (one adaptive render).

--denoise: what the second moment costs and what it buys, at the same configurations (max_spp must be a multiple of 2 * chunk).
Per configuration, interleaved over `reps` passes in one run: the host clock around pt_render_adaptive and around
pt_render_adaptive_moments (best pass each; the second downloads one more frame), and the relMSE of the raw adaptive mean, of
pt_denoise on that mean, of pt_denoise_var_tiles on the adaptive frame, and of pt_denoise_var on a uniform pt_render_moments frame
of the same pixel-sample budget (the mean count rounded to a multiple of the chunk), all with pixel-centre guides. Per workload
one line with the bookkeeping kernel alone (pt_probe_adaptive_moments: HIP events around launches on every tile and on an eighth)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

WORKLOADS = {"c2": "cornell_1920x1080_1024spp_depth8_mis", "mixed": "cornell_mixed_1920x1080_1024spp_depth8_mis"}


def rel_mse(x, r):
    import numpy as np
    x, r = x[..., :3].astype(np.float64), r[..., :3].astype(np.float64)
    ok = np.isfinite(x) & np.isfinite(r)
    return float(np.mean((x[ok] - r[ok]) ** 2 / (r[ok] ** 2 + 0.01)))


def load(workload):
    import bench
    from cudapathtracer_amd import api, scenes
    gen, kw = bench.WORKLOADS[WORKLOADS[workload]]
    info = getattr(scenes, gen)(tempfile.mkdtemp(prefix="adaptive_"), **kw)
    hs = api.HostScene(info["config"])
    return hs, api.Scene(hs), hs.camera(), hs.info["width"], hs.info["height"], hs.info["max_depth"]


def denoise_mode(a, wl, maxes, thresholds, emit):
    import numpy as np
    import torch
    from cudapathtracer_amd import api
    hs, gs, cam, w, h, md = load(wl)
    c = a.chunk
    ref, _ = gs.render(cam, w, h, a.ref_spp, md, seed=api.SEED + 1)
    ref = ref / np.float32(a.ref_spp)
    A, N = gs.render_aovs_centre(cam, w, h)
    T = api.n_tiles(w, h)
    emit({"workload": wl, "moments_kernel_ms_all_tiles": api.probe_adaptive_moments(w, h, T, 50), "tiles": T,
          "moments_kernel_ms_an_eighth": api.probe_adaptive_moments(w, h, max(1, T // 8), 50), "bytes_per_live_pixel": 48})
    gs.render_adaptive(cam, w, h, md, a.min_spp, 4 * c, c, 0.1)                  # warm-up: both entry points' code objects
    gs.render_adaptive_moments(cam, w, h, md, a.min_spp, 4 * c, c, 0.1)
    configs = [(m, t) for m in maxes for t in thresholds]
    best, frames = {}, {}
    for _ in range(a.reps):
        for m, t in configs:
            for kind in ("adaptive", "adaptive_moments"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if kind == "adaptive":
                    gs.render_adaptive(cam, w, h, md, a.min_spp, m, c, t)
                else:
                    frames[(m, t)] = gs.render_adaptive_moments(cam, w, h, md, a.min_spp, m, c, t)
                sec = time.perf_counter() - t0
                best[(kind, m, t)] = min(sec, best.get((kind, m, t), sec))
    for m, t in configs:
        S, Q, tm, _, st = frames[(m, t)]
        mean_spp = st["pixel_samples"] / (w * h)
        uni = max(2 * c, int(round(mean_spp / c)) * c)
        Su, Qu = gs.render_moments(cam, w, h, uni, c, md)
        raw = api.adaptive_mean(S, tm)
        emit({"workload": wl, "max_spp": m, "threshold": t, "min_spp": a.min_spp, "chunk": c, "rounds": st["rounds"],
              "mean_spp": round(mean_spp, 2), "seconds_adaptive": round(best[("adaptive", m, t)], 4),
              "seconds_adaptive_moments": round(best[("adaptive_moments", m, t)], 4),
              "moments_over_adaptive": round(best[("adaptive_moments", m, t)] / best[("adaptive", m, t)], 4),
              "relmse_raw": rel_mse(raw, ref), "relmse_classic_on_mean": rel_mse(api.denoise(raw, 1, A, N), ref),
              "relmse_var_tiles": rel_mse(api.adaptive_mean(api.denoise_var_tiles(S, Q, tm, c, A, N), tm), ref),
              "uniform_spp": uni, "relmse_uniform_raw": rel_mse(Su / np.float32(uni), ref),
              "relmse_uniform_var": rel_mse(api.denoise_var(Su, Qu, uni, uni // c, A, N) / np.float32(uni), ref)})
    gs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,mixed")
    ap.add_argument("--ref-spp", type=int, default=8192)
    ap.add_argument("--uniform", default="64,128,256,512,1024")
    ap.add_argument("--max-spp", default="1024,4096")
    ap.add_argument("--thresholds", default="0.3,0.15,0.08,0.04")
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--denoise", action="store_true", help="pt_render_adaptive_moments + pt_denoise_var_tiles against the alternatives")
    ap.add_argument("--profile-one", default=None, metavar="WORKLOAD:MAX_SPP:THRESHOLD",
                    help="render one adaptive frame and exit (for rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from cudapathtracer_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_time.py needs a HIP device")
    torch.cuda.set_device(0)
    out = open(a.out, "a") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()

    if a.profile_one:
        wl, mx, thr = a.profile_one.split(":")
        hs, gs, cam, w, h, md = load(wl)
        _, spp, _, st = gs.render_adaptive(cam, w, h, md, a.min_spp, int(mx), a.chunk, float(thr))
        emit({"profile_one": a.profile_one, "stats": st, "tiles": int(spp.size)})
        return

    uniform = [int(v) for v in a.uniform.split(",")]
    maxes = [int(v) for v in a.max_spp.split(",")]
    thresholds = [float(v) for v in a.thresholds.split(",")]
    if a.denoise:
        for wl in a.workloads.split(","):
            denoise_mode(a, wl, maxes, thresholds, emit)
        return
    for wl in a.workloads.split(","):
        hs, gs, cam, w, h, md = load(wl)
        t0 = time.perf_counter()
        ref, _ = gs.render(cam, w, h, a.ref_spp, md, seed=api.SEED + 1)
        ref = ref / np.float32(a.ref_spp)
        emit({"workload": wl, "reference_spp": a.ref_spp, "seed": api.SEED + 1, "seconds": time.perf_counter() - t0})
        gs.render(cam, w, h, 8, md)                                          # warm-up: both paths' code objects
        gs.render_adaptive(cam, w, h, md, a.min_spp, 32, a.chunk, 0.1)
        configs = [("uniform", n, None) for n in uniform] + [("adaptive", m, t) for m in maxes for t in thresholds]
        best = {}
        for _ in range(a.reps):
            for kind, n, t in configs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if kind == "uniform":
                    col, _ = gs.render(cam, w, h, n, md)
                    sec = time.perf_counter() - t0
                    res = {"err": rel_mse(col / np.float32(n), ref), "mean_spp": float(n), "rounds": 1}
                else:
                    col, spp, _, st = gs.render_adaptive(cam, w, h, md, a.min_spp, n, a.chunk, t)
                    sec = time.perf_counter() - t0
                    res = {"err": rel_mse(api.adaptive_mean(col, spp), ref), "mean_spp": st["pixel_samples"] / (w * h),
                           "rounds": st["rounds"], "tiles_at_max": st["tiles_at_max"]}
                k = (kind, n, t)
                if k not in best or sec < best[k]["seconds"]:
                    best[k] = dict(res, seconds=sec)
        rows = []
        for (kind, n, t), r in best.items():
            row = {"workload": wl, "kind": kind, "max_spp": n, "threshold": t, "min_spp": a.min_spp if t is not None else None,
                   "chunk": a.chunk if t is not None else None, "seconds": round(r["seconds"], 4), "relmse": r["err"],
                   "mean_spp": round(r["mean_spp"], 2), "rounds": r["rounds"], "tiles_at_max": r.get("tiles_at_max")}
            rows.append(row)
            emit(row)
        top = max(uniform)
        u = best[("uniform", top, None)]
        ok = [r for r in rows if r["kind"] == "adaptive" and r["relmse"] <= u["err"]]
        fast = min(ok, key=lambda r: r["seconds"]) if ok else None
        emit({"workload": wl, "summary": True, "uniform_spp": top, "uniform_seconds": round(u["seconds"], 4), "uniform_relmse": u["err"],
              "adaptive_best": fast, "time_ratio": (fast["seconds"] / u["seconds"]) if fast else None, "goal": 0.7})
        gs.close()


if __name__ == "__main__":
    main()
