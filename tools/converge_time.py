"""What a resting camera costs with and without converged tiles: two pt_preview sessions side by side at 1920x1080.

    python tools/converge_time.py [--w 1920 --h 1080 --frames 64 --scene cornell --ref-spp 1024 --threshold T --min-history N --centre --fused]

Both sessions render the same still camera (tests/temporal_seq.py's) with the session's defaults (4 spp in 2 batches, depth 8,
MIS, 1 feature ray, temporal accumulation, the history filter, tone map) and the same seeds; one of them has
pt_preview_set_converge on, at the library's defaults unless --threshold / --min-history say otherwise. Per frame one line: the
live share of the converging session, its stage times from the session's HIP events, and the wall-clock time of the frame for
both (host clock around a call that ends in a device synchronise). At the end one JSON line: the medians over the frames from
min_history on, both sessions' MSE of the displayed mean against a --ref-spp render with another seed (over the pixels that are
finite in all three), and the share of pixel-samples that were not rendered. --scene blob renders the 82 k-triangle blob in the
box, whose tree lives in HBM. --centre gives BOTH sessions centre guides (pt_preview_set_guide_centre): a resting camera then
launches no feature pass at all, so compare aov_ms and the frame times with a run without the flag. --fused sets the option
"moments_fused" on the sessions' scene (every moments render, on a tile list or not, is one launch; `moments_launches` is what
pt_last_moments_launches reported after the last frame): compare with a run without the flag."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--scene", choices=("cornell", "blob"), default="cornell")
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--min-history", type=int, default=None)
    ap.add_argument("--centre", action="store_true")
    ap.add_argument("--fused", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import temporal_seq as Q
    from cudapathtracer_amd import api, scenes
    if not torch.cuda.is_available():
        raise SystemExit("converge_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h = a.w, a.h
    d = api.preview_defaults()
    spp, batches, depth = d["spp"], d["batches"], d["max_depth"]
    c = api.converge_defaults()
    thr = c["threshold"] if a.threshold is None else a.threshold
    mh = c["min_history"] if a.min_history is None else a.min_history
    make = scenes.cornell if a.scene == "cornell" else scenes.blob_in_box
    sc = api.Scene(api.HostScene(make(tempfile.mkdtemp(), width=w, height=h, spp=spp, max_depth=depth, name="cvt")["config"]))
    if a.fused:
        sc.set_option("moments_fused", 1)
    cam = Q.camera(api, 0, False, w, h)
    conv, plain = api.Preview(sc, w, h).set_converge(thr, mh), api.Preview(sc, w, h)
    if a.centre:
        conv.set_guide_centre(1); plain.set_guide_centre(1)
    keys = ("render_ms", "aov_ms", "accumulate_ms", "filter_ms", "resolve_ms", "total_ms")
    rows = []
    print("frame live_share " + " ".join(keys) + " | wall_ms converging, not converging")
    for t in range(a.frames):
        wall = []
        for pv in (conv, plain):
            t0 = time.perf_counter()
            pv.frame(cam, Q.SEED0 + t)                    # blocks until the frame is on the device
            wall.append(1e3 * (time.perf_counter() - t0))
        live, total = conv.last_live()
        st = conv.stats()
        rows.append((live / total, [st[k] for k in keys], wall, plain.stats()["total_ms"]))
        print("%3d %.4f %s | %.3f %.3f" % (t, live / total, " ".join("%.3f" % st[k] for k in keys), wall[0], wall[1]), flush=True)
    ref = api.finalise(sc.render(cam, w, h, a.ref_spp, depth, seed=Q.REF_SEED)[0], a.ref_spp)
    got, base = conv.read(rgba8=False, hist=False, hist_len=False)["mean"], plain.read(rgba8=False, hist=False, hist_len=False)["mean"]
    ok = np.isfinite(ref[..., :3]).all(-1) & np.isfinite(got[..., :3]).all(-1) & np.isfinite(base[..., :3]).all(-1)
    mse = lambda x: float(((x[..., :3].astype(np.float64) - ref[..., :3])[ok] ** 2).mean())
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    tail = rows[min(mh, len(rows) - 1):]
    res = {"w": w, "h": h, "scene": a.scene, "frames": a.frames, "spp": spp, "batches": batches, "max_depth": depth, "threshold": thr,
           "min_history": mh, "ref_spp": a.ref_spp, "centre": int(a.centre), "guide_passes": conv.guide_passes,
           "fused": int(a.fused), "moments_launches": sc.last_moments_launches(),
           "live_share_last": round(rows[-1][0], 4), "live_share_mean": round(sum(r[0] for r in rows) / len(rows), 4),
           "pixel_samples_saved": round(1.0 - sum(r[0] for r in rows) / len(rows), 4),
           "converging_frame_ms_median": med([r[2][0] for r in tail]), "converging_frame_ms_last": round(rows[-1][2][0], 4),
           "plain_frame_ms_median": med([r[2][1] for r in tail]), "plain_total_ms_median": med([r[3] for r in tail]),
           "mse_converging": mse(got), "mse_plain": mse(base)}
    for i, k in enumerate(keys):
        res["converging_" + k + "_median"] = med([r[1][i] for r in tail])
    res["mse_ratio"] = round(res["mse_converging"] / res["mse_plain"], 4) if res["mse_plain"] > 0 else None
    print(json.dumps(res))
    conv.close(); plain.close(); sc.close()


if __name__ == "__main__":
    main()
