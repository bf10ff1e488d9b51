"""Wall time of one preview frame at 1920x1080: the pt_preview session next to the chain of host calls it replaces, in one run.

    python tools/preview_time.py [--w 1920 --h 1080 --frames 20 --warmup 3 --scale 1 --scene cornell --centre --fused]

Both render the same moving-camera sequence (tests/temporal_seq.py's camera) of the Cornell box with the session's defaults
(4 spp in 2 batches, depth 8, MIS, 1 feature ray, temporal accumulation, the history filter, tone map). The host chain is
render_moments + render_aovs + TemporalHistory.push + denoise_hist + finalise + the tone map, gamma and byte conversion in numpy:
every buffer crosses PCIe, most of them twice. Prints one JSON line: the median and the minimum wall time of a frame for both
(host clock around calls that end in a device synchronise), the session's median stage times from its HIP events, the host
chain's median time per call, and whether the last frames' bytes agree. --scale N runs both at render scale N (the beauty pass at
1 / N of the size in each axis, upsampled by the guides: the host chain then goes through scaled_camera, upsample and
TemporalHistory.push_cur); --scene blob renders the 82 k-triangle blob in the box, whose tree lives in HBM. --centre leaves the host chain out and runs two sessions frame by frame instead, one with centre
guides (pt_preview_set_guide_centre) and one without: `session_*` is the one without, `centre_*` the one with; after the moving
sequence both rest for --frames more frames (`*_resting_*`: the centre session launches no feature pass then). --fused leaves the
host chain out as well and runs two sessions frame by frame, on two scenes that differ in the option "moments_fused": `session_*` is
the one without, `fused_*` the one with (its moments render is one launch); `*_moments_launches` is what pt_last_moments_launches
reported after the last frame, and `bytes_differing` compares the two sessions' last frames."""
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
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--scene", choices=("cornell", "blob"), default="cornell")
    ap.add_argument("--centre", action="store_true")
    ap.add_argument("--fused", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import preview_ref as R
    import temporal_seq as Q
    from cudapathtracer_amd import api, scenes
    if not torch.cuda.is_available():
        raise SystemExit("preview_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h = a.w, a.h
    d = api.preview_defaults()
    spp, batches, depth = d["spp"], d["batches"], d["max_depth"]
    make = scenes.cornell if a.scene == "cornell" else scenes.blob_in_box
    sc = api.Scene(api.HostScene(make(tempfile.mkdtemp(), width=w, height=h, spp=spp, max_depth=depth, name="pvt")["config"]))
    s = a.scale
    n = a.warmup + a.frames
    cams = [Q.camera(api, t, True, w, h) for t in range(n)]
    med = lambda v: round(sorted(v)[len(v) // 2], 4)

    keys = ("render_ms", "aov_ms", "accumulate_ms", "filter_ms", "resolve_ms", "total_ms")
    if a.fused:
        cfg = make(tempfile.mkdtemp(), width=w, height=h, spp=spp, max_depth=depth, name="pvf")["config"]
        scf = api.Scene(api.HostScene(cfg), options={"moments_fused": 1})
        both = {"session": (api.Preview(sc, w, h).set_scale(s), sc), "fused": (api.Preview(scf, w, h).set_scale(s), scf)}
        res = {"w": w, "h": h, "scene": a.scene, "scale": s, "frames": a.frames, "spp": spp, "batches": batches, "max_depth": depth}
        wall, stages = {k: [] for k in both}, {k: [] for k in both}
        for t, cam in enumerate(cams):
            for k, (pv, _) in both.items():
                t0 = time.perf_counter()
                pv.frame(cam, Q.SEED0 + t)
                wall[k].append(1e3 * (time.perf_counter() - t0))
                stages[k].append(pv.stats())
        for k, (pv, scene) in both.items():
            res[k + "_frame_ms_median"] = med(wall[k][a.warmup:]); res[k + "_frame_ms_min"] = round(min(wall[k][a.warmup:]), 4)
            for key in keys:
                res[k + "_" + key + "_median"] = med([st[key] for st in stages[k][a.warmup:]])
            res[k + "_moments_launches"] = scene.last_moments_launches()
        last = [pv.read(mean=False, hist=False, hist_len=False)["rgba8"] for pv, _ in both.values()]
        res["bytes_differing"] = int((last[0] != last[1]).sum())
        print(json.dumps(res))
        for pv, _ in both.values():
            pv.close()
        return
    if a.centre:
        both = {"session": api.Preview(sc, w, h).set_scale(s), "centre": api.Preview(sc, w, h).set_scale(s).set_guide_centre(1)}
        res = {"w": w, "h": h, "scene": a.scene, "scale": s, "frames": a.frames, "spp": spp, "batches": batches, "max_depth": depth}
        for phase, seq in (("", cams), ("_resting", [cams[-1]] * n)):
            wall, stages = {k: [] for k in both}, {k: [] for k in both}
            for t, cam in enumerate(seq):
                for k, pv in both.items():
                    t0 = time.perf_counter()
                    pv.frame(cam, Q.SEED0 + t)
                    wall[k].append(1e3 * (time.perf_counter() - t0))
                    stages[k].append(pv.stats())
            for k in both:
                res[k + phase + "_frame_ms_median"] = med(wall[k][a.warmup:])
                for key in keys:
                    res[k + phase + "_" + key + "_median"] = med([st[key] for st in stages[k][a.warmup:]])
        res["centre_guide_passes"] = both["centre"].guide_passes; res["session_guide_passes"] = both["session"].guide_passes
        print(json.dumps(res))
        for pv in both.values():
            pv.close()
        return
    pv = api.Preview(sc, w, h).set_scale(s)
    wall, stages = [], []
    for t in range(n):
        t0 = time.perf_counter()
        pv.frame(cams[t], Q.SEED0 + t)                    # blocks until the frame is on the device
        wall.append(1e3 * (time.perf_counter() - t0))
        stages.append(pv.stats())
    session8 = pv.read(mean=False, hist=False, hist_len=False)["rgba8"]
    pv.close()
    res = {"w": w, "h": h, "scene": a.scene, "scale": s, "frames": a.frames, "spp": spp, "batches": batches, "max_depth": depth,
           "session_frame_ms_median": med(wall[a.warmup:]), "session_frame_ms_min": round(min(wall[a.warmup:]), 4)}
    for k in ("render_ms", "aov_ms", "accumulate_ms", "filter_ms", "resolve_ms", "total_ms"):
        res["session_" + k + "_median"] = med([s[k] for s in stages[a.warmup:]])

    th = api.TemporalHistory(w, h)
    wall, parts = [], {k: [] for k in ("render_moments", "render_aovs", "push", "denoise_hist", "finalise", "bytes_numpy")}
    for t in range(n):
        marks = [time.perf_counter()]
        lo = api.scaled_camera(cams[t], s)
        S, Qs = sc.render_moments(lo, w // s, h // s, spp, spp // batches, depth, seed=Q.SEED0 + t); marks.append(time.perf_counter())
        A, N = sc.render_aovs(cams[t], w, h, aov_spp=1, seed=Q.SEED0 + t)
        if s > 1:
            Al, Nl = sc.render_aovs(lo, w // s, h // s, aov_spp=1, seed=Q.SEED0 + t)
        marks.append(time.perf_counter())
        if s > 1:
            hist = th.push_cur(cams[t], api.upsample(s, S, Qs, spp, batches, Al, Nl, A, N), N)
        else:
            hist = th.push(cams[t], S, Qs, spp, batches, A, N)
        marks.append(time.perf_counter())
        filt = api.denoise_hist(hist, A, N); marks.append(time.perf_counter())
        mean = api.finalise(filt, 1); marks.append(time.perf_counter())
        host8 = R.display(mean); marks.append(time.perf_counter())
        wall.append(1e3 * (marks[-1] - marks[0]))
        for k, (m0, m1) in zip(parts, zip(marks, marks[1:])):
            parts[k].append(1e3 * (m1 - m0))
    res["host_chain_frame_ms_median"] = med(wall[a.warmup:]); res["host_chain_frame_ms_min"] = round(min(wall[a.warmup:]), 4)
    for k, v in parts.items():
        res["host_" + k + "_ms_median"] = med(v[a.warmup:])
    diff = np.abs(session8.astype(np.int32) - host8.astype(np.int32))
    res["bytes_differing"] = int((diff > 0).sum()); res["bytes_max_difference"] = int(diff.max())
    res["speedup"] = round(res["host_chain_frame_ms_median"] / res["session_frame_ms_median"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
