"""What the responsive history costs, in one run.

    python tools/respond_time.py [--w 1920 --h 1080 --reps 20 --warmup 3 --frames 20 --parts stage,preview] [--resources]

(a) stage: pt_temporal_accumulate_respond_device next to pt_temporal_accumulate_device / pt_temporal_accumulate_cur_device on the same
    buffers (two frames of the Cornell box, the second blended into the first's history): still and moving camera, the sums and the
    `cur` form, radius 1..3. HIP events around each call, median of --reps after --warmup. The base stage moves 120 B a pixel
    (§11); the pair about 276 B: the gather reads as the base and writes 36 B, the walk reads 36 + 16 + 48 and writes 20 to 24.
(b) preview: the animated preview of tools/motion_time.py (the 82 k blob, every vertex moved through the device form before each
    frame, keep_history 1) with the option on and off: median wall time of update + scene_changed + frame, and accumulate_ms.
--resources prints the two kernels' registers, scratch and LDS from the code-object notes and needs no GPU. Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

# What the compile gives, in the hardware's allocation granule of 8; tests/test_respond_api.py pins them.
GATHER_VGPRS, WALK_VGPRS = 48, 64


def respond_kernel_resources():
    """kernel_resources.kernel_resources of pt_temporal.hip's two respond kernels: {mangled instantiation: dict}, ten entries."""
    from kernel_resources import kernel_resources
    return {**kernel_resources("pt_temporal", "(temporal_gather_kernel)"), **kernel_resources("pt_temporal", "(temporal_respond_kernel)")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--parts", default="stage,preview")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps(respond_kernel_resources()))
        return
    import numpy as np
    import torch
    import temporal_seq as Q
    from cudapathtracer_amd import api, scenes
    if not torch.cuda.is_available():
        raise SystemExit("respond_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h = a.w, a.h
    parts = a.parts.split(",")
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    res = {"w": w, "h": h, "reps": a.reps, "warmup": a.warmup}

    def host(maker, name):
        return api.HostScene(maker(tempfile.mkdtemp(), width=w, height=h, spp=4, max_depth=8, name="rt_" + name)["config"])

    def timed(run):
        ms = []
        for _ in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(torch.cuda.default_stream()); run(); e1.record(torch.cuda.default_stream())
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return med(ms[a.warmup:])

    if "stage" in parts:
        sc = api.Scene.from_mesh(host(scenes.cornell, "cornell"))
        f4 = lambda: torch.empty(h, w, 4, device="cuda:0")
        f1 = lambda: torch.empty(h, w, device="cuda:0")
        S, Qs, A, N0, N1, H0, H1, cur = (f4() for _ in range(8))
        L0, L1, lam = f1(), f1(), f1()
        ws = torch.empty(api.temporal_respond_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
        stage = {}
        for moving in (False, True):
            c0, c1 = Q.camera(api, 0, moving, w, h), Q.camera(api, 1, moving, w, h)
            sc.render_moments_device(c0, w, h, 4, 2, 8, S.data_ptr(), Qs.data_ptr(), seed=Q.SEED0)
            sc.render_aovs_centre_device(c0, w, h, 0, A.data_ptr(), N0.data_ptr())
            api.temporal_accumulate_device(w, h, c0, None, S.data_ptr(), Qs.data_ptr(), 4, 2, A.data_ptr(), N0.data_ptr(), 0, 0, 0, H0.data_ptr(),
                                           L0.data_ptr())
            sc.render_moments_device(c1, w, h, 4, 2, 8, S.data_ptr(), Qs.data_ptr(), seed=Q.SEED0 + 1)
            sc.render_aovs_centre_device(c1, w, h, 0, A.data_ptr(), N1.data_ptr())
            api.temporal_accumulate_cur_device(w, h, c1, None, S.data_ptr(), N1.data_ptr(), 0, 0, 0, cur.data_ptr(), L1.data_ptr())  # any (e, V) will do
            torch.cuda.synchronize()
            hist = (N0.data_ptr(), H0.data_ptr(), L0.data_ptr())
            for form in ("sums", "cur"):
                sums = (S.data_ptr(), Qs.data_ptr(), 4, 2, A.data_ptr()) if form == "sums" else (0, 0, 0, 0, 0)
                e = 0 if form == "sums" else cur.data_ptr()
                if form == "sums":
                    base = lambda: api.temporal_accumulate_device(w, h, c1, c0, *sums, N1.data_ptr(), *hist, H1.data_ptr(), L1.data_ptr())
                else:
                    base = lambda: api.temporal_accumulate_cur_device(w, h, c1, c0, e, N1.data_ptr(), *hist, H1.data_ptr(), L1.data_ptr())
                row = {"base_ms": timed(base)}
                for r in (1, 2, 3):
                    on = lambda: api.temporal_accumulate_respond_device(w, h, c1, c0, *sums, e, N1.data_ptr(), *hist, 0, ws.data_ptr(), H1.data_ptr(),
                                                                        L1.data_ptr(), lam.data_ptr(), radius=r)
                    row["respond_r%d_ms" % r] = timed(on)
                    row["r%d_over_base" % r] = round(row["respond_r%d_ms" % r] / row["base_ms"], 3)
                row["short_share"] = round(float((lam < 1).float().mean().item()), 5)
                stage["%s_%s" % ("moving" if moving else "still", form)] = row
        res["stage"] = stage
        sc.close()

    if "preview" in parts:
        blob = host(scenes.blob_in_box, "blob")

        def displaced(phase):                                 # (tools/motion_time.py's animation)
            p = blob.array("points").view(np.float32).reshape(-1, 4).copy()
            p[:, 2] += (0.02 * np.sin(7.0 * p[:, 0] + 3.0 * p[:, 1] + phase)).astype(np.float32)
            return p

        dev = [torch.from_numpy(displaced(ph)).cuda() for ph in (0.0, 1.3)]
        cam = Q.camera(api, 0, True, w, h)
        pvr = {}
        for name, on in (("off", False), ("on", True)):
            sc = api.Scene.from_mesh(blob)
            pv = api.Preview(sc, w, h)
            if on:
                pv.set_respond()
            wall, acc = [], []
            for t in range(a.warmup + a.frames):
                t0 = time.perf_counter()
                sc.update_vertices(dev[t & 1])
                pv.scene_changed(True)
                pv.frame(cam, Q.SEED0 + t)
                wall.append(1e3 * (time.perf_counter() - t0)); acc.append(pv.stats()["accumulate_ms"])
            m = med(wall[a.warmup:])
            pvr[name] = {"frame_ms": m, "fps": round(1e3 / m, 1), "accumulate_ms": med(acc[a.warmup:])}
            pv.close(); sc.close()
        pvr["frame_ms_difference"] = round(pvr["on"]["frame_ms"] - pvr["off"]["frame_ms"], 4)
        res["preview_blob"] = {"frames": a.frames, **pvr}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
