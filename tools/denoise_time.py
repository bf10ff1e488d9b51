"""Device time of the feature-buffer pass and of the denoiser at 1920x1080 (HIP events around each, after warm-up).

    python tools/denoise_time.py [--w 1920 --h 1080 --reps 20 --aov-spp 1 --iterations 5 --scene cornell|blob]

Prints one JSON line: median / min milliseconds of pt_render_aovs_device and pt_denoise_device (all iterations), and of the
16-spp depth-8 frame the pair post-processes, for scale."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--aov-spp", type=int, default=1)
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--scene", choices=("cornell", "blob"), default="cornell")
    a = ap.parse_args()
    import torch
    from cudapathtracer_amd import api, scenes
    if not torch.cuda.is_available():
        raise SystemExit("denoise_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h = a.w, a.h
    d = tempfile.mkdtemp()
    gen = scenes.cornell if a.scene == "cornell" else scenes.blob_in_box
    hs = api.HostScene(gen(d, width=w, height=h, spp=16, max_depth=8, name="dt")["config"])
    sc = api.Scene(hs)
    cam = hs.camera()
    colors = torch.zeros(h, w, 4, device="cuda:0")
    sc.launch_unidirectional(8, cam, 16, True, w, h, colors.data_ptr())
    frame_ms = sc.last_kernel_ms()
    alb = torch.empty(h, w, 4, device="cuda:0"); nd = torch.empty(h, w, 4, device="cuda:0")
    ws = torch.empty(api.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    out = torch.empty(h, w, 4, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def aov():
        sc.render_aovs_device(cam, w, h, alb.data_ptr(), nd.data_ptr(), aov_spp=a.aov_spp, stream=stream)

    def dn():
        api.denoise_device(w, h, colors.data_ptr(), 16, alb.data_ptr(), nd.data_ptr(), ws.data_ptr(), out.data_ptr(),
                           iterations=a.iterations, stream=stream)

    res = {"w": w, "h": h, "scene": a.scene, "aov_spp": a.aov_spp, "iterations": a.iterations or api.denoise_defaults()["iterations"],
           "frame_16spp_depth8_ms": round(frame_ms, 3)}
    for name, fn in (("aov", aov), ("denoise", dn)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        res[name + "_ms_median"] = round(ts[len(ts) // 2], 4)
        res[name + "_ms_min"] = round(ts[0], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
