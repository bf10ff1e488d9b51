"""Device time of the feature-buffer pass and of the denoiser at 1920x1080 (HIP events around each, after warm-up).

    python tools/denoise_time.py [--w 1920 --h 1080 --reps 20 --aov-spp 1 --iterations 5 --scene cornell|mixed|blob --max-links 8 --centre]
    python tools/denoise_time.py --resources          (no device needed: compiles pt_aov.hip and pt_denoise.hip and prints their
                                                       kernels' registers, scratch and LDS)

Prints one JSON line: median / min milliseconds of pt_render_aovs_device, of pt_render_aovs_chain_device (`aov_chain`: the pass that
follows mirrors and glass, --max-links links; on `cornell` no ray has a chain, `mixed` is bench.py --full's mixed Cornell box with
a mirror box, a glass box around a water box and a gold box), of pt_denoise_device and pt_denoise_var_device (all
iterations; --iterations sets both, otherwise the variance-guided filter is timed at the classic filter's count and at its own
default), of pt_denoise_var_tiles_device (`denoise_var_tiles`: the `denoise_var` row's buffers and count with a uniform map of 16
samples in batches of 4) and pt_denoise_hist_device (`denoise_hist`: the same frame's (e, V) as a first-frame history, the same
count), of the 16-spp depth-8 frame they post-process in one launch (the megakernel's device time, and the launcher's wall
time), of the same frame as a moments render of 4 batches of 4 and of 2 batches of 8 (pt_render_moments_device: wall time, it
blocks), of both again with the scene's option "moments_fused" on (`*_fused_wall`: one launch that keeps the squared batch sums
itself; `*_fused_launches` is what pt_last_moments_launches reported, 1 unless the kernel has no fused twin) and as
pt_launch_progressive in 4 chunks (the same launches without the bookkeeping), and the device time of a 4-spp launch. --centre times only the four feature passes, in one run: pt_render_aovs_centre_device with max_links 0 (`aov_centre`) and
with --max-links (`aov_centre_chain`) next to the jittered `aov` and `aov_chain`."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def aov_kernel_resources():
    """kernel_resources.kernel_resources of pt_aov.hip's feature-pass kernels (jittered and centre), by kernel name."""
    from kernel_resources import kernel_resources
    return kernel_resources("pt_aov", r"(aov\w*?_kernel)")


def denoise_kernel_resources():
    """kernel_resources.kernel_resources of pt_denoise.hip's kernels: the instantiations of the three templates and the reduction."""
    from kernel_resources import kernel_resources
    return kernel_resources("pt_denoise", r"(dn_\w+?_kernel|denoise_reduce_kernel)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--aov-spp", type=int, default=1)
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--scene", choices=("cornell", "mixed", "blob"), default="cornell")
    ap.add_argument("--max-links", type=int, default=8)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--centre", action="store_true")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps(dict(aov_kernel_resources(), **denoise_kernel_resources())))
        return
    import torch
    from cudapathtracer_amd import api, scenes
    if not torch.cuda.is_available():
        raise SystemExit("denoise_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h = a.w, a.h
    d = tempfile.mkdtemp()
    gen = scenes.blob_in_box if a.scene == "blob" else scenes.cornell
    kw = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4]) if a.scene == "mixed" else {}
    hs = api.HostScene(gen(d, width=w, height=h, spp=16, max_depth=8, name="dt", **kw)["config"])
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

    lnk = torch.empty(h, w, device="cuda:0")

    def aov_chain():
        sc.render_aovs_chain_device(cam, w, h, a.max_links, alb.data_ptr(), nd.data_ptr(), lnk.data_ptr(), aov_spp=a.aov_spp, stream=stream)

    alb_c = torch.empty(h, w, 4, device="cuda:0"); nd_c = torch.empty(h, w, 4, device="cuda:0")      # the centre passes' own buffers

    def aov_centre():
        sc.render_aovs_centre_device(cam, w, h, 0, alb_c.data_ptr(), nd_c.data_ptr(), stream=stream)

    def aov_centre_chain():
        sc.render_aovs_centre_device(cam, w, h, a.max_links, alb_c.data_ptr(), nd_c.data_ptr(), lnk.data_ptr(), stream=stream)

    iters = a.iterations or api.denoise_defaults()["iterations"]
    iters_var = a.iterations or api.denoise_var_defaults()["iterations"]

    def dn():
        api.denoise_device(w, h, colors.data_ptr(), 16, alb.data_ptr(), nd.data_ptr(), ws.data_ptr(), out.data_ptr(),
                           iterations=iters, stream=stream)

    sq = torch.empty(h, w, 4, device="cuda:0")
    ws_var = torch.empty(api.denoise_var_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")

    def dn_var(n):
        api.denoise_var_device(w, h, colors.data_ptr(), sq.data_ptr(), 16, 4, alb.data_ptr(), nd.data_ptr(), ws_var.data_ptr(), out.data_ptr(),
                               iterations=n, stream=stream)

    tile_spp = torch.full(((h + 7) // 8, (w + 7) // 8), 16, dtype=torch.int32, device="cuda:0")     # a uniform map: denoise_var's frame

    def dn_var_tiles():
        api.denoise_var_tiles_device(w, h, colors.data_ptr(), sq.data_ptr(), tile_spp.data_ptr(), 4, alb.data_ptr(), nd.data_ptr(),
                                     ws_var.data_ptr(), out.data_ptr(), iterations=iters, stream=stream)

    hist = torch.empty(h, w, 4, device="cuda:0"); hist_len = torch.empty(h, w, device="cuda:0")

    def dn_hist():
        api.denoise_hist_device(w, h, hist.data_ptr(), alb.data_ptr(), nd.data_ptr(), ws_var.data_ptr(), out.data_ptr(), iterations=iters,
                                stream=stream)

    # the frame in one launch and as 4 batches of 4: both calls block, so wall time on the host (median of --reps after warm-up)
    def one_launch():
        colors.zero_()
        sc.launch_unidirectional(8, cam, 16, True, w, h, colors.data_ptr())

    def moments(c, fused=0):
        def run():
            sc.set_option("moments_fused", fused)
            sc.render_moments_device(cam, w, h, 16, c, 8, colors.data_ptr(), sq.data_ptr(), stream=stream)
            sc.set_option("moments_fused", 0)
        return run

    def progressive():                                    # the same four launches without the bookkeeping
        colors.zero_()
        sc.launch_progressive(0, 8, cam, 16, True, w, h, colors.data_ptr(), 4)

    res = {"w": w, "h": h, "scene": a.scene, "aov_spp": a.aov_spp, "iterations": iters, "iterations_var_default": iters_var,
           "frame_16spp_depth8_ms": round(frame_ms, 3)}
    colors.zero_()
    sc.launch_unidirectional(8, cam, 4, True, w, h, colors.data_ptr())
    res["frame_4spp_depth8_ms"] = round(sc.last_kernel_ms(), 3)       # what one batch of four costs on the device
    for name, fn in () if a.centre else (("frame_16spp_one_launch_wall", one_launch), ("frame_16spp_moments_4x4_wall", moments(4)),
                                         ("frame_16spp_moments_2x8_wall", moments(8)), ("frame_16spp_moments_4x4_fused_wall", moments(4, 1)),
                                         ("frame_16spp_moments_2x8_fused_wall", moments(8, 1)), ("frame_16spp_progressive_4x4_wall", progressive)):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        res[name + "_ms_median"] = round(ts[len(ts) // 2], 3)
        res[name + "_ms_min"] = round(ts[0], 3)
        if name.endswith("_fused_wall"):
            res[name[:-5] + "_launches"] = sc.last_moments_launches()
    moments(4)()                                          # colors, sq: the 16-spp frame in 4 batches, what the filters below read
    aov()                                                 # the frame's (e, V) as a first-frame history, what denoise_hist reads
    api.temporal_accumulate_device(w, h, cam, None, colors.data_ptr(), sq.data_ptr(), 16, 4, alb.data_ptr(), nd.data_ptr(), 0, 0, 0,
                                   hist.data_ptr(), hist_len.data_ptr(), stream=stream)
    timed = [("aov_chain", aov_chain), ("aov", aov), ("denoise", dn), ("denoise_var", lambda: dn_var(iters))]    # (aov last of the two: the filters read ITS buffers)
    if iters_var != iters:
        timed.append(("denoise_var_default", lambda: dn_var(iters_var)))
    timed += [("denoise_var_tiles", dn_var_tiles), ("denoise_hist", dn_hist)]
    if a.centre:
        timed = [("aov_centre_chain", aov_centre_chain), ("aov_chain", aov_chain), ("aov_centre", aov_centre), ("aov", aov)]
    for name, fn in timed:
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
    res["max_links"] = a.max_links
    res["mean_links"] = round(float(lnk.mean().item()), 4)     # of the chain pass: how much of the frame has a chain at all
    print(json.dumps(res))


if __name__ == "__main__":
    main()
