"""Device time of temporal accumulation and of the history filter at 1920x1080 (HIP events around each, after warm-up).

    python tools/temporal_time.py [--w 1920 --h 1080 --reps 20] [--specular [--max-links 8]]

Prints one JSON line: median / min milliseconds of pt_temporal_accumulate_device for a still camera (the identity instantiation)
and for a moving one (projection and four taps); the same two of _cur_device (the frames' own (e, V) as `cur`), of _motion_device
(a seeded motion buffer: a tenth of the pixels moved, to points inside the box) and of _cur_motion_device, and of _live_device with
every other tile live (accumulate_cur_*, accumulate_motion_*, accumulate_cur_motion_*, accumulate_live_half); of pt_denoise_hist_device at its default iterations and, in the same run for
comparison, of pt_denoise_var_device at its defaults; the bytes the accumulate pass moves per pixel (64 B of this frame's four
buffers, 20 B written, plus the previous guide, history and length once: 36 B, the gathers of neighbouring pixels share their
lines) and the fraction of the 8 TB/s HBM peak that makes at the measured time.
--specular runs the same still and moving frames on the glass + mirror Cornell box, once with first-hit guides and once with the
guides of pt_render_aovs_chain (--max-links): the line then holds both sets of numbers under "first_hit" and "chain", with the
feature pass's own time and the mean history length after the moving frame (what share of the history still validates)."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_PIXEL = 64 + 36 + 20
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--specular", action="store_true")
    ap.add_argument("--max-links", type=int, default=8)
    a = ap.parse_args()
    import torch
    from cudapathtracer_amd import api, scenes
    if not torch.cuda.is_available():
        raise SystemExit("temporal_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h = a.w, a.h
    kw = dict(tall_material=5, short_material=19) if a.specular else {}
    hs = api.HostScene(scenes.cornell(tempfile.mkdtemp(), width=w, height=h, spp=4, max_depth=8, name="tt", **kw)["config"])
    sc = api.Scene(hs)
    if a.specular:
        print(json.dumps({"w": w, "h": h, "scene": "glass + mirror Cornell", "max_links": a.max_links,
                          "first_hit": measure(a, torch, api, sc, 0), "chain": measure(a, torch, api, sc, a.max_links)}))
    else:
        print(json.dumps(measure(a, torch, api, sc, 0)))


def measure(a, torch, api, sc, links):
    """The tool's numbers with first-hit guides (links 0) or chain guides."""
    w, h = a.w, a.h
    cam0 = api.make_camera(True, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 60.0, w, h)
    cam1 = api.make_camera(True, (0.03, 0.01, 1.0), (0.0, 0.8, 0.0), 60.0, w, h)
    stream = torch.cuda.current_stream().cuda_stream
    buf = lambda: torch.empty(h, w, 4, device="cuda:0")

    def frame(cam, seed):
        S, Q, A, N = buf(), buf(), buf(), buf()
        sc.render_moments_device(cam, w, h, 4, 2, 8, S.data_ptr(), Q.data_ptr(), seed=seed, stream=stream)
        aovs(cam, A, N, seed)
        return S, Q, A, N

    def aovs(cam, A, N, seed):
        if links:
            sc.render_aovs_chain_device(cam, w, h, links, A.data_ptr(), N.data_ptr(), None, seed=seed, stream=stream)
        else:
            sc.render_aovs_device(cam, w, h, A.data_ptr(), N.data_ptr(), seed=seed, stream=stream)

    f0, f_still, f_moved = frame(cam0, 1), frame(cam0, 2), frame(cam1, 2)
    hist0, hist1 = buf(), buf()
    len0, len1 = torch.empty(h, w, device="cuda:0"), torch.empty(h, w, device="cuda:0")
    ws = torch.empty(api.denoise_hist_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    out = buf()
    p = lambda t: t.data_ptr()
    api.temporal_accumulate_device(w, h, cam0, None, p(f0[0]), p(f0[1]), 4, 2, p(f0[2]), p(f0[3]), 0, 0, 0, p(hist0), p(len0), stream=stream)

    def accumulate(cam, f):
        return lambda: api.temporal_accumulate_device(w, h, cam, cam0, p(f[0]), p(f[1]), 4, 2, p(f[2]), p(f[3]), p(f0[3]), p(hist0), p(len0),
                                                      p(hist1), p(len1), stream=stream)

    def own_ev(cam, f):                                        # a frame's (e, V): what its first frame leaves as the history
        cur, ln = buf(), torch.empty(h, w, device="cuda:0")
        api.temporal_accumulate_device(w, h, cam, None, p(f[0]), p(f[1]), 4, 2, p(f[2]), p(f[3]), 0, 0, 0, p(cur), p(ln), stream=stream)
        return cur

    gen = torch.Generator(device="cuda:0").manual_seed(7)
    motion = torch.rand(h, w, 4, device="cuda:0", generator=gen) * 1.6 - 0.8
    motion[..., 3] = (torch.rand(h, w, device="cuda:0", generator=gen) < 0.1).float()
    ty, tx = (h + 7) // 8, (w + 7) // 8
    half = ((torch.arange(ty, device="cuda:0")[:, None] + torch.arange(tx, device="cuda:0")[None, :]) % 2).to(torch.int32).contiguous()
    history = (p(f0[3]), p(hist0), p(len0))

    def variants(tag, cam, f):
        cur = own_ev(cam, f)
        sums = (p(f[0]), p(f[1]), 4, 2, p(f[2]), p(f[3]))
        return [("accumulate_cur_" + tag, lambda: api.temporal_accumulate_cur_device(w, h, cam, cam0, p(cur), p(f[3]), *history, p(hist1), p(len1),
                                                                                      stream=stream)),
                ("accumulate_motion_" + tag, lambda: api.temporal_accumulate_motion_device(w, h, cam, cam0, *sums, *history, p(motion), p(hist1),
                                                                                            p(len1), stream=stream)),
                ("accumulate_cur_motion_" + tag, lambda: api.temporal_accumulate_cur_motion_device(w, h, cam, cam0, p(cur), p(f[3]), *history,
                                                                                                    p(motion), p(hist1), p(len1), stream=stream))]

    def live_half():
        api.temporal_accumulate_live_device(w, h, cam0, cam0, p(f_still[0]), p(f_still[1]), 4, 2, p(f_still[2]), p(f_still[3]), *history, p(half),
                                            p(hist1), p(len1), stream=stream)

    def dn_hist():
        api.denoise_hist_device(w, h, p(hist1), p(f_moved[2]), p(f_moved[3]), p(ws), p(out), stream=stream)

    def dn_var():
        api.denoise_var_device(w, h, p(f_moved[0]), p(f_moved[1]), 4, 2, p(f_moved[2]), p(f_moved[3]), p(ws), p(out), stream=stream)

    res = {"w": w, "h": h, "iterations_default": api.denoise_var_defaults()["iterations"], "accumulate_bytes_per_pixel": BYTES_PER_PIXEL}
    timed = [("accumulate_identity", accumulate(cam0, f_still)), ("accumulate_moving", accumulate(cam1, f_moved)),
             ("denoise_hist", dn_hist), ("denoise_var", dn_var)]
    timed += variants("identity", cam0, f_still) + variants("moving", cam1, f_moved) + [("accumulate_live_half", live_half)]
    if a.specular:
        fa, fn_ = buf(), buf()
        timed.insert(0, ("feature_pass", lambda: aovs(cam1, fa, fn_, 2)))
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
        if name in ("accumulate_identity", "accumulate_moving"):
            res[name + "_hbm_fraction"] = round(BYTES_PER_PIXEL * w * h / (ts[len(ts) // 2] * 1e-3) / HBM_PEAK, 4)
            res[name + "_mean_length"] = round(float(len1.mean()), 3)
    return res


if __name__ == "__main__":
    main()
