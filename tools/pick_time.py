"""What picking costs, in one run.

    python tools/pick_time.py [--w 1920 --h 1080 --reps 20 --warmup 3 --scene cornell|mixed|blob --links 4 --parts pass,overlay,pick,preview]
    python tools/pick_time.py --resources      (no device needed: compiles pt_ids.hip and prints its kernels' registers, scratch and LDS)

(a) pass: pt_render_ids_device next to pt_render_aovs_centre_device at max_links 0 and --links, HIP events around each launch,
    median of --reps after --warmup. `cornell` has no chain at all, `mixed` is bench.py --full's mixed Cornell box (mirror box,
    glass box around a water box, gold box), `blob` the 82 k blob in the box.
(b) overlay: pt_select_overlay_device on that frame's IDs with one entry (the material under the image's centre) at radius 1 and 4,
    and with four entries, next to pt_resolve_device on a frame of the same size.
(c) pick: one pt_pick of 1 pixel and of 64 pixels (host wall clock: the call blocks and includes its two copies), max_links --links.
(d) preview: a session's frame with a selection next to one without, camera moving (every frame traces the ID buffer) and resting
    (none does): median wall clock of pt_preview_frame and the stage time resolve_ms, which covers the ID pass and the overlay.
Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def ids_kernel_resources():
    """kernel_resources.kernel_resources of pt_ids.hip's two kernels, by kernel name."""
    from kernel_resources import kernel_resources
    return kernel_resources("pt_ids", r"(ids\w*?_kernel)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scene", choices=("cornell", "mixed", "blob"), default="cornell")
    ap.add_argument("--links", type=int, default=4)
    ap.add_argument("--parts", default="pass,overlay,pick,preview")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps(ids_kernel_resources()))
        return
    import numpy as np
    import torch
    from cudapathtracer_amd import api, scenes
    if not torch.cuda.is_available():
        raise SystemExit("pick_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h, parts = a.w, a.h, a.parts.split(",")
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    gen = scenes.blob_in_box if a.scene == "blob" else scenes.cornell
    kw = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4]) if a.scene == "mixed" else {}
    hs = api.HostScene(gen(tempfile.mkdtemp(), width=w, height=h, spp=4, max_depth=8, name="pk", **kw)["config"])
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

    def wall(run):
        ms = []
        for _ in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); run()
            ms.append(1e3 * (time.perf_counter() - t0))
        return med(ms[a.warmup:])

    res = {"w": w, "h": h, "scene": a.scene, "n_tris": hs.info["n_tris"], "links": a.links, "reps": a.reps, "warmup": a.warmup}
    A, N = torch.empty(h, w, 4, device="cuda:0"), torch.empty(h, w, 4, device="cuda:0")
    ids = torch.empty(h, w, 4, dtype=torch.int32, device="cuda:0")
    if "pass" in parts:
        row = {}
        for ml in (0, a.links):
            row["aovs_centre_links%d_ms" % ml] = events(lambda: sc.render_aovs_centre_device(cam, w, h, ml, A.data_ptr(), N.data_ptr(), stream=stream))
            row["ids_links%d_ms" % ml] = events(lambda: sc.render_ids_device(cam, w, h, ml, ids.data_ptr(), stream=stream))
            row["ids_over_centre_links%d" % ml] = round(row["ids_links%d_ms" % ml] / row["aovs_centre_links%d_ms" % ml], 3)
        res["pass"] = row
    sc.render_ids_device(cam, w, h, a.links, ids.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    centre = ids[h // 2, w // 2].cpu().numpy()
    mat = max(int(centre[1]), 0)
    share = float((ids[..., 1] == mat).float().mean().item())
    if "overlay" in parts:
        rgba8 = torch.zeros(h, w, 4, dtype=torch.uint8, device="cuda:0")
        mean = torch.empty(h, w, 4, device="cuda:0")
        row = {"selected_share": round(share, 4)}
        row["resolve_ms"] = events(lambda: api.resolve_device(w, h, A.data_ptr(), 1, rgba8.data_ptr(), mean.data_ptr(), stream=stream))
        for radius in (1, 4):
            e = [("material", mat, mat, (255, 160, 0, 255), radius, 64)]
            row["overlay_radius%d_ms" % radius] = events(lambda: api.select_overlay_device(w, h, ids.data_ptr(), e, rgba8.data_ptr(), stream=stream))
        e4 = [("material", mat, mat, (255, 160, 0, 255), 4, 64), ("tri", 0, 1 << 30, (0, 255, 0, 128), 3, 16),
              ("light", 0, 1 << 30, (255, 255, 255, 255), 2, 0), ("material", 0, mat, (0, 0, 255, 200), 1, 32)]
        row["overlay_4_entries_ms"] = events(lambda: api.select_overlay_device(w, h, ids.data_ptr(), e4, rgba8.data_ptr(), stream=stream))
        row["overlay_nothing_selected_ms"] = events(lambda: api.select_overlay_device(w, h, ids.data_ptr(), [("tri", 1 << 30, 1 << 30, (1, 1, 1, 1), 4, 1)],
                                                                                      rgba8.data_ptr(), stream=stream))
        res["overlay"] = row
    if "pick" in parts:
        rng = np.random.default_rng(3)
        one = np.array([(w // 2, h // 2)], np.int32)
        many = np.stack([rng.integers(0, w, 64), rng.integers(0, h, 64)], 1).astype(np.int32)
        res["pick"] = {"pick_1_wall_ms": wall(lambda: sc.pick(cam, w, h, one, a.links)), "pick_64_wall_ms": wall(lambda: sc.pick(cam, w, h, many, a.links))}
    if "preview" in parts:
        pos = lambda t: api.make_camera(True, (0.02 * t, 0.0, 2.6), (0.0, 0.0, 0.0), 45.0, w, h)
        row = {}
        for name, entries in (("plain", []), ("selection", [("material", mat, mat, (255, 160, 0, 255), 2, 64)])):
            for mode in ("moving", "resting"):
                pv = api.Preview(sc, w, h).set_guide_centre(1).set_guide_chain(a.links).set_selection(entries, a.links)
                ms, rs = [], []
                for t in range(a.warmup + a.reps):
                    c = pos(t if mode == "moving" else 0)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter(); pv.frame(c, 1000 + t)
                    ms.append(1e3 * (time.perf_counter() - t0)); rs.append(pv.stats()["resolve_ms"])
                row["%s_%s_frame_ms" % (name, mode)] = med(ms[a.warmup:])
                row["%s_%s_resolve_ms" % (name, mode)] = med(rs[a.warmup:])
                row["%s_%s_id_passes" % (name, mode)] = pv.id_passes
                pv.close()
        res["preview"] = row
    sc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
