"""What motion vectors cost and what they buy, in one run.

    python tools/motion_time.py [--w 1920 --h 1080 --reps 20 --warmup 3 --frames 20 --quality-frames 8 --ref-spp 1024
                                 --parts pass,preview,quality --animation all|object] [--chain --links 8 --view front|side] [--resources]

(a) pass: pt_render_motion_device (motion alone, and with the guide outputs) next to pt_render_aovs_centre_device(max_links 0) on
    the Cornell box and on the 82 k blob in the box, after one vertex update (so the scene has previous positions): HIP events
    around each launch, median of --reps after --warmup.
(b) preview: the animated preview of tools/update_time.py — the blob, every vertex moved through the device form before each frame,
    render scale 1 and 2 — with motion on, next to keep_history 1 without it and keep_history 0: median wall time of update +
    scene_changed + frame as frames per second, and the session's aov_ms.
(c) quality: over --quality-frames such frames at 4 spp (each frame's geometry a small step further), the mean relMSE of the
    session's `mean` against a --ref-spp pt_render of the frame's own geometry, for the same three modes, over the whole frame and
    over the pixels whose motion.w is 1. relMSE = mean over pixels and rgb of (x - ref)^2 / (ref^2 + 1e-2), over the pixels
    whose reference is finite. --animation object moves the blob alone, rigidly and sideways by 0.004 a frame (about three
    pixels), in place of the displacement of every vertex: there the walls, floor and light stand still.
--chain measures the pass that follows mirrors and glass instead, with --links as max_links:
(a) pass: pt_render_motion_chain_device (motion alone, and with the guide outputs) next to pt_render_aovs_centre_device(max_links)
    on the Cornell box with a glass and a mirror box and on the 82 k blob in a box with a mirror back wall and a glass pane in front
    of the blob's left half.
(c) quality: the "blob alone" animation in that box, sessions with centre guides and guide chain --links, four columns: motion chain
    on, motion on (first hit), keep_history 1, keep_history 0; relMSE over the whole frame and over the pixels with links > 0 that
    show the moved object (pt_render_motion_chain's links and motion.w), those split into pixels whose first hit is the mirror wall
    and the others (the pane). --view front sees the blob through the pane only, --view side sees its image in the mirror too.
--resources prints the motion kernels' registers, scratch and LDS from the code-object notes and needs no GPU. Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

GEOMETRY = ("points", "normals", "uvs", "mesh", "lights", "materials", "textures")


def motion_kernel_resources():
    """kernel_resources.kernel_resources of pt_motion.hip's motion_kernel: the one kernel's dict."""
    from kernel_resources import kernel_resources
    return kernel_resources("pt_motion", "(motion_kernel)")["motion_kernel"]


def motion_chain_kernel_resources():
    """... of pt_motion_chain.hip's motion_chain_kernel."""
    from kernel_resources import kernel_resources
    return kernel_resources("pt_motion_chain", "(motion_chain_kernel)")["motion_chain_kernel"]


def chain_parts(a, res, api, scenes, Q, np, torch):
    """--chain: the pass and quality parts for pt_render_motion_chain, into res."""
    w, h, links = a.w, a.h, a.links
    parts = a.parts.split(",")
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    # front: the session tests' first pose, which sees the blob through the pane but not in the mirror (the blob hides its own
    # image); side: from the right, where the blob's image stands free on the mirror wall
    cam = Q.camera(api, 0, True, w, h) if a.view == "front" else api.make_camera(True, (1.2, 0.5, 0.2), (-15.0, 35.0, 0.0), Q.FOV, w, h)
    n_blob = 10 * 4 ** 6 + 2                                  # the icosphere's vertices are the scene's last

    def host(maker, name, **kw):
        return api.HostScene(maker(tempfile.mkdtemp(), width=w, height=h, spp=4, max_depth=8, name="mtc_" + name, **kw)["config"])

    def blob_moved(hs, step):
        p = hs.array("points").view(np.float32).reshape(-1, 4).copy()
        p[-n_blob:, 0] += np.float32(step)
        return p

    blob = host(scenes.blob_in_box, "blob", back_material=19, pane_material=5)
    assert blob.info["n_points"] > n_blob and blob.info["n_tris"] == 20 * 4 ** 6 + 12 + 12
    res["links"], res["view"] = links, a.view
    if "pass" in parts:
        buf = [torch.empty(h, w, 4, device="cuda:0") for _ in range(3)]
        A, N, M = (b.data_ptr() for b in buf)
        res["pass"] = {}
        cornell = host(scenes.cornell, "cornell", tall_material=5, short_material=19)
        for name, hs, moved in (("cornell", cornell, None), ("blob", blob, blob_moved(blob, 0.004))):
            sc = api.Scene.from_mesh(hs)
            if moved is None:                                 # the wall behind the boxes, and everything else, a little
                moved = hs.array("points").view(np.float32).reshape(-1, 4).copy()
                moved[:, 2] += (0.02 * np.sin(7.0 * moved[:, 0] + 3.0 * moved[:, 1] + 1.3)).astype(np.float32)
            sc.update_vertices(torch.from_numpy(moved).cuda())
            assert sc.has_motion == 1
            runs = {"aovs_centre_ms": lambda: sc.render_aovs_centre_device(cam, w, h, links, A, N),
                    "motion_first_hit_ms": lambda: sc.render_motion_device(cam, w, h, 0, 0, M),
                    "motion_chain_ms": lambda: sc.render_motion_chain_device(cam, w, h, links, 0, 0, 0, M),
                    "motion_chain_with_guides_ms": lambda: sc.render_motion_chain_device(cam, w, h, links, A, N, 0, M)}
            row = {"n_tris": hs.info["n_tris"]}
            for key, run in runs.items():
                ms = []
                for _ in range(a.warmup + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record(torch.cuda.default_stream()); run(); e1.record(torch.cuda.default_stream())
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                row[key] = med(ms[a.warmup:])
            row["moved_share"] = round(float((buf[2][..., 3] == 1).float().mean().item()), 4)
            row["chain_over_centre"] = round(row["motion_chain_ms"] / row["aovs_centre_ms"], 3)
            row["fused_over_centre"] = round(row["motion_chain_with_guides_ms"] / row["aovs_centre_ms"], 3)
            res["pass"][name] = row
            sc.close()

    if "quality" in parts:
        nq = a.quality_frames
        steps = [blob_moved(blob, 0.004 * (t + 1)) for t in range(nq)]
        sc = api.Scene.from_mesh(blob)
        refs, masks = [], []
        dirs = api.probe_centre_rays(cam, np.array([(x, y) for y in range(h) for x in range(w)], np.int32)).reshape(h, w, 6)
        for t in range(nq):
            sc.update_vertices(steps[t])
            refs.append(sc.render(cam, w, h, a.ref_spp, 8, seed=Q.REF_SEED)[0][..., :3] / np.float32(a.ref_spp))
            _, _, mv, ln = sc.render_motion_chain(cam, w, h, links, guides=True, links=True)
            through = (ln > 0) & (mv[..., 3] == 1)
            first_n = sc.render_aovs_centre(cam, w, h, 0)[1]
            z = dirs[..., 2] + dirs[..., 5] * first_n[..., 3]
            mirror = z < z[first_n[..., 3] > 0].min() + 1e-3  # the first hit lies on the back wall
            masks.append({"moved_direct": (ln == 0) & (mv[..., 3] == 1), "through": through, "through_mirror": through & mirror,
                          "through_pane": through & ~mirror})
            print("reference frame %d of %d" % (t + 1, nq), file=sys.stderr, flush=True)
        sc.close()
        qual = {"frames": nq, "ref_spp": a.ref_spp, "shares": {k: round(float(np.mean([m[k].mean() for m in masks])), 5) for k in masks[0]}}
        modes = (("motion_chain", 1, 1, 1), ("motion", 1, 1, 0), ("keep1", 1, 0, 0), ("keep0", 0, 0, 0))   # (name, keep_history, motion, chain)
        for scale in (1, 2):
            for name, keep, motion, chain in modes:
                sc = api.Scene.from_mesh(blob)
                pv = api.Preview(sc, w, h).set_scale(scale).set_guide_centre(1).set_guide_chain(links).set_motion(motion).set_motion_chain(chain)
                whole, part = [], {k: [] for k in masks[0]}
                for t in range(nq):
                    sc.update_vertices(steps[t])
                    pv.scene_changed(bool(keep))
                    x = pv.frame(cam, Q.SEED0 + t).read(rgba8=False, hist=False, hist_len=False)["mean"][..., :3]
                    err = ((x - refs[t]) ** 2 / (refs[t] ** 2 + 1e-2)).mean(-1)
                    ok = np.isfinite(err)
                    whole.append(float(err[ok].mean()))
                    for k, m in masks[t].items():
                        if (m & ok).any():
                            part[k].append(float(err[m & ok].mean()))
                row = {"relmse": round(float(np.mean(whole)), 6)}
                row.update({"relmse_" + k: round(float(np.mean(v)), 6) if v else None for k, v in part.items()})
                qual["scale%d_%s" % (scale, name)] = row
                pv.close(); sc.close()
        res["quality_blob_mirror_pane"] = qual


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--quality-frames", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--parts", default="pass,preview,quality")
    ap.add_argument("--animation", choices=("all", "object"), default="all", help="what moves in the quality frames")
    ap.add_argument("--chain", action="store_true", help="measure pt_render_motion_chain (the pass and quality parts)")
    ap.add_argument("--links", type=int, default=8, help="max_links of --chain")
    ap.add_argument("--view", choices=("front", "side"), default="front", help="the camera of --chain")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        print(json.dumps({"motion_kernel": motion_kernel_resources(), "motion_chain_kernel": motion_chain_kernel_resources()}))
        return
    import numpy as np
    import torch
    import temporal_seq as Q
    from cudapathtracer_amd import api, scenes
    if not torch.cuda.is_available():
        raise SystemExit("motion_time.py needs a HIP device")
    torch.cuda.set_device(0)
    w, h = a.w, a.h
    parts = a.parts.split(",")
    med = lambda v: round(sorted(v)[len(v) // 2], 4)

    def displaced(hs, phase):
        """The scene's points with every vertex displaced a little, as tools/update_time.py displaces them: float32 [n, 4]."""
        p = hs.array("points").view(np.float32).reshape(-1, 4).copy()
        p[:, 2] += (0.02 * np.sin(7.0 * p[:, 0] + 3.0 * p[:, 1] + phase)).astype(np.float32)
        return p

    def host(maker, name):
        return api.HostScene(maker(tempfile.mkdtemp(), width=w, height=h, spp=4, max_depth=8, name="mt_" + name)["config"])

    res = {"w": w, "h": h, "reps": a.reps, "warmup": a.warmup}
    if a.chain:
        chain_parts(a, res, api, scenes, Q, np, torch)
        print(json.dumps(res))
        return
    cam = Q.camera(api, 0, True, w, h)
    blob = host(scenes.blob_in_box, "blob") if ("preview" in parts or "quality" in parts or "pass" in parts) else None

    if "pass" in parts:
        buf = [torch.empty(h, w, 4, device="cuda:0") for _ in range(3)]
        A, N, M = (b.data_ptr() for b in buf)
        res["pass"] = {}
        for name, hs in (("cornell", host(scenes.cornell, "cornell")), ("blob", blob)):
            sc = api.Scene.from_mesh(hs)
            sc.update_vertices(torch.from_numpy(displaced(hs, 1.3)).cuda())
            assert sc.has_motion == 1
            runs = {"aovs_centre_ms": lambda: sc.render_aovs_centre_device(cam, w, h, 0, A, N),
                    "motion_ms": lambda: sc.render_motion_device(cam, w, h, 0, 0, M),
                    "motion_with_guides_ms": lambda: sc.render_motion_device(cam, w, h, A, N, M)}
            row = {"n_tris": hs.info["n_tris"]}
            for key, run in runs.items():
                ms = []
                for _ in range(a.warmup + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record(torch.cuda.default_stream()); run(); e1.record(torch.cuda.default_stream())
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                row[key] = med(ms[a.warmup:])
            row["moved_share"] = round(float((buf[2][..., 3] == 1).float().mean().item()), 4)
            row["motion_over_centre"] = round(row["motion_ms"] / row["aovs_centre_ms"], 3)
            row["fused_over_centre"] = round(row["motion_with_guides_ms"] / row["aovs_centre_ms"], 3)
            res["pass"][name] = row
            sc.close()

    modes = (("motion", 1, 1), ("keep1", 1, 0), ("keep0", 0, 0))        # (name, keep_history, motion)
    if "preview" in parts:
        dev = [torch.from_numpy(displaced(blob, ph)).cuda() for ph in (0.0, 1.3)]
        nf = a.warmup + a.frames
        pvr = {}
        for scale in (1, 2):
            for name, keep, motion in modes:
                sc = api.Scene.from_mesh(blob)
                pv = api.Preview(sc, w, h).set_scale(scale).set_motion(motion)
                wall, aov = [], []
                for t in range(nf):
                    t0 = time.perf_counter()
                    sc.update_vertices(dev[t & 1])
                    pv.scene_changed(bool(keep))
                    pv.frame(cam, Q.SEED0 + t)
                    wall.append(1e3 * (time.perf_counter() - t0)); aov.append(pv.stats()["aov_ms"])
                m = med(wall[a.warmup:])
                pvr["scale%d_%s" % (scale, name)] = {"frame_ms": m, "fps": round(1e3 / m, 1), "aov_ms": med(aov[a.warmup:])}
                pv.close(); sc.close()
        res["preview_blob"] = {"frames": a.frames, **pvr}

    if "quality" in parts:
        nq = a.quality_frames
        if a.animation == "all":
            steps = [displaced(blob, 0.15 * t) for t in range(nq)]
        else:                                                 # the icosphere's vertices are the scene's last 10 * 4^6 + 2
            n_blob = 10 * 4 ** 6 + 2
            assert blob.info["n_points"] > n_blob and blob.info["n_tris"] == 20 * 4 ** 6 + 12
            steps = []
            for t in range(nq):
                p = blob.array("points").view(np.float32).reshape(-1, 4).copy()
                p[-n_blob:, 0] += np.float32(0.004 * (t + 1))
                steps.append(p)
        sc = api.Scene.from_mesh(blob)
        refs, moved = [], []
        for t in range(nq):
            sc.update_vertices(steps[t])
            refs.append(sc.render(cam, w, h, a.ref_spp, 8, seed=Q.REF_SEED)[0][..., :3] / np.float32(a.ref_spp))
            moved.append(sc.render_motion(cam, w, h)[..., 3] == 1)
            print("reference frame %d of %d" % (t + 1, nq), file=sys.stderr, flush=True)
        sc.close()
        qual = {"frames": nq, "ref_spp": a.ref_spp, "animation": a.animation, "moved_share": round(float(np.mean([m.mean() for m in moved])), 4)}
        for scale in (1, 2):
            for name, keep, motion in modes:
                sc = api.Scene.from_mesh(blob)
                pv = api.Preview(sc, w, h).set_scale(scale).set_motion(motion)
                whole, part = [], []
                for t in range(nq):
                    sc.update_vertices(steps[t])
                    pv.scene_changed(bool(keep))
                    x = pv.frame(cam, Q.SEED0 + t).read(rgba8=False, hist=False, hist_len=False)["mean"][..., :3]
                    err = ((x - refs[t]) ** 2 / (refs[t] ** 2 + 1e-2)).mean(-1)
                    ok = np.isfinite(err)                     # (a pixel whose reference holds a NaN or an Inf sample is left out)
                    whole.append(float(err[ok].mean()))
                    if (moved[t] & ok).any():
                        part.append(float(err[moved[t] & ok].mean()))
                qual["scale%d_%s" % (scale, name)] = {"relmse": round(float(np.mean(whole)), 6), "relmse_moved": round(float(np.mean(part)), 6) if part else None,
                                                      "relmse_last": round(whole[-1], 6)}
                pv.close(); sc.close()
        res["quality_blob"] = qual
    print(json.dumps(res))


if __name__ == "__main__":
    main()
