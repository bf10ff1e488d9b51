"""What an in-place geometry update costs, next to the destroy + create it replaces, in one run.

    python tools/update_time.py [--reps 20 --warmup 3 --w 1920 --h 1080 --frames 20 --scenes cornell,blob,atrium --no-preview]

For the Cornell box (36 triangles), the blob in the box (82 k) and the atrium (263 k), every vertex is displaced a little (two
variants, alternating) and three ways of getting the scene to the new positions are timed with the host clock, each call
complete on return: Scene.update_vertices with a host array, with a device array (pt_scene_update_vertices_device: nothing is
uploaded), and close() + Scene.from_mesh of the new arrays. Medians of --reps after --warmup. The update's split: `device_ms` is the
builder's own (HIP events around its kernels, pt_bvh_build_stats), `renumber_ms` the renumbering of the internal nodes by area
that still passes through the host (pt_debug_update_ms), `rest_ms` what is left of the host-form call: the upload of the
positions, the per-level synchronisations' host side, the light records, the derived tables.

Then, unless --no-preview, a preview session (defaults, 4 spp) of the blob at --w x --h whose vertices change before every
frame (device form), at render scale 1 and 2 and with keep_history 0 and 1: median wall time of update + scene_changed + frame,
as frames per second, and the update's share of it. Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

GEOMETRY = ("points", "normals", "uvs", "mesh", "lights", "materials", "textures")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--scenes", default="cornell,blob,atrium")
    ap.add_argument("--no-preview", action="store_true")
    a = ap.parse_args()
    import ctypes
    import numpy as np
    import torch
    import temporal_seq as Q
    from cudapathtracer_amd import api, scenes
    if not torch.cuda.is_available():
        raise SystemExit("update_time.py needs a HIP device")
    torch.cuda.set_device(0)
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    makers = {"cornell": scenes.cornell, "blob": scenes.blob_in_box, "atrium": scenes.atrium}
    n = a.warmup + a.reps

    def variants(hs):
        """Two displaced copies of the scene's arrays (every vertex moves by a few per cent of the box)."""
        out = []
        for phase in (0.0, 1.3):
            arr = {k: hs.array(k) for k in GEOMETRY}
            p = arr["points"].view(np.float32).reshape(-1, 4)
            p[:, 2] += (0.02 * np.sin(7.0 * p[:, 0] + 3.0 * p[:, 1] + phase)).astype(np.float32)
            out.append(arr)
        return out

    def split_ms(sc):
        out = np.zeros(3, np.float32)
        api.lib().pt_debug_update_ms(sc.h, out.ctypes.data_as(ctypes.c_void_p))
        return float(out[0])                              # the renumbering's share

    res = {"reps": a.reps, "warmup": a.warmup, "scenes": {}}
    blob = None
    for name in a.scenes.split(","):
        hs = api.HostScene(makers[name](tempfile.mkdtemp(), width=a.w, height=a.h, spp=4, max_depth=8, name="ut_" + name)["config"])
        leaf = hs.info["leaf_size"]
        var = variants(hs)
        dev = [torch.from_numpy(v["points"].view(np.float32).reshape(-1, 4).copy()).cuda() for v in var]
        sc = api.Scene.from_mesh(hs)
        row = {"n_tris": hs.info["n_tris"], "n_points": hs.info["n_points"]}
        wall, dms, rms = [], [], []
        for t in range(n):
            t0 = time.perf_counter()
            sc.update_vertices(var[t & 1]["points"])
            wall.append(1e3 * (time.perf_counter() - t0))
            dms.append(sc.build_stats["device_ms"]); rms.append(split_ms(sc))
        row["update_host_ms"] = med(wall[a.warmup:]); row["device_ms"] = med(dms[a.warmup:]); row["renumber_ms"] = med(rms[a.warmup:])
        row["rest_ms"] = round(row["update_host_ms"] - row["device_ms"] - row["renumber_ms"], 4)
        wall = []
        for t in range(n):
            t0 = time.perf_counter()
            sc.update_vertices(dev[t & 1])
            wall.append(1e3 * (time.perf_counter() - t0))
        row["update_device_ms"] = med(wall[a.warmup:])
        sc.close()
        sc = api.Scene.from_mesh(var[1], leaf)
        wall = []
        for t in range(n):
            t0 = time.perf_counter()
            sc.close()
            sc = api.Scene.from_mesh(var[t & 1], leaf)
            wall.append(1e3 * (time.perf_counter() - t0))
        row["destroy_create_ms"] = med(wall[a.warmup:])
        row["create_over_update_host"] = round(row["destroy_create_ms"] / row["update_host_ms"], 2)
        row["create_over_update_device"] = round(row["destroy_create_ms"] / row["update_device_ms"], 2)
        sc.close()
        res["scenes"][name] = row
        if name == "blob":
            blob = (hs, dev)
    if blob is not None and not a.no_preview:
        hs, dev = blob
        w, h = a.w, a.h
        nf = a.warmup + a.frames
        cam = Q.camera(api, 0, True, w, h)
        pvr = {}
        for scale in (1, 2):
            for keep in (0, 1):
                sc = api.Scene.from_mesh(hs)
                pv = api.Preview(sc, w, h).set_scale(scale)
                wall, upd = [], []
                for t in range(nf):
                    t0 = time.perf_counter()
                    sc.update_vertices(dev[t & 1])
                    t1 = time.perf_counter()
                    pv.scene_changed(bool(keep))
                    pv.frame(cam, Q.SEED0 + t)
                    wall.append(1e3 * (time.perf_counter() - t0)); upd.append(1e3 * (t1 - t0))
                m = med(wall[a.warmup:])
                pvr["scale%d_keep%d" % (scale, keep)] = {"frame_ms": m, "update_ms": med(upd[a.warmup:]), "fps": round(1e3 / m, 1)}
                pv.close(); sc.close()
        res["preview_blob"] = {"w": w, "h": h, "frames": a.frames, **pvr}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
