"""What an in-place material or emission edit costs, next to the update_mesh and the destroy + create it replaces, in one run.

    python tools/material_time.py [--reps 20 --warmup 3 --scenes cornell,blob,atrium] [--quality [--ref-spp 1024]]

For the Cornell box (36 triangles), the blob in the box (82 k) and the atrium (263 k), two variants of one edit alternate — the most
used diffuse row repainted, and every light scaled and recoloured — and four ways of getting the scene there are timed with the
host clock, each call complete on return: Scene.update_materials, Scene.update_emission (all lights), Scene.update_mesh of the
edited arrays, and close() + Scene.from_mesh of them. Medians of --reps after --warmup. `kernel_choice_ms` is update_materials with
an edit that alternates the row between diffuse and a delta mirror, so that the scene changes kernel family with every call.

--quality instead: a preview session of the Cornell box at 128 x 128, 8 frames of 4 spp with a resting camera and centre guides. The
lights' emission is halved before frame 4 ("emission"); a second sequence repaints the left wall there ("albedo"). For three
sessions — respond on, respond off (both announce the edit with keep_history 1) and keep_history 0 — it reports per frame the
relMSE of the session's mean against a --ref-spp pt_render of that frame's own scene: mean over pixels and rgb of
(x - ref)^2 / (ref^2 + 1e-2), over the pixels where it is finite. Prints one JSON line."""
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
    ap.add_argument("--scenes", default="cornell,blob,atrium")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--ref-spp", type=int, default=1024)
    a = ap.parse_args()
    import numpy as np
    import torch
    import temporal_seq as Q
    from cudapathtracer_amd import api, scenes
    if not torch.cuda.is_available():
        raise SystemExit("material_time.py needs a HIP device")
    torch.cuda.set_device(0)
    # pt_material (176 B) and pt_triangle (80 B): the fields the edits touch
    MAT = np.dtype({"names": ["type", "albedo", "isSpecular", "boundary"], "formats": ["i4", "4f4", "u1", "u1"], "offsets": [32, 48, 128, 129],
                    "itemsize": 176})
    TRI = np.dtype({"names": ["materialID", "emission", "lightInd"], "formats": ["i4", "4f4", "i4"], "offsets": [36, 48, 64], "itemsize": 80})
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    arrays = lambda hs: {k: hs.array(k) for k in GEOMETRY}

    def diffuse_rows(arr):
        """The diffuse rows triangles use, most used first."""
        m = arr["materials"].view(MAT)
        used = np.bincount(arr["mesh"].view(TRI)["materialID"], minlength=len(m))
        return [int(r) for r in np.argsort(-used, kind="stable") if used[r] and m["type"][r] == 0]

    def with_emission(arr, scale):
        """The arrays with every light, and every triangle of it, emitting `scale` times what it emitted; returns the edit too."""
        lt, tri = arr["lights"].view(TRI), arr["mesh"].view(TRI)
        idx = np.arange(len(lt), dtype=np.int32)
        em = (lt["emission"] * np.asarray(scale, np.float32)).astype(np.float32)
        for li in idx:
            lt["emission"][li] = em[li]
            tri["emission"][tri["lightInd"] == li] = em[li]
        return idx, em

    if a.quality:
        w = h = 128
        hs = api.HostScene(scenes.cornell(tempfile.mkdtemp(), width=w, height=h, spp=4, max_depth=8, name="mt_quality")["config"])
        cam = lambda: Q.camera(api, 0, False, w, h)
        frames, at = 8, 4
        res = {"w": w, "h": h, "frames": frames, "edit_before_frame": at, "spp": 4, "ref_spp": a.ref_spp, "sequences": {}}
        for seq in ("emission", "albedo"):
            new = arrays(hs)
            if seq == "emission":
                edit = with_emission(new, (0.5, 0.5, 0.5, 1.0))
                apply = lambda sc: sc.update_emission(*edit)
            else:                                             # the left wall: the used diffuse row that is reddest
                m = new["materials"].view(MAT)
                row = max(diffuse_rows(new), key=lambda r: m["albedo"][r][0] - m["albedo"][r][1])
                m["albedo"][row][:3] = (0.1, 0.2, 0.9)
                apply = lambda sc: sc.update_materials(new["materials"])
            refs = []
            for src in (hs, new):
                sc = api.Scene.from_mesh(src, hs.info["leaf_size"])
                refs.append(sc.render(cam(), w, h, a.ref_spp, 8, seed=Q.REF_SEED)[0][..., :3] / np.float32(a.ref_spp))
                sc.close()
            out = {}
            for name, keep, respond in (("respond_on", 1, True), ("respond_off", 1, False), ("keep_history_0", 0, False)):
                sc = api.Scene.from_mesh(hs)
                pv = api.Preview(sc, w, h, spp=4).set_guide_centre(1)
                if respond:
                    pv.set_respond(**api.respond_defaults())
                errs = []
                for t in range(frames):
                    if t == at:
                        apply(sc)
                        pv.scene_changed(bool(keep))
                    x = pv.frame(cam(), Q.SEED0 + t).read(rgba8=False, hist=False, hist_len=False)["mean"][..., :3]
                    ref = refs[1 if t >= at else 0]
                    err = ((x - ref) ** 2 / (ref ** 2 + 1e-2)).mean(-1)
                    errs.append(round(float(err[np.isfinite(err)].mean()), 6))
                out[name] = {"relmse_per_frame": errs, "relmse_after_edit": round(float(np.mean(errs[at:])), 6)}
                pv.close(); sc.close()
            res["sequences"][seq] = out
        print(json.dumps(res))
        return

    makers = {"cornell": scenes.cornell, "blob": scenes.blob_in_box, "atrium": scenes.atrium}
    n = a.warmup + a.reps
    res = {"reps": a.reps, "warmup": a.warmup, "scenes": {}}

    def timed(call):
        wall = []
        for t in range(n):
            t0 = time.perf_counter()
            call(t & 1)
            wall.append(1e3 * (time.perf_counter() - t0))
        return med(wall[a.warmup:])

    for name in a.scenes.split(","):
        hs = api.HostScene(makers[name](tempfile.mkdtemp(), width=64, height=64, spp=4, max_depth=8, name="mt_" + name)["config"])
        leaf = hs.info["leaf_size"]
        var, edits, mirror = [], [], []
        for k, (albedo, scale) in enumerate((((0.2, 0.5, 0.8), (0.5, 0.4, 0.3, 1.0)), ((0.8, 0.5, 0.2), (1.0, 1.0, 1.0, 1.0)))):
            arr = arrays(hs)
            row = diffuse_rows(arr)[0]
            arr["materials"].view(MAT)["albedo"][row][:3] = albedo
            edits.append(with_emission(arr, scale))
            var.append(arr)
            mir = arr["materials"].copy()
            if k == 0:
                mm = mir.view(MAT)
                mm["type"][row] = 6; mm["isSpecular"][row] = 1; mm["boundary"][row] = 0
            mirror.append(mir)
        sc = api.Scene.from_mesh(hs)
        row = {"n_tris": hs.info["n_tris"], "n_mats": hs.info["n_mats"], "n_lights": hs.info["n_lights"]}
        row["update_materials_ms"] = timed(lambda k: sc.update_materials(var[k]["materials"]))
        row["kernel_choice_ms"] = timed(lambda k: sc.update_materials(mirror[k]))
        row["update_emission_ms"] = timed(lambda k: sc.update_emission(*edits[k]))
        row["update_mesh_ms"] = timed(lambda k: sc.update_mesh(var[k], leaf))
        holder = [sc]

        def recreate(k):
            holder[0].close()
            holder[0] = api.Scene.from_mesh(var[k], leaf)
        row["destroy_create_ms"] = timed(recreate)
        holder[0].close()
        row["mesh_over_materials"] = round(row["update_mesh_ms"] / row["update_materials_ms"], 1)
        row["mesh_over_emission"] = round(row["update_mesh_ms"] / row["update_emission_ms"], 1)
        res["scenes"][name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
