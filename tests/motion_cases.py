"""The shared input of the motion tests: the 40 x 24 Cornell scene of tests/test_preview_update.py (glass tall box, mirror short box)
with the tall box's vertices 48..71 moved by SHIFT, and the oracle's closest hits along the centre rays for the CPU test."""
import os

import numpy as np

W, H = 40, 24
SHIFT = (0.25, 0.0, 0.15)
GEOMETRY = ("points", "normals", "uvs", "mesh", "lights", "materials", "textures")


def cornell_host(api, scene_dir, name="motion_cornell", w=W, h=H):
    from cudapathtracer_amd import scenes
    cfg = scenes.cornell(os.path.join(scene_dir, name), width=w, height=h, name=name, spp=4, max_depth=4, tall_material=5, short_material=19)["config"]
    hs = api.HostScene(cfg)
    assert hs.info["n_tris"] == 36 and hs.info["n_points"] == 72
    return hs


def arrays(hs):
    return {k: hs.array(k) for k in GEOMETRY}


def moved_arrays(hs, first=48, last=72, shift=SHIFT):
    """The scene's arrays with vertices first..last-1 moved by `shift` (48..71: the tall box; 20..23: the light quad)."""
    a = arrays(hs)
    a["points"].view(np.float32).reshape(-1, 4)[first:last, :3] += np.array(shift, np.float32)
    return a


def cam0_bytes(cam):
    """The camera's 112 bytes with antiAliasJitterDist = 0 and aperture = 0: its camera_ray is the centre ray."""
    from cudapathtracer_amd import api
    c = api.Camera.frombytes(cam.tobytes())
    c.antiAliasJitterDist = 0.0
    c.aperture = 0.0
    return np.frombuffer(c.tobytes(), np.uint8).copy()


def oracle_scene(O, a, leaf):
    bvh, idx, _ = O.build_bvh(a["points"], a["mesh"], leaf)
    return O.OracleScene(arrays=dict(a, bvh=bvh, indices=idx.view(np.uint8)))


def oracle_centre_hits(O, osc, cam, w=W, h=H):
    """The oracle's closest hit along every pixel's centre ray: ((valid, u, v, tri) for motion_ref.motion, albedo [h,w,4],
    normal_depth [h,w,4] as pt_render_aovs_centre(max_links 0) lays them out)."""
    from denoise_ref import aovs_from_hits
    cb = cam0_bytes(cam)
    rays = np.array([O.camera_ray(cb, x, y, 0) for y in range(h) for x in range(w)], np.float32)
    oi, of, _ = osc.trace_closest(rays)
    valid = oi[:, 0] == 1
    alb = osc.array("materials").reshape(-1, 176)[:, 48:64].copy().view(np.float32)[:, :3]
    albedo = np.where(valid[:, None], alb[np.maximum(oi[:, 2], 0)], 0.0).astype(np.float32)
    A, N = aovs_from_hits([(valid, albedo, of[:, 6:9].copy(), of[:, 0].copy())], 1)
    return (valid, of[:, 1].copy(), of[:, 2].copy(), oi[:, 1].copy()), A.reshape(h, w, 4), N.reshape(h, w, 4)
