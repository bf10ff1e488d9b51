"""The shared input of the motion-chain tests. Scene A: the Cornell box with a mirror back wall (scenes.cornell(back_material=19)) at
64 x 40, its last 24 vertices (one diffuse box) moved by motion_cases.SHIFT, so the box moves in the mirror as well as in front
of it. And the pieces both kinds of test need: the centre rays, the chain guides and the motion buffer over a tracer's hits (the
oracle's for the CPU test, the library's own for the GPU tests)."""
import os

import numpy as np

import aov_chain_ref as AC
import motion_cases as MC
import motion_chain_ref as MCR
import motion_ref as MR
from denoise_ref import aovs_from_hits

W, H = 64, 40
MIRROR = 19


def scene_a(api, scene_dir, name="mchain_a", w=W, h=H):
    from cudapathtracer_amd import scenes
    cfg = scenes.cornell(os.path.join(scene_dir, name), width=w, height=h, name=name, spp=4, max_depth=4, back_material=MIRROR)["config"]
    hs = api.HostScene(cfg)
    assert hs.info["n_tris"] == 36 and hs.info["n_points"] == 72
    return hs


def moved_box(hs, shift=MC.SHIFT):
    """The scene's arrays with its last 24 vertices (one box) moved by `shift`."""
    n = hs.info["n_points"]
    return MC.moved_arrays(hs, n - 24, n, shift)


def back_wall_vertices(a):
    """The vertex indices of the triangles that lie in the plane of the back wall (z = the scene's smallest z): the mirror."""
    p = a["points"].view(np.float32).reshape(-1, 4)
    idx = MR.triangle_vertices(a["mesh"])
    z = p[idx, 2]
    return np.unique(idx[(z == p[:, 2].min()).all(-1)])


def oracle_centre_rays(O, cam, w, h):
    cb = MC.cam0_bytes(cam)
    return np.array([O.camera_ray(cb, x, y, 0) for y in range(h) for x in range(w)], np.float32)


def library_centre_rays(api, cam, w, h):
    return api.probe_centre_rays(cam, np.array([(x, y) for y in range(h) for x in range(w)], np.int32))


def chain_guides(tracer, mats, rays, max_links, w, h):
    """(albedo, normal_depth) [h,w,4] as pt_render_aovs_centre(max_links) lays them out, and links [h,w], over the tracer's hits."""
    r = AC.chain_rays(tracer, mats, rays, max_links)
    A, N = aovs_from_hits([(r["valid"], r["albedo"], r["normal"], r["depth"])], 1)
    return A.reshape(h, w, 4), N.reshape(h, w, 4), np.where(r["valid"], r["links"], 0).reshape(h, w)


def want_motion(tracer, mats, rays, max_links, new, old, w, h):
    """motion_chain_ref.motion_chain as [h,w,...] arrays; old None: no previous positions."""
    r = MCR.motion_chain(tracer, mats, rays, max_links, new["points"], None if old is None else old["points"], new["mesh"])
    return {k: v.reshape((h, w) + v.shape[1:]) for k, v in r.items()}
