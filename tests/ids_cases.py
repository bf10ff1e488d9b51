"""The shared input of the ID-pass tests: the 40 x 24 Cornell box of motion_cases (glass tall box, mirror short box) and the mirror and
glass scene of aov_chain_cases, each with the cameras whose centre rays hold, together, every class of pixel the pass distinguishes
(tests/test_ids_ref_cpu.py asserts that without a GPU)."""
import numpy as np

import aov_chain_cases as ACC
import motion_cases as MC

W, H = MC.W, MC.H
LINKS = (0, 1, 4)

# name: (scene, camera or None for the scene's own); camera: (pinhole, pos, rot, fov, aperture, focal_dist)
CAMERAS = {
    "cornell": ("cornell", None),
    "cornell_outside": ("cornell", (True, (2.6, 0.4, 2.4), (-5.0, 38.0, 0.0), 60.0, 0.0, 0.0)),     # from the front right: past the shell, and a wall's back
    "glass_mirror": ("glass_mirror", ACC.CASES["glass_mirror_40x24"][3]),
}


def host(api, scene_dir, scene, name=None):
    if scene == "cornell":
        return MC.cornell_host(api, scene_dir, name or "ids_cornell")
    return api.HostScene(ACC.scene_config(scene, scene_dir))


def camera(api, hs, name, w=W, h=H):
    cam = CAMERAS[name][1]
    if cam is None:
        c = hs.camera()
        assert (c.w, c.h) == (w, h)
        return c
    pinhole, pos, rot, fov, ap, fd = cam
    return api.make_camera(pinhole, pos, rot, fov, w, h, ap, fd)


def pixels(w, h):
    return np.array([(x, y) for y in range(h) for x in range(w)], np.int32)


def oracle_centre_rays(O, cam, w, h):
    cb = MC.cam0_bytes(cam)
    return np.array([O.camera_ray(cb, x, y, 0) for y in range(h) for x in range(w)], np.float32)


def library_centre_rays(api, cam, w, h):
    return api.probe_centre_rays(cam, pixels(w, h))


def host_arrays(hs):
    """The host scene's arrays with its own tree: what ids_ref.light_of_triangle reads."""
    return {k: hs.array(k) for k in MC.GEOMETRY + ("bvh", "indices")}
