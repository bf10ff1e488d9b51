"""The shared input of the radiance-query tests: the three 40 x 24 cases of ids_cases.CAMERAS (the Cornell box with a glass tall box
and a mirror short box from inside and from outside, the mirror and glass scene: no leaf triangle and no texture, the LEAN kernel) and
scenes.textured() at 40 x 24 from TEXTURED_CAMERA, near the floor and looking up at the two canopy quads from below: their leaf
materials force the generic, non-LEAN kernel (tests/test_radiance_api.py asserts on the oracle, without a GPU, that 110 centre rays
hit them, 263 the textured back wall, and 17 leave through the open front). Every case renders with cam0, the case's
camera with antiAliasJitterDist = 0 and aperture = 0 (motion_cases.cam0_bytes): its camera_ray is the centre ray, so the centre rays
on streams 0 .. w*h - 1 are that camera's render. 4 samples, depth 8: 960 rays, 15 tiles; CROP = 950 leaves a ragged last tile."""
import os

import numpy as np

import ids_cases as IC
import motion_cases as MC
import query_cases as QC

W, H = MC.W, MC.H
N = W * H
SPP, DEPTH = 4, 8
CROP = 950
CASES = ("cornell", "cornell_outside", "glass_mirror", "textured")
# (integrator, use_mis) per case: both integrators; the Cornell box also without MIS
SETTINGS = {name: ((0, True), (2, True)) + (((0, False),) if name == "cornell" else ()) for name in CASES}
LEAF_MATERIALS = (13, 16)            # scenes.textured()'s canopy quads
TEXTURED_CAMERA = (True, (-0.6, -0.9, -0.9), (45.0, -25.0, 0.0), 70.0)      # pinhole, pos, rot, fov


def host(api, scene_dir, name, prefix="radiance_"):
    if name == "textured":
        from cudapathtracer_amd import scenes
        return api.HostScene(scenes.textured(os.path.join(scene_dir, prefix + name), width=W, height=H, name=prefix + name)["config"])
    return IC.host(api, scene_dir, IC.CAMERAS[name][0], prefix + name)


def camera(api, hs, name):
    if name == "textured":
        pinhole, pos, rot, fov = TEXTURED_CAMERA
        return api.make_camera(pinhole, pos, rot, fov, W, H)
    return IC.camera(api, hs, name)


def cam0(api, hs, name):
    """The case's camera without jitter and aperture, as an api.Camera."""
    cam = camera(api, hs, name)
    assert (cam.w, cam.h) == (W, H)
    return api.Camera.frombytes(MC.cam0_bytes(cam).tobytes())


def arrays(hs):
    return QC.arrays(hs)


def centre_records(api, cam, max_t=QC.MAX_T):
    """The [N, 8] pt_ray records of cam's centre rays (the library's probe: pt_query_camera_rays_device's o and d), pad = 0."""
    return QC.records(IC.library_centre_rays(api, cam, W, H), max_t)


def as_rays(image):
    """An [H, W, 4] image as [N, 4] rows, ray y*W + x."""
    return np.ascontiguousarray(image, np.float32).reshape(N, 4)
