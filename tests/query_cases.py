"""The shared input of the ray-query tests: per scene ONE set of N = 997 rays (not a multiple of 64) of four kinds, from fixed numpy
seeds. The scenes are the 40 x 24 scenes of ids_cases (the Cornell box with a glass tall box and a mirror short box from inside and
from outside, the mirror and glass scene) and scenes.textured(), whose two canopy quads carry leaf materials: a shadow ray through
them keeps a fractional throughput. tests/test_query_cases_cpu.py asserts without a GPU, on the oracle, that every class of result
the GPU comparisons rely on is present in every set; no comparison leaves a ray out.

Kinds (KIND_SLICES): the centre rays (250 of them, spread evenly over the frame), rays from points in the scene's bounds grown by
15 % per side (so that some start inside the boxes and some outside the shell: backfaces and misses) in uniformly random
directions, the same with directions of lengths 0.1 .. 10, and axis-aligned directions: one non-zero component, or two in every
second ray, each with exact zeros in the others."""
import os

import numpy as np

import ids_cases as IC
import motion_cases as MC

N = 997
SCENES = ("cornell", "cornell_outside", "glass_mirror", "textured")
KIND_SLICES = {"centre": slice(0, 250), "inside": slice(250, 499), "unnormalised": slice(499, 748), "axis": slice(748, 997)}
MAX_T = np.float32(999999.0)          # the max_t of the library's own closest-hit rays, and of the oracle's trace_closest


def host(api, scene_dir, name, prefix="query_"):
    if name == "textured":
        from cudapathtracer_amd import scenes
        return api.HostScene(scenes.textured(os.path.join(scene_dir, prefix + name), name=prefix + name)["config"])
    return IC.host(api, scene_dir, IC.CAMERAS[name][0], prefix + name)


def camera(api, hs, name):
    return hs.camera() if name == "textured" else IC.camera(api, hs, name)


def arrays(hs):
    """The host scene's arrays with its own tree: what the oracle scene and Scene.from_arrays are made from."""
    return {k: hs.array(k) for k in MC.GEOMETRY + ("bvh", "indices")}


def lights_of_triangles(a):
    """Per ORIGINAL triangle the index of the light it is, or -1, from the triangles' own lightInd field."""
    n_lights = a["lights"].size // 80
    own = np.ascontiguousarray(a["mesh"]).view(np.uint8).reshape(-1, 80)[:, 64:68].copy().view(np.int32)[:, 0]
    return np.where((own >= 0) & (own < n_lights), own, -1).astype(np.int32)


def ray_set(O, cam, a, name):
    """[N, 6] float32 (o, d) of scene `name`; O: the oracle (its camera_ray gives the centre rays the library's passes trace)."""
    rng = np.random.default_rng(1000 + SCENES.index(name))
    centre = IC.oracle_centre_rays(O, cam, cam.w, cam.h)
    centre = centre[np.linspace(0, len(centre) - 1, 250).astype(np.int64)]
    pts = np.ascontiguousarray(a["points"]).view(np.float32).reshape(-1, 4)[:, :3]
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    ext = hi - lo

    def origins(k):
        return lo - 0.15 * ext + 1.3 * ext * rng.random((k, 3))

    def directions(k):
        d = rng.standard_normal((k, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    inside = np.concatenate([origins(249), directions(249)], 1)
    unnorm = np.concatenate([origins(249), directions(249) * (0.1 + 9.9 * rng.random((249, 1)))], 1)
    d = np.zeros((249, 3))
    rows = np.arange(249)
    first = rng.integers(0, 3, 249)
    d[rows, first] = rng.choice([-1.0, 1.0], 249)
    second = (first + 1 + rng.integers(0, 2, 249)) % 3
    d[rows[1::2], second[1::2]] = rng.choice([-1.0, 1.0], 249)[1::2] * (0.25 + rng.random(249)[1::2])
    axis = np.concatenate([origins(249), d], 1)
    rays = np.concatenate([centre, inside, unnorm, axis], 0).astype(np.float32)
    assert rays.shape == (N, 6) and ((rays[KIND_SLICES["axis"], 3:] == 0).sum(1) >= 1).all()
    return rays


def records(rays6, max_t=MAX_T):
    """[n, 8] float32 pt_ray records of [n, 6] rays: (o, max_t, d, pad = 0); max_t a scalar or one per ray."""
    rays6 = np.asarray(rays6, np.float32).reshape(-1, 6)
    out = np.zeros((len(rays6), 8), np.float32)
    out[:, 0:3] = rays6[:, 0:3]
    out[:, 3] = max_t
    out[:, 4:7] = rays6[:, 3:6]
    return out


def shadow_max_t(oi, of, seed=77):
    """One max_t per ray drawn AROUND the oracle's closest distances t: half of it (nothing below: clear), t itself (the hit is not
    below max_t: clear), the next float after t (exactly the closest triangle lies below: occluded, or attenuated by a leaf), twice t
    (whatever lies behind it too); a ray that hits nothing gets a distance in 0.5 .. 4."""
    rng = np.random.default_rng(seed)
    n = len(oi)
    t = of[:, 0].astype(np.float32)
    choice = rng.integers(0, 4, n)
    hit = oi[:, 0] == 1
    cand = np.stack([t * np.float32(0.5), t, np.nextafter(t, np.float32(np.inf)), t * np.float32(2.0)], 1).astype(np.float32)
    out = np.where(hit, cand[np.arange(n), choice], (0.5 + 3.5 * rng.random(n)).astype(np.float32)).astype(np.float32)
    return out


def classes(oi, of, thr, lights):
    """How many rays of a set fall into each class the comparisons rely on: closest (oi, of) at MAX_T, shadow throughput thr.
    partial: neither exactly 0 nor exactly 1, the product of leaf transmissions (with an unnormalised direction the reference's
    Fresnel term leaves [0, 1], and such a product may exceed 1: it is compared bit for bit like any other)."""
    hit = oi[:, 0] == 1
    top = thr.max(1)
    return {"hit": int(hit.sum()), "miss": int((~hit).sum()), "backface": int((hit & (oi[:, 3] != 0)).sum()),
            "light": int((hit & (lights[np.maximum(oi[:, 1], 0)] >= 0)).sum()), "occluded": int((top == 0).sum()),
            "clear": int((thr == 1).all(1).sum()), "partial": int(((top != 0) & ~(thr == 1).all(1)).sum())}
