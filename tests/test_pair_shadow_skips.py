"""Shadow work the image never reads, left out of the timed kernels:

  A. the DEFER logic step (pt_path.h: bounce_core) starts the NEE shadow ray only when its term is valid (light_pdf > EPSILON) —
     every hit on Cornell's ceiling samples a light that faces away from it;
  B. the pair pass of the SIMPLE pair kernel (pt_trace.h: trace_pair_flat) does not test a shadow ray against the light triangle
     it was aimed at: the bounce has made that very test, and its result is the ray's own bound.

Both are exact by construction; every frame here is compared bit for bit with a live oracle render (NaNs must coincide)."""
import os

import numpy as np
import pytest

from util import assert_bits_equal

MIXED = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4])      # bench.py's cornell_mixed
# name: (scenes.cornell arguments, width, height, spp, options, flags the launch must report)
CASES = {
    "cornell": (dict(), 64, 40, 32, {}, dict(flat_pair=True, simple=True)),
    "cornell_ceiling_light": (dict(ceiling_light=True), 64, 40, 32, {}, dict(flat_pair=True, simple=True)),
    "cornell_mixed": (MIXED, 64, 40, 16, {}, dict(flat_pair=True, simple=False, lean=True)),
    # change A outside the pair pass: the REFILL kernels scenes in HBM run, on the smallest scene there is — its 4-wave form
    # (what a frame of few tiles gets) and the 8-wave production kernel
    "cornell_refill_4wave": (dict(), 32, 24, 8, {"onchip": 0}, dict(flat_pair=False, onchip=False, refill=True, hbm_kernel=False)),
    "cornell_refill_hbm": (dict(), 32, 24, 8, {"onchip": 0, "waves_hbm": 2}, dict(flat_pair=False, onchip=False, refill=True, hbm_kernel=True)),
}


def _config(scene_dir, case):
    from cudapathtracer_amd import scenes
    kw, w, h, spp, _, _ = CASES[case]
    name = "skips_" + case.replace("_refill_4wave", "").replace("_refill_hbm", "")      # the three REFILL / plain cases share one scene
    return scenes.cornell(os.path.join(scene_dir, name + "_%dx%d" % (w, h)), w, h, spp, 8, name=name, **kw)["config"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_frames_equal_the_oracle(api, oracle, gpu_ready, scene_dir, case):
    _, w, h, spp, opts, want_flags = CASES[case]
    cfg = _config(scene_dir, case)
    hs = api.HostScene(cfg)
    sc = api.Scene(hs, options=opts)
    got, _ = sc.render(hs.camera(), w, h, spp, 8)                 # depth 8, MIS
    fl = sc.flags()
    assert {k: fl[k] for k in want_flags} == want_flags, fl
    assert sc.queue_stalls() == 0
    want, _, _ = oracle.OracleScene(cfg).render(threads=8)
    assert np.isfinite(want[..., :3]).mean() > 0.99 and float(np.nan_to_num(want[..., :3], nan=0.0, posinf=0.0, neginf=0.0).sum()) > 0.0
    assert_bits_equal(got, want, case)


def _records(hs):
    """(light, packed triangle) vertex data as the kernels see it: a, b - a, c - a in binary32, triangles in leaf order."""
    pts = hs.array("points").view(np.float32).reshape(-1, 4)[:, :3]
    mesh = hs.array("mesh").view(np.int32).reshape(-1, 20)
    lights = hs.array("lights").view(np.int32).reshape(-1, 20)
    order = hs.array("indices").view(np.int32)

    def rec(t):
        a, b, c = pts[t[0]], pts[t[1]], pts[t[2]]
        return np.concatenate([a, b - a, c - a]).astype(np.float32).view(np.uint32)
    return [rec(t) for t in lights], [rec(mesh[i]) for i in order], [int(mesh[i][16]) for i in order]


@pytest.mark.parametrize("case", ["cornell", "cornell_ceiling_light", "cornell_mixed"])
def test_every_light_names_its_triangle(api, scene_dir, case):
    """CPU only. pt_light_triangles: the stored index is >= 0 for every light of the scenes above, and the triangle it names has the
    light's v0, e1, e2 bit for bit (checked here independently of the library) and the light's index as its lightInd."""
    hs = api.HostScene(_config(scene_dir, case))
    idx = api.light_triangles(hs)
    lights, tris, light_ind = _records(hs)
    assert len(idx) == len(lights) >= 2
    for i, p in enumerate(idx):
        assert 0 <= p < len(tris), (i, p)
        assert np.array_equal(tris[p], lights[i]) and light_ind[p] == i, (i, p)


def test_a_permuted_light_names_no_triangle(api, scene_dir):
    """CPU only. A light whose vertices are in another order than its triangle's is the same set of points but not the same test
    (other v0, e1, e2): the bitwise check fails and the shadow rays aimed at it are tested against every triangle, as before."""
    hs = api.HostScene(_config(scene_dir, "cornell"))
    arrays = {k: hs.array(k) for k in ("points", "normals", "uvs", "mesh", "lights", "bvh", "indices", "materials")}
    good = api.light_triangles(arrays=arrays)
    assert np.array_equal(good, api.light_triangles(hs)) and (good >= 0).all()
    lights = arrays["lights"].view(np.int32).reshape(-1, 20).copy()
    lights[0, [0, 1, 2]] = lights[0, [1, 2, 0]]                   # light 0: (a, b, c) -> (b, c, a)
    arrays["lights"] = lights.view(np.uint8).reshape(-1)
    bad = api.light_triangles(arrays=arrays)
    assert bad[0] == -1 and np.array_equal(bad[1:], good[1:]), (good, bad)
