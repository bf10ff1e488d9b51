"""The timed pair kernels test each DISTINCT leaf box once, with the triangle masks ready in the table and the records grouped by
the interval they share on one axis, which is computed once per group (pt_box_table.h; pt_trace.h: trace_pair_flat under ARMS;
DESIGN.md §6, round 9). Equal boxes give equal slab results and the axes may enter the test in any order, so no result changes: every
frame here is compared bit for bit (NaNs must coincide) with a live oracle render and with the generic pair kernel
(megakernel_flat2<0, false, false>, options {"simple": 0, "lean": 0}), which keeps the loop over the leaves and its machine code.

  cornell32, mixed32   the golden scenes at 4 spp: the SIMPLE (headline) and the LEAN pair kernel
  fuzz_*               scenes.fuzz seeds chosen on the CPU (tests/box_table_cases.py: FUZZ; tests/test_box_table.py checks what each
                       one is there for): an odd and an even record count; shared boxes whose mask has bits on both sides of bit 32;
                       mask bits up to 62; records grouped on x, on y and on z; groups of one record and of up to five
  open_floor           no duplicate box at all: no fuzz scene has that (the Cornell shell's wall leaves always share the whole-scene
                       box), so a floor, a light and two boxes without walls
  axis_parallel        no lens, no jitter: the centre column's d.x and the centre row's d.y are exactly 0, so the waves with those
                       pixels take the lockstep node walk (inv_is_regular) while the others read the table
  update               pt_scene_update_vertices moves the tall box: the table is rebuilt with the tree, the frame equals the oracle's
                       render of the moved scene"""
import os

import numpy as np
import pytest

import box_table_cases as BT
from conftest import golden_scene
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

GENERIC = {"simple": 0, "lean": 0}
SIMPLE = dict(flat_pair=True, leaf_table=True, simple=True)
LEAN = dict(flat_pair=True, leaf_table=True, simple=False, lean=True)
ON_AXIS = (False, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 0.0, 2.0, 0.0)      # as tests/test_logic_arms.py: pinhole off, aperture 0, jitter 0
GOLDEN_SPP, DEPTH = 4, 8


def _frames(api, oracle, hs, cfg, cam, w, h, spp, depth, want_flags, what):
    """The timed pair kernel's frame and the generic pair kernel's, both against the oracle's."""
    want = oracle.OracleScene(cfg).render(camera=np.frombuffer(cam.tobytes(), np.uint8).copy(), width=w, height=h, spp=spp, max_depth=depth,
                                          integrator=0, threads=8)[0]
    assert np.isfinite(want[..., :3]).mean() > 0.99 and float(np.nan_to_num(want[..., :3], nan=0.0, posinf=0.0, neginf=0.0).sum()) > 0.0
    for opts, flags in (({}, want_flags), (GENERIC, dict(flat_pair=True, leaf_table=True, simple=False, lean=False))):
        sc = api.Scene(hs, options=opts)
        got, _ = sc.render(cam, w, h, spp, depth)                  # MIS
        fl = sc.flags()
        assert {k: fl[k] for k in flags} == flags, (what, opts, fl)
        assert sc.queue_stalls() == 0
        assert_bits_equal(got, want, "%s %s" % (what, opts))
        sc.close()


@pytest.mark.parametrize("scene,flags", [("cornell32", SIMPLE), ("mixed32", LEAN)])
def test_golden_scenes_equal_the_oracle_and_the_generic_kernel(api, oracle, gpu_ready, scene, flags):
    cfg = golden_scene(scene)
    hs = api.HostScene(cfg)
    _frames(api, oracle, hs, cfg, hs.camera(), hs.info["width"], hs.info["height"], GOLDEN_SPP, DEPTH, flags, scene)


@pytest.mark.parametrize("seed", sorted(BT.FUZZ))
def test_fuzz_scenes_equal_the_oracle_and_the_generic_kernel(api, oracle, gpu_ready, scene_dir, seed):
    cfg = BT.fuzz_config(scene_dir, seed)
    hs = api.HostScene(cfg)
    i = hs.info
    _frames(api, oracle, hs, cfg, hs.camera(), i["width"], i["height"], 3, 6, dict(flat_pair=True, leaf_table=True), "fuzz %d" % seed)


def test_a_scene_without_a_duplicate_box(api, oracle, gpu_ready, scene_dir):
    cfg = BT.open_floor(scene_dir)
    hs = api.HostScene(cfg)
    _frames(api, oracle, hs, cfg, hs.camera(), 32, 24, 4, DEPTH, SIMPLE, "open floor")


def test_axis_parallel_rays_walk_the_nodes_beside_the_table(api, oracle, gpu_ready, scene_dir):
    from cudapathtracer_amd import scenes
    w, h, spp = 32, 24, 4
    cfg = scenes.cornell(os.path.join(scene_dir, "boxes_axis"), w, h, spp, DEPTH, name="boxes_axis")["config"]
    hs = api.HostScene(cfg)
    pinhole, pos, rot, aperture, focal, jitter = ON_AXIS
    cam = api.make_camera(pinhole, pos, rot, scenes.FOV, w, h, aperture, focal)
    cam.antiAliasJitterDist = jitter
    rays = np.array([oracle.camera_ray(np.frombuffer(cam.tobytes(), np.uint8).copy(), x, y) for x, y in ((w // 2, 3), (5, h // 2), (5, 3))])
    assert rays[0, 3] == 0.0 and rays[1, 4] == 0.0 and (rays[2, 3:6] != 0.0).all(), rays      # tile 8x8: the other tiles' rays are regular
    _frames(api, oracle, hs, cfg, cam, w, h, spp, DEPTH, SIMPLE, "axis-parallel")


def test_the_table_is_rebuilt_by_a_vertex_update(api, oracle, gpu_ready):
    cfg = golden_scene("cornell32")
    hs = api.HostScene(cfg)
    w, h, leaf = hs.info["width"], hs.info["height"], hs.info["leaf_size"]
    cam = hs.camera()
    a = {k: hs.array(k) for k in ("points", "normals", "uvs", "mesh", "lights", "materials", "textures")}
    sc = api.Scene.from_mesh(hs)
    before, _ = sc.render(cam, w, h, GOLDEN_SPP, DEPTH)
    a["points"].view(np.float32).reshape(-1, 4)[48:72, :3] += np.array([0.07, 0.0, 0.05], np.float32)      # cornell32's tall box
    sc.update_vertices(a["points"])
    got, _ = sc.render(cam, w, h, GOLDEN_SPP, DEPTH)
    fl = sc.flags()
    assert fl["flat_pair"] and fl["simple"] and fl["leaf_table"], fl
    bvh, idx, _ = oracle.build_bvh(a["points"], a["mesh"], leaf)
    moved = dict(a, bvh=bvh, indices=idx.view(np.uint8))
    # the move changes leaf boxes, so a table kept from before the update would test the wrong boxes
    old = BT.pnodes_from_bvh(hs.array("bvh"))[0]
    new = BT.pnodes_from_bvh(bvh)[0]
    assert old.shape != new.shape or old.tobytes() != new.tobytes()
    want = oracle.OracleScene(arrays=moved).render(camera=np.frombuffer(cam.tobytes(), np.uint8).copy(), width=w, height=h, spp=GOLDEN_SPP,
                                                   max_depth=DEPTH, integrator=0)[0]
    assert not np.array_equal(got, before), "the change did not reach the image"
    assert_bits_equal(got, want, "after pt_scene_update_vertices")
    sc.close()
