"""The pair kernels' leaf loop folds a record's high mask dword only where it is non-zero (pt_trace.h: trace_pair_flat under ARMS;
DESIGN.md §6, round 11). The skipped instructions compute x | (c ? 0 : 0), so no frame changes: every frame here, 32 x 24 at 4 spp,
depth 8, MIS, is compared bit for bit (NaNs must coincide) with a live oracle render. The scenes are the smallest that put a record
into each case the branch distinguishes, and what each table holds is asserted on the host first (pt_box_table.h through
tests/box_table_driver.hip), so that a scene generator that drifts cannot turn a case vacuous:

  open_floor    28 triangles: every record's high word is empty                                              SIMPLE
  tri33         33 triangles (a shell, a box, an open box with one triangle cut away): one high bit          SIMPLE
  cornell       the headline's 36 triangles: high bits 32..35, one record with only high bits                SIMPLE
  cornell60     60 triangles (two more boxes): records with an empty low word, records with an empty high
                word, and records with bits in both (a shared box and a leaf across triangles 31 / 32)       SIMPLE
  cornell60m    the same with a mirror tall box: the straddling records in the LEAN pair kernel              LEAN
cornell60 is rendered a second time with an unrelated frame between: the halves keep nothing across passes or launches."""
import os

import numpy as np
import pytest

import box_table_cases as BT
from util import assert_bits_equal

W, H, SPP, DEPTH = 32, 24, 4, 8
SIMPLE = dict(flat_pair=True, leaf_table=True, simple=True)
LEAN = dict(flat_pair=True, leaf_table=True, simple=False, lean=True)
FLAGS = {"open_floor": SIMPLE, "tri33": SIMPLE, "cornell": SIMPLE, "cornell60": SIMPLE, "cornell60m": LEAN}
LO = 0xffffffff


def _tri33(outdir):
    """The Cornell shell (12 triangles), a closed box (12) and a box without its bottom whose last side is one triangle (9)."""
    from cudapathtracer_amd import scenes
    meshes, zc = scenes._shell(W / H)
    closed = scenes.Mesh("closed", 2)
    scenes._box(closed, -0.4, zc - 0.3, 0.3, 1.0, 0.3, -1.0 + 1e-3, 17.0)
    cut = scenes.Mesh("cut", 2)
    scenes._box(cut, 0.5, zc + 0.3, 0.25, 0.5, 0.25, -1.0 + 1e-3, -18.0, with_bottom=False)
    cut.faces[-1] = cut.faces[-1][:3]
    return scenes._emit(os.path.join(str(outdir), "words_tri33"), "words_tri33", meshes + [closed, cut], W, H, SPP, DEPTH)["config"]


def _config(scene_dir, case):
    from cudapathtracer_amd import scenes
    if case == "open_floor":
        return BT.open_floor(scene_dir, W, H, SPP, DEPTH)
    if case == "tri33":
        return _tri33(scene_dir)
    kw = {"cornell": {}, "cornell60": dict(extra_boxes=2), "cornell60m": dict(extra_boxes=2, tall_material=19)}[case]
    return scenes.cornell(os.path.join(str(scene_dir), "words_" + case), W, H, SPP, DEPTH, name="words_" + case, **kw)["config"]


@pytest.fixture(scope="module")
def masks(api, scene_dir, tmp_path_factory):
    """case -> (triangles, the records' masks), from the host's table builder."""
    d = tmp_path_factory.mktemp("mask_words")
    t = {c: BT.pnodes_from_bvh(api.HostScene(_config(scene_dir, c)).array("bvh")) for c in FLAGS}
    r = BT.run_driver(BT.build_driver(d), d, t)
    return {c: (t[c][1], [m for m, _ in r[c]["records"]]) for c in FLAGS}


def test_the_scenes_hold_the_cases_they_are_there_for(masks):
    n = {c: v[0] for c, v in masks.items()}
    kinds = {c: (sum(1 for m in ms if m >> 32 == 0), sum(1 for m in ms if m & LO == 0), sum(1 for m in ms if m & LO and m >> 32)) for c, (_, ms) in masks.items()}
    print(n, kinds)                                                 # (records with an empty high word, with an empty low word, with bits in both)
    assert n == {"open_floor": 28, "tri33": 33, "cornell": 36, "cornell60": 60, "cornell60m": 60}
    for c, (nt, ms) in masks.items():
        union = 0
        for m in ms:
            assert m and union & m == 0
            union |= m
        assert union == (1 << nt) - 1, c
    assert kinds["open_floor"][1:] == (0, 0) and kinds["open_floor"][0] == len(masks["open_floor"][1])          # no high bit anywhere
    assert [m >> 32 for m in masks["tri33"][1] if m >> 32] == [1]                                                # a single high bit
    assert kinds["cornell"][0] >= 10 and kinds["cornell"][1] >= 1 and sum(bin(m >> 32).count("1") for m in masks["cornell"][1]) == 4
    for c in ("cornell60", "cornell60m"):
        assert kinds[c][0] >= 1 and kinds[c][1] >= 1 and kinds[c][2] >= 1, (c, kinds[c])
        assert any(m & (1 << 31) and m & (1 << 32) for m in masks[c][1]), "a leaf across triangles 31 / 32"


_FRAMES = {}      # config -> the oracle's frame: rendered once, read by every test below, never written to


def _oracle(oracle, cfg):
    if cfg not in _FRAMES:
        frame = oracle.OracleScene(cfg).render(threads=8)[0]         # size, spp, depth, integrator: the scene file's
        frame.setflags(write=False)
        assert np.isfinite(frame[..., :3]).mean() >= 0.99 and float(np.nan_to_num(frame[..., :3], nan=0.0, posinf=0.0, neginf=0.0).sum()) != 0.0
        _FRAMES[cfg] = frame
    return _FRAMES[cfg]


def _render(api, cfg, case):
    hs = api.HostScene(cfg)
    sc = api.Scene(hs)
    got, _ = sc.render(hs.camera(), W, H, SPP, DEPTH)               # MIS
    fl = sc.flags()
    assert {k: fl[k] for k in FLAGS[case]} == FLAGS[case], (case, fl)
    assert sc.queue_stalls() == 0
    sc.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(FLAGS))
def test_frames_equal_the_oracle(api, oracle, gpu_ready, scene_dir, case):
    cfg = _config(scene_dir, case)
    assert_bits_equal(_render(api, cfg, case), _oracle(oracle, cfg), case)


@pytest.mark.gpu
def test_the_straddling_scene_twice_with_another_frame_between(api, oracle, gpu_ready, scene_dir):
    """cornell60, then the 28-triangle scene whose records have no high word at all, then cornell60 again in the same process."""
    cfg = _config(scene_dir, "cornell60")
    first = _render(api, cfg, "cornell60")
    other = _render(api, _config(scene_dir, "open_floor"), "open_floor")
    assert np.isfinite(other[..., :3]).mean() >= 0.99
    second = _render(api, cfg, "cornell60")
    assert_bits_equal(second, first, "cornell60, again")
    assert_bits_equal(first, _oracle(oracle, cfg), "cornell60")
