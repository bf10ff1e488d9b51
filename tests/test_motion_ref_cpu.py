"""The numpy restatement of the motion pass and of the history stage with motion (tests/motion_ref.py), checked without a GPU on the
input the GPU tests reuse (tests/motion_cases.py): hits and guides are the CPU oracle's along the centre rays, moments are
postfx_cases' synthetic ones. The floors below are conditions on the INPUT, not tolerances: a scene that misses them needs a larger
displacement."""
import numpy as np
import pytest

import motion_cases as MC
import motion_ref as M
import postfx_cases as PC
import temporal_ref as T
from test_temporal import _cams
from util import assert_bits_equal

MIN_MOVED, MIN_RESCUED = 16, 4


@pytest.fixture(scope="module")
def case(api, oracle, scene_dir):
    assert hasattr(api.lib(), "pt_render_motion") and hasattr(api, "temporal_accumulate_motion"), "no motion pass to restate"
    hs = MC.cornell_host(api, scene_dir, "motion_cpu")
    old, new = MC.arrays(hs), MC.moved_arrays(hs)
    leaf = hs.info["leaf_size"]
    still = _cams(api, "identity", MC.W, MC.H, 1)[0]
    moving = _cams(api, "pinhole", MC.W, MC.H, 4)[2:4]
    out = {"old": old, "new": new, "still": still, "moving": moving}
    o_old, o_new = MC.oracle_scene(oracle, old, leaf), MC.oracle_scene(oracle, new, leaf)
    for name, cam_prev, cam in (("still", still, still), ("moving", moving[0], moving[1])):
        _, A0, N0 = MC.oracle_centre_hits(oracle, o_old, cam_prev)
        hits, A1, N1 = MC.oracle_centre_hits(oracle, o_new, cam)
        f0, f1 = PC.moments(A0, N0, 11), PC.moments(A1, N1, 12)
        hist, ln, _ = T.accumulate(cam_prev, None, f0[0], f0[1], PC.SPP, PC.BATCHES, f0[2], f0[3])
        ln = (ln * np.float32(3)).astype(np.float32)
        out[name] = {"hits": hits, "prev": cam_prev, "cam": cam, "f1": f1, "N0": N0, "hist": hist, "ln": ln,
                     "motion": M.motion(new["points"], old["points"], new["mesh"], hits).reshape(MC.H, MC.W, 4)}
    return out


@pytest.mark.parametrize("name", ["still", "moving"])
def test_equal_positions_are_static_and_the_base_restatement(case, name):
    c = case[name]
    S, Q, A, N = c["f1"]
    zero = M.motion(case["new"]["points"], case["new"]["points"], case["new"]["mesh"], c["hits"]).reshape(MC.H, MC.W, 4)
    assert not zero.any()
    assert not M.motion(case["new"]["points"], None, case["new"]["mesh"], c["hits"]).any()
    want = T.accumulate(c["cam"], c["prev"], S, Q, PC.SPP, PC.BATCHES, A, N, c["N0"], c["hist"], c["ln"], **T.DEFAULTS)
    assert (want[1] > 1).sum() > 100                        # the history is found
    for mv in (zero, None):
        got = M.accumulate(c["cam"], c["prev"], S, Q, PC.SPP, PC.BATCHES, A, N, c["N0"], c["hist"], c["ln"], motion=mv, **T.DEFAULTS)
        assert_bits_equal(got[0], want[0], name + ": hist"); assert_bits_equal(got[1], want[1], name + ": hist_len")
        assert np.array_equal(got[2], want[2])
    first = M.accumulate(c["cam"], None, S, Q, PC.SPP, PC.BATCHES, A, N, motion=c["motion"])
    assert_bits_equal(first[0], T.accumulate(c["cam"], None, S, Q, PC.SPP, PC.BATCHES, A, N)[0], "no history: the motion is not read")


def test_the_moved_box_is_seen_and_the_motion_is_its_displacement(case):
    c = case["still"]
    mv = c["motion"]
    moved = mv[..., 3] == 1
    print("moved pixels: %d of %d" % (moved.sum(), moved.size))
    assert moved.sum() >= MIN_MOVED
    assert not mv[~moved].any() and set(np.unique(mv[..., 3])) <= {0.0, 1.0}
    # a rigid translation: the previous point is the hit point minus the shift (the hit point from the guide's depth: a few ulps)
    o, d = PC.centre_rays(c["cam"])
    P = o + d * c["f1"][3][..., 3:4].astype(np.float64)
    np.testing.assert_allclose((P - mv[..., :3])[moved], np.broadcast_to(MC.SHIFT, (moved.sum(), 3)), atol=1e-5)
    tri = c["hits"][3].reshape(MC.H, MC.W)
    verts = M.triangle_vertices(case["new"]["mesh"])[tri[moved]]
    assert ((verts >= 48) & (verts < 72)).all()


def test_pixels_are_rescued(case):
    c = case["still"]
    S, Q, A, N = c["f1"]
    resc = M.rescued(c["cam"], N, c["N0"], c["motion"])
    print("rescued pixels: %d" % resc.sum())
    assert resc.sum() >= MIN_RESCUED
    base = T.accumulate(c["cam"], c["cam"], S, Q, PC.SPP, PC.BATCHES, A, N, c["N0"], c["hist"], c["ln"], **T.DEFAULTS)
    got = M.accumulate(c["cam"], c["cam"], S, Q, PC.SPP, PC.BATCHES, A, N, c["N0"], c["hist"], c["ln"], motion=c["motion"], **T.DEFAULTS)
    assert (base[1][resc] == 1).all() and (got[1][resc] > 1).all()
    static = c["motion"][..., 3] != 1
    assert_bits_equal(got[0][static], base[0][static], "static pixels: the identity path")
    assert_bits_equal(got[1][static], base[1][static], "static pixels: lengths")
    # the cur form on the same working pixels is the same blend
    cur = np.concatenate([T.frame_ev(S, Q, PC.SPP, PC.BATCHES, A)[1], T.frame_ev(S, Q, PC.SPP, PC.BATCHES, A)[2][..., None]], -1).astype(np.float32)
    skip = T.frame_ev(S, Q, PC.SPP, PC.BATCHES, A)[3]
    cur[skip, 3] = -1
    gc = M.accumulate_cur(c["cam"], None, cur, N, c["N0"], c["hist"], c["ln"], motion=c["motion"], **T.DEFAULTS)
    assert_bits_equal(gc[0][~skip], got[0][~skip], "cur form"); assert_bits_equal(gc[1], got[1], "cur form: lengths")
