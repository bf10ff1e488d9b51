"""The numpy restatement of the motion pass through mirrors and glass (tests/motion_chain_ref.py), checked without a GPU on the input
the GPU tests reuse (tests/motion_chain_cases.py, scene A): hits and guides are the CPU oracle's along the centre rays, link by link;
moments are postfx_cases' synthetic ones. The floors are conditions on the INPUT, not tolerances.

Counts of the float32 restatement on scene A at 64 x 40, still camera, max_links 1 (2 and 8 give the same: one mirror): 125 pixels
moved, 18 of them seen through the mirror (links >= 1 and motion.w == 1), 12 of those rescued (motion_ref.rescued on the chain
guides); first-hit motion (max_links 0) reports 107 moved pixels and none through the mirror."""
import numpy as np
import pytest

import aov_chain_ref as AC
import motion_cases as MC
import motion_chain_cases as CC
import motion_ref as M
import postfx_cases as PC
import temporal_ref as T
from test_temporal import _cams
from util import assert_bits_equal

MIN_THROUGH, MIN_RESCUED = 12, 6
W, H = CC.W, CC.H
LINKS = (1, 2, 8)


@pytest.fixture(scope="module")
def case(api, oracle, scene_dir):
    assert hasattr(api.lib(), "pt_render_motion_chain"), "no motion-chain pass to restate"
    hs = CC.scene_a(api, scene_dir, "mchain_cpu")
    old, new = MC.arrays(hs), CC.moved_box(hs)
    leaf = hs.info["leaf_size"]
    o_old, o_new = MC.oracle_scene(oracle, old, leaf), MC.oracle_scene(oracle, new, leaf)
    mats = AC.Materials(o_new)
    out = {"hs": hs, "old": old, "new": new, "o_new": o_new, "mats": mats, "leaf": leaf}
    still = _cams(api, "identity", W, H, 1)[0]
    moving = _cams(api, "pinhole", W, H, 4)[2:4]
    for name, cam_prev, cam in (("still", still, still), ("moving", moving[0], moving[1])):
        rays = CC.oracle_centre_rays(oracle, cam, W, H)
        A0, N0, _ = CC.chain_guides(o_old, AC.Materials(o_old), CC.oracle_centre_rays(oracle, cam_prev, W, H), 2, W, H)
        A1, N1, L1 = CC.chain_guides(o_new, mats, rays, 2, W, H)
        f0, f1 = PC.moments(A0, N0, 11), PC.moments(A1, N1, 12)
        hist, ln, _ = T.accumulate(cam_prev, None, f0[0], f0[1], PC.SPP, PC.BATCHES, f0[2], f0[3])
        ln = (ln * np.float32(3)).astype(np.float32)
        out[name] = {"rays": rays, "prev": cam_prev, "cam": cam, "f1": f1, "N0": N0, "links": L1, "hist": hist, "ln": ln,
                     "want": CC.want_motion(o_new, mats, rays, 2, new, old, W, H)}
    return out


def _first_hit(case, rays, new, old):
    oi, of, _ = case["o_new"].trace_closest(rays)
    return M.motion(new["points"], None if old is None else old["points"], new["mesh"], (oi[:, 0] == 1, of[:, 1], of[:, 2], oi[:, 1])).reshape(H, W, 4)


@pytest.mark.parametrize("name", ["still", "moving"])
def test_no_links_is_the_first_hit_pass(case, name):
    c = case[name]
    first = _first_hit(case, c["rays"], case["new"], case["old"])
    assert (first[..., 3] == 1).sum() >= 16
    zero = CC.want_motion(case["o_new"], case["mats"], c["rays"], 0, case["new"], case["old"], W, H)
    assert_bits_equal(zero["motion"], first, "max_links 0")
    assert not zero["links"].any()
    for ml in LINKS:
        r = CC.want_motion(case["o_new"], case["mats"], c["rays"], ml, case["new"], case["old"], W, H)
        direct = r["links"] == 0
        assert direct.sum() > 100 and (~direct).sum() > 100
        assert_bits_equal(r["motion"][direct], first[direct], "max_links %d: the pixels without a link" % ml)
        assert np.array_equal(r["links"], c["links"])          # (one mirror: the guide of max_links 2 has every chain)
        assert set(np.unique(r["motion"][..., 3])) <= {0.0, 1.0} and not r["motion"][r["motion"][..., 3] == 0].any()


@pytest.mark.parametrize("name", ["still", "moving"])
def test_equal_or_no_previous_positions_are_static(case, name):
    c = case[name]
    for ml in (0,) + LINKS:
        for old in (case["new"], None):
            assert not CC.want_motion(case["o_new"], case["mats"], c["rays"], ml, case["new"], old, W, H)["motion"].any()


def test_a_moving_mirror_zeroes_what_is_seen_through_it(case, oracle):
    """The back wall's own vertices pushed back as well: every pixel whose chain passes the wall is static, the others are not."""
    both = CC.moved_box(case["hs"])
    wall = CC.back_wall_vertices(case["old"])
    assert len(wall) == 4
    both["points"].view(np.float32).reshape(-1, 4)[wall, 2] -= np.float32(0.05)
    osc = MC.oracle_scene(oracle, both, case["leaf"])
    rays = case["still"]["rays"]
    r = CC.want_motion(osc, AC.Materials(osc), rays, 2, both, case["old"], W, H)
    through = r["links"] >= 1
    assert through.sum() > 100 and r["link_moved"][through].all()
    assert not r["motion"][through].any()
    assert (r["motion"][~through][:, 3] == 1).sum() >= 16
    # the first hit on the moving mirror itself, where the chain falls back to it (the cap): pt_render_motion's pixel, not zero
    capped = CC.want_motion(osc, AC.Materials(osc), rays, 0, both, case["old"], W, H)
    assert (capped["motion"][through][:, 3] == 1).all()


def test_the_box_in_the_mirror_moves_by_the_mirrored_shift(case):
    """A rigid translation t seen in ONE planar mirror with normal n: the motion point is V - (t - 2 (t . n) n), V the virtual image
    of the hit (the centre ray at the chain guide's depth: a few ulps)."""
    c = case["still"]
    r = c["want"]
    mv = r["motion"]
    through = (r["links"] >= 1) & (mv[..., 3] == 1)
    print("moved pixels: %d, seen through the mirror: %d" % ((mv[..., 3] == 1).sum(), through.sum()))
    assert through.sum() >= MIN_THROUGH
    assert (r["links"][through] == 1).all() and (r["reflections"][through] == 1).all() and not r["link_moved"].any()
    o, d = PC.centre_rays(c["cam"])
    V = o + d * c["f1"][3][..., 3:4].astype(np.float64)
    t, n = np.array(MC.SHIFT, np.float64), np.array((0.0, 0.0, 1.0))
    np.testing.assert_allclose((V - mv[..., :3])[through], np.broadcast_to(t - 2 * t.dot(n) * n, (through.sum(), 3)), atol=1e-5)
    direct = (r["links"] == 0) & (mv[..., 3] == 1)
    np.testing.assert_allclose((V - mv[..., :3])[direct], np.broadcast_to(t, (direct.sum(), 3)), atol=1e-5)      # (§19's form)


def test_pixels_seen_through_the_mirror_are_rescued(case):
    c = case["still"]
    S, Q, A, N = c["f1"]
    mv = c["want"]["motion"]
    through = (c["want"]["links"] >= 1) & (mv[..., 3] == 1)
    resc = M.rescued(c["cam"], N, c["N0"], mv) & through
    print("seen through the mirror: %d, rescued: %d" % (through.sum(), resc.sum()))
    assert through.sum() >= MIN_THROUGH and resc.sum() >= MIN_RESCUED
    first = _first_hit(case, c["rays"], case["new"], case["old"])
    assert not first[through].any()                          # first-hit motion reports the static mirror there
    base = T.accumulate(c["cam"], c["cam"], S, Q, PC.SPP, PC.BATCHES, A, N, c["N0"], c["hist"], c["ln"], **T.DEFAULTS)
    fh = M.accumulate(c["cam"], c["cam"], S, Q, PC.SPP, PC.BATCHES, A, N, c["N0"], c["hist"], c["ln"], motion=first, **T.DEFAULTS)
    got = M.accumulate(c["cam"], c["cam"], S, Q, PC.SPP, PC.BATCHES, A, N, c["N0"], c["hist"], c["ln"], motion=mv, **T.DEFAULTS)
    assert (base[1][resc] == 1).all() and (fh[1][resc] == 1).all() and (got[1][resc] > 1).all()


@pytest.mark.parametrize("name", ["still", "moving"])
def test_static_pixels_of_accumulate_are_the_base_restatement(case, name):
    c = case[name]
    S, Q, A, N = c["f1"]
    mv = c["want"]["motion"]
    static = mv[..., 3] != 1
    base = T.accumulate(c["cam"], c["prev"], S, Q, PC.SPP, PC.BATCHES, A, N, c["N0"], c["hist"], c["ln"], **T.DEFAULTS)
    got = M.accumulate(c["cam"], c["prev"], S, Q, PC.SPP, PC.BATCHES, A, N, c["N0"], c["hist"], c["ln"], motion=mv, **T.DEFAULTS)
    assert static.sum() > 1000 and (base[1] > 1).sum() > 100
    assert_bits_equal(got[0][static], base[0][static], name + ": static pixels")
    assert_bits_equal(got[1][static], base[1][static], name + ": static pixels' lengths")
    assert not np.array_equal(got[1], base[1])
