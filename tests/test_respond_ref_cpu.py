"""The numpy restatement of the responsive history stage (tests/respond_ref.py), checked without a GPU on the inputs the GPU tests
reuse (tests/respond_cases.py: the CPU oracle's frames, which equal the library's bit for bit). The floors in respond_cases are
conditions on the INPUT, not tolerances."""
import numpy as np
import pytest

import motion_ref as M
import respond_cases as RC
import respond_ref as R
import temporal_ref as T
from util import assert_bits_equal

INF = float("inf")
CASES = [(w, h, change, kind) for (w, h) in RC.SIZES for change in RC.CHANGES for kind in ("identity", "pinhole")]


@pytest.fixture(scope="module")
def cases(api, oracle, scene_dir):
    assert hasattr(api.lib(), "pt_temporal_accumulate_respond"), "no responsive history stage to restate"
    out = {}
    for (w, h) in RC.SIZES:
        hs = RC.MC.cornell_host(api, scene_dir, "respond_cpu_%dx%d" % (w, h), w, h)
        for change in RC.CHANGES:
            for kind in ("identity", "pinhole"):
                out[(w, h, change, kind)] = RC.build(api, lambda: RC.OracleRenderer(api, oracle, hs), w, h, change, kind)
    return out


@pytest.mark.parametrize("key", CASES, ids=lambda k: "%dx%d-%s-%s" % k)
def test_an_infinite_threshold_is_the_base_restatement(cases, key):
    c = cases[key]
    want = T.accumulate(c["cam"], c["prev_cam"], c["S"], c["Q"], RC.SPP, RC.BATCHES, c["A"], c["N"], c["prev_n"], c["hist"], c["ln"], **T.DEFAULTS)
    if key[:2] != (5, 4):
        assert (want[1] > 1).sum() > 100                      # the history is found
    for radius in (1, 3):
        got = RC.restate(R, c, radius=radius, power=2, threshold=INF)
        assert_bits_equal(got[0], want[0], "hist"); assert_bits_equal(got[1], want[1], "hist_len")
        assert (got[2] == 1).all()
    wm = M.accumulate(c["cam"], c["prev_cam"], c["S"], c["Q"], RC.SPP, RC.BATCHES, c["A"], c["N"], c["prev_n"], c["hist"], c["ln"],
                      motion=c["motion"], **T.DEFAULTS)
    gm = RC.restate(R, c, motion=True, radius=2, power=4, threshold=INF)
    assert_bits_equal(gm[0], wm[0], "motion: hist"); assert_bits_equal(gm[1], wm[1], "motion: hist_len")
    wc = M.accumulate_cur(c["cam"], c["prev_cam"], c["cur"], c["N"], c["prev_n"], c["hist"], c["ln"], motion=c["motion"], **T.DEFAULTS)
    gc = RC.restate(R, c, form="cur", motion=True, radius=2, power=1, threshold=INF)
    assert_bits_equal(gc[0], wc[0], "cur, motion: hist"); assert_bits_equal(gc[1], wc[1], "cur, motion: hist_len")
    first = R.accumulate(c["cam"], None, c["S"], c["Q"], RC.SPP, RC.BATCHES, c["A"], c["N"], **R.DEFAULTS)
    assert_bits_equal(first[0], T.accumulate(c["cam"], None, c["S"], c["Q"], RC.SPP, RC.BATCHES, c["A"], c["N"])[0], "no history: the base function")
    assert (first[2] == 1).all()


def test_lambda_by_hand_on_a_five_by_five_case(api):
    """One surface, an identity camera, a history of e_h = 1, V_h = 0.01, N_h = 8 everywhere; the frame is e = 1 except a 3 x 3 block
    of e = 2 in the middle, V = 0.03. With radius 1 the centre pixel's window holds nine witnesses of d = (1, 1, 1), v = 0.04:
    D = (9, 9, 9), T = 243, Vs = 0.36, lim = k^2 Vs = 1.44 at k = 2, rho = 1.44 / 243. The image's corner pixel has a window of four with one
    such witness: D = (1, 1, 1), T = 3, lim = 4 (4 x 0.04) = 0.64: still over."""
    f32 = np.float32
    w = h = 5
    cam = api.make_camera(True, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 60.0, w, h)
    N = np.zeros((h, w, 4), f32); N[..., 2] = 1; N[..., 3] = 2
    hist = np.ones((h, w, 4), f32); hist[..., 3] = 0.01
    ln = np.full((h, w), 8, f32)
    cur = np.ones((h, w, 4), f32); cur[..., 3] = 0.03
    cur[1:4, 1:4, :3] = 2
    for power in (1, 2, 4):
        out, out_len, lam, _ = R.accumulate_cur(cam, None, cur, N, N, hist, ln, radius=1, power=power, threshold=2.0)
        nine = f32(f32(0.03) + f32(0.01))
        vs = f32(0)
        for _ in range(9):
            vs = f32(vs + nine)
        lim = f32(f32(4) * vs)
        rho = f32(lim / f32(243))
        want = {1: rho, 2: f32(rho * rho), 4: f32(f32(rho * rho) * f32(rho * rho))}[power]
        assert lam[2, 2] == want and abs(float(rho) - 1.44 / 243) < 1e-6
        # the corner of the image: its window of four holds the block's corner alone
        vs4 = f32(0)
        for _ in range(4):
            vs4 = f32(vs4 + nine)
        rho4 = f32(f32(f32(4) * vs4) / f32(3))
        assert lam[0, 0] == {1: rho4, 2: f32(rho4 * rho4), 4: f32(f32(rho4 * rho4) * f32(rho4 * rho4))}[power]
        n = min(f32(f32(want * f32(8)) + f32(1)), f32(32))
        assert out_len[2, 2] == n
        a = f32(f32(1) / n)
        assert out[2, 2, 0] == f32(f32(1) + f32(a * f32(f32(2) - f32(1))))
        keep = f32(f32(1) - a)
        assert out[2, 2, 3] == f32(f32(f32(keep * keep) * f32(0.01)) + f32(f32(a * a) * f32(0.03)))
    # an all-equal frame: d = 0 everywhere, nothing is shortened, whatever the threshold
    flat = np.ones((h, w, 4), f32); flat[..., 3] = 0.03
    assert (R.accumulate_cur(cam, None, flat, N, N, hist, ln, radius=3, power=4, threshold=1e-3)[2] == 1).all()
    # a neighbour on another surface (its normal turned away) does not count: the centre sees eight
    N2 = N.copy(); N2[1, 1, :3] = (1, 0, 0)
    lam2 = R.accumulate_cur(cam, None, cur, N2, N2, hist, ln, radius=1, power=1, threshold=2.0)[2]
    vs8 = f32(0)
    for _ in range(8):
        vs8 = f32(vs8 + f32(f32(0.03) + f32(0.01)))
    assert lam2[2, 2] == f32(f32(f32(4) * vs8) / f32(192))


@pytest.mark.parametrize("key", [k for k in CASES if k[3] == "identity"], ids=lambda k: "%dx%d-%s-%s" % k)
def test_the_change_shortens_histories_and_a_planted_equal_history_shortens_none(cases, key):
    c = cases[key]
    out, out_len, lam, _ = RC.restate(R, c, **R.DEFAULTS)
    base = T.accumulate(c["cam"], c["prev_cam"], c["S"], c["Q"], RC.SPP, RC.BATCHES, c["A"], c["N"], c["prev_n"], c["hist"], c["ln"], **T.DEFAULTS)
    short = lam < 1
    print("%s: lambda < 1 on %d of %d pixels" % (key, short.sum(), short.size))
    assert short.sum() >= RC.MIN_SHORTENED[key[:2]]
    assert ((lam >= 0) & (lam <= 1)).all()
    assert_bits_equal(out[~short], base[0][~short], "lambda 1: the base function"); assert_bits_equal(out_len[~short], base[1][~short], "lengths")
    assert (out_len[short] <= base[1][short]).all()
    # the history IS this frame (every witness has d = 0): no pixel is shortened at any threshold
    same = c["cur"].copy()
    eq = RC.restate(R, dict(c, hist=same, ln=np.where(same[..., 3] >= 0, np.float32(5), np.float32(0)).astype(np.float32)), form="cur",
                    radius=3, power=4, threshold=1e-3)
    assert (eq[2] == 1).all()


@pytest.mark.parametrize("key", CASES, ids=lambda k: "%dx%d-%s-%s" % k)
def test_hazards_are_skipped_and_the_fragile_share_stays_below_the_cap(cases, key):
    c, spots = RC.plant_hazards(cases[key])
    for form in ("sums", "cur"):
        for motion in (False, True):
            for radius in (1, 2, 3):
                out, out_len, lam, fragile = RC.restate(R, c, form, motion, radius=radius, power=2, threshold=R.DEFAULTS["threshold"])
                assert fragile.mean() <= RC.FRAGILE_CAP, (form, motion, radius, fragile.sum())
                for (y, x) in spots:
                    assert lam[y, x] == 1
                (y0, x0), (y1, x1), (y2, x2) = spots
                assert out[y0, x0, 3] == -1 and out_len[y0, x0] == 0 and out[y1, x1, 3] == -1
                # the history pixel with a non-finite e: the same neighbours' results as with no history there at all
                if form == "sums" and not motion and key[3] == "identity":
                    d = dict(c, hist=c["hist"].copy())
                    d["hist"][y2, x2, 3] = -1
                    alt = RC.restate(R, d, form, motion, radius=radius, power=2, threshold=R.DEFAULTS["threshold"])
                    others = np.ones(lam.shape, bool); others[y2, x2] = False
                    assert_bits_equal(alt[2][others], lam[others], "neighbours of the non-finite pixel")
                    assert_bits_equal(alt[0][others], out[others], "neighbours' histories")
    clean = RC.restate(R, cases[key], **R.DEFAULTS)
    assert clean[3].mean() <= RC.FRAGILE_CAP
