"""tests/postfx_cases.py without a GPU: the analytic frames against their closed form, and the restatements alone (temporal_ref,
upsample_ref, denoise_ref, denoise_var_ref) on every case tests/test_postfx_edges.py runs on the kernels: each case reaches the
branch it is named for, the fragile masks stay under test_temporal.py's cap, and the off-default parameters are told apart."""
import numpy as np
import pytest

import postfx_cases as C
import temporal_ref as T
import upsample_ref as U
from denoise_ref import denoise as denoise_ref
from denoise_var_ref import denoise_var as denoise_var_ref
from test_temporal import FRAGILE_CAP

f32 = np.float32
TAN30 = np.tan(np.radians(30.0))


# ---- the frames ------------------------------------------------------------------------------------------------------------------------
def test_depth_and_normal_of_chosen_pixels_equal_the_closed_form(api):
    """16 x 8 from home: pixel (x, y) looks along (u, v, -1) with u = (x / 8 - 1) 2 tan 30 and v = (y / 4 - 1) tan 30."""
    cam = C.camera(api, 16, 8)
    c = T.camera_fields(cam)
    assert np.allclose(c["forward"], (0, 0, -1), atol=1e-6) and np.allclose(c["right"], (1, 0, 0), atol=1e-6) and np.allclose(c["up"], (0, 1, 0), atol=1e-6)
    A, N = C.guides(cam)
    u = lambda x: (x / 8.0 - 1.0) * 2.0 * TAN30
    v = lambda y: (y / 4.0 - 1.0) * TAN30
    # the wall straight ahead: 3 units away
    assert np.allclose(N[4, 8], (0, 0, 0.5, 3.0), rtol=1e-6) and np.allclose(A[4, 8], (0.7, 0.7, 0.7, 1.0))
    # the wall to the right of the tilted plane, 3 sqrt(1 + u^2) along the ray
    assert np.allclose(N[4, 13], (0, 0, 0.5, 3.0 * np.sqrt(1 + u(13) ** 2)), rtol=1e-6)
    # the slab: z = 1 is 2 units in front of the camera, and -0.9 <= 2 u <= -0.2
    assert -0.9 <= 2 * u(6) <= -0.2
    assert np.allclose(N[4, 6], (0, 0, 0.5, 2.0 * np.sqrt(1 + u(6) ** 2)), rtol=1e-6) and np.allclose(A[4, 6], (0.8, 0.3, 0.2, 1.0))
    # the floor y = -1 under the bottom row: 1 / |v| along -z, and a green albedo below the demodulation threshold
    s = 1.0 / abs(v(0))
    assert 0.0 <= 3.0 - s <= 2.5
    assert np.allclose(N[0, 8], (0, 0.5, 0, s * np.sqrt(1 + v(0) ** 2)), rtol=1e-6) and A[0, 8, 1] < 0.01 and A[0, 8, 3] == 1
    # the tilted plane: sin 37 (x - 0.9) + cos 37 (z - 0.6) = 0 along (u s, 0, 3 - s)
    sn, cs = np.sin(C.TILT), np.cos(C.TILT)
    s = (2.4 * cs - 0.9 * sn) / (cs - u(10) * sn)
    assert np.allclose(N[4, 10], (0.5 * sn, 0, 0.5 * cs, s * np.sqrt(1 + u(10) ** 2)), rtol=1e-6) and np.allclose(A[4, 10, :3], (0.2, 0.5, 0.8))
    n_unit, zero = T.unit_normals(N)
    assert abs(float(n_unit[4, 10] @ n_unit[4, 8]) - np.cos(np.radians(37.0))) < 1e-6 and float(n_unit[4, 10] @ n_unit[4, 8]) < T.DEFAULTS["normal_tol"]
    # above the wall (3 v > 1.2): nothing, all zeros
    assert 3.0 * v(7) > 1.2 and not A[7, 8].any() and not N[7, 8].any()
    assert np.array_equal(zero, A[..., 3] == 0)
    # the stored normals have length 0.5 wherever something is hit
    assert np.allclose(np.linalg.norm(N[..., :3], axis=-1)[A[..., 3] > 0], C.NORMAL_LEN)


@pytest.mark.parametrize("w,h", [(17, 9), (61, 43)])
def test_the_filters_view_holds_every_surface_and_empty_space(api, w, h):
    which, _ = C.trace(C.filter_camera(api, w, h))
    for name, i in C.SURFACE.items():
        assert (which == i).sum() >= 5, name
    assert (which == C.MISS).sum() >= 5
    N = C.guides(C.filter_camera(api, w, h))[1]
    z = N[..., 3][which != C.MISS]
    assert z.max() > 1.5 * z.min()                          # depth steps


@pytest.mark.parametrize("w,h", C.FILTER_SIZES[1:])
def test_moments_and_planted_pixels(api, w, h):
    S, Q, A, N = C.filter_frame(api, w, h)
    places = C.edge_places(A)
    assert set(places) == set(C.EDGE_KINDS) and len(set(places.values())) == 5 and all(A[p][3] == 1 for p in places.values())
    miss = A[..., 3] == 0
    assert miss.any() and not S[miss].any() and not Q[miss][:, :3].any() and (Q[..., 3] == C.BATCHES).all()
    m, e, V, skip = T.frame_ev(S, Q, C.SPP, C.BATCHES, A)
    assert np.isnan(S[places["s_nan"]][0]) and np.isinf(S[places["s_inf"]][1]) and np.isnan(Q[places["q_nan"]][2])
    assert skip[places["s_nan"]] and skip[places["s_inf"]] and skip[places["q_nan"]]
    assert not N[places["zero_normal"]][:3].any() and N[places["zero_normal"]][3] > 0 and not skip[places["zero_normal"]]
    assert V[places["v_zero"]] == 0 and not skip[places["v_zero"]] and (e[places["v_zero"]] > 0).all()
    assert skip.sum() == miss.sum() + 3
    plain = ~skip & (np.arange(h * w).reshape(h, w) != places["v_zero"][0] * w + places["v_zero"][1])
    assert (V[plain] > 0).all() and np.isfinite(e[~skip]).all()
    floor = (A[..., 1] < f32(0.01)) & ~skip                 # the demodulation fallback: e = m where the albedo is below 0.01
    assert floor.any() and np.array_equal(e[floor][:, 1], m[floor][:, 1]) and not np.array_equal(e[floor][:, 0], m[floor][:, 0])
    # the guides without planted pixels are the generator's own
    A0, N0 = C.guides(C.filter_camera(api, w, h))
    N0[places["zero_normal"]][:3] = 0
    assert np.array_equal(A, A0) and np.array_equal(N, N0)


def test_pass_through_and_black_frames():
    from cudapathtracer_amd import api
    S, Q, A, N = C.pass_through_frame(17, 9)
    assert T.frame_ev(S, Q, C.SPP, C.BATCHES, A)[3].all() and S[..., :3].min() > 0
    want, skip, L = denoise_ref(S, C.SPP, A, N)
    assert skip.all() and L == 0 and np.array_equal(want, S)
    S, Q, A, N = C.black_frame(api, 17, 9)
    m, e, V, skip = T.frame_ev(S, Q, C.SPP, C.BATCHES, A)
    assert np.array_equal(skip, A[..., 3] == 0) and not e[~skip].any() and not V[~skip].any()
    for want, skip, L in (denoise_ref(S, C.SPP, A, N), denoise_var_ref(S, Q, C.SPP, C.BATCHES, A, N)):
        assert L == 0 and np.isfinite(want).all() and not want.any()


# ---- the temporal pairs ----------------------------------------------------------------------------------------------------------------
def _temporal_cases():
    return [(name, w, h) for w, h in C.TEMPORAL_SIZES for name in C.PAIRS] + [(name, 1, 1) for name in ("same", "sideways")]


@pytest.mark.parametrize("name,w,h", _temporal_cases())
def test_every_pair_reaches_its_branch_in_the_restatement(api, name, w, h):
    case = C.temporal_case(api, name, w, h)
    if case["planted"] is not None:
        assert np.isnan(case["hist"][case["planted"]][:3]).all() and case["hist"][case["planted"]][3] == -1
    for params in (T.DEFAULTS, C.OFF_DEFAULT):
        out, ln, fragile = C.restate_temporal(case, **params)
        counts = C.branch_counts(case, ln, params)
        print(name, w, h, params, "fragile share %.4f" % fragile.mean(), counts)
        C.check_branches(case, counts, params)
        assert fragile.mean() <= FRAGILE_CAP
        skip = out[..., 3] < 0
        assert np.isfinite(out[~skip]).all() and np.isfinite(ln).all()          # the planted NaN of the history reached nobody
        assert ln.max() <= min(params["max_history"], C.HIST_LEN_SCALE + 1) + 1e-3


@pytest.mark.parametrize("name", C.RAGGED_PAIRS)
def test_the_ragged_dispatch_case_in_the_restatement(api, name):
    """The motion buffer and the map of test_every_entry_point_at_a_ragged_size reach what they are made for."""
    import motion_ref as M
    case = C.ragged_case(api, name)
    S, Q, A, N = case["frame"]
    history = (case["prev_nd"], case["hist"], case["hist_len"])
    out, ln, fragile = M.accumulate(case["cur"], case["prev"], S, Q, C.SPP, C.BATCHES, A, N, *history, motion=case["motion"])
    C.check_ragged_case(case, ln)
    base_len = T.accumulate(case["cur"], case["prev"], S, Q, C.SPP, C.BATCHES, A, N, *history)[1]
    assert (ln != base_len).any()                               # the buffer changes the result
    cur_out = M.accumulate_cur(case["cur"], case["prev"], case["working"], N, *history)[0]
    assert ((cur_out[..., 3] < 0) & ~(out[..., 3] < 0)).sum() == 1      # the NaN variance passes through


@pytest.mark.parametrize("w,h", [(17, 9), (61, 43)])
def test_the_behind_pair_tells_the_sign_of_zc(api, monkeypatch, w, h):
    """A restatement that takes z_c != 0 for z_c > 0 finds history for slab pixels that lay behind the previous camera (their mirrored
    projection falls on the wall, at their own distance and with their normal): the pair separates the two. 7 x 19 is too narrow for it."""
    case = C.temporal_case(api, "behind", w, h)
    want, want_len, _ = C.restate_temporal(case, **T.DEFAULTS)
    reproject = T.reproject

    def any_sign(cam, cam_prev, depth):
        xp, yp, zexp, ok = reproject(cam, cam_prev, depth)
        return xp, yp, zexp, np.ones_like(ok)
    monkeypatch.setattr(T, "reproject", any_sign)
    got, got_len, _ = C.restate_temporal(case, **T.DEFAULTS)
    wrong = got_len != want_len
    print(w, h, "pixels that would take history from behind the camera:", int(wrong.sum()))
    assert wrong.any() and not np.allclose(got[wrong], want[wrong], rtol=1e-3)


def test_the_yaw_pair_would_show_a_dropped_left_edge_test(api, w=61, h=43):
    """x' in [-1, 0): the taps of column -1 lie outside. A gather that forgot `xq < 0` would read index y w - 1, the last pixel of
    the row above. From home the wall's two ends are equally far and share a normal, so that pixel passes the depth and the normal
    test for some of these pixels, with a bilinear weight that counts: the wrong tap would move the result."""
    case = C.temporal_case(api, "yaw25", w, h)
    S, Qm, A, N = case["frame"]
    skip = T.frame_ev(S, Qm, C.SPP, C.BATCHES, A)[3]
    xp, yp, zexp, front = T.reproject(case["cur"], case["prev"], N[..., 3])
    n_cur, _ = T.unit_normals(N)
    n_prev, zero_prev = T.unit_normals(case["prev_nd"])
    would = 0
    for y, x in zip(*np.nonzero(~skip & front & (xp >= -1) & (xp < 0) & (yp >= 1) & (yp < h))):
        yq, weight = int(np.floor(yp[y, x])) - 1, 1.0 - (xp[y, x] - np.floor(xp[y, x]))
        z = case["prev_nd"][yq, w - 1, 3]
        would += bool(case["hist"][yq, w - 1, 3] >= 0 and abs(z - zexp[y, x]) <= 0.1 * zexp[y, x] and not zero_prev[yq, w - 1]
                      and n_cur[y, x] @ n_prev[yq, w - 1] >= 0.9 and weight > 0.05)
    print(w, h, "pixels whose wrapped tap would be taken:", would)
    assert would >= 1


@pytest.mark.parametrize("name", ["sideways", "yaw25"])
def test_exchanged_temporal_parameters_move_the_restatement(api, name):
    case = C.temporal_case(api, name, 61, 43)

    def restate(**p):
        out, ln, fragile = C.restate_temporal(case, **p)
        use = ~(out[..., 3] < 0) & ~fragile
        return np.concatenate([out, ln[..., None]], -1), use, 1e-6
    C.assert_exchanges_matter(restate, C.OFF_DEFAULT, ("max_history", "depth_tol", "normal_tol"), name)
    a, b = restate(**C.OFF_DEFAULT)[0], restate(**T.DEFAULTS)[0]
    assert not np.allclose(a[..., :4][a[..., 3] >= 0], b[..., :4][a[..., 3] >= 0], rtol=1e-3)    # and the defaults are another result


# ---- the filters -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(17, 9), (61, 43)])
def test_exchanged_filter_parameters_move_the_restatement(api, w, h):
    S, Q, A, N = C.filter_frame(api, w, h)
    hist = C.history_of(S, Q, A, N)

    def classic(iterations, **p):
        out, skip, L = denoise_ref(S, C.SPP, A, N, iterations=iterations, **p)
        return out[..., :3], ~skip, 1e-6 * L * C.SPP

    def var(iterations, **p):
        out, skip, L = denoise_var_ref(S, Q, C.SPP, C.BATCHES, A, N, iterations=iterations, **p)
        return out[..., :3], ~skip, 1e-6 * L * C.SPP

    def hist_filter(iterations, **p):
        out, skip, L = T.denoise_hist(hist, A, N, iterations=iterations, **p)
        return out[..., :3], ~skip, 1e-6 * L
    C.assert_exchanges_matter(classic, C.DENOISE_OFF, ("sigma_color", "sigma_normal", "sigma_depth"), "pt_denoise")
    C.assert_exchanges_matter(var, C.VAR_OFF, ("sigma_var", "sigma_normal", "sigma_depth"), "pt_denoise_var")
    C.assert_exchanges_matter(hist_filter, C.VAR_OFF, ("sigma_var", "sigma_normal", "sigma_depth"), "pt_denoise_hist")
    # sigma_normal = 0 is a branch of its own: the tilted plane and the wall, 37 degrees apart, exchange values only there
    a, use, atol = var(**C.VAR_OFF)
    b = var(**dict(C.VAR_OFF, sigma_normal=64.0))[0]
    assert not np.isclose(a[use], b[use], rtol=1e-3, atol=atol).all()


# ---- upsample --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yawed", [False, True])
@pytest.mark.parametrize("wl,hl,s", C.UPSAMPLE_SHAPES)
def test_upsample_cases_in_the_restatement(api, wl, hl, s, yawed):
    b = C.upsample_case(api, wl, hl, s, yawed)
    assert b[0].shape == (hl, wl, 4) and b[4].shape == (hl * s, wl * s, 4)
    # low-res pixel X sits on display pixel s X: the same ray, the same guide
    assert np.array_equal(b[2], b[4][::s, ::s]) and np.array_equal(b[3][..., 3], b[5][::s, ::s, 3])
    out, kind, fragile = U.upsample(s, b[0], b[1], C.SPP, C.BATCHES, *b[2:], **U.DEFAULTS)
    print(wl, hl, s, yawed, "pass-through %.2f, fallback %.2f, weighted %.2f, fragile %.4f" % (
        (kind == U.PASS).mean(), (kind == U.FALLBACK).mean(), (kind == U.WEIGHTED).mean(), fragile.mean()))
    assert fragile.mean() <= FRAGILE_CAP
    assert (kind == U.PASS).any() and (kind == U.WEIGHTED).any()
    if (wl, hl, s) == (1, 1, 8):
        assert (kind == U.FALLBACK).any()
