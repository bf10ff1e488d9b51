"""The post-process kernels on the GPU against their numpy restatements at ragged sizes, edge cameras and their own parameters:
pt_denoise, pt_denoise_var, pt_denoise_hist (denoise_ref, denoise_var_ref, temporal_ref.denoise_hist), pt_temporal_accumulate, _cur,
_live, _motion and _cur_motion (temporal_ref, upsample_ref.accumulate_cur, converge_ref, motion_ref) and pt_upsample (upsample_ref), on the analytic frames of tests/postfx_cases.py.

Nothing is rendered and no scene is loaded: every case goes through the host form of the API, one allocation, a few small copies and
the launches. The comparisons and tolerances are those of test_denoise.py, test_denoise_var.py, test_temporal.py and test_upsample.py;
tests/test_postfx_cases.py shows without a GPU that each case reaches the branch it is named for (DESIGN.md §15 lists which size and
which pair pins which guard)."""
import numpy as np
import pytest

import converge_ref as R
import postfx_cases as C
import temporal_ref as T
import upsample_ref as U
from denoise_ref import LUMA, denoise as denoise_ref
from denoise_var_ref import denoise_var as denoise_var_ref
from test_temporal import FRAGILE_CAP, _assert_hist_close
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SPP, BATCHES = C.SPP, C.BATCHES
f32 = np.float32


# ---- a. the filters ----------------------------------------------------------------------------------------------------------------------
def _assert_rgb_close(got, want, use, atol, what):
    """rtol 1e-3 and the filter's atol on the filtered pixels' rgb, after printing the largest deviations."""
    if use.any():
        err = np.abs(got[use][:, :3].astype(np.float64) - want[use][:, :3])
        print("%s: max |got - want| = %.3g (atol %.3g), max relative %.3g" % (
            what, err.max(), atol, (err / np.maximum(np.abs(want[use][:, :3]), 1e-30)).max()))
    else:
        print("%s: every pixel passes through" % what)
    np.testing.assert_allclose(got[use][:, :3], want[use][:, :3], rtol=1e-3, atol=atol, err_msg=what)


def _check_denoise(api, frame, what, **params):
    """test_denoise.py's comparison, with parameters."""
    S, Q, A, N = frame
    got = api.denoise(S, SPP, A, N, **params)
    want, skip, L = denoise_ref(S, SPP, A, N, **dict(api.denoise_defaults(), **params))
    assert_bits_equal(got[skip], S[skip], what + ": pass-through pixels")
    assert_bits_equal(got[..., 3], S[..., 3], what + ": w channel")
    _assert_rgb_close(got, want, ~skip, 1e-6 * L * SPP, what)
    return got, skip


def _check_denoise_var(api, frame, what, **params):
    """test_denoise_var.py's comparison, with parameters."""
    S, Q, A, N = frame
    got = api.denoise_var(S, Q, SPP, BATCHES, A, N, **params)
    want, skip, L = denoise_var_ref(S, Q, SPP, BATCHES, A, N, **dict(api.denoise_var_defaults(), **params))
    assert_bits_equal(got[skip], S[skip], what + ": pass-through pixels")
    assert_bits_equal(got[..., 3], S[..., 3], what + ": w channel")
    _assert_rgb_close(got, want, ~skip, 1e-6 * L * SPP, what)
    return got, skip


def _check_denoise_hist(api, frame, what, **params):
    """test_temporal.py's comparison of the history filter, with parameters; the frame's own (e, V) is the history."""
    S, Q, A, N = frame
    hist = C.history_of(S, Q, A, N)
    got = api.denoise_hist(hist, A, N, **params)
    want, skip, L = T.denoise_hist(hist, A, N, **dict(api.denoise_var_defaults(), **params))
    assert_bits_equal(got[skip][:, :3], hist[skip][:, :3], what + ": pass-through pixels")
    assert np.all(got[..., 3] == 0), what
    _assert_rgb_close(got, want, ~skip, 1e-6 * L, what)
    return got, skip


FILTERS = {"denoise": (_check_denoise, C.DENOISE_OFF), "denoise_var": (_check_denoise_var, C.VAR_OFF), "denoise_hist": (_check_denoise_hist, C.VAR_OFF)}


@pytest.fixture(scope="module")
def filter_frames(api):
    """The yawed analytic frame with planted edge pixels at every size, made once and left unchanged."""
    frames = {}
    for w, h in C.FILTER_SIZES:
        frames[(w, h)] = C.filter_frame(api, w, h)
        for a in frames[(w, h)]:
            a.setflags(write=False)
    return frames


@pytest.mark.parametrize("w,h", C.FILTER_SIZES)
@pytest.mark.parametrize("name", list(FILTERS))
def test_filter_matches_numpy_at_ragged_sizes(api, gpu_ready, filter_frames, name, w, h):
    check, off = FILTERS[name]
    frame = filter_frames[(w, h)]
    plain = None
    for iterations in C.ITERATIONS[(w, h)]:
        kw = {} if iterations is None else {"iterations": iterations}
        got, skip = check(api, frame, "%s %d x %d, iterations %s" % (name, w, h, iterations), **kw)
        assert np.isfinite(got[~skip]).all()
        if iterations == 0:
            plain = got
        elif w * h > 1:
            assert not np.array_equal(got, plain)            # the filter ran
    # every parameter off its default, sigma_normal = 0 among them: they arrive, each at its own place
    moved, _ = check(api, frame, "%s %d x %d, %s" % (name, w, h, off), **off)
    if w * h > 1:
        default, _ = check(api, frame, "%s %d x %d, %d iterations" % (name, w, h, off["iterations"]), iterations=off["iterations"])
        assert not np.allclose(moved[~skip], default[~skip], rtol=1e-3)
    if (w, h) != (1, 1):
        assert set(C.edge_places(frame[2])) == set(C.EDGE_KINDS) and skip.sum() > (frame[2][..., 3] == 0).sum()


@pytest.mark.parametrize("name", list(FILTERS))
def test_exchanging_two_parameters_moves_the_restatement(api, gpu_ready, filter_frames, name):
    """The off-default values are distinct enough that a launch site which passed two of them in each other's place would leave the
    tolerance: shown on the restatement, at the size the 16-iteration case runs at."""
    S, Q, A, N = filter_frames[(61, 43)]
    hist = C.history_of(S, Q, A, N)

    def restate(iterations, **p):
        if name == "denoise":
            out, skip, L = denoise_ref(S, SPP, A, N, iterations=iterations, **p)
            return out[..., :3], ~skip, 1e-6 * L * SPP
        if name == "denoise_var":
            out, skip, L = denoise_var_ref(S, Q, SPP, BATCHES, A, N, iterations=iterations, **p)
            return out[..., :3], ~skip, 1e-6 * L * SPP
        out, skip, L = T.denoise_hist(hist, A, N, iterations=iterations, **p)
        return out[..., :3], ~skip, 1e-6 * L
    off = FILTERS[name][1]
    C.assert_exchanges_matter(restate, off, [k for k in off if k != "iterations"], name)


@pytest.mark.parametrize("w,h", [(17, 9), (300, 221)])
@pytest.mark.parametrize("name", list(FILTERS))
def test_a_frame_of_pass_through_pixels_comes_back_bit_for_bit(api, gpu_ready, name, w, h):
    """Coverage 0 everywhere: no pixel counts towards L (0 / 0 pixels), and every kernel of the chain copies."""
    frame = C.pass_through_frame(w, h)
    got, skip = FILTERS[name][0](api, frame, "%s %d x %d, all pass-through" % (name, w, h))
    assert skip.all()
    if name == "denoise_hist":
        assert_bits_equal(got[..., :3], C.history_of(*frame)[..., :3], "hist.rgb")
    else:
        assert_bits_equal(got, frame[0], "the input")


@pytest.mark.parametrize("name", list(FILTERS))
def test_a_black_frame_stays_finite(api, gpu_ready, name):
    """Every hit pixel filtered with e = 0, V = 0 and L = 0: the weights' denominators are their 1e-20 floors. atol is 0 here, and the
    restatement's answer is 0 exactly."""
    w, h = 17, 9
    frame = C.black_frame(api, w, h)
    for iterations in (1, None):
        kw = {} if iterations is None else {"iterations": iterations}
        got, skip = FILTERS[name][0](api, frame, "%s %d x %d, black, iterations %s" % (name, w, h, iterations), **kw)
        assert np.array_equal(skip, frame[2][..., 3] == 0) and (~skip).sum() > 100
        assert np.isfinite(got).all() and not got[..., :3].any()


# ---- b. temporal -------------------------------------------------------------------------------------------------------------------------
def _temporal_cases():
    return [(name, w, h) for w, h in C.TEMPORAL_SIZES for name in C.PAIRS] + [(name, 1, 1) for name in ("same", "sideways")]


def _compare_hist(got, got_len, want, want_len, fragile, what):
    """test_temporal._assert_hist_close; a frame of pass-through pixels only (it has nothing to take a maximum over) is that
    function's first three assertions on the whole frame."""
    if (want[..., 3] < 0).all():
        assert_bits_equal(got, want, what + ": pass-through pixels")
        assert np.all(got_len == 0) and not fragile.any()
        print("%s: every pixel passes through, bit-equal" % what)
    else:
        _assert_hist_close(got, got_len, want, want_len, fragile, what)


@pytest.mark.parametrize("name,w,h", _temporal_cases())
def test_accumulate_matches_numpy_on_every_pair(api, gpu_ready, name, w, h):
    case = C.temporal_case(api, name, w, h)
    S, Qm, A, N = case["frame"]
    history = (case["prev_nd"], case["hist"], case["hist_len"])
    m, e, V, skip = T.frame_ev(S, Qm, SPP, BATCHES, A)
    cur = np.concatenate([np.where(skip[..., None], m, e), np.where(skip, f32(-1), V)[..., None]], -1).astype(f32)
    for params in (T.DEFAULTS, C.OFF_DEFAULT):
        what = "%s %d x %d, %s" % (name, w, h, "defaults" if params is T.DEFAULTS else params)
        got, got_len = api.temporal_accumulate(case["cur"], S, Qm, SPP, BATCHES, A, N, case["prev"], *history, **params)
        want, want_len, fragile = C.restate_temporal(case, **params)
        _compare_hist(got, got_len, want, want_len, fragile, what)
        counts = C.branch_counts(case, want_len, params)
        print(what, counts)
        C.check_branches(case, counts, params)
        live = got[..., 3] >= 0
        assert np.isfinite(got[live]).all() and np.isfinite(got_len).all()      # the NaN planted in the history reached nobody
        # the frame's working pixels handed over: pt_temporal_accumulate_cur is pt_temporal_accumulate from step 2 on
        got_cur, got_cur_len = api.temporal_accumulate_cur(case["cur"], cur, N, case["prev"], *history, **params)
        assert_bits_equal(got_cur, got, what + ": accumulate_cur hist"); assert_bits_equal(got_cur_len, got_len, what + ": accumulate_cur hist_len")
        want_cur, want_cur_len, fragile_cur = U.accumulate_cur(case["cur"], case["prev"], cur, N, *history, **params)
        _compare_hist(got_cur, got_cur_len, want_cur, want_cur_len, fragile_cur, what + ", accumulate_cur")


def test_the_parameters_reach_the_blend(api, gpu_ready):
    """max_history, depth_tol and normal_tol are neighbours on their way to the kernel: with the off-default values the restatement
    tells every exchange of two apart, and the kernel agrees with the restatement (test_accumulate_matches_numpy_on_every_pair)."""
    case = C.temporal_case(api, "yaw25", 61, 43)

    def restate(**p):
        out, ln, fragile = C.restate_temporal(case, **p)
        return np.concatenate([out, ln[..., None]], -1), ~(out[..., 3] < 0) & ~fragile, 1e-6
    C.assert_exchanges_matter(restate, C.OFF_DEFAULT, ("max_history", "depth_tol", "normal_tol"), "pt_temporal_accumulate")
    S, Qm, A, N = case["frame"]
    got = [api.temporal_accumulate(case["cur"], S, Qm, SPP, BATCHES, A, N, case["prev"], case["prev_nd"], case["hist"], case["hist_len"], **p)
           for p in (T.DEFAULTS, C.OFF_DEFAULT)]
    assert abs(got[0][1].max() - (C.HIST_LEN_SCALE + 1)) < 1e-3 and got[1][1].max() == C.OFF_DEFAULT["max_history"]
    assert ((got[0][1] > 1) != (got[1][1] > 1)).any()         # the tighter tolerances drop taps the defaults take


def test_accumulate_with_a_map_at_a_ragged_size(api, gpu_ready):
    """17 x 9 is 3 x 2 tiles, the last column one pixel wide and the last row one pixel high."""
    w, h = 17, 9
    case = C.temporal_case(api, "same", w, h)
    S, Qm, A, N = case["frame"]
    hist, ln = case["hist"], case["hist_len"]
    live = np.array([[1, 0, 1], [0, 1, 0]], np.int32)
    assert live.shape == R.tile_grid(h, w)
    m = R.per_pixel(live != 0, h, w)
    full, full_len = api.temporal_accumulate(case["cur"], S, Qm, SPP, BATCHES, A, N, None, case["prev_nd"], hist, ln)
    got, got_len = api.temporal_accumulate_live(case["cur"], S, Qm, SPP, BATCHES, A, N, case["prev_nd"], hist, ln, live)
    assert_bits_equal(got[~m], hist[~m], "carried tiles: hist"); assert_bits_equal(got_len[~m], ln[~m], "carried tiles: hist_len")
    assert_bits_equal(got[m], full[m], "live tiles: hist"); assert_bits_equal(got_len[m], full_len[m], "live tiles: hist_len")
    assert (full_len[~m] != ln[~m]).any() and (full_len[m] != ln[m]).any()
    want_len = R.accumulate_live(case["cur"], S, Qm, SPP, BATCHES, A, N, case["prev_nd"], hist, ln, live)[1]
    assert_bits_equal(got_len, want_len, "restatement: hist_len")


def test_every_entry_point_at_a_ragged_size(api, gpu_ready):
    """All nine instantiations of temporal_kernel share one pixel map and one argument block: each entry point, host and device form,
    at 17 x 9 (two workgroups in x, partial tiles in both directions) on the identity and on a projecting pair, bit for bit against
    the numpy restatements, with the planted pass-through and NaN pixels, a synthetic motion buffer and a map of live tiles."""
    import motion_ref as M
    torch = gpu_ready
    w, h = C.RAGGED
    for name in C.RAGGED_PAIRS:
        case = C.ragged_case(api, name)
        cam, prev, (S, Qm, A, N), cur, mv = case["cur"], case["prev"], case["frame"], case["working"], case["motion"]
        history = (case["prev_nd"], case["hist"], case["hist_len"])
        sums = (S, Qm, SPP, BATCHES, A, N)
        want = {"accumulate": T.accumulate(cam, prev, *sums, *history)[:2],
                "accumulate_cur": M.accumulate_cur(cam, prev, cur, N, *history)[:2],
                "accumulate_motion": M.accumulate(cam, prev, *sums, *history, motion=mv)[:2],
                "accumulate_cur_motion": M.accumulate_cur(cam, prev, cur, N, *history, motion=mv)[:2]}
        C.check_ragged_case(case, want["accumulate_motion"][1])          # (on the CPU, before the GPU is asked anything)
        host = {"accumulate": api.temporal_accumulate(cam, *sums, prev, *history),
                "accumulate_cur": api.temporal_accumulate_cur(cam, cur, N, prev, *history),
                "accumulate_motion": api.temporal_accumulate_motion(cam, *sums, prev, *history, mv),
                "accumulate_cur_motion": api.temporal_accumulate_cur_motion(cam, cur, N, prev, *history, mv),
                "motion NULL": api.temporal_accumulate_motion(cam, *sums, prev, *history, None),
                "map NULL": api.temporal_accumulate_live(cam, *sums, *history, None, prev)}
        dev = lambda a: torch.from_numpy(a.copy()).to("cuda:0")
        p = lambda t: t.data_ptr()
        dS, dQ, dA, dN, dC, dM, dPN, dH, dL = (dev(a) for a in (S, Qm, A, N, cur, mv) + history)
        dsums, dhist = (p(dS), p(dQ), SPP, BATCHES, p(dA), p(dN)), (p(dPN), p(dH), p(dL))
        outs = {k: (torch.full((h, w, 4), 3.0, device="cuda:0"), torch.full((h, w), 3.0, device="cuda:0")) for k in list(host) + ["accumulate_live"]}
        o = lambda k: (p(outs[k][0]), p(outs[k][1]))
        api.temporal_accumulate_device(w, h, cam, prev, *dsums, *dhist, *o("accumulate"))
        api.temporal_accumulate_cur_device(w, h, cam, prev, p(dC), p(dN), *dhist, *o("accumulate_cur"))
        api.temporal_accumulate_motion_device(w, h, cam, prev, *dsums, *dhist, p(dM), *o("accumulate_motion"))
        api.temporal_accumulate_cur_motion_device(w, h, cam, prev, p(dC), p(dN), *dhist, p(dM), *o("accumulate_cur_motion"))
        api.temporal_accumulate_motion_device(w, h, cam, prev, *dsums, *dhist, 0, *o("motion NULL"))
        api.temporal_accumulate_live_device(w, h, cam, prev, *dsums, *dhist, 0, *o("map NULL"))
        if name == "same":
            want["accumulate_live"] = R.accumulate_live(cam, *sums, *history, C.RAGGED_LIVE)
            host["accumulate_live"] = api.temporal_accumulate_live(cam, *sums, *history, C.RAGGED_LIVE, prev)
            dT = dev(C.RAGGED_LIVE)
            api.temporal_accumulate_live_device(w, h, cam, prev, *dsums, *dhist, p(dT), *o("accumulate_live"))
        torch.cuda.synchronize()
        for k in host:
            got = (outs[k][0].cpu().numpy(), outs[k][1].cpu().numpy())
            ref = want[k if k in want else "accumulate"]                 # motion NULL and a NULL map are the base entry
            for form, res in (("host", host[k]), ("device", got)):
                what = "%s, %s, %s form" % (name, k, form)
                differ = (res[0].view(np.uint32) != ref[0].view(np.uint32)).any(-1) | (res[1].view(np.uint32) != ref[1].view(np.uint32))
                print("%s: %d of %d pixels differ from the restatement" % (what, int(differ.sum()), w * h))
                assert_bits_equal(res[0], ref[0], what + ": hist"); assert_bits_equal(res[1], ref[1], what + ": hist_len")
                if k in ("motion NULL", "map NULL"):
                    assert_bits_equal(res[0], host["accumulate"][0], what + " against the base entry: hist")
                    assert_bits_equal(res[1], host["accumulate"][1], what + " against the base entry: hist_len")


def test_every_filter_entry_at_a_ragged_size(api, gpu_ready, filter_frames):
    """The four filters share dn_prepare_kernel, dn_atrous_kernel and dn_finish_kernel, picked from one table: each entry point at
    17 x 9 (two workgroups in x, partial tiles in both directions, 41 of 153 pixels pass-through) with one iteration, the default
    count and every parameter off its default. Bit for bit: (a) the host form against the device form, (b) the device form with out
    = in against it, (c) denoise_var_tiles with a uniform map against denoise_var, (d) denoise_var against SPP times denoise_hist of
    the frame's own (e, V) on the filtered pixels' rgb: the same reduce and a-trous kernels behind two prepare and finish sources
    (SPP = 4 scales exactly, and test_temporal shows the restatement's first-frame (e, V) bit-equal to the device's dn_var_pixel)."""
    torch = gpu_ready
    w, h = C.RAGGED
    S, Q, A, N = filter_frames[(w, h)]
    hist = C.history_of(S, Q, A, N)
    skip = T.frame_ev(S, Q, SPP, BATCHES, A)[3]
    assert np.array_equal(skip, hist[..., 3] < 0) and int(skip.sum()) == 41 and skip.size == 153      # one pass-through set
    tm = np.full(((h + 7) // 8, (w + 7) // 8), SPP, np.int32)
    dev = lambda a: torch.from_numpy(a.copy()).to("cuda:0")
    dQ, dA, dN, dT = (dev(a) for a in (Q, A, N, tm))
    # name: (host form, device form, their input, its arguments between w, h and the workspace: in is a place holder)
    entries = {"denoise": (api.denoise, api.denoise_device, S, lambda i: (i, SPP, dA.data_ptr(), dN.data_ptr()), (S, SPP, A, N)),
               "denoise_var": (api.denoise_var, api.denoise_var_device, S,
                               lambda i: (i, dQ.data_ptr(), SPP, BATCHES, dA.data_ptr(), dN.data_ptr()), (S, Q, SPP, BATCHES, A, N)),
               "denoise_var_tiles": (api.denoise_var_tiles, api.denoise_var_tiles_device, S,
                                     lambda i: (i, dQ.data_ptr(), dT.data_ptr(), SPP // BATCHES, dA.data_ptr(), dN.data_ptr()),
                                     (S, Q, tm, SPP // BATCHES, A, N)),
               "denoise_hist": (api.denoise_hist, api.denoise_hist_device, hist, lambda i: (i, dA.data_ptr(), dN.data_ptr()), (hist, A, N))}
    ws = torch.empty(api.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    assert all(getattr(api, k + "_workspace_bytes")(w, h) == ws.numel() for k in entries)
    plain = {name: e[0](*e[4], iterations=0) for name, e in entries.items()}
    for var_kw in ({"iterations": 1}, {}, C.VAR_OFF):
        got = {}
        for name, (host_form, device_form, src, dargs, hargs) in entries.items():
            kw = C.DENOISE_OFF if name == "denoise" and var_kw is C.VAR_OFF else var_kw
            what = "%s %s" % (name, kw or "defaults")
            got[name] = host_form(*hargs, **kw)
            dIn, out = dev(src), torch.full((h, w, 4), 3.0, device="cuda:0")
            device_form(w, h, *dargs(dIn.data_ptr()), ws.data_ptr(), out.data_ptr(), **kw)
            device_form(w, h, *dargs(dIn.data_ptr()), ws.data_ptr(), dIn.data_ptr(), **kw)
            torch.cuda.synchronize()
            apart, inplace = out.cpu().numpy(), dIn.cpu().numpy()
            for other, res in (("device form", apart), ("device form, out = in", inplace)):
                differ = (res.view(np.uint32) != got[name].view(np.uint32)).any(-1)
                print("%s: %d of %d pixels differ between the host form and the %s" % (what, int(differ.sum()), w * h, other))
            assert_bits_equal(apart, got[name], what + ": (a) host form against device form")
            assert_bits_equal(inplace, apart, what + ": (b) out = in against out apart")
            assert not np.array_equal(got[name], plain[name]), what                     # the filter ran
        assert_bits_equal(got["denoise_var_tiles"], got["denoise_var"], "(c) a uniform map, %s" % (var_kw or "defaults"))
        assert_bits_equal(got["denoise_var"][skip], S[skip], "pass-through pixels of denoise_var")
        assert_bits_equal(got["denoise_hist"][skip][:, :3], hist[skip][:, :3], "pass-through pixels of denoise_hist")
        scaled = (f32(SPP) * got["denoise_hist"][~skip][:, :3]).astype(f32)
        differ = (scaled.view(np.uint32) != np.ascontiguousarray(got["denoise_var"][~skip][:, :3]).view(np.uint32)).any(-1)
        print("(d) %s: %d of %d filtered pixels differ between denoise_var and SPP * denoise_hist" % (var_kw or "defaults", int(differ.sum()), differ.size))
        assert_bits_equal(got["denoise_var"][~skip][:, :3], scaled, "(d) denoise_var against SPP * denoise_hist, %s" % (var_kw or "defaults"))


# ---- c. upsample -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yawed", [False, True])
@pytest.mark.parametrize("wl,hl,s", C.UPSAMPLE_SHAPES)
def test_upsample_matches_numpy_at_small_sizes(api, gpu_ready, wl, hl, s, yawed):
    """test_upsample.py's comparison on frames of one, six and 35 low-res pixels: every display pixel of the first sits in the last
    low-res column and row, where only tap (0, 0) is a candidate."""
    b = C.upsample_case(api, wl, hl, s, yawed)
    got = api.upsample(s, b[0], b[1], SPP, BATCHES, *b[2:])
    want, kind, fragile = U.upsample(s, b[0], b[1], SPP, BATCHES, *b[2:], **U.DEFAULTS)
    what = "%d x %d scale %d %s" % (wl * s, hl * s, s, "yawed" if yawed else "front")
    skip = kind == U.PASS
    assert np.array_equal(got[..., 3] < 0, skip), what
    assert_bits_equal(got[skip], want[skip], what + ": pass-through pixels")
    fb = (kind == U.FALLBACK) & ~fragile
    assert_bits_equal(got[fb], want[fb], what + ": fallback pixels")
    cmp = (kind == U.WEIGHTED) & ~fragile
    L = float((want[~skip][:, :3].astype(np.float64) @ LUMA).mean())
    err = np.abs(got[cmp].astype(np.float64) - want[cmp])
    print("%s: pass-through %.2f %%, fallback %.2f %%, fragile %.4f %% of the pixels; max |got - want| = %.3g (atol %.3g), max relative %.3g" % (
        what, 100 * skip.mean(), 100 * (kind == U.FALLBACK).mean(), 100 * fragile.mean(), err.max(), 1e-6 * L,
        (err / np.maximum(np.abs(want[cmp]), 1e-30)).max()))
    assert fragile.mean() <= FRAGILE_CAP, what
    np.testing.assert_allclose(got[cmp], want[cmp], rtol=1e-3, atol=1e-6 * L, err_msg=what)
    assert skip.any() and cmp.any(), what
    if (wl, hl, s) == (1, 1, 8):
        assert fb.any(), what                                # one low-res pixel: the wall's display pixels have no tap on their plane
