"""The responsive history stage (pt_temporal_accumulate_respond) on the GPU against its numpy restatement (tests/respond_ref.py), bit
for bit outside the restatement's FRAGILE mask, on the library's own frames (tests/respond_cases.py; tests/test_respond_ref_cpu.py
checks the same inputs from the CPU oracle without a GPU), and the quality checks on the sequences of tests/respond_seq.py."""
import numpy as np
import pytest

import respond_cases as RC
import respond_ref as R
import respond_seq as RS
import temporal_ref as T
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

INF = float("inf")
CASES = [(w, h, change, kind) for (w, h) in RC.SIZES for change in RC.CHANGES for kind in ("identity", "pinhole")]
SETTINGS = ((1, 1, 1.5), (2, 2, 3.0), (3, 4, 2.0), (3, 1, 4.0))       # (radius, power, threshold): every radius and power, the defaults


@pytest.fixture(scope="module")
def cases(api, gpu_ready, scene_dir):
    out = {}
    for (w, h) in RC.SIZES:
        hs = RC.MC.cornell_host(api, scene_dir, "respond_gpu_%dx%d" % (w, h), w, h)
        for change in RC.CHANGES:
            for kind in ("identity", "pinhole"):
                out[(w, h, change, kind)] = RC.build(api, lambda: RC.LibraryRenderer(api, hs), w, h, change, kind)
    return out


def _compare(api, c, what, settings=SETTINGS):
    worst = 0.0
    for form in ("sums", "cur"):
        for motion in (False, True):
            for radius, power, k in settings:
                p = dict(radius=radius, power=power, threshold=k)
                got = RC.library(api, c, form, motion, **p)
                want = RC.restate(R, c, form, motion, **p)
                ok = ~want[3]
                tag = "%s %s motion %d r %d p %d k %g" % (what, form, motion, radius, power, k)
                worst = max(worst, float(want[3].mean()))
                assert want[3].mean() <= RC.FRAGILE_CAP, tag
                assert_bits_equal(got[2][ok], want[2][ok], tag + ": out_scale")
                assert_bits_equal(got[0][ok], want[0][ok], tag + ": out_hist")
                assert_bits_equal(got[1][ok], want[1][ok], tag + ": out_hist_len")
    return worst


# ---- 1. the kernels against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES, ids=lambda k: "%dx%d-%s-%s" % k)
def test_respond_is_the_restatement(api, cases, key):
    c = cases[key]
    if key[3] == "identity":
        assert c["cam"].tobytes() == c["prev_cam"].tobytes()
    worst = _compare(api, c, "%dx%d %s %s" % key)
    lam = RC.library(api, c, **R.DEFAULTS)[2]
    print("%s: fragile share at most %.3f %%; lambda < 1 on %d of %d pixels at the defaults" % (key, 100 * worst, (lam < 1).sum(), lam.size))
    if key[3] == "identity":
        assert (lam < 1).sum() >= RC.MIN_SHORTENED[key[:2]]


@pytest.mark.parametrize("key", [k for k in CASES if k[2] == "box"], ids=lambda k: "%dx%d-%s-%s" % k)
def test_planted_hazards_are_skipped(api, cases, key):
    """A pass-through pixel, a miss pixel with a zero normal and a non-finite e in the history: each is skipped, never multiplied by
    zero, so its neighbours' results are the restatement's, in which nothing non-finite has spread."""
    c, spots = RC.plant_hazards(cases[key])
    _compare(api, c, "hazards %dx%d %s %s" % key, SETTINGS[1:3])
    out, out_len, lam = RC.library(api, c, radius=3, power=2, threshold=2.0)
    for (y, x) in spots:
        assert lam[y, x] == 1
    (y0, x0), (y1, x1), (y2, x2) = spots
    assert out[y0, x0, 3] == -1 and out_len[y0, x0] == 0 and out[y1, x1, 3] == -1 and out_len[y1, x1] == 0
    others = np.ones(lam.shape, bool); others[y2, x2] = False
    base = api.temporal_accumulate(c["cam"], c["S"], c["Q"], RC.SPP, RC.BATCHES, c["A"], c["N"], c["prev_cam"], c["prev_n"], c["hist"], c["ln"])[0]
    assert np.isfinite(lam).all() and (np.isfinite(out[others]).all(-1) == np.isfinite(base[others]).all(-1)).all()


# ---- 2. equalities, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [k for k in CASES if k[2] == "box"], ids=lambda k: "%dx%d-%s-%s" % k)
def test_an_infinite_threshold_is_the_base_function(api, cases, key):
    c = cases[key]
    h = (c["prev_cam"], c["prev_n"], c["hist"], c["ln"])
    base = {("sums", False): api.temporal_accumulate(c["cam"], c["S"], c["Q"], RC.SPP, RC.BATCHES, c["A"], c["N"], *h),
            ("sums", True): api.temporal_accumulate_motion(c["cam"], c["S"], c["Q"], RC.SPP, RC.BATCHES, c["A"], c["N"], *h, motion=c["motion"]),
            ("cur", False): api.temporal_accumulate_cur(c["cam"], c["cur"], c["N"], *h),
            ("cur", True): api.temporal_accumulate_cur_motion(c["cam"], c["cur"], c["N"], *h, motion=c["motion"])}
    for (form, motion), want in base.items():
        for radius in (1, 3):
            got = RC.library(api, c, form, motion, radius=radius, power=2, threshold=INF)
            tag = "%s motion %d radius %d" % (form, motion, radius)
            assert_bits_equal(got[0], want[0], tag + ": hist"); assert_bits_equal(got[1], want[1], tag + ": hist_len")
            assert (got[2] == 1).all()
    # a first frame has no history: the base function, and lambda 1
    first = api.temporal_accumulate_respond(c["cam"], c["N"], c["S"], c["Q"], RC.SPP, RC.BATCHES, c["A"], motion=c["motion"])
    want = api.temporal_accumulate(c["cam"], c["S"], c["Q"], RC.SPP, RC.BATCHES, c["A"], c["N"])
    assert_bits_equal(first[0], want[0], "first frame: hist"); assert_bits_equal(first[1], want[1], "first frame: hist_len")
    assert (first[2] == 1).all()


@pytest.mark.parametrize("key", [(37, 21, "box", "pinhole"), (40, 24, "light", "identity"), (5, 4, "box", "pinhole")], ids=lambda k: "%dx%d-%s-%s" % k)
def test_device_form_is_the_host_form_with_and_without_out_scale(api, gpu_ready, cases, key):
    torch = gpu_ready
    c = cases[key]
    w, h = c["w"], c["h"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d = {k: dev(c[k]) for k in ("S", "Q", "A", "N", "prev_n", "hist", "ln", "motion", "cur")}
    ws = torch.empty(api.temporal_respond_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    for form in ("sums", "cur"):
        for motion in (False, True):
            want = RC.library(api, c, form, motion, **R.DEFAULTS)
            none = RC.library(api, c, form, motion, scale=False, **R.DEFAULTS)
            assert none[2] is None
            assert_bits_equal(none[0], want[0], "out_scale NULL: hist"); assert_bits_equal(none[1], want[1], "out_scale NULL: hist_len")
            sums = (d["S"].data_ptr(), d["Q"].data_ptr(), RC.SPP, RC.BATCHES, d["A"].data_ptr(), 0) if form == "sums" else (0, 0, 0, 0, 0, d["cur"].data_ptr())
            for with_scale in (True, False):
                oh, ol, os_ = torch.full((h, w, 4), 3.0, device="cuda:0"), torch.full((h, w), 3.0, device="cuda:0"), torch.full((h, w), 3.0, device="cuda:0")
                s = torch.cuda.Stream()
                torch.cuda.synchronize()
                with torch.cuda.stream(s):
                    api.temporal_accumulate_respond_device(w, h, c["cam"], c["prev_cam"], *sums, d["N"].data_ptr(), d["prev_n"].data_ptr(),
                                                           d["hist"].data_ptr(), d["ln"].data_ptr(), d["motion"].data_ptr() if motion else 0,
                                                           ws.data_ptr(), oh.data_ptr(), ol.data_ptr(), os_.data_ptr() if with_scale else 0,
                                                           stream=s.cuda_stream, **R.DEFAULTS)
                s.synchronize()
                tag = "%s motion %d scale %d" % (form, motion, with_scale)
                assert_bits_equal(oh.cpu().numpy(), want[0], tag + ": device hist"); assert_bits_equal(ol.cpu().numpy(), want[1], tag + ": device hist_len")
                if with_scale:
                    assert_bits_equal(os_.cpu().numpy(), want[2], tag + ": device out_scale")
                else:
                    assert (os_.cpu().numpy() == 3).all()
    with pytest.raises(api.PtError, match="workspace must not alias"):
        api.temporal_accumulate_respond_device(w, h, c["cam"], c["prev_cam"], d["S"].data_ptr(), d["Q"].data_ptr(), RC.SPP, RC.BATCHES, d["A"].data_ptr(),
                                               0, d["N"].data_ptr(), d["prev_n"].data_ptr(), d["hist"].data_ptr(), d["ln"].data_ptr(), 0,
                                               d["hist"].data_ptr(), oh.data_ptr(), ol.data_ptr())


# ---- 3. quality: the 64 x 64 changed-scene sequences, and the unchanged still sequence ------------------------------------------------
def _lib_accumulate(api):
    def acc(cam, S, Qs, A, N, prev_n, hist, ln, respond):
        if respond is None or hist is None:
            h, l = api.temporal_accumulate(cam, S, Qs, RS.SPP, RS.BATCHES, A, N, None, prev_n, hist, ln)
            return h, l, None
        return api.temporal_accumulate_respond(cam, N, S, Qs, RS.SPP, RS.BATCHES, A, prev_normal_depth=prev_n, hist=hist, hist_len=ln, **respond)
    return acc


@pytest.mark.parametrize("which", list(RS.EXPERIMENTS))
def test_quality_after_a_change(api, gpu_ready, scene_dir, which):
    """The library over the sequence of tests/respond_seq.py: (1) its changed-pixel ratios on frames 7..13 are the restatement's
    recorded ones within test_temporal.py's margin of 1.05; (2) on every frame after the change the changed pixels are better with
    respond on than off."""
    hs = RS.host(api, scene_dir, "respond_q_" + which)
    first, last, shift = RS.EXPERIMENTS[which]
    cam = RS.camera(api)
    sc = api.Scene.from_mesh(hs)
    frames, refs, guides = [], [], []
    for t in range(RS.N_FRAMES):
        if t in (0, RS.CHANGE):
            if t:
                sc.update_vertices(RC.MC.moved_arrays(hs, first, last, shift)["points"])
            guides.append(sc.render_aovs_centre(cam, RS.W, RS.H, 0))
            refs.append(sc.render(cam, RS.W, RS.H, RS.REF_SPP, RS.DEPTH, seed=RS.REF_SEED)[0])
        S, Qs = sc.render_moments(cam, RS.W, RS.H, RS.SPP, RS.SPP // RS.BATCHES, RS.DEPTH, seed=RS.SEED0 + t)
        frames.append((S, Qs, *guides[-1]))
    sc.close()
    seq = {"frames": frames, "ref": tuple(refs), "changed": RS.changed_mask(refs[0], refs[1], guides[0], guides[1])}
    print("%s: changed pixels %.1f %% of the frame" % (which, 100 * seq["changed"].mean()))
    filt = lambda hist, A, N: api.denoise_hist(hist, A, N)
    off = RS.ratios(seq, RS.run(seq, cam, _lib_accumulate(api), filt, None))
    on = RS.ratios(seq, RS.run(seq, cam, _lib_accumulate(api), filt, api.respond_defaults()))
    for t in range(RS.CHANGE, RS.N_FRAMES):
        want = RS.RECORDED[which][t - RS.CHANGE]
        print("frame %2d: changed pixels off %.4f on %.4f (restatement %.4f); whole frame off %.4f on %.4f; lambda < 1 on %.2f %%" % (
            t, off[t][0], on[t][0], want, off[t][1], on[t][1], 100 * on[t][2]))
    for t in range(RS.CHANGE, RS.N_FRAMES):
        assert on[t][0] <= 1.05 * RS.RECORDED[which][t - RS.CHANGE], t
        assert on[t][0] < off[t][0], t


def test_quality_unchanged_still_sequence_stays_within_ten_percent(api, gpu_ready, scene_dir):
    """The still 8-frame sequence of tests/temporal_centre_seq.py through the library with respond off and on: the whole-frame error
    of history + filter with the option on stays within the 10 % of the selection rule."""
    import temporal_seq as Q
    from test_temporal import _cornell
    gs, _ = _cornell(api, scene_dir, "respond_still", Q.W, Q.H, spp=Q.SPP, max_depth=Q.DEPTH)
    out = {}
    frames = []
    for t in range(Q.N_FRAMES):
        cam = Q.camera(api, t, False)
        S, Qs = gs.render_moments(cam, Q.W, Q.H, Q.SPP, Q.SPP // Q.BATCHES, Q.DEPTH, seed=Q.SEED0 + t)
        frames.append((cam, S, Qs, *gs.render_aovs_centre(cam, Q.W, Q.H, 0)))
    ref, _ = gs.render_moments(cam, Q.W, Q.H, Q.REF_SPP, Q.REF_SPP // 16, Q.DEPTH, seed=Q.REF_SEED)
    for name, respond in (("off", None), ("on", True)):
        th = api.TemporalHistory(Q.W, Q.H, respond=respond)
        for cam, S, Qs, A, N in frames:
            hist = th.push(cam, S, Qs, Q.SPP, Q.BATCHES, A, N)
        m = Q.errors([f[1:] for f in frames], ref, hist, api.denoise_hist(hist, A, N))
        out[name] = m["hist_filter"] / m["raw"]
        if respond:
            print("share of lambda < 1 on the last frame: %.3f %%" % (100 * float((th.scale < 1).mean())))
    print("still: history + filter over raw: respond off %.4f, on %.4f (%.3f x)" % (out["off"], out["on"], out["on"] / out["off"]))
    assert out["on"] <= 1.10 * out["off"]
