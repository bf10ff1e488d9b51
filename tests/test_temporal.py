"""pt_temporal_accumulate and pt_denoise_hist on the GPU against their numpy restatement (tests/temporal_ref.py), and what history
does to image error next to pt_denoise_var on a single frame (the sequences of tests/temporal_seq.py)."""
import os

import numpy as np
import pytest

import temporal_ref as T
import temporal_seq as Q
from denoise_ref import LUMA, mse, passthrough_mask
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SPP, BATCHES, BATCH_SPP = 4, 2, 2
FRAGILE_CAP = 0.005          # the share of pixels of a frame whose tap decisions may sit within an ulp's reach of a threshold


def _cornell(api, scene_dir, name, w, h, **kw):
    from cudapathtracer_amd import scenes
    cfg = scenes.cornell(os.path.join(scene_dir, name), width=w, height=h, name=name, **kw)["config"]
    hs = api.HostScene(cfg)
    return api.Scene(hs), hs.camera()


def _frame(gs, cam, w, h, seed, depth=4, aov_spp=1):
    S, Qs = gs.render_moments(cam, w, h, SPP, BATCH_SPP, depth, seed=seed)
    A, N = gs.render_aovs(cam, w, h, aov_spp=aov_spp, seed=seed)
    return S, Qs, A, N


def _lum(hist):
    use = ~T.hist_passthrough(hist)
    return float((hist[use][:, :3].astype(np.float64) @ LUMA).mean())


def _assert_hist_close(got, got_len, want, want_len, fragile, what):
    """The comparison of the issue: pass-through pixels bit for bit; everywhere else but on fragile pixels rgb and V within
    rtol 1e-3 and atol 1e-6 L (test_denoise_var.py's tolerances, applied to the mean), the length within 1e-3."""
    skip = want[..., 3] < 0
    assert np.array_equal(got[..., 3] < 0, skip), what
    assert_bits_equal(got[skip], want[skip], what + ": pass-through pixels")
    assert np.all(got_len[skip] == 0)
    share = fragile.mean()
    cmp = ~skip & ~fragile
    L = _lum(want)
    err = np.abs(got[cmp].astype(np.float64) - want[cmp])
    print("%s: fragile %.4f %% of the pixels; max |got - want| = %.3g (atol %.3g), max relative %.3g; bit-equal pixels %.4f %%; max length error %.3g" % (
        what, 100 * share, err.max(), 1e-6 * L, (err / np.maximum(np.abs(want[cmp]), 1e-30)).max(),
        100 * (got[cmp].view(np.uint32) == want[cmp].view(np.uint32)).all(-1).mean(), np.abs(got_len[cmp] - want_len[cmp]).max()))
    assert share <= FRAGILE_CAP, "%s: the fragile mask covers %.3f %% of the frame" % (what, 100 * share)
    np.testing.assert_allclose(got[cmp], want[cmp], rtol=1e-3, atol=1e-6 * L, err_msg=what)
    np.testing.assert_allclose(got_len[cmp], want_len[cmp], rtol=0, atol=1e-3, err_msg=what)


def _cams(api, kind, w, h, n):
    if kind == "identity":
        return [api.make_camera(True, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), Q.FOV, w, h) for _ in range(n)]
    if kind == "pinhole":
        return [Q.camera(api, t, True, w, h) for t in range(n)]
    return [api.Camera.NotPinhole(Q.camera_pose(t, True)[0], w, h, Q.camera_pose(t, True)[1], Q.FOV, 0.02, 2.0) for t in range(n)]


@pytest.fixture(scope="module")
def scene64(api, gpu_ready, scene_dir):
    return _cornell(api, scene_dir, "tp64", 64, 48, spp=4, max_depth=4)[0]


# ---- 1. the kernel against the restatement, frame by frame ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["identity", "pinhole", "thin_lens"])
def test_accumulate_matches_numpy_after_every_frame(api, scene64, kind):
    """Both sides blend frame t into the SAME history (the library's of frame t - 1), so a decision that an ulp flipped on a
    fragile pixel cannot reach its neighbours' comparison one frame later."""
    w, h = 64, 48
    cams = _cams(api, kind, w, h, 4)
    hist = ln = prev_n = prev_cam = None
    lengths = []
    for t, cam in enumerate(cams):
        S, Qs, A, N = _frame(scene64, cam, w, h, Q.SEED0 + t)
        got, got_len = api.temporal_accumulate(cam, S, Qs, SPP, BATCHES, A, N, prev_cam, prev_n, hist, ln)
        want, want_len, fragile = T.accumulate(cam, prev_cam, S, Qs, SPP, BATCHES, A, N, prev_n, hist, ln, **T.DEFAULTS)
        _assert_hist_close(got, got_len, want, want_len, fragile, "%s frame %d" % (kind, t))
        if t == 0:
            assert_bits_equal(got, want, "first frame: this frame's own estimate")
            assert np.all(got_len[got[..., 3] >= 0] == 1)
        hist, ln, prev_n, prev_cam = got, got_len, N, cam
        lengths.append(float(ln.mean()))
    print(kind, "mean history length per frame:", lengths)
    assert lengths[-1] > 2.5                                             # history is found, not only rejected
    assert (ln == 1).sum() > 0                                           # ... and some of it is rejected: disocclusions, the frame's edge


def test_a_null_previous_camera_is_the_identity(api, scene64):
    w, h = 64, 48
    cam = _cams(api, "identity", w, h, 1)[0]
    f0 = _frame(scene64, cam, w, h, 11)
    f1 = _frame(scene64, cam, w, h, 12)
    h0, l0 = api.temporal_accumulate(cam, *f0[:2], SPP, BATCHES, *f0[2:])
    a = api.temporal_accumulate(cam, *f1[:2], SPP, BATCHES, *f1[2:], None, f0[3], h0, l0)
    b = api.temporal_accumulate(cam, *f1[:2], SPP, BATCHES, *f1[2:], api.Camera.frombytes(cam.tobytes()), f0[3], h0, l0)
    assert_bits_equal(a[0], b[0], "hist"); assert_bits_equal(a[1], b[1], "hist_len")


# ---- 2. a still camera is a running mean -------------------------------------------------------------------------------------------
def test_identity_is_the_running_mean(api, scene64):
    w, h = 64, 48
    cam = _cams(api, "identity", w, h, 1)[0]
    th = api.TemporalHistory(w, h)
    es, Vs = [], []
    for k in range(1, 6):
        S, Qs, A, N = _frame(scene64, cam, w, h, 500 + k)
        hist = th.push(cam, S, Qs, SPP, BATCHES, A, N)
        _, e, V, skip = T.frame_ev(S, Qs, SPP, BATCHES, A)
        es.append(e.astype(np.float64)); Vs.append(V.astype(np.float64))
        full = (th.hist_len == k) & ~skip
        assert full.mean() > 0.5, (k, full.mean())       # (a still camera's feature rays are jittered too: some taps fail the depth test)
        L = _lum(hist)
        np.testing.assert_allclose(hist[full][:, :3], np.mean(es, axis=0)[full], rtol=1e-3, atol=1e-6 * L)
        np.testing.assert_allclose(hist[full][:, 3], (np.sum(Vs, axis=0) / k ** 2)[full], rtol=1e-3, atol=1e-6 * L)
    assert th.hist_len.max() == 5


# ---- 3. forms, aliasing, pass-through -------------------------------------------------------------------------------------------
def test_device_form_is_the_host_form(api, gpu_ready, scene64):
    torch = gpu_ready
    w, h = 64, 48
    cams = _cams(api, "pinhole", w, h, 2)
    f0 = _frame(scene64, cams[0], w, h, 21)
    f1 = _frame(scene64, cams[1], w, h, 22)
    h0, l0 = api.temporal_accumulate(cams[0], *f0[:2], SPP, BATCHES, *f0[2:])
    h1, l1 = api.temporal_accumulate(cams[1], *f1[:2], SPP, BATCHES, *f1[2:], cams[0], f0[3], h0, l0)
    dev = lambda a: torch.from_numpy(a.copy()).to("cuda:0")
    d0 = [dev(a) for a in f0]; d1 = [dev(a) for a in f1]
    hist = [torch.full((h, w, 4), 3.0, device="cuda:0") for _ in range(2)]
    ln = [torch.full((h, w), 3.0, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        api.temporal_accumulate_device(w, h, cams[0], None, d0[0].data_ptr(), d0[1].data_ptr(), SPP, BATCHES, d0[2].data_ptr(), d0[3].data_ptr(),
                                       0, 0, 0, hist[0].data_ptr(), ln[0].data_ptr(), stream=s.cuda_stream)
        api.temporal_accumulate_device(w, h, cams[1], cams[0], d1[0].data_ptr(), d1[1].data_ptr(), SPP, BATCHES, d1[2].data_ptr(), d1[3].data_ptr(),
                                       d0[3].data_ptr(), hist[0].data_ptr(), ln[0].data_ptr(), hist[1].data_ptr(), ln[1].data_ptr(),
                                       stream=s.cuda_stream)
    s.synchronize()
    assert_bits_equal(hist[0].cpu().numpy(), h0, "first frame, device"); assert_bits_equal(ln[0].cpu().numpy(), l0, "first length, device")
    assert_bits_equal(hist[1].cpu().numpy(), h1, "second frame, device"); assert_bits_equal(ln[1].cpu().numpy(), l1, "second length, device")
    with pytest.raises(api.PtError, match="alias"):       # in and out history must be two buffers
        api.temporal_accumulate_device(w, h, cams[1], cams[0], d1[0].data_ptr(), d1[1].data_ptr(), SPP, BATCHES, d1[2].data_ptr(), d1[3].data_ptr(),
                                       d0[3].data_ptr(), hist[0].data_ptr(), ln[0].data_ptr(), hist[0].data_ptr(), ln[1].data_ptr())
    # pt_denoise_hist: device = host, and out may be hist itself (in both forms)
    want = api.denoise_hist(h1, f1[2], f1[3])
    inplace = h1.copy()
    api.denoise_hist(inplace, f1[2], f1[3], out=inplace)
    assert_bits_equal(inplace, want, "denoise_hist host, out = hist")
    ws = torch.empty(api.denoise_hist_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    out = torch.full((h, w, 4), 3.0, device="cuda:0")
    api.denoise_hist_device(w, h, hist[1].data_ptr(), d1[2].data_ptr(), d1[3].data_ptr(), ws.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert_bits_equal(out.cpu().numpy(), want, "denoise_hist device")
    assert_bits_equal(hist[1].cpu().numpy(), h1, "the history is left as it was")
    api.denoise_hist_device(w, h, hist[1].data_ptr(), d1[2].data_ptr(), d1[3].data_ptr(), ws.data_ptr(), hist[1].data_ptr())
    torch.cuda.synchronize()
    assert_bits_equal(hist[1].cpu().numpy(), want, "denoise_hist device, out = hist")


def test_nan_inf_and_miss_pixels_pass_through_both_stages(api, scene64):
    w, h = 64, 48
    cams = _cams(api, "pinhole", w, h, 2)
    S0, Q0, A0, N0 = _frame(scene64, cams[0], w, h, 31)
    S1, Q1, A1, N1 = (a.copy() for a in _frame(scene64, cams[1], w, h, 32))
    h0, l0 = api.temporal_accumulate(cams[0], S0, Q0, SPP, BATCHES, A0, N0)
    h0 = h0.copy()
    h0[24, 30] = (np.nan, np.nan, np.nan, -1.0)           # a pass-through pixel of the previous frame that holds a NaN
    h0[10, 12] = (np.inf, 1.0, 1.0, -1.0)
    S1[5, 7, 0] = np.nan; S1[20, 40, 1] = np.inf; S1[41, 2, :3] = np.nan; Q1[30, 9, 1] = np.nan
    A1[10:18, 40:52, 3] = 0.0                             # a miss region: coverage 0
    got, ln = api.temporal_accumulate(cams[1], S1, Q1, SPP, BATCHES, A1, N1, cams[0], N0, h0, l0)
    want, want_len, fragile = T.accumulate(cams[1], cams[0], S1, Q1, SPP, BATCHES, A1, N1, N0, h0, l0, **T.DEFAULTS)
    _assert_hist_close(got, ln, want, want_len, fragile, "frame with NaN / Inf / miss pixels")
    skip = got[..., 3] < 0
    for y, x in ((5, 7), (20, 40), (41, 2), (30, 9), (12, 45)):
        assert skip[y, x] and ln[y, x] == 0
    m = S1[..., :3] / np.float32(SPP)
    assert_bits_equal(got[skip][:, :3], m[skip], "a pass-through pixel holds its raw mean")
    assert np.isfinite(got[~skip]).all() and np.isfinite(ln).all()       # the NaN of the history reached nobody
    assert (ln[~skip] >= 2).mean() > 0.5
    out = api.denoise_hist(got, A1, N1)
    ref, rskip, L = T.denoise_hist(got, A1, N1)
    assert np.array_equal(rskip, skip)
    assert_bits_equal(out[skip][:, :3], got[skip][:, :3], "denoise_hist: pass-through pixels")
    assert np.all(out[..., 3] == 0) and np.isfinite(out[~skip]).all()
    np.testing.assert_allclose(out[~skip][:, :3], ref[~skip][:, :3], rtol=1e-3, atol=1e-6 * L)
    fin = api.finalise(out, 1)                            # novum_finalise still paints them
    assert np.allclose(fin[5, 7, :3], (1, 0, 1)) and np.allclose(fin[20, 40, :3], (0, 1, 0))


# ---- 4. the history filter against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [0, 1, None])
def test_denoise_hist_matches_numpy(api, scene64, iterations):
    w, h = 64, 48
    cams = _cams(api, "pinhole", w, h, 3)
    th = api.TemporalHistory(w, h)
    for t, cam in enumerate(cams):
        S, Qs, A, N = _frame(scene64, cam, w, h, 40 + t, aov_spp=2)
        hist = th.push(cam, S, Qs, SPP, BATCHES, A, N)
    kw = {} if iterations is None else {"iterations": iterations}
    got = api.denoise_hist(hist, A, N, **kw)
    d = api.denoise_var_defaults()
    want, skip, L = T.denoise_hist(hist, A, N, iterations=d["iterations"] if iterations is None else iterations, sigma_var=d["sigma_var"],
                                   sigma_normal=d["sigma_normal"], sigma_depth=d["sigma_depth"])
    assert_bits_equal(got[skip][:, :3], hist[skip][:, :3], "pass-through pixels")
    assert np.all(got[..., 3] == 0)
    use = ~skip
    assert use.sum() > 0.8 * skip.size
    err = np.abs(got[use][:, :3] - want[use][:, :3])
    print("iterations %s: max |got - want| = %.3g of atol %.3g; max relative %.3g" % (
        iterations, err.max(), 1e-6 * L, (err / np.maximum(np.abs(want[use][:, :3]), 1e-30)).max()))
    np.testing.assert_allclose(got[use][:, :3], want[use][:, :3], rtol=1e-3, atol=1e-6 * L)
    if iterations != 0:
        assert not np.allclose(got[use][:, :3], T.denoise_hist(hist, A, N, iterations=0)[0][use][:, :3], rtol=1e-3)


# ---- 5. quality -----------------------------------------------------------------------------------------------------------------
# mse / mse(raw 4 spp) on the last of 8 frames, of the numpy restatement with the library's defaults on exactly these frames (they
# are the CPU reference's frames bit for bit, so the restatement runs without a GPU: python tests/temporal_seq.py).
# The ceiling is that value times 1.05 for the kernel's f32 arithmetic, as in test_denoise_var.py.
RESTATEMENT_RATIO = {"still": 0.1004, "moving": 0.3136}       # (history without the filter: 0.1357, 0.2785; pt_denoise_var alone: 0.4455, 0.4465)


def _sequence(api, gs, moving, w=Q.W, h=Q.H):
    """Q.N_FRAMES frames through the library; returns the errors of Q.errors (against a GPU reference render) and the history."""
    th = api.TemporalHistory(w, h)
    frames = []
    for t in range(Q.N_FRAMES):
        cam = Q.camera(api, t, moving, w, h)
        S, Qs = gs.render_moments(cam, w, h, Q.SPP, Q.SPP // Q.BATCHES, Q.DEPTH, seed=Q.SEED0 + t)
        A, N = gs.render_aovs(cam, w, h, aov_spp=1, seed=Q.SEED0 + t)
        hist = th.push(cam, S, Qs, Q.SPP, Q.BATCHES, A, N)
        frames.append((S, Qs, A, N))
    ref, _ = gs.render_moments(cam, w, h, Q.REF_SPP, Q.REF_SPP // 16, Q.DEPTH, seed=Q.REF_SEED)
    filt = api.denoise_hist(hist, A, N)
    m = Q.errors(frames, ref, hist, filt)
    S, Qs, A, N = frames[-1]
    mask = ~passthrough_mask(S, Q.SPP, A) & ~passthrough_mask(ref, Q.REF_SPP, A) & ~T.hist_passthrough(hist)
    m["var_gpu"] = mse(api.denoise_var(S, Qs, Q.SPP, Q.BATCHES, A, N) / Q.SPP, ref / np.float32(Q.REF_SPP), mask)
    m["mean_len"] = float(th.hist_len.mean())
    return m


def _report(name, m):
    print("%s: MSE raw %.5g; ratios to raw: pt_denoise_var on the last frame alone %.4f, history %.4f, history + pt_denoise_hist %.4f; "
          "mean history length %.2f" % (name, m["raw"], m["var_gpu"] / m["raw"], m["hist"] / m["raw"], m["hist_filter"] / m["raw"], m["mean_len"]))


@pytest.mark.parametrize("name", ["still", "moving"])
def test_quality_history_beats_the_spatial_filter(api, gpu_ready, scene_dir, name):
    gs, _ = _cornell(api, scene_dir, "tq_" + name, Q.W, Q.H, spp=Q.SPP, max_depth=Q.DEPTH)
    m = _sequence(api, gs, name == "moving")
    _report(name, m)
    assert m["hist_filter"] <= m["var_gpu"]
    assert m["hist_filter"] <= 1.05 * RESTATEMENT_RATIO[name] * m["raw"]


def test_quality_specular_cornell_is_reported(api, gpu_ready, scene_dir):
    """Glass and mirror: reflections do not reproject with first-hit geometry (DESIGN.md §11 says what happens). Printed, not
    asserted, as the issue asks; only that the sequences run and give finite errors."""
    gs, _ = _cornell(api, scene_dir, "tq_specular", Q.W, Q.H, spp=Q.SPP, max_depth=Q.DEPTH, tall_material=5, short_material=19)
    for moving in (False, True):
        m = _sequence(api, gs, moving)
        _report("specular, " + ("moving" if moving else "still"), m)
        assert all(np.isfinite(v) for v in m.values())


# ---- 6. full HD -----------------------------------------------------------------------------------------------------------------
def test_full_hd_two_frames_device_forms_equal_host_forms(api, gpu_ready, scene_dir):
    torch = gpu_ready
    w, h = 1920, 1080
    gs, _ = _cornell(api, scene_dir, "tphd", w, h, spp=4, max_depth=4)
    cams = [Q.camera(api, t, True, w, h) for t in (0, 1)]
    host = [_frame(gs, cams[t], w, h, 60 + t) for t in (0, 1)]
    h0, l0 = api.temporal_accumulate(cams[0], *host[0][:2], SPP, BATCHES, *host[0][2:])
    h1, l1 = api.temporal_accumulate(cams[1], *host[1][:2], SPP, BATCHES, *host[1][2:], cams[0], host[0][3], h0, l0)
    want = api.denoise_hist(h1, host[1][2], host[1][3])
    assert (l1 == 2).mean() > 0.5 and not np.array_equal(want[..., :3], h1[..., :3])
    buf = lambda: torch.empty(h, w, 4, device="cuda:0")
    dS, dQ, dA, dN, dPN = buf(), buf(), buf(), buf(), buf()
    hist = [buf(), buf()]; ln = [torch.empty(h, w, device="cuda:0") for _ in range(2)]
    ws = torch.empty(api.denoise_hist_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    out = buf()
    for t in (0, 1):
        gs.render_moments_device(cams[t], w, h, SPP, BATCH_SPP, 4, dS.data_ptr(), dQ.data_ptr(), seed=60 + t)
        gs.render_aovs_device(cams[t], w, h, dA.data_ptr(), dN.data_ptr(), seed=60 + t)
        api.temporal_accumulate_device(w, h, cams[t], cams[0] if t else None, dS.data_ptr(), dQ.data_ptr(), SPP, BATCHES, dA.data_ptr(), dN.data_ptr(),
                                       dPN.data_ptr() if t else 0, hist[0].data_ptr() if t else 0, ln[0].data_ptr() if t else 0,
                                       hist[t].data_ptr(), ln[t].data_ptr())
        dPN.copy_(dN)
    api.denoise_hist_device(w, h, hist[1].data_ptr(), dA.data_ptr(), dN.data_ptr(), ws.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert_bits_equal(hist[0].cpu().numpy(), h0, "first history"); assert_bits_equal(ln[0].cpu().numpy(), l0, "first lengths")
    assert_bits_equal(hist[1].cpu().numpy(), h1, "second history"); assert_bits_equal(ln[1].cpu().numpy(), l1, "second lengths")
    assert_bits_equal(out.cpu().numpy(), want, "device vs host denoise_hist")
