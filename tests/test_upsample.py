"""pt_upsample and pt_temporal_accumulate_cur on the GPU against their numpy restatement (tests/upsample_ref.py), and what the render
scale does to image error next to nearest replication of the low-res frame (the frames of tests/upsample_seq.py)."""
import numpy as np
import pytest

import temporal_ref as T
import temporal_seq as Q
import upsample_ref as U
import upsample_seq as S
from denoise_ref import LUMA
from test_temporal import FRAGILE_CAP, _assert_hist_close, _cornell, _frame
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SPP, BATCHES = 4, 2
f32 = np.float32


@pytest.fixture(scope="module")
def scene(api, gpu_ready, scene_dir):
    return _cornell(api, scene_dir, "up64", 64, 48, spp=4, max_depth=4)[0]


def _scaled_frame(api, gs, cam, w, h, s, seed, depth=4):
    """What a scaled frame renders: (S, Q, albedo_lo, normal_depth_lo) with the low-res camera, (albedo, normal_depth) with cam."""
    lo = _frame(gs, api.scaled_camera(cam, s), w // s, h // s, seed, depth)
    A, N = gs.render_aovs(cam, w, h, aov_spp=1, seed=seed)
    return lo, (A, N)


# ---- 1. the kernel against the restatement on rendered frames ---------------------------------------------------------------------
@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("w,h,s", [(64, 48, 2), (64, 48, 4), (63, 45, 3)])
def test_upsample_matches_numpy_on_rendered_frames(api, scene, w, h, s, moving):
    cam = Q.camera(api, 3 if moving else 0, moving, w, h)
    lo, (A, N) = _scaled_frame(api, scene, cam, w, h, s, Q.SEED0)
    got = api.upsample(s, lo[0], lo[1], SPP, BATCHES, lo[2], lo[3], A, N)
    want, kind, fragile = U.upsample(s, lo[0], lo[1], SPP, BATCHES, lo[2], lo[3], A, N, **U.DEFAULTS)
    what = "%d x %d scale %d %s" % (w, h, s, "moving" if moving else "still")
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
    # the case exercises every branch
    assert (kind == U.FALLBACK).any() and skip.any(), what
    assert (kind == U.WEIGHTED).sum() > 0.5 * (~skip).sum(), what


# ---- 2. hand-made buffers straight through the device form ------------------------------------------------------------------------
def _device_upsample(api, torch, s, bufs, **kw):
    lo_h, lo_w = bufs[0].shape[:2]
    h, w = bufs[4].shape[:2]
    d = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in bufs]
    out = torch.full((h, w, 4), 7.0, device="cuda:0")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.upsample_device(w, h, s, d[0].data_ptr(), d[1].data_ptr(), SPP, BATCHES, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(),
                        out.data_ptr(), stream=st.cuda_stream, **kw)
    st.synchronize()
    for a, b in zip(d, bufs):
        assert_bits_equal(a.cpu().numpy(), b, "the inputs are left as they were")
    assert (lo_h * s, lo_w * s) == (h, w)
    return out.cpu().numpy()


@pytest.mark.parametrize("wl,hl,s", [(8, 8, 2), (8, 4, 3)])
def test_synthetic_buffers_through_the_device_form(api, gpu_ready, wl, hl, s):
    torch = gpu_ready
    w = wl * s
    # constant guides: the bilinear interpolation, V = sum b^2 V. Four taps, each a few f32 roundings of 6e-8: rtol 1e-5 is 20 times that.
    bufs = U.synthetic(wl, hl, s, 1)
    got = _device_upsample(api, torch, s, bufs)
    assert_bits_equal(got, api.upsample(s, bufs[0], bufs[1], SPP, BATCHES, *bufs[2:]), "device form vs host form")
    _, e, V, _ = T.frame_ev(bufs[0], bufs[1], SPP, BATCHES, bufs[2])
    want_e, want_V, _ = U.bilinear_closed_form(s, e.astype(np.float64), V.astype(np.float64))
    np.testing.assert_allclose(got[..., :3], want_e, rtol=1e-5)
    np.testing.assert_allclose(got[..., 3], want_V, rtol=1e-5)
    assert_bits_equal(got[::s, ::s], np.concatenate([e, V[..., None]], -1), "on the low-res grid: the frame itself")
    # a depth step: no value crosses it
    bufs = U.synthetic(wl, hl, s, 2, depth_split=True)
    got = _device_upsample(api, torch, s, bufs)
    _, e, _, _ = T.frame_ev(bufs[0], bufs[1], SPP, BATCHES, bufs[2])
    for side, lo_side in ((np.s_[:, :w // 2], np.s_[:, :wl // 2]), (np.s_[:, w // 2:], np.s_[:, wl // 2:])):
        assert got[side][..., :3].min() >= e[lo_side].min() - 1e-6 and got[side][..., :3].max() <= e[lo_side].max() + 1e-6
        assert (got[side][..., 3] >= 0).all()
    # coverage 0 at display resolution: the raw mean of low-res pixel (x / s, y / s), V = -1; a NaN in one low-res S reaches no
    # pixel that has another usable tap
    S_, Q_, Al, Nl, A, N = U.synthetic(wl, hl, s, 3)
    y, x = 2 * s + 1, 3 * s + 1                           # fx = fy = 1 / s <= 0.5: tap (0, 0) is the nearest, or wins the tie
    A[y, x, 3] = 0.0
    S_[1, 1, 0] = np.nan
    got = _device_upsample(api, torch, s, (S_, Q_, Al, Nl, A, N))
    assert_bits_equal(got[y, x], np.append(S_[2, 3, :3] / f32(SPP), f32(-1)), "coverage 0")
    bad = ~np.isfinite(got).all(-1)
    assert bad.sum() == 1 and bad[s, s] and got[s, s, 3] == -1          # the display pixel that sits on the NaN pixel has no other tap
    want, kind, fragile = U.upsample(s, S_, Q_, SPP, BATCHES, Al, Nl, A, N, **U.DEFAULTS)
    assert not fragile.any() and np.array_equal(kind == U.PASS, got[..., 3] < 0)
    assert_bits_equal(got[kind == U.PASS], want[kind == U.PASS], "pass-through pixels")
    np.testing.assert_allclose(got[kind == U.WEIGHTED], want[kind == U.WEIGHTED], rtol=1e-5)
    # the parameters reach the kernel: a wide depth tolerance lets the step through
    bufs = U.synthetic(wl, hl, s, 2, depth_split=True)
    loose = _device_upsample(api, torch, s, bufs, sigma_depth=100.0)
    assert loose[0, w // 2 - 1, 0] > 0.3                   # (left e <= 0.22, right e >= 0.9)


# ---- 3. pt_temporal_accumulate_cur ------------------------------------------------------------------------------------------------
def test_accumulate_cur_matches_numpy_after_every_frame(api, scene):
    """test_temporal.py's method: both sides blend frame t into the library's history of frame t - 1."""
    w, h, s = 64, 48, 2
    hist = ln = prev_n = prev_cam = None
    for t in range(4):
        cam = Q.camera(api, t, True, w, h)
        lo, (A, N) = _scaled_frame(api, scene, cam, w, h, s, Q.SEED0 + t)
        cur = api.upsample(s, lo[0], lo[1], SPP, BATCHES, lo[2], lo[3], A, N)
        got, got_len = api.temporal_accumulate_cur(cam, cur, N, prev_cam, prev_n, hist, ln)
        want, want_len, fragile = U.accumulate_cur(cam, prev_cam, cur, N, prev_n, hist, ln, **T.DEFAULTS)
        _assert_hist_close(got, got_len, want, want_len, fragile, "scale 2 frame %d" % t)
        if t == 0:
            assert_bits_equal(got[cur[..., 3] >= 0], cur[cur[..., 3] >= 0], "first frame: this frame's own estimate")
        hist, ln, prev_n, prev_cam = got, got_len, N, cam
    assert ln.mean() > 2.5 and (ln == 1).sum() > 0


def test_accumulate_cur_on_a_full_resolution_frame_is_accumulate(api, scene):
    w, h = 64, 48
    cams = [Q.camera(api, t, True, w, h) for t in range(2)]
    f0 = _frame(scene, cams[0], w, h, 21)
    f1 = [a.copy() for a in _frame(scene, cams[1], w, h, 22)]
    f1[0][5, 7, 0] = np.nan; f1[2][10:14, 20:30, 3] = 0.0  # pass-through pixels: a NaN, a miss region
    th = api.TemporalHistory(w, h)
    want = [th.push(cams[0], *f0[:2], SPP, BATCHES, *f0[2:]).copy(), th.push(cams[1], *f1[:2], SPP, BATCHES, *f1[2:]).copy()]
    want_len = th.hist_len
    tc = api.TemporalHistory(w, h)
    for t, (cam, f) in enumerate(zip(cams, (f0, f1))):
        m, e, V, skip = T.frame_ev(f[0], f[1], SPP, BATCHES, f[2])
        cur = np.concatenate([np.where(skip[..., None], m, e), np.where(skip, f32(-1), V)[..., None]], -1).astype(f32)
        got = tc.push_cur(cam, cur, f[3])
        assert_bits_equal(got, want[t], "frame %d: hist" % t)
    assert_bits_equal(tc.hist_len, want_len, "hist_len")
    assert tc.hist_len[5, 7] == 0 and (tc.hist_len == 2).mean() > 0.3


# ---- 4. quality -------------------------------------------------------------------------------------------------------------------
# All-pixel MSE of upsample + 3 iterations of pt_denoise_hist, of the numpy restatement with the library's defaults on exactly these
# frames (they are the CPU reference's frames bit for bit, so the restatement runs without a GPU: python tests/upsample_seq.py;
# DESIGN.md §13). The ceiling is that value times 1.05 for the kernels' f32 arithmetic, as in test_temporal.py.
RESTATEMENT_MSE = {2: 0.076915, 4: 0.36723}              # (more than 4 px from the emitter: 0.0020933, 0.005276; nearest replication: 0.14104, 0.47838)


@pytest.fixture(scope="module")
def quality_frames(api, gpu_ready, scene_dir):
    gs, _ = _cornell(api, scene_dir, "uq", S.W, S.H, spp=S.SPP, max_depth=S.DEPTH)
    cam = S.camera(api)
    guides = gs.render_aovs(cam, S.W, S.H, aov_spp=1, seed=S.SEED)
    ref, _ = gs.render_moments(cam, S.W, S.H, S.REF_SPP, S.REF_SPP // 16, S.DEPTH, seed=S.REF_SEED)
    return gs, cam, guides, ref


@pytest.mark.parametrize("s", S.SCALES)
def test_quality_upsampling_beats_nearest_replication(api, quality_frames, s):
    gs, cam, guides, ref = quality_frames
    lo, _ = _scaled_frame(api, gs, cam, S.W, S.H, s, S.SEED, S.DEPTH)
    m = S.errors(s, lo, guides, ref, api.upsample, api.denoise_hist)
    print("scale %d: MSE over all pixels (more than 4 px from the emitter): nearest %.5g (%.5g); upsampled %.5g (%.5g); upsampled + %d "
          "iterations %.5g (%.5g); restatement %.5g" % (s, m["nearest"], m["nearest_far"], m["up"], m["up_far"], S.ITERATIONS, m["up_filter"],
                                                        m["up_filter_far"], RESTATEMENT_MSE[s]))
    assert m["up_filter"] < m["nearest"]
    assert m["up_filter"] <= 1.05 * RESTATEMENT_MSE[s]
