"""pt_render_adaptive_moments and pt_denoise_var_tiles on the GPU: the adaptive frame's second moment against pt_render_moments at
each tile's own count and against the replay (tests/adaptive_moments_ref.py) over the CPU reference's partial sums; everything
else against pt_render_adaptive; the filter against pt_denoise_var (uniform map) and against its restatement (a real map)."""
import ctypes
import os

import numpy as np
import pytest

import adaptive_moments_ref as MR
import adaptive_ref as R
from denoise_ref import mse, passthrough_mask
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SEED = 103033


def _frames(render):
    cache = {}

    def frame_at(n):
        if n not in cache:
            cache[n] = render(n)
        return cache[n]
    return frame_at


def _cornell_cfg(scene_dir, name, w, h, **kw):
    from cudapathtracer_amd import scenes
    return scenes.cornell(os.path.join(scene_dir, name), width=w, height=h, spp=4, max_depth=8, name=name, **kw)["config"]


def _cornell(api, scene_dir, name, w, h, **kw):
    hs = api.HostScene(_cornell_cfg(scene_dir, name, w, h, **kw))
    return hs, hs.camera()


def _check_rounds(gs, cam, w, h, depth, frame_at, mn, mx, c, want_rounds=3):
    """A threshold that spreads the tiles over the rounds; then S and Q.rgb of every tile against render_moments at the tile's own
    count, Q.w = n / c, and everything else against render_adaptive. Returns (threshold, S, Q, tile_spp)."""
    t = R.pick_threshold(frame_at, w, h, mn, mx, c, want_rounds)
    assert t is not None, "no threshold spreads the tiles over %d rounds" % want_rounds
    S, Q, spp, err, st = gs.render_adaptive_moments(cam, w, h, depth, mn, mx, c, t)
    assert gs.queue_stalls() == 0
    assert np.unique(spp).size >= want_rounds, np.unique(spp, return_counts=True)
    for n in np.unique(spp):
        Sn, Qn = gs.render_moments(cam, w, h, int(n), c, depth)
        mask = MR.pixel_map(spp == n, w, h)
        assert_bits_equal(S[mask], Sn[mask], "S of the tiles that stopped at %d" % n)
        assert_bits_equal(Q[mask][:, :3], Qn[mask][:, :3], "Q.rgb of the tiles that stopped at %d" % n)
        assert (Q[mask][:, 3] == n // c).all()
    col, spp0, err0, st0 = gs.render_adaptive(cam, w, h, depth, mn, mx, c, t)
    assert_bits_equal(S, col, "S vs render_adaptive")
    assert np.array_equal(spp, spp0) and st == st0
    assert_bits_equal(err, err0, "tile_err vs render_adaptive")
    return t, S, Q, spp


# ---- 1. threshold 0: the frame of pt_render_moments ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell64(api, gpu_ready, scene_dir):
    return _cornell(api, scene_dir, "am_c64", 64, 48)


def test_threshold_zero_is_render_moments_at_max_spp(api, cornell64):
    hs, cam = cornell64
    gs = api.Scene(hs)
    S, Q, spp, err, st = gs.render_adaptive_moments(cam, 64, 48, 8, 4, 16, 2, 0.0)
    S0, Q0 = gs.render_moments(cam, 64, 48, 16, 2, 8)
    assert_bits_equal(S, S0, "S")
    assert_bits_equal(Q, Q0, "Q, w included")
    assert (Q[..., 3] == 8).all() and (Q[..., :3] > 0).mean() > 0.5
    col, spp0, err0, st0 = gs.render_adaptive(cam, 64, 48, 8, 4, 16, 2, 0.0)
    assert_bits_equal(S, col, "S vs render_adaptive")
    assert np.array_equal(spp, spp0) and (spp == 16).all()
    assert_bits_equal(err, err0, "tile_err")
    assert st == st0 == {"rounds": 4, "tiles_at_max": 48, "pixel_samples": 16 * 64 * 48}
    gs.close()


# ---- 2. tiles that stop in different rounds ---------------------------------------------------------------------------------------
def test_rounds_against_the_cpu_reference(api, oracle, cornell64, scene_dir):
    """(a) the replay over the CPU reference's partial sums: Q is tied to the reference, not only to pt_render_moments."""
    hs, cam = cornell64
    gs = api.Scene(hs)
    camb = np.frombuffer(cam.tobytes(), np.uint8).copy()
    osc = oracle.OracleScene(_cornell_cfg(scene_dir, "am_c64", 64, 48))
    frame_at = _frames(lambda n: osc.render(camera=camb, width=64, height=48, spp=n, max_depth=8, integrator=0, threads=16)[0])
    t, S, Q, spp = _check_rounds(gs, cam, 64, 48, 8, frame_at, 4, 16, 2)
    r = MR.replay_moments(frame_at, 64, 48, 4, 16, 2, t)
    assert np.array_equal(spp, r["tile_spp"])
    assert_bits_equal(S, r["colors"], "S vs the replay over the CPU reference")
    assert_bits_equal(Q, r["sq"], "Q vs the replay over the CPU reference")
    gs.close()


@pytest.fixture(scope="module")
def specular61(api, gpu_ready, scene_dir):
    """(b) 61 x 43 with a mirror and a glass box: ragged last tile row and column, the LEAN kernels. Shared with the filter's tests."""
    hs, cam = _cornell(api, scene_dir, "am_s61", 61, 43, tall_material=19, short_material=5)
    gs = api.Scene(hs)
    frame_at = _frames(lambda n: gs.render(cam, 61, 43, n, 8)[0])
    t, S, Q, spp = _check_rounds(gs, cam, 61, 43, 8, frame_at, 4, 16, 2)
    flags = gs.flags()
    A, N = gs.render_aovs(cam, 61, 43, aov_spp=2)
    gs.close()
    return {"S": S, "Q": Q, "spp": spp, "A": A, "N": N, "flags": flags, "t": t}


def test_rounds_on_a_ragged_frame_with_mirror_and_glass(specular61):
    f = specular61
    assert f["flags"]["lean"], f["flags"]
    assert f["spp"].shape == (6, 8)
    # lanes outside the image carried zeros along and nothing of them reached the frame: the last row and column are plain pixels
    assert np.isfinite(f["Q"][42]).all() and np.isfinite(f["Q"][:, 60]).all() and (f["Q"][..., :3] >= 0).all()


def test_rounds_on_a_scene_in_hbm_with_time_slices(api, gpu_ready, scene_dir):
    """(c) the 82 k blob: the scene is in HBM, and with time slices tiles change hands between the two launches of a round."""
    from cudapathtracer_amd import scenes
    cfg = scenes.blob_in_box(os.path.join(scene_dir, "am_blob"), 160, 128, 4, 8, name="am_blob")["config"]
    hs = api.HostScene(cfg)
    gs = api.Scene(hs, options={"slice_iters": 16, "sched_mask": 3})
    cam = hs.camera()
    _check_rounds(gs, cam, 160, 128, 8, _frames(lambda n: gs.render(cam, 160, 128, n, 8)[0]), 4, 16, 2)
    assert not gs.flags()["onchip"] and gs.flags()["time_slices"], gs.flags()
    S, Q, _, _, _ = gs.render_adaptive_moments(cam, 160, 128, 8, 0, 16, 8, 0.0)      # 8 samples per launch: waves yield tiles
    print("tile handovers in the last launch: %d" % gs.tile_handovers())
    assert gs.tile_handovers() > 0 and gs.queue_stalls() == 0
    S0, Q0 = gs.render_moments(cam, 160, 128, 16, 8, 8)
    assert_bits_equal(S, S0, "S with time slices")
    assert_bits_equal(Q, Q0, "Q with time slices")
    gs.close()


# ---- 3. forms, isolation, the variant -------------------------------------------------------------------------------------------
def test_host_and_device_forms_agree(api, gpu_ready, cornell64):
    torch = gpu_ready
    hs, cam = cornell64
    gs = api.Scene(hs)
    S, Q, spp, err, st = gs.render_adaptive_moments(cam, 64, 48, 8, 2, 16, 2, 0.05)
    dS = torch.full((48, 64, 4), 9.0, device="cuda:0")                    # the call writes both, it does not add
    dQ = torch.full((48, 64, 4), 7.0, device="cuda:0")
    dspp = torch.zeros((6, 8), dtype=torch.int32, device="cuda:0")
    derr = torch.zeros((6, 8), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    st2 = gs.render_adaptive_moments_device(cam, 64, 48, 8, 2, 16, 2, 0.05, dS.data_ptr(), dQ.data_ptr(), dspp.data_ptr(), derr.data_ptr(),
                                            stream=stream)
    torch.cuda.synchronize()
    assert_bits_equal(dS.cpu().numpy(), S, "device form: S")
    assert_bits_equal(dQ.cpu().numpy(), Q, "device form: Q")
    assert np.array_equal(dspp.cpu().numpy(), spp) and st2 == st
    assert_bits_equal(derr.cpu().numpy(), err, "device form: tile_err")
    dQ.fill_(1.0)
    gs.render_adaptive_moments_device(cam, 64, 48, 8, 2, 16, 2, 0.05, dS.data_ptr(), dQ.data_ptr(), dspp.data_ptr(), None)    # no error buffer
    assert_bits_equal(dQ.cpu().numpy(), Q, "device form without an error buffer: Q")
    gs.close()


def test_counters_and_a_later_render_are_untouched(api, cornell64):
    hs, cam = cornell64
    fresh = api.Scene(hs)
    want, _ = fresh.render(cam, 64, 48, 6, 8)
    fresh.close()
    gs = api.Scene(hs)
    gs.render(cam, 64, 48, 2, 8, counters=True)                          # something in the counters
    before = gs.counters()
    assert sum(before.values()) > 0
    gs.render_adaptive_moments(cam, 64, 48, 8, 2, 12, 2, 0.05)
    assert gs.counters() == before
    got, _ = gs.render(cam, 64, 48, 6, 8)
    assert_bits_equal(got, want, "pt_render after pt_render_adaptive_moments")
    gs.close()


def test_wavefront_variant_is_refused_and_outputs_stay(api, cornell64):
    hs, cam = cornell64
    gs = api.Scene(hs).set_variant("wavefront")
    col = np.full((48, 64, 4), 7.0, np.float32)
    sq = np.full((48, 64, 4), 2.0, np.float32)
    spp = np.full((6, 8), 3, np.int32)
    err = np.full((6, 8), 5.0, np.float32)
    p = api.adaptive_params(2, 8, 2, 0.1)
    rc = api.lib().pt_render_adaptive_moments(gs.h, ctypes.byref(cam), 64, 48, 8, 0, 1, SEED, ctypes.byref(p), api._p(col), api._p(sq),
                                              api._p(spp), api._p(err), None)
    assert rc == -1 and "wavefront" in api.lib().pt_last_error().decode()
    assert (col == 7.0).all() and (sq == 2.0).all() and (spp == 3).all() and (err == 5.0).all()
    with pytest.raises(api.PtError):
        gs.render_adaptive_moments(cam, 64, 48, 8, 2, 8, 2, 0.1)
    gs.close()


# ---- 4. pt_denoise_var_tiles with a uniform map is pt_denoise_var -------------------------------------------------------------------
def _device_tiles(api, torch, S, Q, tm, c, A, N, out_is_in=False, **kw):
    h, w = S.shape[:2]
    dS, dQ, dA, dN = (torch.from_numpy(x.copy()).to("cuda:0") for x in (S, Q, A, N))
    dM = torch.from_numpy(tm.copy()).to("cuda:0")
    ws = torch.empty(api.denoise_var_tiles_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    out = dS if out_is_in else torch.full_like(dS, 3.0)
    api.denoise_var_tiles_device(w, h, dS.data_ptr(), dQ.data_ptr(), dM.data_ptr(), c, dA.data_ptr(), dN.data_ptr(), ws.data_ptr(),
                                 out.data_ptr(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ws.cpu().numpy()


def test_a_uniform_map_is_denoise_var_bit_for_bit(api, gpu_ready, scene_dir):
    torch = gpu_ready
    hs, cam = _cornell(api, scene_dir, "am_u61", 61, 43)
    gs = api.Scene(hs)
    S, Q = gs.render_moments(cam, 61, 43, 8, 2, 8)
    A, N = gs.render_aovs(cam, 61, 43, aov_spp=2)
    gs.close()
    tm = np.full((6, 8), 8, np.int32)
    want = api.denoise_var(S, Q, 8, 4, A, N)
    assert not np.array_equal(want, S)
    assert_bits_equal(api.denoise_var_tiles(S, Q, tm, 2, A, N), want, "host form")
    assert_bits_equal(_device_tiles(api, torch, S, Q, tm, 2, A, N)[0], want, "device form")
    inplace = S.copy()
    api.denoise_var_tiles(inplace, Q, tm, 2, A, N, out=inplace)
    assert_bits_equal(inplace, want, "host form, out = in")
    assert_bits_equal(_device_tiles(api, torch, S, Q, tm, 2, A, N, out_is_in=True)[0], want, "device form, out = in")
    assert_bits_equal(api.denoise_var_tiles(S, Q, tm, 4, A, N, iterations=1), api.denoise_var(S, Q, 8, 2, A, N, iterations=1), "batch_spp 4")


# ---- 5. a real adaptive map against the restatement ----------------------------------------------------------------------------------
def _check_against_numpy(api, S, Q, tm, c, A, N, iterations):
    """tests/test_denoise_var.py::_check_against_numpy with the count per pixel: the same tolerance (rtol 1e-3, atol 1e-6 L spp,
    here with the pixel's own spp), the same exclusion (the pass-through pixels, which must be bit-exact instead)."""
    kw = {} if iterations is None else {"iterations": iterations}
    got = api.denoise_var_tiles(S, Q, tm, c, A, N, **kw)
    d = api.denoise_var_defaults()
    want, skip, L = MR.denoise_var_tiles(S, Q, tm, c, A, N, iterations=d["iterations"] if iterations is None else iterations,
                                         sigma_var=d["sigma_var"], sigma_normal=d["sigma_normal"], sigma_depth=d["sigma_depth"])
    assert_bits_equal(got[skip], S[skip], "pass-through pixels")
    assert_bits_equal(got[..., 3], S[..., 3], "w channel")
    use = ~skip
    spp = MR.pixel_map(tm, S.shape[1], S.shape[0]).astype(np.float64)[use][:, None]
    err = np.abs(got[use][:, :3] - want[use][:, :3])
    print("iterations %s: max |got - want| / (atol + rtol |want|) = %.3g; max relative %.3g" % (
        iterations, (err / (1e-6 * L * spp + 1e-3 * np.abs(want[use][:, :3]))).max(),
        (err / np.maximum(np.abs(want[use][:, :3]), 1e-30)).max()))
    assert (err <= 1e-6 * L * spp + 1e-3 * np.abs(want[use][:, :3])).all()
    return got, skip


@pytest.mark.parametrize("iterations", [0, 1, None])
def test_real_map_matches_numpy(api, specular61, iterations):
    f = specular61
    got, skip = _check_against_numpy(api, f["S"], f["Q"], f["spp"], 2, f["A"], f["N"], iterations)
    assert (~skip).sum() > 0.9 * skip.size
    if iterations != 0:
        assert not np.array_equal(got, f["S"])


def test_real_map_pass_through_and_forms(api, gpu_ready, specular61):
    torch = gpu_ready
    f = specular61
    S, Q, A, N, tm = f["S"].copy(), f["Q"], f["A"].copy(), f["N"], f["spp"]
    counts = MR.pixel_map(tm, 61, 43)
    lo, hi = np.argwhere(counts == counts.min())[3], np.argwhere(counts == counts.max())[3]
    assert counts[tuple(lo)] != counts[tuple(hi)]                        # two tiles with different counts
    S[lo[0], lo[1], 0] = np.nan
    S[hi[0], hi[1], 1] = np.inf
    A[10:18, 40:52, 3] = 0.0                                             # a miss region: coverage 0, across tiles
    got, skip = _check_against_numpy(api, S, Q, tm, 2, A, N, None)
    assert skip[tuple(lo)] and skip[tuple(hi)] and skip[10:18, 40:52].all()
    dev, _ = _device_tiles(api, torch, S, Q, tm, 2, A, N)
    assert_bits_equal(dev, got, "device form vs host form")
    mean = api.adaptive_mean(got, tm)                                    # the result is in the units of the input
    assert np.isfinite(mean[~skip]).all()


# ---- 6. the map's indexing, on a synthetic frame -----------------------------------------------------------------------------------
def test_map_indexing_on_a_checkerboard(api, gpu_ready):
    """61 x 43, constant e, constant per-sample variance, a checkerboard of 8 and 16 samples. After a 0-iteration call the first
    colour buffer of the workspace holds what the filter's iterations read: (e, V) per pixel (include/pt_api.h states the layout).
    V must be the restatement's, and differ across every tile edge, the partial tiles' included, by the factor the counts imply;
    an index built with w / 8 = 7 tile columns instead of ceil(w / 8) = 8 turns the checkerboard into stripes and fails here."""
    torch = gpu_ready
    w, h, c = 61, 43, 2
    ty, tx = 6, 8
    tm = np.where((np.arange(ty)[:, None] + np.arange(tx)[None, :]) % 2 == 0, 8, 16).astype(np.int32)
    n = MR.pixel_map(tm, w, h).astype(np.float32)
    B = n / c
    S = np.zeros((h, w, 4), np.float32)
    Q = np.zeros((h, w, 4), np.float32)
    S[..., :3] = B[..., None]                                            # batch sums alternately 0 and 2: mean sample 1/2 everywhere
    Q[..., :3] = (2 * B)[..., None]
    A = np.ones((h, w, 4), np.float32)
    A[..., :3] = 0.5
    N = np.zeros((h, w, 4), np.float32)
    N[..., 2] = 1.0
    N[..., 3] = 2.0
    out, ws = _device_tiles(api, torch, S, Q, tm, c, A, N, iterations=0)
    want, skip, L, v = MR.denoise_var_tiles(S, Q, tm, c, A, N, iterations=0, return_variance=True)
    assert not skip.any()
    ev = ws[:w * h * 16].view(np.float32).reshape(h, w, 4)
    assert_bits_equal(ev[..., 3], v.astype(np.float32), "prepared variance")
    assert (v.astype(np.float32) == v).all()                             # (the restatement's V is f32 arithmetic held in f64)
    assert_bits_equal(ev[..., :3], np.full((h, w, 3), 1.0, np.float32), "prepared e = (S / spp) / a")
    assert_bits_equal(out, S, "0 iterations: spp a e")
    # var of the mean per channel 1 / (4 (B - 1)); over a^2 = 1/4; three channels
    np.testing.assert_allclose(ev[..., 3], 3.0 / (B - 1), rtol=1e-6)
    V = ev[..., 3]
    edges = 0
    for x in range(8, w, 8):
        assert np.allclose(np.maximum(V[:, x - 1], V[:, x]) / np.minimum(V[:, x - 1], V[:, x]), 7.0 / 3.0), x
        edges += 1
    for y in range(8, h, 8):
        assert np.allclose(np.maximum(V[y - 1], V[y]) / np.minimum(V[y - 1], V[y]), 7.0 / 3.0), y
        edges += 1
    assert edges == 7 + 5
    for (j, i), cnt in np.ndenumerate(tm):                               # constant within every tile
        assert np.unique(V[8 * j:8 * j + 8, 8 * i:8 * i + 8]).size == 1
    got1 = api.denoise_var_tiles(S, Q, tm, c, A, N, iterations=1)        # constant e: the filter leaves it where it is
    np.testing.assert_allclose(got1[..., :3], S[..., :3], rtol=1e-5)


# ---- 7. what it does to image error ----------------------------------------------------------------------------------------------
def test_quality_adaptive_cornell(api, gpu_ready, scene_dir):
    """128 x 128 diffuse Cornell box, depth 8, MIS; schedule 8 / 32 / 4; centre guides; reference 2048 spp with another seed.
    The CPU restatement of this set-up gave var-tiles / raw = 0.435, classic / raw = 0.693, uniform + denoise_var / raw = 0.529."""
    from cudapathtracer_amd import scenes
    w = h = 128
    hs = api.HostScene(scenes.cornell(os.path.join(scene_dir, "am_q"), width=w, height=h, spp=16, max_depth=8, name="am_q")["config"])
    gs, cam = api.Scene(hs), hs.camera()
    mn, mx, c = 8, 32, 4
    t = R.pick_threshold(_frames(lambda n: gs.render(cam, w, h, n, 8)[0]), w, h, mn, mx, c)
    assert t is not None
    S, Q, tm, _, st = gs.render_adaptive_moments(cam, w, h, 8, mn, mx, c, t)
    assert np.unique(tm).size >= 3
    ref, _ = gs.render(cam, w, h, 2048, 8, seed=777)
    A, N = gs.render_aovs_centre(cam, w, h)
    refm = ref / 2048
    raw = api.adaptive_mean(S, tm)
    mask = ~passthrough_mask(raw, 1, A) & ~passthrough_mask(ref, 2048, A)
    mean_spp = st["pixel_samples"] / (w * h)
    uni = max(2 * c, int(round(mean_spp / c)) * c)                        # the uniform frame of the same mean budget
    Su, Qu = gs.render_moments(cam, w, h, uni, c, 8)
    gs.close()
    m = {"raw": mse(raw, refm, mask),
         "classic": mse(api.denoise(raw, 1, A, N), refm, mask),
         "var_tiles": mse(api.adaptive_mean(api.denoise_var_tiles(S, Q, tm, c, A, N), tm), refm, mask),
         "uniform_var": mse(api.denoise_var(Su, Qu, uni, uni // c, A, N) / uni, refm, mask)}
    d = api.denoise_var_defaults()
    want = MR.denoise_var_tiles(S, Q, tm, c, A, N, iterations=d["iterations"], sigma_var=d["sigma_var"], sigma_normal=d["sigma_normal"],
                                sigma_depth=d["sigma_depth"])[0]
    n = MR.pixel_map(tm, w, h).astype(np.float64)[..., None]
    m["restatement"] = mse(want / n, refm, mask)
    print("adaptive %d / %d / %d, threshold %.4g, mean %.1f spp: MSE raw %.5g; relative to raw: classic denoise of the mean %.3f, "
          "variance-guided with the tile map %.3f (restatement %.3f), uniform %d spp + denoise_var %.3f; var-tiles / classic %.3f" % (
              mn, mx, c, t, mean_spp, m["raw"], m["classic"] / m["raw"], m["var_tiles"] / m["raw"], m["restatement"] / m["raw"], uni,
              m["uniform_var"] / m["raw"], m["var_tiles"] / m["classic"]))
    assert m["var_tiles"] <= 1.05 * m["restatement"]
    assert m["var_tiles"] <= 0.85 * m["classic"]
