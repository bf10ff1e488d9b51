"""pt_render_aovs_chain on the GPU: bit for bit against the numpy reference (tests/aov_chain_ref.py, every hit the CPU oracle's),
its invariants against pt_render_aovs, and what chain guides do to the filters' error on specular pixels."""
import os

import numpy as np
import pytest

import aov_chain_cases as K
import aov_chain_ref as R
import temporal_ref as T
import temporal_seq as Q
from conftest import golden_scene
from denoise_ref import mse, passthrough_mask
from denoise_var_ref import demod_albedo
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SEED = K.SEED
_classes = {}                                              # case -> classes of its rays, for the test that wants every class


# ---- 1. parity with the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_chain_aovs_are_bit_exact_against_the_reference(api, oracle, gpu_ready, scene_dir, name):
    cfg, cam, w, h, aov_spp, max_links = K.case(api, name, scene_dir)
    gs, osc = api.Scene(api.HostScene(cfg)), oracle.OracleScene(cfg)
    alb, nd, links = gs.render_aovs_chain(cam, w, h, max_links, aov_spp=aov_spp, seed=SEED, links=True)
    ra, rn, rl, per_k = R.chain_aovs(oracle, osc, cam, w, h, aov_spp, max_links, SEED)
    _classes[name] = R.classes(per_k)
    print(name, _classes[name])
    assert_bits_equal(alb.reshape(-1, 4), ra, "albedo + coverage")
    assert_bits_equal(nd.reshape(-1, 4), rn, "normal + depth")
    assert_bits_equal(links.reshape(-1), rl, "links")
    if name == "textured_mirror_wall":                     # a texture sample at a chain's end
        mats = R.Materials(osc)
        r = per_k[0]
        ends = r["links"] >= 1
        assert ends.any() and len(np.unique(r["albedo"][ends], axis=0)) > 20 and mats.has_tex.any()
    # the invariants against the first-hit pass, on every case
    fa, fn = gs.render_aovs(cam, w, h, aov_spp=aov_spp, seed=SEED)
    assert_bits_equal(alb[..., 3], fa[..., 3], "coverage")
    untouched = np.ones(w * h, bool)                       # every ray of the pixel missed or hit a non-specular surface first
    for r in per_k:
        untouched &= ~r["first_spec"]
    assert untouched.any()
    assert_bits_equal(alb.reshape(-1, 4)[untouched], fa.reshape(-1, 4)[untouched], "albedo where no ray met a specular surface")
    assert_bits_equal(nd.reshape(-1, 4)[untouched], fn.reshape(-1, 4)[untouched], "normal + depth where no ray met a specular surface")
    assert np.all(links.reshape(-1)[untouched] == 0)
    a0, n0, l0 = gs.render_aovs_chain(cam, w, h, 0, aov_spp=aov_spp, seed=SEED, links=True)
    assert_bits_equal(a0, fa, "max_links 0: albedo"); assert_bits_equal(n0, fn, "max_links 0: normal + depth")
    assert not l0.any()


def test_every_class_of_ray_is_exercised(api, oracle, scene_dir):
    total = {}
    for name in K.CASES:
        if name not in _classes:                           # (run alone: from the reference, which needs no device)
            cfg, cam, w, h, aov_spp, max_links = K.case(api, name, scene_dir)
            _classes[name] = R.classes(R.chain_aovs(oracle, oracle.OracleScene(cfg), cam, w, h, aov_spp, max_links, SEED)[3])
        for k, v in _classes[name].items():
            total[k] = total.get(k, 0) + v
    print(total)
    assert set(total) == {"diffuse_first", "one_link", "two_or_more", "tir", "fallback", "miss"}
    assert all(v > 0 for v in total.values()), total


# ---- 2. forms and side effects ------------------------------------------------------------------------------------------------
def test_device_form_matches_host_form(api, gpu_ready):
    torch = gpu_ready
    hs = api.HostScene(golden_scene("mixed32"))
    gs = api.Scene(hs)
    cam = hs.camera()
    w, h = cam.w, cam.h
    ha, hn, hl = gs.render_aovs_chain(cam, w, h, 8, aov_spp=2, seed=11, links=True)
    assert hl.max() >= 2
    a = torch.full((h, w, 4), 7.0, device="cuda:0"); n = torch.full((h, w, 4), 7.0, device="cuda:0"); ln = torch.full((h, w), 7.0, device="cuda:0")
    s = torch.cuda.Stream()
    gs.render_aovs_chain_device(cam, w, h, 8, a.data_ptr(), n.data_ptr(), ln.data_ptr(), aov_spp=2, seed=11, stream=s.cuda_stream)
    s.synchronize()
    assert_bits_equal(a.cpu().numpy(), ha, "albedo"); assert_bits_equal(n.cpu().numpy(), hn, "normal + depth")
    assert_bits_equal(ln.cpu().numpy(), hl, "links")
    a.fill_(7.0); n.fill_(7.0)
    gs.render_aovs_chain_device(cam, w, h, 8, a.data_ptr(), n.data_ptr(), None, aov_spp=2, seed=11, stream=s.cuda_stream)     # no links buffer
    s.synchronize()
    assert_bits_equal(a.cpu().numpy(), ha, "albedo, links NULL"); assert_bits_equal(n.cpu().numpy(), hn, "normal + depth, links NULL")
    a2, n2 = gs.render_aovs_chain(cam, w, h, 8, aov_spp=2, seed=11)                  # the host form without links
    assert_bits_equal(a2, ha, "host form, links NULL"); assert_bits_equal(n2, hn, "host form, links NULL")


def test_a_chain_pass_between_chunks_leaves_the_render_untouched(api, gpu_ready):
    torch = gpu_ready
    hs = api.HostScene(golden_scene("mixed32"))
    gs = api.Scene(hs)
    cam = hs.camera()
    w, h = cam.w, cam.h
    gs.render(cam, w, h, 2, 4, counters=True)             # non-zero counters to watch
    before = gs.counters()
    assert before["rays_closest"] > 0
    seen = []

    def progress(done):
        c0 = gs.counters()
        a, n, ln = gs.render_aovs_chain(cam, w, h, 8, aov_spp=3, seed=SEED, links=True)
        seen.append((done, c0 == gs.counters(), float(a[..., 3].sum()), float(ln.max())))
        return 0

    prog = torch.zeros(h, w, 4, device="cuda:0")
    gs.launch_progressive(0, 4, cam, 8, True, w, h, prog.data_ptr(), 2, progress=progress)
    one = torch.zeros(h, w, 4, device="cuda:0")
    gs.launch_unidirectional(4, cam, 8, True, w, h, one.data_ptr())
    assert [d for d, _, _, _ in seen] == [2, 4, 6, 8]
    assert all(same for _, same, _, _ in seen) and gs.counters() == before
    assert all(cov > 0 and ml >= 2 for _, _, cov, ml in seen)
    assert_bits_equal(prog.cpu().numpy(), one.cpu().numpy(), "progressive with chain passes vs one-shot")


# ---- 3. quality -----------------------------------------------------------------------------------------------------------------
def _specular_pixels(api, oracle, cfg, cam, w, h, aov_spp, seed):
    """Pixels one of whose feature rays meets a specular surface first (from the oracle's first hits)."""
    osc = oracle.OracleScene(cfg)
    mats = R.Materials(osc)
    spec = np.zeros(w * h, bool)
    for k in range(aov_spp):
        spec |= R.chain_rays(osc, mats, R.camera_rays(oracle, cam, w, h, seed + k), 0)["first_spec"]
    return spec.reshape(h, w)


@pytest.fixture(scope="module")
def specular_cornell(api, gpu_ready, scene_dir):
    from cudapathtracer_amd import scenes
    cfg = scenes.cornell(os.path.join(scene_dir, "chq"), width=128, height=128, name="chq", spp=16, max_depth=8, tall_material=5, short_material=19)["config"]
    hs = api.HostScene(cfg)
    return cfg, api.Scene(hs), hs.camera()


def test_quality_chain_guides_on_one_frame(api, oracle, specular_cornell):
    """test_denoise.py's _quality frames on the glass + mirror Cornell box: pt_denoise_var's error with chain guides against its
    error with first-hit guides. Measured (MI355X): on the 2105 specular pixels 7.05e-4 with first-hit guides,
    5.71e-4 with chain guides (ratio 0.810); over the frame the ratio is 0.996."""
    cfg, gs, cam = specular_cornell
    w = h = 128
    raw, Qs = gs.render_moments(cam, w, h, 16, 4, 8)
    ref, _ = gs.render_moments(cam, w, h, 4096, 256, 8, seed=777)
    fa, fn = gs.render_aovs(cam, w, h, aov_spp=4)
    ca, cn = gs.render_aovs_chain(cam, w, h, 8, aov_spp=4)
    spec = _specular_pixels(api, oracle, cfg, cam, w, h, 4, SEED)
    mask = ~passthrough_mask(raw, 16, fa) & ~passthrough_mask(ref, 4096, fa)         # (coverage is the same in both guides)
    refm = ref / 4096
    first = api.denoise_var(raw, Qs, 16, 4, fa, fn) / 16
    chain = api.denoise_var(raw, Qs, 16, 4, ca, cn) / 16
    assert (spec & mask).sum() > 1000
    m_raw = mse(raw / 16, refm, mask)
    fs, cs = mse(first, refm, mask & spec), mse(chain, refm, mask & spec)
    fw, cw = mse(first, refm, mask), mse(chain, refm, mask)
    print("one frame, 16 spp: MSE raw %.5g; specular pixels (%d): first-hit guides %.5g, chain guides %.5g (ratio %.4f); whole frame: "
          "first-hit %.5g (%.4f of raw), chain %.5g (%.4f of raw, ratio %.4f)" % (m_raw, (spec & mask).sum(), fs, cs, cs / fs, fw, fw / m_raw, cw, cw / m_raw, cw / fw))
    assert cs <= fs
    assert cw <= 1.02 * fw


def test_quality_chain_guides_in_the_moving_history(api, oracle, specular_cornell):
    """The accumulated history after temporal_seq's 8 moving frames of 4 spp, chain guides against first-hit guides. Measured
    (MI355X): specular pixels 1.941e-3 against 1.883e-3 (ratio 0.970); over the frame the ratio is 0.9997."""
    cfg, gs, _ = specular_cornell
    w, h = Q.W, Q.H
    hist = {}
    for kind in ("first", "chain"):
        th = api.TemporalHistory(w, h)
        for t in range(Q.N_FRAMES):
            cam = Q.camera(api, t, True, w, h)
            S, Qs = gs.render_moments(cam, w, h, Q.SPP, Q.SPP // Q.BATCHES, Q.DEPTH, seed=Q.SEED0 + t)
            if kind == "first":
                A, N = gs.render_aovs(cam, w, h, aov_spp=4, seed=Q.SEED0 + t)
            else:
                A, N = gs.render_aovs_chain(cam, w, h, 8, aov_spp=4, seed=Q.SEED0 + t)
            hh = th.push(cam, S, Qs, Q.SPP, Q.BATCHES, A, N)
        mean = hh.astype(np.float64).copy()
        mean[..., :3] *= demod_albedo(A)
        hist[kind] = (mean, hh, A, S, float(th.hist_len.mean()))
    ref, _ = gs.render_moments(cam, w, h, Q.REF_SPP, Q.REF_SPP // 16, Q.DEPTH, seed=Q.REF_SEED)
    refm = ref / np.float32(Q.REF_SPP)
    S, A = hist["first"][3], hist["first"][2]
    mask = ~passthrough_mask(S, Q.SPP, A) & ~passthrough_mask(ref, Q.REF_SPP, A) & ~T.hist_passthrough(hist["first"][1]) & ~T.hist_passthrough(hist["chain"][1])
    spec = _specular_pixels(api, oracle, cfg, cam, w, h, 4, Q.SEED0 + Q.N_FRAMES - 1)
    assert (spec & mask).sum() > 1000
    m_raw = mse(S / np.float32(Q.SPP), refm, mask)
    fs, cs = mse(hist["first"][0], refm, mask & spec), mse(hist["chain"][0], refm, mask & spec)
    fw, cw = mse(hist["first"][0], refm, mask), mse(hist["chain"][0], refm, mask)
    print("moving history, 8 x 4 spp: MSE raw %.5g; specular pixels (%d): first-hit guides %.5g, chain guides %.5g (ratio %.4f); whole frame: "
          "first-hit %.5g (%.4f of raw), chain %.5g (%.4f of raw, ratio %.4f); mean history length %.2f / %.2f"
          % (m_raw, (spec & mask).sum(), fs, cs, cs / fs, fw, fw / m_raw, cw, cw / m_raw, cw / fw, hist["first"][4], hist["chain"][4]))
    assert cs <= fs
    assert cw <= 1.02 * fw
