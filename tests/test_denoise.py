"""pt_denoise on the GPU against its numpy restatement (tests/denoise_ref.py), and what it does to image error."""
import os

import numpy as np
import pytest

from denoise_ref import denoise as denoise_ref, mse, passthrough_mask
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SEED = 103033


def _cornell(api, scene_dir, name, w, h, **kw):
    from cudapathtracer_amd import scenes
    cfg = scenes.cornell(os.path.join(scene_dir, name), width=w, height=h, name=name, **kw)["config"]
    hs = api.HostScene(cfg)
    return api.Scene(hs), hs.camera()


def _check_against_numpy(api, S, spp, A, N, iterations):
    got = api.denoise(S, spp, A, N, iterations=iterations)
    want, skip, L = denoise_ref(S, spp, A, N, iterations=iterations)
    assert_bits_equal(got[skip], S[skip], "pass-through pixels")
    assert_bits_equal(got[..., 3], S[..., 3], "w channel")
    use = ~skip
    np.testing.assert_allclose(got[use][:, :3], want[use][:, :3], rtol=1e-3, atol=1e-6 * L * spp)
    return got, skip


@pytest.fixture(scope="module")
def frame64(api, gpu_ready, scene_dir):
    gs, cam = _cornell(api, scene_dir, "dn64", 64, 48, spp=4, max_depth=4)
    S, _ = gs.render(cam, 64, 48, 4, 4)
    A, N = gs.render_aovs(cam, 64, 48, aov_spp=2)
    return S, A, N


@pytest.mark.parametrize("iterations", [0, 1, 5])
def test_denoise_matches_numpy(api, frame64, iterations):
    S, A, N = frame64
    got, skip = _check_against_numpy(api, S, 4, A, N, iterations)
    assert (~skip).sum() > 0.9 * skip.size
    if iterations:
        assert not np.array_equal(got, S)


def test_nan_inf_and_miss_pixels_pass_through(api, frame64):
    S, A, N = frame64
    S = S.copy(); A = A.copy()
    S[5, 7, 0] = np.nan; S[20, 30, 1] = np.inf; S[40, 2, 2] = -np.inf; S[41, 2, :3] = np.nan
    A[10:18, 40:52, 3] = 0.0                              # a miss region: coverage 0
    got, skip = _check_against_numpy(api, S, 4, A, N, 5)
    assert skip[5, 7] and skip[20, 30] and skip[40, 2] and skip[41, 2] and skip[10:18, 40:52].all()
    fin = api.finalise(got, 4)                            # novum_finalise still paints them
    assert np.allclose(fin[5, 7, :3], (1, 0, 1)) and np.allclose(fin[20, 30, :3], (0, 1, 0))


def test_out_may_alias_in_and_device_form_is_the_host_form(api, gpu_ready, frame64):
    torch = gpu_ready
    S, A, N = frame64
    h, w = S.shape[:2]
    want = api.denoise(S, 4, A, N)
    inplace = S.copy()
    api.denoise(inplace, 4, A, N, out=inplace)
    assert_bits_equal(inplace, want, "host, out = in")
    dS, dA, dN = (torch.from_numpy(x.copy()).to("cuda:0") for x in (S, A, N))
    ws = torch.empty(api.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    out = torch.full_like(dS, 3.0)
    api.denoise_device(w, h, dS.data_ptr(), 4, dA.data_ptr(), dN.data_ptr(), ws.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert_bits_equal(out.cpu().numpy(), want, "device form")
    api.denoise_device(w, h, dS.data_ptr(), 4, dA.data_ptr(), dN.data_ptr(), ws.data_ptr(), dS.data_ptr())
    torch.cuda.synchronize()
    assert_bits_equal(dS.cpu().numpy(), want, "device form, out = in")


def _quality(api, scene_dir, name, **kw):
    """Cornell 128 x 128, depth 8, MIS: raw 16 spp, reference 4096 spp (another seed), features at 4 rays per pixel."""
    gs, cam = _cornell(api, scene_dir, name, 128, 128, spp=16, max_depth=8, **kw)
    raw, _ = gs.render(cam, 128, 128, 16, 8)
    ref, _ = gs.render(cam, 128, 128, 4096, 8, seed=777)
    A, N = gs.render_aovs(cam, 128, 128, aov_spp=4)
    mask = ~passthrough_mask(raw, 16, A) & ~passthrough_mask(ref, 4096, A)
    refm = ref / 4096
    m_raw = mse(raw / 16, refm, mask)
    m_dn = mse(api.denoise(raw, 16, A, N) / 16, refm, mask)
    m_conv = mse(api.denoise(ref, 4096, A, N) / 4096, refm, mask)
    print("%s: MSE raw16 %.5g, denoised16 %.5g (ratio %.3f), denoised ref %.5g (ratio %.4f)" % (name, m_raw, m_dn, m_dn / m_raw, m_conv, m_conv / m_raw))
    return m_raw, m_dn, m_conv


def test_quality_diffuse_cornell(api, gpu_ready, scene_dir):
    m_raw, m_dn, m_conv = _quality(api, scene_dir, "dnq_diffuse")
    # measured 0.74: the error left is at the light's silhouette, which no feature buffer separates from the ceiling
    assert m_dn <= 0.8 * m_raw
    assert m_conv <= 0.05 * m_raw                         # a converged image keeps its edges


def test_quality_specular_cornell_is_not_harmed(api, gpu_ready, scene_dir):
    m_raw, m_dn, m_conv = _quality(api, scene_dir, "dnq_specular", tall_material=5, short_material=19)     # glass, mirror
    assert m_dn <= m_raw
    assert m_conv <= 0.05 * m_raw


def test_full_hd_aovs_and_denoise(api, gpu_ready, scene_dir):
    torch = gpu_ready
    w, h = 1920, 1080
    gs, cam = _cornell(api, scene_dir, "dnhd", w, h, spp=4, max_depth=4)
    S, _ = gs.render(cam, w, h, 4, 4)
    A, N = gs.render_aovs(cam, w, h)
    assert (A[..., 3] > 0).mean() > 0.9
    host = api.denoise(S, 4, A, N)
    dS = torch.from_numpy(S).to("cuda:0")
    dA = torch.empty(h, w, 4, device="cuda:0"); dN = torch.empty(h, w, 4, device="cuda:0")
    gs.render_aovs_device(cam, w, h, dA.data_ptr(), dN.data_ptr())
    ws = torch.empty(api.denoise_workspace_bytes(w, h), dtype=torch.uint8, device="cuda:0")
    out = torch.empty_like(dS)
    api.denoise_device(w, h, dS.data_ptr(), 4, dA.data_ptr(), dN.data_ptr(), ws.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert_bits_equal(dA.cpu().numpy(), A, "albedo")
    assert_bits_equal(dN.cpu().numpy(), N, "normal + depth")
    assert_bits_equal(out.cpu().numpy(), host, "device vs host denoise")
