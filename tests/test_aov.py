"""First-hit feature buffers (pt_render_aovs) against the CPU oracle's camera_ray + trace_closest, bit for bit."""
import os

import numpy as np
import pytest

from conftest import golden_scene
from denoise_ref import aovs_from_hits, sample_texture
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SEED = 103033


def _cam_bytes(cam):
    return np.frombuffer(cam.tobytes(), np.uint8).copy()


def _materials(osc):
    m = osc.array("materials").reshape(-1, 176)
    alb = m[:, 48:64].copy().view(np.float32)[:, :3]
    has_tex = m[:, 0] != 0
    tex_info = m[:, 4:16].copy().view(np.int32)            # startInd, width, height
    return alb, has_tex, tex_info


def _oracle_hits(O, osc, cam, w, h, seed):
    """Ray of every pixel from camera_ray(seed) through the oracle's trace_closest: (valid, material, albedo, normal, t, uv)."""
    cb = _cam_bytes(cam)
    rays = np.array([O.camera_ray(cb, x, y, seed) for y in range(h) for x in range(w)], np.float32)
    oi, of, _ = osc.trace_closest(rays)
    valid = oi[:, 0] == 1
    alb, _, _ = _materials(osc)
    albedo = np.where(valid[:, None], alb[np.maximum(oi[:, 2], 0)], 0.0).astype(np.float32)
    return valid, oi[:, 2], albedo, of[:, 6:9].copy(), of[:, 0].copy(), of[:, 9:11].copy()


def _pair(api, oracle, cfg):
    hs = api.HostScene(cfg)
    return api.Scene(hs), hs, oracle.OracleScene(cfg)


def _blob(scene_dir):
    from cudapathtracer_amd import scenes
    return scenes.blob_in_box(os.path.join(scene_dir, "aovblob3"), 40, 24, 1, 4, subdiv=3, name="aovblob3")["config"]


@pytest.mark.parametrize("which", ["cornell32", "mixed32", "thin_lens", "blob3"])
def test_aovs_are_bit_exact_against_the_oracle(api, oracle, gpu_ready, scene_dir, which):
    cfg = _blob(scene_dir) if which == "blob3" else golden_scene("cornell32" if which == "thin_lens" else which)
    gs, hs, osc = _pair(api, oracle, cfg)
    cam = hs.camera()
    w, h = cam.w, cam.h
    if which == "thin_lens":
        w, h = 40, 24
        cam = api.Camera.NotPinhole((0.15, -0.1, 1.2), w, h, (3.0, -8.0, 2.0), 55.0, 0.08, 2.2)
    alb, nd = gs.render_aovs(cam, w, h, aov_spp=1, seed=SEED)
    valid, _, a, n, t, _ = _oracle_hits(oracle, osc, cam, w, h, SEED)
    ra, rn = aovs_from_hits([(valid, a, n, t)], 1)
    assert valid.any()
    assert_bits_equal(alb.reshape(-1, 4), ra, "albedo + coverage")
    assert_bits_equal(nd.reshape(-1, 4), rn, "normal + depth")


def test_textured_albedo_is_the_texture_sample(api, oracle, gpu_ready):
    cfg = golden_scene("textured32", "scenes_tex")
    gs, hs, osc = _pair(api, oracle, cfg)
    cam = hs.camera()
    w, h = cam.w, cam.h
    alb, nd = gs.render_aovs(cam, w, h, aov_spp=1, seed=SEED)
    alb = alb.reshape(-1, 4); nd = nd.reshape(-1, 4)
    valid, mat, a, n, t, uv = _oracle_hits(oracle, osc, cam, w, h, SEED)
    _, has_tex, tex_info = _materials(osc)
    tex = osc.array("textures").view(np.float32).reshape(-1, 4)
    textured = valid & has_tex[np.maximum(mat, 0)]
    assert textured.any() and (valid & ~textured).any()
    plain = ~textured
    ra, rn = aovs_from_hits([(valid, a, n, t)], 1)
    assert_bits_equal(alb[plain], ra[plain], "untextured albedo")
    assert_bits_equal(nd, rn, "normal + depth")
    assert np.all(alb[textured, 3] == 1.0)
    for i in np.flatnonzero(textured):
        start, tw, th = (int(v) for v in tex_info[mat[i]])
        want = sample_texture(tex, start, tw, th, uv[i])
        if want is None:
            want = a[i]
        np.testing.assert_allclose(alb[i, :3], want, rtol=0, atol=1e-6)


def test_four_rays_per_pixel_compose_exactly(api, oracle, gpu_ready):
    gs, hs, osc = _pair(api, oracle, golden_scene("cornell32"))
    w, h = 40, 24
    cam = api.Camera.NotPinhole((0.0, 0.0, 2.2), w, h, (0.0, 0.0, 0.0), 70.0, 0.05, 2.5)    # wider than the box: some rays miss
    seed = 4242
    alb, nd = gs.render_aovs(cam, w, h, aov_spp=4, seed=seed)
    hits = [_oracle_hits(oracle, osc, cam, w, h, seed + k) for k in range(4)]
    ra, rn = aovs_from_hits([(v, a, n, t) for v, _, a, n, t, _ in hits], 4)
    assert_bits_equal(alb.reshape(-1, 4), ra, "albedo + coverage")
    assert_bits_equal(nd.reshape(-1, 4), rn, "normal + depth")
    cov = set(np.unique(alb[..., 3]).tolist())
    assert cov <= {0.0, 0.25, 0.5, 0.75, 1.0}
    assert 1.0 in cov and len(cov) >= 2


def test_an_aov_pass_between_chunks_leaves_the_render_untouched(api, gpu_ready):
    torch = gpu_ready
    hs = api.HostScene(golden_scene("cornell32"))
    gs = api.Scene(hs)
    cam = hs.camera()
    w, h = cam.w, cam.h
    gs.render(cam, w, h, 2, 4, counters=True)             # non-zero counters to watch
    before = gs.counters()
    assert before["rays_closest"] > 0
    seen = []

    def progress(done):
        c0 = gs.counters()
        a, n = gs.render_aovs(cam, w, h, aov_spp=3, seed=SEED)
        seen.append((done, c0 == gs.counters(), float(a[..., 3].sum())))
        return 0

    prog = torch.zeros(h, w, 4, device="cuda:0")
    gs.launch_progressive(0, 4, cam, 8, True, w, h, prog.data_ptr(), 2, progress=progress)
    one = torch.zeros(h, w, 4, device="cuda:0")
    gs.launch_unidirectional(4, cam, 8, True, w, h, one.data_ptr())
    assert [d for d, _, _ in seen] == [2, 4, 6, 8]
    assert all(same for _, same, _ in seen) and gs.counters() == before
    assert all(cov > 0 for _, _, cov in seen)
    assert_bits_equal(prog.cpu().numpy(), one.cpu().numpy(), "progressive with AOV passes vs one-shot")


def test_device_form_matches_host_form(api, gpu_ready):
    torch = gpu_ready
    hs = api.HostScene(golden_scene("mixed32"))
    gs = api.Scene(hs)
    cam = hs.camera()
    w, h = cam.w, cam.h
    a = torch.full((h, w, 4), 7.0, device="cuda:0")
    n = torch.full((h, w, 4), 7.0, device="cuda:0")
    s = torch.cuda.Stream()
    gs.render_aovs_device(cam, w, h, a.data_ptr(), n.data_ptr(), aov_spp=2, seed=11, stream=s.cuda_stream)
    s.synchronize()
    ha, hn = gs.render_aovs(cam, w, h, aov_spp=2, seed=11)
    assert_bits_equal(a.cpu().numpy(), ha, "albedo")
    assert_bits_equal(n.cpu().numpy(), hn, "normal + depth")
