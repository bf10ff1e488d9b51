"""The pair kernels' logic step with its duplicate arms merged (pt_megakernel.h: the ARMS switch): the uniform inv3
at the head of the pair pass, one basis normalise, one light pdf and MIS weight for the emitter and the NEE arm, one direction
normalise for bounce and regeneration. No arithmetic changed, only how often a wave issues it:
every frame here equals a live oracle render bit for bit (NaNs must coincide). Each case is the smallest frame in which some lanes of
a wave enter a changed arm and others do not."""
import os

import numpy as np
import pytest

from util import assert_bits_equal

MIXED = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4])      # bench.py's cornell_mixed
SIMPLE = dict(flat_pair=True, simple=True)
LEAN = dict(flat_pair=True, simple=False, lean=True)
# camera: None = the scene file's; else (pinhole, position, rotation in degrees, aperture, focal distance, jitter or None = the default)
AT_LIGHT = (True, (0.0, -0.4, -1.4), (65.0, 0.0, 0.0), 0.0, 0.0, None)      # from below the light, looking up at it: emitter hits at depth >= 1 are common
ON_AXIS = (False, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 0.0, 2.0, 0.0)           # no lens, no jitter: the centre column's d.x and the centre row's d.y are exactly 0
# name: (scene, scenes.cornell arguments, width, height, spp, camera, flags the launch must report)
CASES = {
    "cornell": ("cornell", dict(), 64, 40, 32, None, SIMPLE),                                  # every step
    "light_in_view": ("cornell", dict(), 64, 40, 32, AT_LIGHT, SIMPLE),                        # steps 1 and 3: emitter hits with MIS
    "ceiling_light": ("cornell", dict(ceiling_light=True), 64, 40, 32, None, SIMPLE),          # every upward hit takes the emitter arm, no shadow ray is valid
    "both_basis_arms": ("cornell", dict(), 64, 40, 16, (True, (0.3, 0.2, 1.0), (0.0, 12.0, 0.0), 0.0, 0.0, None), SIMPLE),   # the rotated boxes, seen from the side
    "basis_boundary": ("box45", dict(), 64, 40, 16, None, SIMPLE),                             # a face normal with |n.x| == |n.z| exactly
    "aperture": ("cornell", dict(), 64, 40, 16, (False, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 0.05, 2.5, None), SIMPLE),   # the lens arm's two draws before the merged normalise
    "no_aperture": ("cornell", dict(), 64, 40, 16, (False, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 0.0, 2.5, None), SIMPLE),
    "axis_parallel": ("cornell", dict(), 64, 40, 16, ON_AXIS, SIMPLE),                         # the uniform inv3's IEEE fallback, for lanes that have the ray
    "ragged": ("cornell", dict(), 20, 12, 8, None, SIMPLE),                                    # lanes outside the image never have a ray
    "mixed": ("cornell", MIXED, 64, 40, 16, None, LEAN),                                       # the LEAN pair kernel shares steps 1 to 4
    "mixed_light_in_view": ("cornell", MIXED, 64, 40, 16, AT_LIGHT, LEAN),
}


def _box45(outdir, w, h, spp, name):
    """The Cornell shell with ONE box, rotated by 45 degrees about y: its side faces' normals are (+-s, 0, +-s)."""
    from cudapathtracer_amd import scenes
    meshes, zc = scenes._shell(w / h)
    box = scenes.Mesh("box45", 2)
    scenes._box(box, 0.0, zc, 0.4, 0.9, 0.4, -1.0 + 1e-3, 45.0)
    return scenes._emit(outdir, name, meshes + [box], w, h, spp, 8)["config"]


def _config(scene_dir, case):
    from cudapathtracer_amd import scenes
    kind, kw, w, h, spp, _, _ = CASES[case]
    name = "arms_%s_%s_%dx%d_%d" % (kind, "_".join(sorted(kw)) or "plain", w, h, spp)      # cases that differ by camera alone share one scene
    out = os.path.join(scene_dir, name)
    if kind == "box45":
        return _box45(out, w, h, spp, name)
    return scenes.cornell(out, w, h, spp, 8, name=name, **kw)["config"]


def _camera(api, hs, case):
    from cudapathtracer_amd import scenes
    _, _, w, h, _, spec, _ = CASES[case]
    if spec is None:
        return hs.camera()
    pinhole, pos, rot, aperture, focal, jitter = spec
    cam = api.make_camera(pinhole, pos, rot, scenes.FOV, w, h, aperture, focal)
    if jitter is not None:
        cam.antiAliasJitterDist = jitter
    return cam


_FRAMES = {}      # (config, camera bytes) -> the oracle's frame: rendered once, read by both tests below, never written to


def _oracle_frame(oracle, cfg, cam):
    key = (cfg, cam.tobytes())
    if key not in _FRAMES:
        _FRAMES[key] = oracle.OracleScene(cfg).render(camera=np.frombuffer(cam.tobytes(), np.uint8).copy(), threads=8)[0]
        _FRAMES[key].setflags(write=False)
    return _FRAMES[key]


def _reference_is_sound(want):
    return np.isfinite(want[..., :3]).mean() > 0.99 and float(np.nan_to_num(want[..., :3], nan=0.0, posinf=0.0, neginf=0.0).sum()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_frames_equal_the_oracle(api, oracle, gpu_ready, scene_dir, case):
    _, _, w, h, spp, _, want_flags = CASES[case]
    cfg = _config(scene_dir, case)
    hs = api.HostScene(cfg)
    cam = _camera(api, hs, case)
    sc = api.Scene(hs)
    got, _ = sc.render(cam, w, h, spp, 8)                          # depth 8, MIS
    fl = sc.flags()
    assert {k: fl[k] for k in want_flags} == want_flags, fl
    assert sc.queue_stalls() == 0
    want = _oracle_frame(oracle, cfg, cam)
    assert _reference_is_sound(want)
    assert_bits_equal(got, want, case)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_references_are_sound_and_enter_the_arms(api, oracle, scene_dir, case):
    """CPU only: what the GPU test asserts about its reference, and that the case's camera does what its comment says."""
    _, _, w, h, _, spec, _ = CASES[case]
    cfg = _config(scene_dir, case)
    hs = api.HostScene(cfg)
    cam = _camera(api, hs, case)
    want = _oracle_frame(oracle, cfg, cam)
    assert _reference_is_sound(want)
    if case == "basis_boundary":
        n = hs.array("normals").view(np.float32).reshape(-1, 4)[:, :3]
        tie = (np.abs(n[:, 0]) == np.abs(n[:, 2])) & (n[:, 0] != 0.0)
        assert tie.any(), n
    if case == "axis_parallel":
        rays = np.array([oracle.camera_ray(np.frombuffer(cam.tobytes(), np.uint8).copy(), x, y) for x, y in ((w // 2, 3), (5, h // 2))])
        assert rays[0, 3] == 0.0 and rays[1, 4] == 0.0 and rays[0, 4] != 0.0, rays
    if case in ("light_in_view", "mixed_light_in_view"):
        # the light fills a good part of the frame: its pixels carry the emission (10 per sample and channel, times spp)
        assert (want[..., 0] > 5.0 * CASES[case][4]).mean() > 0.05
