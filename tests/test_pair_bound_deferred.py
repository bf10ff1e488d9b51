"""The pair kernels' trips accept every positive finite t, and the ray's owner applies the range bound to the minimum (pt_trace.h:
trace_pair_flat, BOUND and ONEB). Exact by construction (tests/test_pair_bound_rule.py states the rule);
every frame here is compared bit for bit with a live oracle render (NaNs must coincide), and with the generic pair kernel, which
keeps the bounded trips, on the same device.

  cornell, cornell_mixed     the SIMPLE and the LEAN pair kernel
  cornell_ceiling_light      the whole ceiling emits: every unoccluded shadow ray now records a hit beyond its bound (the light)
  *_generic                  the same three scenes with {"simple": 0, "lean": 0}: megakernel_flat2<0, false, false>, the old trips
  moments                    pt_render_moments with "moments_fused" 1 (the sum buffer is the frame)
  far                        the Cornell scene times 2^18: part of the room lies beyond 999999 from the camera, part does not"""
import os

import numpy as np
import pytest

from util import assert_bits_equal

MIXED = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4])      # bench.py's cornell_mixed
GENERIC = {"simple": 0, "lean": 0}
# name: (scene, scenes.cornell arguments, width, height, spp, options, flags the launch must report)
CASES = {
    "cornell": ("cornell", dict(), 64, 40, 32, {}, dict(flat_pair=True, simple=True)),
    "cornell_ceiling_light": ("cornell_ceiling_light", dict(ceiling_light=True), 64, 40, 32, {}, dict(flat_pair=True, simple=True)),
    "cornell_mixed": ("cornell_mixed", MIXED, 64, 40, 16, {}, dict(flat_pair=True, simple=False, lean=True)),
    "cornell_generic": ("cornell", dict(), 64, 40, 32, GENERIC, dict(flat_pair=True, simple=False, lean=False)),
    "cornell_ceiling_light_generic": ("cornell_ceiling_light", dict(ceiling_light=True), 64, 40, 32, GENERIC, dict(flat_pair=True, simple=False, lean=False)),
    "cornell_mixed_generic": ("cornell_mixed", MIXED, 64, 40, 16, GENERIC, dict(flat_pair=True, simple=False, lean=False)),
}
FAR_FACTOR = 2.0 ** 18     # chosen with the oracle: at 2^17 the whole room is nearer than 999999, at 2^19 no pixel sees anything
_ORACLE = {}               # scene -> the oracle's frame: rendered once, shared by the pair kernel's case and the generic kernel's


def _config(scene_dir, case):
    from cudapathtracer_amd import scenes
    scene, kw, w, h, spp, _, _ = CASES[case]
    name = "bound_" + scene
    return scenes.cornell(os.path.join(scene_dir, name + "_%dx%d" % (w, h)), w, h, spp, 8, name=name, **kw)["config"]


def _want(oracle, cfg):
    if cfg not in _ORACLE:
        want, _, _ = oracle.OracleScene(cfg).render(threads=8)
        want.setflags(write=False)
        _ORACLE[cfg] = want
    return _ORACLE[cfg]


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_frames_equal_the_oracle(api, oracle, gpu_ready, scene_dir, case):
    _, _, w, h, spp, opts, want_flags = CASES[case]
    cfg = _config(scene_dir, case)
    hs = api.HostScene(cfg)
    sc = api.Scene(hs, options=opts)
    got, _ = sc.render(hs.camera(), w, h, spp, 8)                 # depth 8, MIS
    fl = sc.flags()
    assert {k: fl[k] for k in want_flags} == want_flags, fl
    assert sc.queue_stalls() == 0
    want = _want(oracle, cfg)
    assert np.isfinite(want[..., :3]).mean() > 0.99 and float(np.nan_to_num(want[..., :3], nan=0.0, posinf=0.0, neginf=0.0).sum()) > 0.0
    assert_bits_equal(got, want, case)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "cornell_mixed"])
def test_the_moments_entry_point_sums_the_same_frame(api, oracle, gpu_ready, scene_dir, scene):
    """pt_render_moments with "moments_fused" 1: S is render(spp) bit for bit. (`cornell` is the case asked for; the SIMPLE pair
    kernel's fused twin is out of the dispatch, DESIGN.md §9a, so that frame is summed in batches by the headline kernel itself.
    `cornell_mixed` is the one launch of the LEAN pair kernel's twin.)"""
    from cudapathtracer_amd import scenes
    w, h, spp, c = 32, 24, 8, 2
    name = "bound_moments_" + scene
    cfg = scenes.cornell(os.path.join(scene_dir, name), w, h, spp, 8, name=name, **(MIXED if scene == "cornell_mixed" else {}))["config"]
    hs = api.HostScene(cfg)
    sc = api.Scene(hs, options={"moments_fused": 1})
    S, Q = sc.render_moments(hs.camera(), w, h, spp, c, 8)
    fl = sc.flags()
    assert fl["flat_pair"] and fl["simple"] == (scene == "cornell") and fl["lean"] == (scene == "cornell_mixed"), fl
    assert sc.last_moments_launches() == (spp // c if scene == "cornell" else 1), sc.last_moments_launches()
    assert (Q[..., 3] == spp // c).all() and sc.queue_stalls() == 0
    want, _, _ = oracle.OracleScene(cfg).render(threads=8)
    assert float(np.nan_to_num(want[..., :3], nan=0.0, posinf=0.0, neginf=0.0).sum()) > 0.0
    assert_bits_equal(S, want, "moments " + scene)
    sc.close()


def _scaled(src_cfg, dst_dir, factor):
    """A copy of the files scenes.cornell wrote with every vertex and the camera position times `factor` (a power of two: exact)."""
    os.makedirs(dst_dir, exist_ok=True)
    src_dir = os.path.dirname(src_cfg)
    f32 = np.float32

    def times(words):
        return " ".join("%.9g" % float(f32(x) * f32(factor)) for x in words)
    for fn in sorted(os.listdir(src_dir)):
        with open(os.path.join(src_dir, fn)) as f:
            lines = f.read().split("\n")
        for i, ln in enumerate(lines):
            if ln.startswith("v "):
                lines[i] = "v " + times(ln.split()[1:])
            elif ln.startswith("Camera Position:"):
                lines[i] = "Camera Position: " + times(ln.split()[2:])
        with open(os.path.join(dst_dir, fn), "w") as f:
            f.write("\n".join(lines))
    return os.path.join(dst_dir, os.path.basename(src_cfg))


@pytest.mark.gpu
def test_a_room_that_reaches_beyond_the_extension_bound(api, oracle, gpu_ready, scene_dir):
    """The extension ray's bound itself: surfaces beyond 999999 are hit by the unbounded trips and must be a miss in stage 3."""
    from cudapathtracer_amd import scenes
    w, h, spp = 32, 24, 8
    base = scenes.cornell(os.path.join(scene_dir, "bound_far_base"), w, h, spp, 8, name="bound_far")["config"]
    cfg = _scaled(base, os.path.join(scene_dir, "bound_far_scaled"), FAR_FACTOR)
    want, _, _ = oracle.OracleScene(cfg).render(threads=8)
    dark = (want.view(np.uint32) << 1 == 0).all(axis=-1)          # exactly zero in all channels (either sign of zero)
    print("far scene: %d pixels exactly zero, %d not" % (int(dark.sum()), int((~dark).sum())))
    assert dark.sum() >= 16 and (~dark).sum() >= 16
    hs = api.HostScene(cfg)
    pts = hs.array("points").view(np.float32).reshape(-1, 4)[:, :3]
    reach = np.linalg.norm(pts.astype(np.float64) - np.array([0.0, 0.0, FAR_FACTOR]), axis=1)
    assert reach.min() < 999999.0 < reach.max(), (reach.min(), reach.max())      # part of the room on each side of the bound
    for opts, flags in (({}, dict(flat_pair=True, simple=True)), (GENERIC, dict(flat_pair=True, simple=False, lean=False))):
        sc = api.Scene(hs, options=opts)
        got, _ = sc.render(hs.camera(), w, h, spp, 8)
        fl = sc.flags()
        assert {k: fl[k] for k in flags} == flags, fl
        assert sc.queue_stalls() == 0
        assert_bits_equal(got, want, "far scene %s" % (opts,))
        sc.close()
