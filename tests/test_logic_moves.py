"""The pair kernels' logic step without the register fills and copies nothing reads (pt_device.h:
indeterminate): values that only one arm of a split defines are no longer zero-filled on the other, so a lane that does not take the
arm holds whatever its register held. No arithmetic changed and no lane reads such a value: every frame here equals a live oracle
render bit for bit (NaNs must coincide). Each case is the smallest shape in which some lanes of a wave hold a value and others never
receive it; a register that leaked into a result would differ from lane to lane and from launch to launch."""
import os

import numpy as np
import pytest

from util import assert_bits_equal

MIXED = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4])      # bench.py's cornell_mixed
SIMPLE = dict(flat_pair=True, simple=True)
LEAN = dict(flat_pair=True, simple=False, lean=True)
# name: (scene, scenes.cornell arguments, width, height, spp, max_depth, flags the launch must report)
CASES = {
    "ragged_1spp": ("cornell", dict(), 9, 9, 1, 8, SIMPLE),          # four tiles; most lanes never own a path: their state stays what tile start leaves
    "ragged": ("cornell", dict(), 20, 12, 8, 8, SIMPLE),             # lanes outside the image
    "ragged_mixed": ("cornell", MIXED, 20, 12, 8, 8, LEAN),          # ... in the LEAN pair kernel
    "ceiling_light": ("cornell", dict(ceiling_light=True), 24, 16, 8, 8, SIMPLE),      # NEE records are written but never valid
    "roulette": ("cornell", dict(), 24, 16, 16, 2, SIMPLE),          # the conditional draw in nearly every pass, beside lanes that do not draw
    "misses": ("open_back", dict(), 24, 16, 8, 8, SIMPLE),           # some lanes miss (h.tri < 0) while others bounce
}


def _open_back(outdir, w, h, spp, depth, name):
    """The Cornell shell with its back wall left out and no boxes: the rays through the middle of the frame leave the scene."""
    from cudapathtracer_amd import scenes
    meshes, _ = scenes._shell(w / h, back_material=0)
    return scenes._emit(outdir, name, meshes, w, h, spp, depth)["config"]


def _config(scene_dir, case):
    from cudapathtracer_amd import scenes
    kind, kw, w, h, spp, depth, _ = CASES[case]
    name = "moves_%s_%s_%dx%d_%d_%d" % (kind, "_".join(sorted(kw)) or "plain", w, h, spp, depth)
    out = os.path.join(scene_dir, name)
    if kind == "open_back":
        return _open_back(out, w, h, spp, depth, name)
    return scenes.cornell(out, w, h, spp, depth, name=name, **kw)["config"]


_FRAMES = {}      # config -> (the oracle's frame, its counters): rendered once, read by every test below, never written to


def _oracle(oracle, cfg):
    if cfg not in _FRAMES:
        frame, counters, _ = oracle.OracleScene(cfg).render(counters=True, threads=8)      # size, spp, depth, integrator: the scene file's
        frame.setflags(write=False); counters.setflags(write=False)
        _FRAMES[cfg] = (frame, counters)
    return _FRAMES[cfg]


def _reference_is_sound(want):
    return np.isfinite(want[..., :3]).mean() >= 0.99 and float(np.nan_to_num(want[..., :3], nan=0.0, posinf=0.0, neginf=0.0).sum()) != 0.0


def _render(api, cfg, case, options=None):
    _, _, w, h, spp, depth, want_flags = CASES[case]
    hs = api.HostScene(cfg)
    sc = api.Scene(hs, options=options or {})
    got, _ = sc.render(hs.camera(), w, h, spp, depth)
    fl = sc.flags()
    print(case, options, {k: fl[k] for k in want_flags})
    assert {k: fl[k] for k in want_flags} == want_flags, fl
    assert sc.queue_stalls() == 0
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_frames_equal_the_oracle(api, oracle, gpu_ready, scene_dir, case):
    """(misses: the plan gives the shell without its back wall the SIMPLE pair kernel, as the flags assert.)"""
    cfg = _config(scene_dir, case)
    want, _ = _oracle(oracle, cfg)
    assert _reference_is_sound(want)
    assert_bits_equal(_render(api, cfg, case), want, case)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_references_are_sound_and_enter_the_arms(oracle, scene_dir, case):
    """CPU only: what the GPU tests assume about their reference, and that each case does what its comment says. The counters are
    the reference's, per pixel: rays_closest, rays_shadow, pops, boxes, tris, hits, draws, iters (logic steps)."""
    _, _, w, h, spp, depth, _ = CASES[case]
    want, cnt = _oracle(oracle, _config(scene_dir, case))
    assert want.shape == (h, w, 4) and _reference_is_sound(want)
    iters, shadow = cnt[..., 7].astype(np.int64), cnt[..., 1].astype(np.int64)
    if case == "ragged_1spp":
        assert (-(-w // 8)) * (-(-h // 8)) == 4 and w * h < 4 * 64 // 2             # four tiles, most of their lanes without a pixel
    if case.startswith("ragged"):
        assert w % 8 != 0 and h % 8 != 0
    if case == "ceiling_light":
        assert shadow.sum() > 0                                                     # NEE samples are drawn and their records written
        assert (want[0, :, :3] > 0.0).all()                                         # the top row sees the emitter itself
    if case == "roulette":
        # the draw comes at the end of a path's fourth logic step (depth 3 > max_depth 2) and of every later one, so a pixel with more
        # than 3 steps per sample has a path that took it; every tile (wave) has such pixels, and a path's first three steps, which
        # every sample has, draw nothing there
        assert depth == 2
        drew = (iters > 3 * spp).reshape(h // 8, 8, w // 8, 8).any(axis=(1, 3))
        assert drew.all(), drew
    if case == "misses":
        # a pixel whose every path left through the missing wall at once is exactly 0, beside pixels that see a wall: both kinds in
        # the four middle tiles' rows
        mid = want[4:12, :, :3].sum(axis=-1)
        assert (mid == 0.0).any() and (mid > 0.0).any()
        assert (iters[4:12] == spp).any() and (iters[4:12] > spp).any()              # one logic step per sample: the miss itself


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ragged", "ragged_mixed"])
def test_chunked_launches_equal_the_one_shot_frame(api, oracle, gpu_ready, scene_dir, case):
    """The progressive launcher in chunks of 3 stores and reloads every pixel's stream and sum between its launches; with the
    smallest slice length the scene options accept a tile changes hands inside one launch, its state written back by one wave and
    continued by another. Both are the one-shot frame, which is the oracle's."""
    torch = gpu_ready
    _, _, w, h, spp, depth, want_flags = CASES[case]
    cfg = _config(scene_dir, case)
    want, _ = _oracle(oracle, cfg)
    assert _reference_is_sound(want)
    hs = api.HostScene(cfg)
    sc = api.Scene(hs)
    colors = torch.zeros(h, w, 4, device="cuda")
    seen = []
    sc.launch_progressive(0, depth, hs.camera(), spp, True, w, h, colors.data_ptr(), 3, lambda done: seen.append(done))
    assert seen == [3, 6, 8]
    fl = sc.flags()
    assert {k: fl[k] for k in want_flags} == want_flags, fl
    assert_bits_equal(colors.cpu().numpy(), want, case + ": chunks of 3")
    sliced = dict(slice_always=1, sched_mask=0, slice_iters=1)
    assert_bits_equal(_render(api, cfg, case, sliced), want, case + ": slices of one pass")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ragged", "ragged_mixed"])
def test_moments_fused_equals_the_batch_form(api, oracle, gpu_ready, scene_dir, case):
    """Batches of 2: the sum and the squared batch sums with "moments_fused" on equal those with it off bit for bit, for the scene of
    either pair kernel, and the sum is the frame."""
    _, _, w, h, spp, depth, _ = CASES[case]
    cfg = _config(scene_dir, case)
    want, _ = _oracle(oracle, cfg)
    hs = api.HostScene(cfg)
    off, on = api.Scene(hs), api.Scene(hs, options={"moments_fused": 1})
    try:
        S0, Q0 = off.render_moments(hs.camera(), w, h, spp, 2, depth)
        S1, Q1 = on.render_moments(hs.camera(), w, h, spp, 2, depth)
        assert off.queue_stalls() == 0 and on.queue_stalls() == 0
    finally:
        off.close(); on.close()
    assert_bits_equal(S1, S0, case + ": S"); assert_bits_equal(Q1, Q0, case + ": Q")
    assert_bits_equal(S0, want, case + ": S is the frame")


@pytest.mark.gpu
def test_the_same_frame_twice_with_another_between(api, oracle, gpu_ready, scene_dir):
    """`ragged`, then an unrelated 64 x 40 frame that leaves other values in the registers and in LDS, then `ragged` again in the same
    process: the two frames are equal bit for bit (and the oracle's). A leaked indeterminate register would differ."""
    from cudapathtracer_amd import scenes
    cfg = _config(scene_dir, "ragged")
    want, _ = _oracle(oracle, cfg)
    first = _render(api, cfg, "ragged")
    other = scenes.cornell(os.path.join(scene_dir, "moves_other_64x40"), 64, 40, 4, 8, name="moves_other_64x40", **MIXED)["config"]
    hs = api.HostScene(other)
    frame, _ = api.Scene(hs).render(hs.camera(), 64, 40, 4, 8)
    assert np.isfinite(frame[..., :3]).mean() >= 0.99
    second = _render(api, cfg, "ragged")
    assert_bits_equal(second, first, "ragged, again")
    assert_bits_equal(first, want, "ragged")
