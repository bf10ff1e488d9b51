"""The pt_preview session's selection (pt_preview_set_selection, pt_preview_pick, pt_preview_read_ids) at 40 x 24 on the glass + mirror
Cornell box: a session with a selection is the same session without one in everything but rgba8, its rgba8 is select_overlay of
the other's over render_ids of the frame's camera, the ID buffer is traced only when it is stale, and turning the selection off
restores the frame's bytes."""
import numpy as np
import pytest

import ids_cases as IC
import temporal_seq as Q
from test_temporal import _cams
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SPP, BATCHES, DEPTH = 4, 2, 4
W, H = IC.W, IC.H
LINKS = 4
ENTRIES = [("material", 0, 3, (255, 160, 0, 255), 2, 64), ("light", 0, 7, (255, 255, 255, 200), 1, 0), ("tri", 0, 11, (0, 90, 255, 255), 4, 30)]
AS_TUPLES = [({"tri": 0, "material": 1, "light": 2}[c],) + tuple(rest) for c, *rest in ENTRIES]


@pytest.fixture(scope="module")
def scene(api, gpu_ready, scene_dir):
    return api.Scene(IC.host(api, scene_dir, "cornell", "pvselect"))


def _session(api, scene, scale=1):
    return api.Preview(scene, W, H, spp=SPP, batches=BATCHES, max_depth=DEPTH).set_scale(scale).set_guide_centre(1).set_guide_chain(LINKS)


def _same_but_rgba8(got, want, what):
    for k in ("mean", "hist", "hist_len"):
        assert_bits_equal(got[k], want[k], "%s: %s" % (what, k))


@pytest.mark.parametrize("scale", [1, 2])
def test_a_selection_changes_nothing_but_the_bytes_and_traces_only_stale_ids(api, scene, scale):
    import ids_ref as IR
    cams = _cams(api, "pinhole", W, H, 2)
    rest = [api.Camera.frombytes(cams[1].tobytes()) for _ in range(2)]
    plain, sel = _session(api, scene, scale), _session(api, scene, scale).set_selection(ENTRIES, LINKS)
    assert sel.id_passes == 0 and plain.device_ids() is None and sel.device_ids() is not None
    with pytest.raises(api.PtError, match="pt_preview_pick: no frame"):
        sel.pick(3, 3, LINKS)
    with pytest.raises(api.PtError, match="pt_preview_read_ids"):
        sel.read_ids()
    passes = []
    for t, cam in enumerate(cams + rest):
        a, b = plain.frame(cam, Q.SEED0 + t).read(), sel.frame(cam, Q.SEED0 + t).read()
        what = "scale %d frame %d" % (scale, t)
        _same_but_rgba8(b, a, what)
        assert sel.guide_passes == plain.guide_passes and plain.id_passes == 0
        ids = scene.render_ids(cam, W, H, LINKS)
        assert np.array_equal(sel.read_ids(), ids), what
        want = IR.overlay(ids, a["rgba8"], AS_TUPLES)
        assert np.array_equal(b["rgba8"], want) and np.array_equal(api.select_overlay(ids, a["rgba8"], ENTRIES), want), what
        assert (b["rgba8"] != a["rgba8"]).any(-1).sum() >= 32 and np.array_equal(b["rgba8"][..., 3], a["rgba8"][..., 3])
        passes.append(sel.id_passes)
        # the session's pick is the scene's with the frame's camera, at display size at any render scale
        for x, y in ((0, 0), (W - 1, H - 1), (W // 2, H // 3)):
            got, want_p = sel.pick(x, y, LINKS), scene.pick(cam, W, H, [(x, y)], LINKS)
            assert np.array_equal(got[0], want_p[0][0]) and np.array_equal(got[1].view(np.uint32), want_p[1][0].view(np.uint32))
            assert np.array_equal(got[0], ids[y, x])
            assert np.array_equal(plain.pick(x, y, 0)[0], scene.render_ids(cam, W, H, 0)[y, x])
    assert passes == [1, 2, 2, 2]                               # two cameras, then two resting frames
    with pytest.raises(api.PtError, match="outside the 40 x 24 image"):
        sel.pick(W, 0, 0)
    plain.close(); sel.close()


def test_the_id_buffer_is_traced_once_while_nothing_changes_and_again_when_something_does(api, scene):
    cam = _cams(api, "pinhole", W, H, 2)
    same = lambda c: api.Camera.frombytes(c.tobytes())
    pv = _session(api, scene).set_selection(ENTRIES, LINKS)
    for t in range(3):
        pv.frame(same(cam[0]), Q.SEED0 + t)
    assert pv.id_passes == 1                                    # three resting frames
    pv.frame(cam[1], Q.SEED0 + 3); assert pv.id_passes == 2     # a camera move
    pv.frame(same(cam[1]), Q.SEED0 + 4); assert pv.id_passes == 2
    pv.scene_changed(True)
    pv.frame(same(cam[1]), Q.SEED0 + 5); assert pv.id_passes == 3     # pt_preview_scene_changed
    pv.frame(same(cam[1]), Q.SEED0 + 6); assert pv.id_passes == 3
    pv.set_selection(ENTRIES, 1)
    pv.frame(same(cam[1]), Q.SEED0 + 7); assert pv.id_passes == 4     # another max_links
    assert np.array_equal(pv.read_ids(), scene.render_ids(cam[1], W, H, 1))
    pv.set_selection(ENTRIES[:1], 1)                            # other entries: the IDs are not stale
    pv.frame(same(cam[1]), Q.SEED0 + 8); assert pv.id_passes == 4
    pv.reset()
    with pytest.raises(api.PtError, match="pt_preview_pick: no frame"):
        pv.pick(0, 0, 0)
    pv.frame(same(cam[1]), Q.SEED0 + 9); assert pv.id_passes == 5     # a reset
    pv.set_selection([], 0)
    pv.frame(cam[0], Q.SEED0 + 10); assert pv.id_passes == 5          # off: no pass at all
    pv.set_selection(ENTRIES, 1)
    pv.frame(same(cam[0]), Q.SEED0 + 11); assert pv.id_passes == 6    # on again: the buffer is another camera's
    assert np.array_equal(pv.read_ids(), scene.render_ids(cam[0], W, H, 1))
    with pytest.raises(api.PtError, match="radius 9 must be 1..4"):
        pv.set_selection([("tri", 0, 1, (1, 1, 1, 1), 9, 0)], 0)
    with pytest.raises(api.PtError, match="max_links 17 must be 0..16"):
        pv.set_selection(ENTRIES, 17)
    pv.close()


def test_turning_the_selection_off_restores_the_frames_bytes(api, scene):
    cams = _cams(api, "pinhole", W, H, 3)
    plain, sel = _session(api, scene), _session(api, scene).set_selection(ENTRIES, LINKS)
    for t, cam in enumerate(cams):
        if t == 2:
            sel.set_selection([])
        a, b = plain.frame(cam, Q.SEED0 + t).read(), sel.frame(cam, Q.SEED0 + t).read()
        _same_but_rgba8(b, a, "frame %d" % t)
        assert np.array_equal(a["rgba8"], b["rgba8"]) == (t == 2)
    assert sel.id_passes == 2
    plain.close(); sel.close()
