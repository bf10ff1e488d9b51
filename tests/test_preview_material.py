"""The pt_preview session across a material or emission edit (pt_scene_update_materials / pt_scene_update_emission), at 40 x 24 with
3 + 1..2 frames as tests/test_preview_update.py: an announced edit keeps the history and every frame stays the chain of host calls
on the edited scene (plain, with respond on, and with centre guides, whose guide is traced again although the camera rests); an
unannounced edit is a fresh session on a fresh scene; and a vertex update followed by an edit is no motion frame. The session's
code needed no change for any of it."""
import numpy as np
import pytest

import motion_cases as MC
from test_material_update import MAT, TRI
from test_preview import _assert_frame
from test_preview_respond import _chain_step as _respond_step
from test_preview_update import _chain_step
from test_temporal import _cams

pytestmark = pytest.mark.gpu

SPP, BATCHES, DEPTH = 4, 2, 4
W, H = MC.W, MC.H
BEFORE, AFTER = 3, 2
EDIT = ([0, 1], np.array([[2.5, 4.6, 8.0, 0.0], [2.5, 4.6, 8.0, 0.0]], np.float32))        # both lights dimmer and bluer


@pytest.fixture(scope="module")
def host(api, gpu_ready, scene_dir):
    return MC.cornell_host(api, scene_dir, "material_pv")


def _params(**kw):
    return dict(spp=SPP, batches=BATCHES, max_depth=DEPTH, **kw)


def _same_frame(got, want, what):
    _assert_frame(got, (want["mean"], want["hist"], want["hist_len"], None), what)
    assert np.array_equal(got["rgba8"], want["rgba8"]), what + ": bytes"


def _painted(host):
    """The scene's arrays with the most used diffuse row (walls, floor, ceiling) repainted."""
    a = MC.arrays(host)
    m = a["materials"].view(MAT)
    used = np.bincount(a["mesh"].view(TRI)["materialID"], minlength=len(m))
    row = int(np.argmax(np.where(m["type"] == 0, used, 0)))
    assert used[row] > 0 and m["type"][row] == 0
    m["albedo"][row][:3] = (0.35, 0.7, 0.5)
    return a


# ---- (a) an announced edit: the history is kept, every frame is the chain of host calls ---------------------------------------------------
@pytest.mark.parametrize("name,centre,kind,respond", [
    ("plain", 0, "pinhole", False),
    ("centre, resting camera", 1, "identity", False),        # the guide must be traced again although the camera rests
    ("respond", 0, "identity", True),
    ("respond, centre", 1, "identity", True)])
def test_an_announced_emission_edit_equals_the_chain_of_host_calls(api, host, name, centre, kind, respond):
    cams = _cams(api, kind, W, H, BEFORE + AFTER)
    seeds = [70 + t for t in range(BEFORE + AFTER)]
    sc = api.Scene.from_mesh(host)
    pv = api.Preview(sc, W, H, **_params()).set_guide_centre(centre)
    rp = api.respond_defaults()
    if respond:
        pv.set_respond(**rp)
    state = (None,) * 5
    for t, (cam, seed) in enumerate(zip(cams, seeds)):
        changed = t == BEFORE
        if changed:
            sc.update_emission(*EDIT)
            pv.scene_changed(True)
        before = pv.guide_passes
        if respond:
            state, want, _ = _respond_step(api, sc, state, cam, seed, centre, 1, changed, False, rp)
        else:
            state, want = _chain_step(api, sc, state, cam, seed, centre, changed)
        got = pv.frame(cam, seed).read()
        what = "%s frame %d" % (name, t)
        _assert_frame(got, want, what)
        assert np.array_equal(got["rgba8"], api.resolve(want[3], 1)[0]), what
        if centre and kind == "identity":
            assert pv.guide_passes - before == (1 if t == 0 or changed else 0), what
    assert got["hist_len"].max() > AFTER                      # history from before the edit is still in the frame
    pv.close(); sc.close()


# ---- (b) an unannounced edit: the generation check resets the session ----------------------------------------------------------------------
def test_an_unannounced_material_edit_is_a_fresh_session_on_a_fresh_scene(api, host):
    cams = _cams(api, "pinhole", W, H, BEFORE + AFTER)
    seeds = [50 + t for t in range(BEFORE + AFTER)]
    new = _painted(host)
    sc = api.Scene.from_mesh(host)
    pv = api.Preview(sc, W, H, **_params())
    for t in range(BEFORE):
        pv.frame(cams[t], seeds[t])
    assert pv.read()["hist_len"].max() == BEFORE
    sc.update_materials(new["materials"])
    fresh_scene = api.Scene.from_mesh(new, host.info["leaf_size"])
    fresh = api.Preview(fresh_scene, W, H, **_params())
    for t in range(BEFORE, BEFORE + AFTER):
        got, want = pv.frame(cams[t], seeds[t]).read(), fresh.frame(cams[t], seeds[t]).read()
        _same_frame(got, want, "unannounced, frame %d" % t)
        assert got["hist_len"].max() == t - BEFORE + 1        # a first frame, then a second
    pv.close(); fresh.close(); sc.close(); fresh_scene.close()


# ---- (c) a vertex update, then an edit, before one frame: no motion frame -----------------------------------------------------------------
def test_a_vertex_update_then_an_edit_is_no_motion_frame(api, host):
    cams = _cams(api, "pinhole", W, H, BEFORE + 1)
    new = _painted(host)
    moved = MC.moved_arrays(host)["points"]
    scs = [api.Scene.from_mesh(host) for _ in range(2)]
    pvs = [api.Preview(sc, W, H, **_params()).set_motion(on) for sc, on in zip(scs, (0, 1))]
    for t in range(BEFORE):
        for pv in pvs:
            pv.frame(cams[t], 30 + t)
    for sc, pv in zip(scs, pvs):
        sc.update_vertices(moved)
        assert sc.has_motion == 1
        sc.update_materials(new["materials"])
        assert sc.has_motion == 0                             # the previous positions are kept, the flag drops
        pv.scene_changed(True)
    off, on = (pv.frame(cams[BEFORE], 33).read() for pv in pvs)
    _same_frame(on, off, "vertex update + edit")
    assert pvs[1].guide_passes == BEFORE + 1 and on["hist_len"].max() > 1     # no motion pass; keep_history 1: the history was kept
    for pv in pvs:
        pv.close()
    for sc in scs:
        sc.close()
