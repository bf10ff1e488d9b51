"""The motion pass (pt_render_motion) and the history stage with motion (pt_temporal_accumulate_motion, _cur_motion) on the GPU against
their numpy restatement (tests/motion_ref.py), bit for bit: the restatement reads the library's own closest hits
(pt_probe_centre_rays + pt_probe_trace_closest), so what is compared is the motion arithmetic, the choice of positions and the
reprojection. The Cornell input is tests/motion_cases.py's, which tests/test_motion_ref_cpu.py checks without a GPU."""
import os

import numpy as np
import pytest

import motion_cases as MC
import motion_ref as M
import temporal_ref as T
from test_scene_update import _moved
from test_temporal import _cams
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SPP, BATCHES, DEPTH = 4, 2, 4
W, H = MC.W, MC.H


@pytest.fixture(scope="module")
def hosts(api, gpu_ready, scene_dir):
    from cudapathtracer_amd import scenes
    blob = scenes.blob_in_box(os.path.join(scene_dir, "motion_blob"), 48, 32, 2, 5, subdiv=4, name="motion_blob")["config"]
    return {"cornell": MC.cornell_host(api, scene_dir), "ragged": MC.cornell_host(api, scene_dir, "motion_ragged", 37, 21),
            "blob": api.HostScene(blob)}


def _want_motion(api, sc, cam, w, h, cur, prev, mesh):
    """motion_ref.motion over the library's own closest hits along the centre rays."""
    xy = np.array([(x, y) for y in range(h) for x in range(w)], np.int32)
    gi, gf, _ = sc.trace_closest(api.probe_centre_rays(cam, xy))
    return M.motion(cur, prev, mesh, (gi[:, 0] == 1, gf[:, 1], gf[:, 2], gi[:, 1])).reshape(h, w, 4)


# ---- (a), (b) the pass against the restatement, and its guide outputs ------------------------------------------------------------------
@pytest.mark.parametrize("case", ["box", "light", "blob"])
def test_motion_is_the_restatement_and_the_guides_are_the_centre_pass(api, hosts, case):
    hs = hosts["blob" if case == "blob" else "ragged"]
    w, h = hs.info["width"], hs.info["height"]
    assert (w, h) == ((48, 32) if case == "blob" else (37, 21))
    old = MC.arrays(hs)
    new = _moved(hs, "displace") if case == "blob" else MC.moved_arrays(hs, *((48, 72) if case == "box" else (20, 24)))
    cam = hs.camera()
    sc = api.Scene.from_mesh(hs)
    if case == "blob":
        assert not sc.flags()["onchip"]                      # a scene in HBM, with a spill area
    sc.update_vertices(new["points"])
    assert sc.has_motion == 1
    A, N, mv = sc.render_motion(cam, w, h, guides=True)
    want = _want_motion(api, sc, cam, w, h, new["points"], old["points"], new["mesh"])
    moved = want[..., 3] == 1
    print("%s: %d of %d pixels moved" % (case, moved.sum(), moved.size))
    # (the light quad is a few pixels of the ceiling at this size; every blob vertex moves, the box's walls with it)
    assert moved.sum() >= (4 if case == "light" else 16) and (case == "blob" or (~moved).sum() >= 16)
    assert_bits_equal(mv, want, case + ": motion")
    assert_bits_equal(sc.render_motion(cam, w, h), mv, case + ": motion without the guide outputs")
    ca, cn = sc.render_aovs_centre(cam, w, h, 0)
    assert_bits_equal(A, ca, case + ": albedo"); assert_bits_equal(N, cn, case + ": normal_depth")
    sc.close()


def test_device_form_is_the_host_form(api, gpu_ready, hosts):
    torch = gpu_ready
    hs = hosts["ragged"]
    w, h = 37, 21
    cam = hs.camera()
    sc = api.Scene.from_mesh(hs)
    sc.update_vertices(MC.moved_arrays(hs)["points"])
    A, N, mv = sc.render_motion(cam, w, h, guides=True)
    d = [torch.full((h, w, 4), 3.0, device="cuda:0") for _ in range(4)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sc.render_motion_device(cam, w, h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), stream=s.cuda_stream)
        sc.render_motion_device(cam, w, h, 0, 0, d[3].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    for got, want, what in zip(d, (A, N, mv, mv), ("albedo", "normal_depth", "motion", "motion alone")):
        assert_bits_equal(got.cpu().numpy(), want, what)
    sc.close()


# ---- (c) all-zero cases -------------------------------------------------------------------------------------------------------------
def test_scenes_without_previous_positions_and_unmoved_vertices_are_static(api, hosts):
    hs = hosts["cornell"]
    cam = hs.camera()
    new = MC.moved_arrays(hs)
    fresh = api.Scene.from_mesh(hs)
    assert fresh.has_motion == 0 and not fresh.render_motion(cam, W, H).any()
    caller = api.Scene(hs)                                   # the caller's own tree: it keeps no positions at all
    assert caller.has_motion == 0
    A, N, mv = caller.render_motion(cam, W, H, guides=True)
    assert not mv.any()
    ca, cn = caller.render_aovs_centre(cam, W, H, 0)
    assert_bits_equal(A, ca, "albedo"); assert_bits_equal(N, cn, "normal_depth")
    fresh.update_vertices(new["points"])
    assert fresh.has_motion == 1 and fresh.render_motion(cam, W, H).any()
    fresh.update_mesh(new, hs.info["leaf_size"])             # the topology may have changed: the previous positions are dropped
    assert fresh.has_motion == 0 and not fresh.render_motion(cam, W, H).any()
    fresh.update_vertices(new["points"])                     # the positions it already has
    assert fresh.has_motion == 1 and not fresh.render_motion(cam, W, H).any()
    caller.close(); fresh.close()


# ---- (d) a refused update, and two updates in a row ---------------------------------------------------------------------------------
def test_a_refused_update_keeps_the_motion_and_a_second_update_moves_on(api, hosts):
    hs = hosts["cornell"]
    cam = hs.camera()
    old, first = MC.arrays(hs), MC.moved_arrays(hs)
    second = MC.moved_arrays(hs, shift=(0.35, 0.05, 0.2))
    sc = api.Scene.from_mesh(hs)
    bad = MC.arrays(hs)["points"].copy()
    bad.view(np.float32)[4 * 50] = np.nan
    with pytest.raises(api.PtError):
        sc.update_vertices(bad)
    assert sc.has_motion == 0 and sc.generation == 0 and not sc.render_motion(cam, W, H).any()
    sc.update_vertices(first["points"])
    mv1 = sc.render_motion(cam, W, H)
    assert_bits_equal(mv1, _want_motion(api, sc, cam, W, H, first["points"], old["points"], first["mesh"]), "after the first update")
    with pytest.raises(api.PtError):
        sc.update_vertices(bad)
    assert sc.has_motion == 1 and sc.generation == 1
    assert_bits_equal(sc.render_motion(cam, W, H), mv1, "after a refused update")
    sc.update_vertices(second["points"])
    mv2 = sc.render_motion(cam, W, H)
    assert_bits_equal(mv2, _want_motion(api, sc, cam, W, H, second["points"], first["points"], second["mesh"]), "against the first update's positions")
    assert not np.array_equal(mv2, _want_motion(api, sc, cam, W, H, second["points"], old["points"], second["mesh"]))
    sc.close()


# ---- (e), (f) the history stage -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def histories(api, hosts):
    """Three frames of history on the old geometry, then the update: per camera kind everything the last frame's accumulation reads."""
    hs = hosts["cornell"]
    out = {}
    for kind in ("identity", "pinhole"):
        cams = _cams(api, kind, W, H, 4)
        sc = api.Scene.from_mesh(hs)
        hist = ln = prev_n = prev_cam = None
        for t in range(3):
            S, Qs = sc.render_moments(cams[t], W, H, SPP, SPP // BATCHES, DEPTH, seed=20 + t)
            A, N = sc.render_aovs_centre(cams[t], W, H, 0)
            hist, ln = api.temporal_accumulate(cams[t], S, Qs, SPP, BATCHES, A, N, prev_cam, prev_n, hist, ln)
            prev_n, prev_cam = N, cams[t]
        sc.update_vertices(MC.moved_arrays(hs)["points"])
        cam = cams[3]
        S, Qs = sc.render_moments(cam, W, H, SPP, SPP // BATCHES, DEPTH, seed=23)
        A, N, mv = sc.render_motion(cam, W, H, guides=True)
        lo = api.scaled_camera(cam, 2)
        Sl, Ql = sc.render_moments(lo, W // 2, H // 2, SPP, SPP // BATCHES, DEPTH, seed=23)
        cur = api.upsample(2, Sl, Ql, SPP, BATCHES, *api.guide_subsample(2, A, N), A, N)
        out[kind] = dict(cam=cam, prev_cam=prev_cam, S=S, Q=Qs, A=A, N=N, prev_n=prev_n, hist=hist, ln=ln, motion=mv, cur=cur)
        sc.close()
    return out


@pytest.mark.parametrize("kind", ["identity", "pinhole"])
def test_accumulate_motion_is_the_restatement(api, gpu_ready, histories, kind):
    torch = gpu_ready
    c = histories[kind]
    if kind == "identity":
        assert c["cam"].tobytes() == c["prev_cam"].tobytes()
    moved = c["motion"][..., 3] == 1
    assert moved.sum() >= 16
    got = api.temporal_accumulate_motion(c["cam"], c["S"], c["Q"], SPP, BATCHES, c["A"], c["N"], c["prev_cam"], c["prev_n"], c["hist"], c["ln"],
                                         motion=c["motion"])
    want = M.accumulate(c["cam"], c["prev_cam"], c["S"], c["Q"], SPP, BATCHES, c["A"], c["N"], c["prev_n"], c["hist"], c["ln"], motion=c["motion"],
                        **T.DEFAULTS)
    print("%s: %d moved pixels, %d of them with history; fragile %d" % (kind, moved.sum(), (got[1][moved] > 1).sum(), want[2].sum()))
    assert_bits_equal(got[0], want[0], kind + ": hist"); assert_bits_equal(got[1], want[1], kind + ": hist_len")
    base = api.temporal_accumulate(c["cam"], c["S"], c["Q"], SPP, BATCHES, c["A"], c["N"], c["prev_cam"], c["prev_n"], c["hist"], c["ln"])
    none = api.temporal_accumulate_motion(c["cam"], c["S"], c["Q"], SPP, BATCHES, c["A"], c["N"], c["prev_cam"], c["prev_n"], c["hist"], c["ln"])
    assert_bits_equal(none[0], base[0], "motion None: hist"); assert_bits_equal(none[1], base[1], "motion None: hist_len")
    assert_bits_equal(got[0][~moved], base[0][~moved], "static pixels are the base function's")
    assert_bits_equal(got[1][~moved], base[1][~moved], "static pixels' lengths")
    assert not np.array_equal(got[1], base[1])
    first = api.temporal_accumulate_motion(c["cam"], c["S"], c["Q"], SPP, BATCHES, c["A"], c["N"], motion=c["motion"])
    assert_bits_equal(first[0], api.temporal_accumulate(c["cam"], c["S"], c["Q"], SPP, BATCHES, c["A"], c["N"])[0], "no history: motion is not read")
    # the _cur_ form, on pt_upsample's output at scale 2
    gc = api.temporal_accumulate_cur_motion(c["cam"], c["cur"], c["N"], c["prev_cam"], c["prev_n"], c["hist"], c["ln"], motion=c["motion"])
    wc = M.accumulate_cur(c["cam"], c["prev_cam"], c["cur"], c["N"], c["prev_n"], c["hist"], c["ln"], motion=c["motion"], **T.DEFAULTS)
    assert_bits_equal(gc[0], wc[0], kind + ": cur hist"); assert_bits_equal(gc[1], wc[1], kind + ": cur hist_len")
    bc = api.temporal_accumulate_cur(c["cam"], c["cur"], c["N"], c["prev_cam"], c["prev_n"], c["hist"], c["ln"])
    nc = api.temporal_accumulate_cur_motion(c["cam"], c["cur"], c["N"], c["prev_cam"], c["prev_n"], c["hist"], c["ln"])
    assert_bits_equal(nc[0], bc[0], "cur, motion None: hist"); assert_bits_equal(nc[1], bc[1], "cur, motion None: hist_len")
    # the device forms
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d = {k: dev(c[k]) for k in ("S", "Q", "A", "N", "prev_n", "hist", "ln", "motion", "cur")}
    oh, ol = torch.full((H, W, 4), 3.0, device="cuda:0"), torch.full((H, W), 3.0, device="cuda:0")
    api.temporal_accumulate_motion_device(W, H, c["cam"], c["prev_cam"], d["S"].data_ptr(), d["Q"].data_ptr(), SPP, BATCHES, d["A"].data_ptr(),
                                          d["N"].data_ptr(), d["prev_n"].data_ptr(), d["hist"].data_ptr(), d["ln"].data_ptr(),
                                          d["motion"].data_ptr(), oh.data_ptr(), ol.data_ptr())
    torch.cuda.synchronize()
    assert_bits_equal(oh.cpu().numpy(), got[0], "device hist"); assert_bits_equal(ol.cpu().numpy(), got[1], "device hist_len")
    api.temporal_accumulate_cur_motion_device(W, H, c["cam"], c["prev_cam"], d["cur"].data_ptr(), d["N"].data_ptr(), d["prev_n"].data_ptr(),
                                              d["hist"].data_ptr(), d["ln"].data_ptr(), d["motion"].data_ptr(), oh.data_ptr(), ol.data_ptr())
    torch.cuda.synchronize()
    assert_bits_equal(oh.cpu().numpy(), gc[0], "device cur hist"); assert_bits_equal(ol.cpu().numpy(), gc[1], "device cur hist_len")
    with pytest.raises(api.PtError, match="alias the motion"):
        api.temporal_accumulate_motion_device(W, H, c["cam"], c["prev_cam"], d["S"].data_ptr(), d["Q"].data_ptr(), SPP, BATCHES, d["A"].data_ptr(),
                                              d["N"].data_ptr(), d["prev_n"].data_ptr(), d["hist"].data_ptr(), d["ln"].data_ptr(),
                                              d["motion"].data_ptr(), d["motion"].data_ptr(), ol.data_ptr())


def test_rescued_pixels_keep_their_history(api, histories):
    """The pixels the CPU test counts (motion_ref.rescued, on the still camera): history with the motion buffer, none without."""
    c = histories["identity"]
    resc = M.rescued(c["cam"], c["N"], c["prev_n"], c["motion"])
    print("rescued pixels: %d" % resc.sum())
    assert resc.sum() >= 4
    with_m = api.temporal_accumulate_motion(c["cam"], c["S"], c["Q"], SPP, BATCHES, c["A"], c["N"], c["prev_cam"], c["prev_n"], c["hist"], c["ln"],
                                            motion=c["motion"])[1]
    without = api.temporal_accumulate(c["cam"], c["S"], c["Q"], SPP, BATCHES, c["A"], c["N"], c["prev_cam"], c["prev_n"], c["hist"], c["ln"])[1]
    assert (with_m[resc] > 1).all() and (without[resc] == 1).all()
