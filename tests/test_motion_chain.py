"""The motion pass through mirrors and glass (pt_render_motion_chain) on the GPU against its numpy restatement
(tests/motion_chain_ref.py), bit for bit: the restatement reads the library's own closest hits, link by link (pt_probe_centre_rays +
pt_probe_trace_closest), so what is compared is the choice of pixels, the unfolding, the virtual image and the previous point. The
inputs are tests/motion_chain_cases.py's, which tests/test_motion_chain_ref_cpu.py checks without a GPU. The floors are conditions on
the input (the oracle's counts stand next to them), not tolerances."""
import os

import numpy as np
import pytest

import aov_chain_ref as AC
import motion_cases as MC
import motion_chain_cases as CC
import motion_ref as M
import temporal_ref as T
from test_temporal import _cams
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

SPP, BATCHES, DEPTH = 4, 2, 4
W, H = CC.W, CC.H
N_BLOB = 10 * 4 ** 3 + 2                                     # the vertices of a subdiv-3 icosphere: the scene's last


@pytest.fixture(scope="module")
def cases(api, gpu_ready, scene_dir):
    """name -> (host scene, camera, old arrays, new arrays, floors by max_links on the pixels seen through a chain)."""
    from cudapathtracer_amd import scenes
    out = {}
    for name, (w, h), floors in (("a", (W, H), {1: 12, 2: 12, 8: 12}), ("ragged", (37, 21), {1: 4, 2: 4, 8: 4})):      # oracle: 18; 6
        hs = CC.scene_a(api, scene_dir, "mchain_" + name, w, h)
        out[name] = (hs, _cams(api, "identity", w, h, 1)[0], MC.arrays(hs), CC.moved_box(hs), floors)
    # glass tall box, mirror short box, the diffuse back wall behind them moved: refraction chains, and total internal reflection
    hs = MC.cornell_host(api, scene_dir, "mchain_glass")
    new = MC.arrays(hs)
    wall = CC.back_wall_vertices(new)
    assert len(wall) == 4
    new["points"].view(np.float32).reshape(-1, 4)[wall, :3] += np.array((0.05, 0.0, -0.1), np.float32)
    out["glass"] = (hs, hs.camera(), MC.arrays(hs), new, {1: 3, 2: 16, 8: 20})                                         # oracle: 5, 26, 33
    # test_aov's blob (subdiv 3 at 40 x 24), with a mirror back wall, seen from the side so that the blob does not hide its own image
    cfg = scenes.blob_in_box(os.path.join(scene_dir, "mchain_blob3"), 40, 24, 1, 4, subdiv=3, name="mchain_blob3", back_material=CC.MIRROR)["config"]
    hs = api.HostScene(cfg)
    n = hs.info["n_points"]
    out["blob"] = (hs, api.make_camera(True, (1.2, 0.5, 0.2), (-15.0, 35.0, 0.0), 60.0, 40, 24), MC.arrays(hs),
                   MC.moved_arrays(hs, n - N_BLOB, n, (0.1, 0.0, 0.05)), {1: 10, 2: 10, 8: 10})                        # oracle: 19
    return out


def _want(api, sc, hs, cam, w, h, max_links, new, old):
    return CC.want_motion(sc, AC.Materials(hs), CC.library_centre_rays(api, cam, w, h), max_links, new, old, w, h)


# ---- the pass against the restatement, and its guide outputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_links", [1, 2, 8])
@pytest.mark.parametrize("name", ["a", "ragged", "glass", "blob"])
def test_motion_chain_is_the_restatement_and_the_guides_are_the_centre_pass(api, cases, name, max_links):
    hs, cam, old, new, floors = cases[name]
    w, h = cam.w, cam.h
    sc = api.Scene.from_mesh(hs)
    if name == "blob":
        assert not sc.flags()["onchip"]                      # a scene in HBM
    sc.update_vertices(new["points"])
    assert sc.has_motion == 1
    A, N, mv, ln = sc.render_motion_chain(cam, w, h, max_links, guides=True, links=True)
    want = _want(api, sc, hs, cam, w, h, max_links, new, old)
    through = (want["links"] >= 1) & (want["motion"][..., 3] == 1)
    refl, refr, tir = (through & (want["reflections"] > 0)).sum(), (through & (want["reflections"] == 0)).sum(), (through & want["tir"]).sum()
    print("%s, max_links %d: %d pixels moved, %d seen through a chain (%d with a reflection, %d refracted only, %d with a total internal "
          "reflection); links up to %d" % (name, max_links, (want["motion"][..., 3] == 1).sum(), through.sum(), refl, refr, tir, want["links"].max()))
    assert through.sum() >= floors[max_links] and (want["motion"][..., 3] == 0).sum() >= 16
    if name == "glass" and max_links >= 2:
        assert refr >= 12 and refl >= 3                      # oracle: 21 and 5 (12 at max_links 8)
    if name == "glass" and max_links == 8:
        assert tir >= 1 and want["links"].max() >= 3         # oracle: 7, and chains of 4 links
    assert_bits_equal(mv, want["motion"], "%s %d: motion" % (name, max_links))
    assert np.array_equal(ln, want["links"].astype(np.float32))
    assert_bits_equal(sc.render_motion_chain(cam, w, h, max_links), mv, "motion without the guide outputs")
    ca, cn, cl = sc.render_aovs_centre(cam, w, h, max_links, links=True)
    assert_bits_equal(A, ca, "albedo"); assert_bits_equal(N, cn, "normal_depth"); assert_bits_equal(ln, cl, "links")
    first = sc.render_motion(cam, w, h)
    assert not first[through].any()                          # what the first-hit pass says there: static
    assert_bits_equal(mv[want["links"] == 0], first[want["links"] == 0], "the pixels without a link")
    sc.close()


@pytest.mark.parametrize("name", ["a", "glass"])
def test_no_links_is_render_motion_in_every_output(api, cases, name):
    hs, cam, old, new, _ = cases[name]
    w, h = cam.w, cam.h
    sc = api.Scene.from_mesh(hs)
    sc.update_vertices(new["points"])
    A, N, mv, ln = sc.render_motion_chain(cam, w, h, 0, guides=True, links=True)
    fa, fn, fm = sc.render_motion(cam, w, h, guides=True)
    assert (fm[..., 3] == 1).sum() >= 16
    assert_bits_equal(mv, fm, "motion"); assert_bits_equal(A, fa, "albedo"); assert_bits_equal(N, fn, "normal_depth")
    assert not ln.any()
    assert_bits_equal(sc.render_motion_chain(cam, w, h, 0), fm, "motion alone")
    sc.close()


def test_device_form_is_the_host_form(api, gpu_ready, cases):
    torch = gpu_ready
    hs, cam, old, new, _ = cases["ragged"]
    w, h = 37, 21
    sc = api.Scene.from_mesh(hs)
    sc.update_vertices(new["points"])
    A, N, mv, ln = sc.render_motion_chain(cam, w, h, 2, guides=True, links=True)
    d = [torch.full((h, w, 4), 3.0, device="cuda:0") for _ in range(6)]
    dl = torch.full((h, w), 3.0, device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sc.render_motion_chain_device(cam, w, h, 2, d[0].data_ptr(), d[1].data_ptr(), dl.data_ptr(), d[2].data_ptr(), stream=s.cuda_stream)
        sc.render_motion_chain_device(cam, w, h, 2, d[3].data_ptr(), d[4].data_ptr(), 0, d[5].data_ptr(), stream=s.cuda_stream)
        sc.render_motion_chain_device(cam, w, h, 2, 0, 0, 0, d[0].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    for got, want, what in zip(d[1:], (N, mv, A, N, mv), ("normal_depth", "motion", "albedo, no links", "normal_depth, no links", "motion, no links")):
        assert_bits_equal(got.cpu().numpy(), want, what)
    assert_bits_equal(d[0].cpu().numpy(), mv, "motion alone")
    assert_bits_equal(dl.cpu().numpy(), ln, "links")
    sc.close()


# ---- all-zero cases, a refused update, two updates in a row ----------------------------------------------------------------------------
def test_static_scenes_a_refused_update_and_a_second_update(api, cases):
    hs, cam, old, first, _ = cases["a"]
    second = CC.moved_box(hs, shift=(0.35, 0.05, 0.2))
    fresh = api.Scene.from_mesh(hs)
    assert fresh.has_motion == 0 and not fresh.render_motion_chain(cam, W, H, 2).any()
    caller = api.Scene(hs)                                   # the caller's own tree: it keeps no positions at all
    A, N, mv = caller.render_motion_chain(cam, W, H, 2, guides=True)
    ca, cn = caller.render_aovs_centre(cam, W, H, 2)
    assert not mv.any()
    assert_bits_equal(A, ca, "albedo"); assert_bits_equal(N, cn, "normal_depth")
    caller.close()
    bad = MC.arrays(hs)["points"].copy()
    bad.view(np.float32)[4 * 50] = np.nan
    with pytest.raises(api.PtError):
        fresh.update_vertices(bad)
    assert fresh.has_motion == 0 and not fresh.render_motion_chain(cam, W, H, 2).any()
    fresh.update_vertices(first["points"])
    mv1 = fresh.render_motion_chain(cam, W, H, 2)
    assert_bits_equal(mv1, _want(api, fresh, hs, cam, W, H, 2, first, old)["motion"], "after the first update")
    with pytest.raises(api.PtError):
        fresh.update_vertices(bad)
    assert fresh.has_motion == 1
    assert_bits_equal(fresh.render_motion_chain(cam, W, H, 2), mv1, "after a refused update")
    fresh.update_vertices(second["points"])
    mv2 = fresh.render_motion_chain(cam, W, H, 2)
    assert_bits_equal(mv2, _want(api, fresh, hs, cam, W, H, 2, second, first)["motion"], "against the first update's positions")
    assert not np.array_equal(mv2, _want(api, fresh, hs, cam, W, H, 2, second, old)["motion"])
    fresh.update_vertices(second["points"])                  # the positions it already has
    assert fresh.has_motion == 1 and not fresh.render_motion_chain(cam, W, H, 2).any()
    fresh.update_mesh(second, hs.info["leaf_size"])          # the topology may have changed: the previous positions are dropped
    assert fresh.has_motion == 0 and not fresh.render_motion_chain(cam, W, H, 2).any()
    fresh.close()


def test_a_moving_mirror_zeroes_what_is_seen_through_it(api, cases):
    hs, cam, old, _, _ = cases["a"]
    both = CC.moved_box(hs)
    both["points"].view(np.float32).reshape(-1, 4)[CC.back_wall_vertices(old), 2] -= np.float32(0.05)
    sc = api.Scene.from_mesh(hs)
    sc.update_vertices(both["points"])
    mv, ln = sc.render_motion_chain(cam, W, H, 2, guides=True, links=True)[2:]
    assert (ln >= 1).sum() > 100 and not mv[ln >= 1].any() and (mv[ln == 0][:, 3] == 1).sum() >= 16
    assert_bits_equal(mv, _want(api, sc, hs, cam, W, H, 2, both, old)["motion"], "motion")
    sc.close()


# ---- the history stage fed this buffer --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def histories(api, cases):
    """Three frames of history with chain guides on the old geometry, then the update: what the last frame's accumulation reads."""
    hs, _, old, new, _ = cases["a"]
    out = {}
    for kind in ("identity", "pinhole"):
        cams = _cams(api, kind, W, H, 4)
        sc = api.Scene.from_mesh(hs)
        hist = ln = prev_n = prev_cam = None
        for t in range(3):
            S, Qs = sc.render_moments(cams[t], W, H, SPP, SPP // BATCHES, DEPTH, seed=20 + t)
            A, N = sc.render_aovs_centre(cams[t], W, H, 2)
            hist, ln = api.temporal_accumulate(cams[t], S, Qs, SPP, BATCHES, A, N, prev_cam, prev_n, hist, ln)
            prev_n, prev_cam = N, cams[t]
        sc.update_vertices(new["points"])
        cam = cams[3]
        S, Qs = sc.render_moments(cam, W, H, SPP, SPP // BATCHES, DEPTH, seed=23)
        A, N, mv, links = sc.render_motion_chain(cam, W, H, 2, guides=True, links=True)
        out[kind] = dict(cam=cam, prev_cam=prev_cam, S=S, Q=Qs, A=A, N=N, prev_n=prev_n, hist=hist, ln=ln, motion=mv, links=links,
                         first=sc.render_motion(cam, W, H))
        sc.close()
    return out


@pytest.mark.parametrize("kind", ["identity", "pinhole"])
def test_accumulate_takes_the_buffer_as_the_restatement_does(api, histories, kind):
    c = histories[kind]
    through = (c["links"] >= 1) & (c["motion"][..., 3] == 1)
    assert through.sum() >= (12 if kind == "identity" else 6)
    args = (c["cam"], c["S"], c["Q"], SPP, BATCHES, c["A"], c["N"], c["prev_cam"], c["prev_n"], c["hist"], c["ln"])
    got = api.temporal_accumulate_motion(*args, motion=c["motion"])
    want = M.accumulate(c["cam"], c["prev_cam"], c["S"], c["Q"], SPP, BATCHES, c["A"], c["N"], c["prev_n"], c["hist"], c["ln"], motion=c["motion"],
                        **T.DEFAULTS)
    fh = api.temporal_accumulate_motion(*args, motion=c["first"])
    print("%s: %d pixels through the mirror; with history: chain %d, first hit %d; fragile %d" % (
        kind, through.sum(), (got[1][through] > 1).sum(), (fh[1][through] > 1).sum(), want[2].sum()))
    assert_bits_equal(got[0], want[0], kind + ": hist"); assert_bits_equal(got[1], want[1], kind + ": hist_len")
    static = c["motion"][..., 3] != 1
    base = api.temporal_accumulate(*args)
    assert_bits_equal(got[0][static], base[0][static], "static pixels are the base function's")
    assert_bits_equal(got[1][static], base[1][static], "static pixels' lengths")
    assert kind != "identity" or (got[1][through] > 1).sum() >= 6


def test_pixels_seen_through_the_mirror_keep_their_history(api, histories):
    """The pixels the CPU test counts (motion_ref.rescued on the chain guides, still camera): history with this buffer, none with the
    first-hit pass's, none without a buffer."""
    c = histories["identity"]
    resc = M.rescued(c["cam"], c["N"], c["prev_n"], c["motion"]) & (c["links"] >= 1)
    print("rescued pixels seen through the mirror: %d" % resc.sum())
    assert resc.sum() >= 6                                   # oracle: 12
    args = (c["cam"], c["S"], c["Q"], SPP, BATCHES, c["A"], c["N"], c["prev_cam"], c["prev_n"], c["hist"], c["ln"])
    with_m = api.temporal_accumulate_motion(*args, motion=c["motion"])[1]
    first = api.temporal_accumulate_motion(*args, motion=c["first"])[1]
    without = api.temporal_accumulate(*args)[1]
    assert (with_m[resc] > 1).all() and (first[resc] == 1).all() and (without[resc] == 1).all()
