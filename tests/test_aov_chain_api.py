"""pt_render_aovs_chain and pt_preview_set_guide_chain without a GPU: the C ABI's argument checks (they fire before any HIP
call), and the numpy reference itself (tests/aov_chain_ref.py) against geometry it does not compute with: a mirror wall's
virtual image, a hand-built pair of facing mirrors, and the classes of ray the GPU cases must hold."""
import ctypes
import os

import numpy as np
import pytest

import aov_chain_cases as K
import aov_chain_ref as R

NEW_SYMBOLS = ("pt_render_aovs_chain", "pt_render_aovs_chain_device", "pt_preview_set_guide_chain", "pt_preview_guide_chain")


def _err(api):
    return api.lib().pt_last_error().decode()


def _cam(api, w=16, h=8):
    return api.make_camera(True, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 45.0, w, h)


def test_new_symbols_are_exported(api):
    L = api.lib()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    assert all(hasattr(api.Scene, n) for n in ("render_aovs_chain", "render_aovs_chain_device"))
    assert all(hasattr(api.Preview, n) for n in ("set_guide_chain", "guide_chain"))


def test_render_aovs_chain_argument_checks(api):
    L = api.lib()
    buf = np.zeros((8, 16, 4), np.float32)
    links = np.zeros((8, 16), np.float32)
    cam = _cam(api)
    c = ctypes.byref(cam)
    p, q = buf.ctypes.data, links.ctypes.data
    cases = [
        ((None, c, 0, 8, 1, 4, 1, p, p, q), "size"),
        ((None, c, 16, -1, 1, 4, 1, p, p, q), "size"),
        ((None, c, 16, 8, 0, 4, 1, p, p, q), "aov_spp"),
        ((None, c, 16, 8, 1, -1, 1, p, p, q), "max_links -1 must be 0..16"),
        ((None, c, 16, 8, 1, 17, 1, p, p, q), "max_links 17 must be 0..16"),
        ((None, None, 16, 8, 1, 4, 1, p, p, q), "null camera"),
        ((None, c, 16, 9, 1, 4, 1, p, p, q), "camera is 16 x 8"),                     # a size mismatch
        ((None, ctypes.byref(_cam(api, 17, 8)), 16, 8, 1, 4, 1, p, p, q), "camera is 17 x 8"),
        ((None, c, 16, 8, 1, 4, 1, None, p, q), "null output"),
        ((None, c, 16, 8, 1, 4, 1, p, None, q), "null output"),
        # everything else in order, links given or NULL: the scene is what is refused, so a NULL out_links was accepted
        ((None, c, 16, 8, 1, 0, 1, p, p, q), "null scene"),
        ((None, c, 16, 8, 1, 16, 1, p, p, None), "null scene"),
    ]
    for args, msg in cases:
        assert L.pt_render_aovs_chain(*args) == -1, args
        assert msg in _err(api), (args, _err(api))
        assert L.pt_render_aovs_chain_device(*args, None) == -1, args
        assert msg in _err(api), (args, _err(api))


def test_guide_chain_setter_refuses_a_null_session(api):
    L = api.lib()
    assert L.pt_preview_set_guide_chain(None, 4) == -1 and "pt_preview_set_guide_chain: null session" in _err(api)
    assert L.pt_preview_guide_chain(None) == -1 and "pt_preview_guide_chain: null session" in _err(api)


# ---- the reference against geometry ---------------------------------------------------------------------------------------

MIRROR_CAM = (True, (0.6, 0.3, 0.2), (-10.0, 25.0, 0.0), 60.0)          # looks at the mirror wall from the right, slightly down


def test_a_mirror_wall_shows_the_virtual_image(oracle, scene_dir):
    """One link in a planar mirror: the chain's depth is the distance a camera mirrored in the wall's plane sees along the
    mirrored ray in the box WITHOUT that wall. Both are sums of the same two segments up to f32 rounding of a few ulp per
    link and the two 1e-5 offsets, at distances of 1..4: 1e-4 relative."""
    from cudapathtracer_amd import scenes
    O = oracle
    w = h = 32
    mirror = O.OracleScene(scenes.cornell(os.path.join(scene_dir, "chain_mw"), width=w, height=h, name="chain_mw", back_material=19)["config"])
    open_box = O.OracleScene(scenes.cornell(os.path.join(scene_dir, "chain_ow"), width=w, height=h, name="chain_ow", back_material=0)["config"])
    pinhole, pos, rot, fov = MIRROR_CAM
    cam = O.make_camera(pinhole, pos, rot, fov, w, h)
    rays = R.camera_rays(O, cam, w, h, K.SEED)
    mats = R.Materials(mirror)
    r = R.chain_rays(mirror, mats, rays, 8)
    oi, of, _ = mirror.trace_closest(rays)
    on_wall = r["first_spec"] & (mats.type[np.maximum(oi[:, 2], 0)] == R.MAT_MIRROR)
    ok = on_wall & (r["links"] == 1)
    assert on_wall.sum() >= 100 and ok.sum() * 4 >= on_wall.sum(), (int(on_wall.sum()), int(ok.sum()))
    zb = float(of[on_wall, 5].mean())                        # the wall's plane z = zb (its hit points)
    assert np.abs(of[on_wall, 5] - zb).max() < 1e-5 and np.all(of[on_wall, 6:9] == (0.0, 0.0, 1.0))
    m = rays[ok].astype(np.float64)
    m[:, 2] = 2.0 * zb - m[:, 2]; m[:, 5] = -m[:, 5]         # the camera and its rays mirrored in z = zb
    ui, uf, _ = open_box.trace_closest(m.astype(np.float32))
    assert np.all(ui[:, 0] == 1)
    np.testing.assert_allclose(r["depth"][ok], uf[:, 0], rtol=1e-4, atol=0)
    np.testing.assert_allclose(r["normal"][ok], uf[:, 6:9], rtol=0, atol=1e-6)     # (the mirrored ray IS the reflected ray's line: the same surface)
    assert np.array_equal(r["albedo"][ok], R.Materials(open_box).albedo[ui[:, 2]])
    assert np.all(r["depth"][ok] > of[ok, 0])


def _facing_mirrors(scene_dir):
    """Two mirrors z = -1 and z = +1 facing each other over a diffuse floor y = -1."""
    from cudapathtracer_amd import scenes
    a = scenes.Mesh("mirror_a", 19); a.quad((-5, -1, -1), (5, -1, -1), (5, 5, -1), (-5, 5, -1), (0, 0, 1))
    b = scenes.Mesh("mirror_b", 19); b.quad((5, -1, 1), (-5, -1, 1), (-5, 5, 1), (5, 5, 1), (0, 0, -1))
    floor = scenes.Mesh("floor", 2); floor.quad((-5, -1, 1), (5, -1, 1), (5, -1, -1), (-5, -1, -1), (0, 1, 0))
    return scenes._emit(os.path.join(scene_dir, "chain_two_mirrors"), "chain_two_mirrors", [a, b, floor], 8, 8, 1, 4)["config"]


def test_two_facing_mirrors_fall_back_after_max_links(oracle, scene_dir):
    osc = oracle.OracleScene(_facing_mirrors(scene_dir))
    mats = R.Materials(osc)
    down = np.array([0.0, -0.25, -1.0]) / np.sqrt(1.0625)
    rays = np.array([[0, 0, 0, 0, 0, -1], [0, 0, 0, *down], [0, 0, 0, 0, 1, 0]], np.float32)   # for ever | floor after 2 links | a miss
    first = R.chain_rays(osc, mats, rays, 0)
    assert list(first["valid"]) == [True, True, False] and list(first["links"]) == [0, 0, 0]
    assert first["out"][0] and first["out"][1]               # max_links 0: a specular first hit is out of links at once
    np.testing.assert_allclose(first["depth"][:2], [1.0, np.sqrt(1.0625)], rtol=1e-6)
    for max_links in (1, 2, 4, 16):
        r = R.chain_rays(osc, mats, rays, max_links)
        # the perpendicular ray never leaves the mirrors: its first hit, links 0, whatever the cap
        assert r["out"][0] and r["links"][0] == 0 and not r["left"][0]
        for key in ("albedo", "normal", "depth"):
            assert np.array_equal(r[key][0], first[key][0])
        assert np.array_equal(r["normal"][0], (0.0, 0.0, 1.0)) and np.array_equal(r["albedo"][0], mats.albedo[19])
        if max_links < 2:                                    # the tilted one: out of links, so its first hit too
            assert r["out"][1] and r["links"][1] == 0
            for key in ("albedo", "normal", "depth"):
                assert np.array_equal(r[key][1], first[key][1])
        else:                                                # ... or the floor after A, B: four unit crossings of the gap
            assert not r["out"][1] and r["links"][1] == 2
            assert np.array_equal(r["albedo"][1], mats.albedo[2])
            np.testing.assert_allclose(r["normal"][1], (0.0, 1.0, 0.0), atol=1e-6)
            np.testing.assert_allclose(r["depth"][1], 4.0 * np.sqrt(1.0625), rtol=1e-4)
        assert not r["valid"][2]


def test_the_gpu_cases_hold_every_class_of_ray(api, oracle, scene_dir):
    """What test_aov_chain.py asserts again from the same reference on the GPU machine: chosen here, where no GPU is needed."""
    total = {}
    for name in K.CASES:
        cfg, cam, w, h, aov_spp, max_links = K.case(api, name, scene_dir)
        _, _, links, per_k = R.chain_aovs(oracle, oracle.OracleScene(cfg), cam, w, h, aov_spp, max_links, K.SEED)
        for k, v in R.classes(per_k).items():
            total[k] = total.get(k, 0) + v
        assert links.max() <= max_links
    assert all(v > 0 for v in total.values()), total


def test_python_wrapper_refuses_what_the_library_refuses(api):
    cam = _cam(api)
    sc = api.Scene.__new__(api.Scene)                        # no device scene: the checks fire before it is looked at
    sc.h = None
    with pytest.raises(api.PtError, match="max_links 17"):
        sc.render_aovs_chain(cam, 16, 8, 17)
    with pytest.raises(api.PtError, match="null scene"):
        sc.render_aovs_chain(cam, 16, 8, 4, links=True)


def test_the_chain_kernel_fits_the_occupancy_its_launch_assumes():
    """aov_chain_blocks launches 6 workgroups per CU: 6 waves per SIMD need at most 80 VGPRs, 6 workgroups at most 160 KB / 6 of
    LDS each, and a kernel that spills would pay for the registers in scratch traffic. The first-hit kernel keeps its own budget."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import denoise_time
    res = denoise_time.aov_kernel_resources()
    chain, first = res["aov_chain_kernel"], res["aov_kernel"]
    print(res)
    assert chain["vgpr_count"] <= 80 and chain["vgpr_spill_count"] == 0 and chain["private_segment_fixed_size"] == 0, chain
    assert 6 * chain["group_segment_fixed_size"] <= 160 * 1024, chain
    assert first["vgpr_count"] <= 80 and first["private_segment_fixed_size"] == 0 and first["group_segment_fixed_size"] == 16384, first
