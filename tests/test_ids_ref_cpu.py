"""The numpy restatement of the ID pass and of the selection overlay (tests/ids_ref.py), checked without a GPU on the input the GPU
tests reuse (tests/ids_cases.py): the hits are the CPU oracle's along the centre rays, link by link. The floors are conditions on the
INPUT, not tolerances.

Counts of the restatement at 40 x 24 (miss, light, backface, behind glass, in a mirror, chain left the scene, chain capped):
  cornell          max_links 0: 63 5 0 0 0 0 0     1: 63 5 0 0 16 21 32      4: 63 5 0 32 24 21 0
  cornell_outside  max_links 0: 776 0 36 0 0 0 0   1: 776 0 36 0 12 2 10     4: 776 0 36 10 12 2 0
  glass_mirror     max_links 0: 160 8 0 0 0 0 0    1: 160 8 0 0 11 19 41     4: 160 8 0 40 18 20 0"""
import numpy as np
import pytest

import aov_chain_ref as AC
import ids_cases as IC
import ids_ref as IR

W, H = IC.W, IC.H
# the classes every GPU comparison relies on, and a floor for each in the case that is there to hold it
FLOORS = {("cornell", 0): {"miss": 16, "light": 3}, ("cornell_outside", 0): {"miss": 16, "backface": 16},
          ("cornell", 1): {"in_mirror": 8, "left": 8, "capped": 16}, ("cornell", 4): {"behind_glass": 16, "in_mirror": 8, "left": 8},
          ("glass_mirror", 1): {"capped": 16, "left": 8}, ("glass_mirror", 4): {"behind_glass": 16, "in_mirror": 8, "light": 3, "miss": 16}}


@pytest.fixture(scope="module")
def cases(api, oracle, scene_dir):
    out = {}
    for name, (scene, _) in IC.CAMERAS.items():
        hs = IC.host(api, scene_dir, scene, "ids_cpu_" + scene)
        a = IC.host_arrays(hs)
        osc = oracle.OracleScene(arrays=a)
        out[name] = {"osc": osc, "mats": AC.Materials(osc), "rays": IC.oracle_centre_rays(oracle, IC.camera(api, hs, name), W, H),
                     "lights": IR.light_of_triangle(api, a), "arrays": a}
    return out


def _ids(c, max_links):
    return IR.ids_chain(c["osc"], c["mats"], c["rays"], max_links, c["lights"])


@pytest.mark.parametrize("name", list(IC.CAMERAS))
def test_no_links_is_the_oracles_closest_hit(cases, name):
    c = cases[name]
    r = _ids(c, 0)
    oi, of, _ = c["osc"].trace_closest(c["rays"])
    hit = oi[:, 0] == 1
    assert hit.sum() >= 100 and (~hit).sum() >= 16
    assert np.array_equal(r["ids"][hit, 0], oi[hit, 1]) and np.array_equal(r["ids"][hit, 1], oi[hit, 2])
    assert np.array_equal(r["ids"][hit, 3], (oi[hit, 3] != 0).astype(np.int32))            # no links: the info word is the backface bit
    assert np.array_equal(r["ids"][~hit], np.tile(np.array(IR.MISS, np.int32), ((~hit).sum(), 1))) and not r["hit"][~hit].any()
    assert np.array_equal(r["hit"][hit, :3].view(np.uint32), of[hit, 3:6].view(np.uint32))
    assert np.array_equal(r["hit"][hit, 3].view(np.uint32), of[hit, 0].view(np.uint32))
    # the light word: exactly the triangles of the light quad, by the scene's own light list
    lit = r["ids"][:, 2] >= 0
    assert np.array_equal(lit, hit & (c["lights"][np.maximum(r["ids"][:, 0], 0)] >= 0))
    n_lights = c["arrays"]["lights"].size // 80
    assert n_lights >= 1 and set(np.unique(c["lights"])) == set(range(-1, n_lights))


@pytest.mark.parametrize("max_links", [1, 4])
@pytest.mark.parametrize("name", list(IC.CAMERAS))
def test_a_chain_reports_the_surface_the_guides_hold(cases, name, max_links):
    """The reported material's albedo is aov_chain_ref's albedo (the materials are untextured), the depth its depth, the links its."""
    c = cases[name]
    r = _ids(c, max_links)
    g = AC.chain_rays(c["osc"], c["mats"], c["rays"], max_links)
    v = g["valid"]
    assert np.array_equal(v, r["valid"])
    assert not c["mats"].has_tex[r["ids"][v, 1]].any()          # (the table has textured rows; no triangle of these scenes uses one)
    assert np.array_equal(c["mats"].albedo[r["ids"][v, 1]].view(np.uint32), g["albedo"][v].view(np.uint32))
    assert np.array_equal(r["hit"][v, 3].view(np.uint32), g["depth"][v].view(np.uint32))
    assert np.array_equal(r["ids"][v, 3] >> 8, g["links"][v]) and np.array_equal(r["left"], g["left"])
    assert np.array_equal(r["capped"], g["out"])
    # a chain that left the scene or was capped reports its FIRST hit, with no links
    zero = _ids(c, 0)
    fb = r["left"] | r["capped"]
    assert np.array_equal(r["ids"][fb], zero["ids"][fb]) and np.array_equal(r["hit"][fb].view(np.uint32), zero["hit"][fb].view(np.uint32))
    assert c["mats"].in_chain[r["ids"][fb, 1]].all()           # ... which is the mirror or the glass itself
    direct = v & ~r["first_spec"]
    assert np.array_equal(r["ids"][direct], zero["ids"][direct])
    done = v & ~fb
    assert not c["mats"].in_chain[r["ids"][done, 1]].any()      # every other chain ends on a non-specular surface


def test_the_cameras_hold_every_class(cases):
    got = {(name, ml): IR.classes(_ids(cases[name], ml)) for name in IC.CAMERAS for ml in IC.LINKS}
    for k, v in got.items():
        print(k, v)
    for k, floors in FLOORS.items():
        for cls, floor in floors.items():
            assert got[k][cls] >= floor, (k, cls, got[k])
    for cls in ("miss", "light", "backface", "behind_glass", "in_mirror", "left", "capped"):
        assert any(v[cls] > 0 for v in got.values()), cls


# ---- the overlay ------------------------------------------------------------------------------------------------------------------------
def _frame(h, w, seed=5):
    rng = np.random.default_rng(seed)
    rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    ids = np.zeros((h, w, 4), np.int32)
    return ids, rgba


def test_overlay_identities():
    ids, rgba = _frame(11, 13)
    ids[..., 0] = 7
    assert np.array_equal(IR.overlay(ids, rgba, []), rgba)
    assert np.array_equal(IR.overlay(ids, rgba, [(0, 8, 9, (255, 0, 0, 255), 2, 128), (2, 1, 1, (1, 2, 3, 4), 1, 5)]), rgba)
    miss = np.tile(np.array(IR.MISS, np.int32), (11, 13, 1))
    for comp in range(3):                                       # a miss is in no range: lo >= 0
        assert np.array_equal(IR.overlay(miss, rgba, [(comp, 0, 2 ** 31 - 1, (9, 9, 9, 255), 4, 255)]), rgba)


def test_a_mask_over_the_whole_image_is_fill_only():
    ids, rgba = _frame(11, 13)
    for radius in (1, 4):
        out = IR.overlay(ids, rgba, [(1, 0, 0, (200, 100, 50, 255), radius, 0)])          # fill alpha 0: nothing may change
        assert np.array_equal(out, rgba)
        out = IR.overlay(ids, rgba, [(1, 0, 0, (200, 100, 50, 7), radius, 255)])          # fill alpha 255: the colour everywhere
        assert (out[..., :3] == np.array((200, 100, 50), np.uint8)).all() and np.array_equal(out[..., 3], rgba[..., 3])


def test_one_pixel_is_all_outline_and_the_blend_rounds_to_nearest():
    ids, rgba = _frame(11, 13)
    ids[5, 6, 0] = 3
    out = IR.overlay(ids, rgba, [(0, 3, 3, (10, 250, 99, 77), 1, 255)])
    want = rgba.copy()
    for c, col in enumerate((10, 250, 99)):
        want[5, 6, c] = (int(rgba[5, 6, c]) * (255 - 77) + col * 77 + 127) // 255
    assert np.array_equal(out, want) and not np.array_equal(out, rgba)
    # a selection touching the frame has no outline along it: a 3 x 3 block in the corner keeps (0, 0) as fill at radius 1
    ids, rgba = _frame(11, 13)
    ids[:3, :3, 2] = 1
    out = IR.overlay(ids, rgba, [(2, 1, 1, (255, 255, 255, 255), 1, 0)])
    assert np.array_equal(out[:2, :2], rgba[:2, :2]) and (out[2, :3, :3] == 255).all() and (out[:3, 2, :3] == 255).all()
    assert np.array_equal(out[3:], rgba[3:]) and np.array_equal(out[:, 3:], rgba[:, 3:])
