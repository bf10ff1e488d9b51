"""CPU only. The pair kernels' box table (pt_box_table.h: build_box_table): one record per distinct leaf box —
six floats equal as bit patterns — with the OR of the triangle ranges of the leaves that carry it. tests/box_table_driver.hip calls
the builders on trees written here as files (tests/box_table_cases.py), and every table is put to the same checks:

  * every leaf's range lies in exactly one record's mask, and the records' masks are disjoint;
  * their union is all the triangles;
  * the leaves behind a record have its box bit for bit, and no two records have bit-equal boxes;
  * a record's mask is exactly the union of those leaves' ranges;
  * grouping (group_box_table) keeps every record, its mask and its floats, rotated so that the grouped axis comes first;
  * every record of a group has the group's interval bit for bit, and no two groups have the same interval;
  * the chosen axis has the minimum number of distinct intervals (ties: the lowest axis).

Cases: the headline Cornell box (16 leaves, two of them with the whole-scene box: 15 records) and the mixed Cornell row (25 leaves,
23 records), as measured on the reference's tree for those scenes; a single leaf pair; all boxes distinct; duplicate leaves whose
ranges straddle triangles 31 / 32 (both mask words); a 64-triangle tree (the union is ~0, and no shift by 64 on the way); boxes that
differ only in the sign of a zero (bit patterns, not values, decide); a tree of more than 64 triangles (no box table, the leaf table
stays); and trees that fail boxes_nested_and_finite (a child larger than its parent, an infinite bound): no table at all.
The driver is built a second time with -fsanitize=address,undefined and run as a plain program on the same trees."""
import os

import numpy as np
import pytest

import box_table_cases as BT

MIXED = dict(tall_material=19, short_material=5, nested=True, extra_boxes=1, extra_materials=[4])      # bench.py's cornell_mixed


def _box(lo, hi):
    return (np.array(lo, np.float32), np.array(hi, np.float32))


def _synthetic():
    rng = np.random.default_rng(9)

    def rnd():
        lo = rng.random(3).astype(np.float32)
        return _box(lo, lo + rng.random(3).astype(np.float32) + np.float32(0.01))
    shared, whole = rnd(), _box([-1, -1, -1], [3, 3, 3])
    t = {}
    t["pair"] = BT.chain([rnd(), rnd()], [3, 2])
    t["pair_same_box"] = BT.chain([shared, shared], [1, 4])
    t["distinct"] = BT.chain([rnd() for _ in range(7)], [1, 2, 3, 4, 1, 2, 3])
    t["straddle"] = BT.chain([rnd(), shared, rnd(), shared, rnd()], [26, 4, 2, 4, 5])          # the shared box: bits 26..29 and 32..35
    t["straddle_adjacent"] = BT.chain([rnd(), shared, shared, rnd()], [29, 3, 3, 6])             # ... bits 29..31 and 32..34
    t["tri64"] = BT.chain([whole, rnd(), whole, rnd(), rnd()], [20, 12, 20, 11, 1])
    t["tri64_one_box"] = BT.chain([whole, whole], [63, 1])                                       # one record, mask ~0
    t["zero_signs"] = BT.chain([_box([0.0, 0, 0], [1, 1, 1]), _box([-0.0, 0, 0], [1, 1, 1]), _box([0.0, 0, 0], [1, 1, 1])], [2, 2, 2])
    t["tri65"] = BT.chain([rnd() for _ in range(5)], [13] * 5)
    loose, n = BT.chain([rnd() for _ in range(4)], [2, 2, 2, 2])
    loose[1]["lmax"][1] = loose[0]["rmax"][1] + np.float32(0.5)                                  # a child's box reaches out of its parent's
    t["not_nested"] = (loose, n)
    inf, n = BT.chain([rnd() for _ in range(3)], [2, 2, 2])
    inf[0]["lmax"][0] = np.inf
    t["not_finite"] = (inf, n)
    return t


@pytest.fixture(scope="module")
def trees(api, scene_dir):
    """The synthetic trees and the two Cornell scenes' own (the host loader builds the reference's tree; no GPU)."""
    from cudapathtracer_amd import scenes
    t = _synthetic()
    for name, kw in (("cornell", {}), ("cornell_mixed", MIXED)):
        # (the room's width follows the image's aspect: the benchmark's scenes are the 1920x1080 ones)
        cfg = scenes.cornell(os.path.join(scene_dir, "boxes_" + name), 1920, 1080, 1024, 8, name="boxes_" + name, **kw)["config"]
        t[name] = BT.pnodes_from_bvh(api.HostScene(cfg).array("bvh"))
    return t


@pytest.fixture(scope="module")
def tables(trees, tmp_path_factory):
    d = tmp_path_factory.mktemp("box_table")
    return BT.run_driver(BT.build_driver(d), d, trees)


def _range(first, count):
    return ((1 << count) - 1) << first


def check_table(r, n_tris):
    """The properties every box table must have, from the leaf table printed beside it."""
    leaves, boxes = r["leaves"], r["boxes"]
    assert sum(c for _, c, _ in leaves) == n_tris and sorted(f for f, _, _ in leaves)[0] == 0
    union = 0
    for m, _ in boxes:
        assert m != 0 and m >> 64 == 0 and union & m == 0, "masks are disjoint"
        union |= m
    assert union == (1 << n_tris) - 1, "the union is all triangles"
    assert len({b for _, b in boxes}) == len(boxes), "no two records have bit-equal boxes"
    want = {}
    for f, c, b in leaves:
        inside = [k for k, (m, _) in enumerate(boxes) if m & _range(f, c)]
        assert len(inside) == 1 and boxes[inside[0]][0] & _range(f, c) == _range(f, c), "a leaf's range lies in exactly one record's mask"
        assert boxes[inside[0]][1] == b, "the leaves behind a record have its box bit for bit"
        want[b] = want.get(b, 0) | _range(f, c)
    assert {b: m for m, b in boxes} == want
    assert [b for _, b in boxes] == list(dict.fromkeys(b for _, _, b in leaves)), "records in the order their box first appears"
    if not boxes:
        return
    # the groups
    ax, recs, groups = r["axis"], r["records"], r["groups"]
    intervals = [len({(b[a], b[3 + a]) for _, b in boxes}) for a in range(3)]
    assert len(groups) == min(intervals) and ax == intervals.index(min(intervals)), (ax, intervals)
    unrot = lambda b: tuple(b[3 * h + (a - ax) % 3] for h in (0, 1) for a in range(3))      # record floats {g, u, v} back to {x, y, z}
    assert sorted((m, unrot(b)) for m, b in recs) == sorted(boxes), "grouping keeps every record and its mask"
    assert sum(c for c, _, _ in groups) == len(recs) and all(c >= 1 for c, _, _ in groups)
    assert len({(lo, hi) for _, lo, hi in groups}) == len(groups), "no two groups share an interval"
    k = 0
    for c, lo, hi in groups:
        assert all((b[0], b[3]) == (lo, hi) for _, b in recs[k:k + c]), "every record of a group has the group's interval bit for bit"
        k += c


@pytest.mark.parametrize("name", ["pair", "pair_same_box", "distinct", "straddle", "straddle_adjacent", "tri64", "tri64_one_box", "zero_signs",
                                  "cornell", "cornell_mixed"])
def test_every_table_partitions_the_triangles_by_distinct_box(trees, tables, name):
    r = tables[name]
    assert r["nested"] == 1 and r["n_leaves"] == len(trees[name][0]) + 1
    check_table(r, trees[name][1])


def test_the_cases_are_what_they_are_meant_to_be(trees, tables):
    n = {k: (r["n_leaves"], r["n_boxes"]) for k, r in tables.items()}
    print(n)
    assert n["cornell"] == (16, 15) and trees["cornell"][1] == 36                  # triangles 8..11 and 24..26 carry the whole-scene box
    m = [m for m, _ in tables["cornell"]["boxes"] if bin(m).count("1") == 7]
    assert m == [_range(8, 4) | _range(24, 3)], [hex(x) for x, _ in tables["cornell"]["boxes"]]
    assert n["cornell_mixed"] == (25, 23)
    c, mx = tables["cornell"], tables["cornell_mixed"]
    assert c["axis"] == 1 and sorted(g[0] for g in c["groups"]) == [2, 2, 3, 3, 5]          # y: 5 intervals (z has 8, x 12)
    assert [len({(b[a], b[3 + a]) for _, b in c["boxes"]}) for a in range(3)] == [12, 5, 8]
    assert mx["axis"] == 1 and len(mx["groups"]) == 9
    assert tables["distinct"]["n_groups"] == 7 and tables["pair_same_box"]["n_groups"] == 1        # no sharing: a group per record
    assert n["pair"] == (2, 2) and n["pair_same_box"] == (2, 1) and n["distinct"] == (7, 7) and n["zero_signs"] == (3, 2)
    assert n["straddle"] == (5, 4) and _range(26, 4) | _range(32, 4) in [m for m, _ in tables["straddle"]["boxes"]]
    assert n["straddle_adjacent"] == (4, 3) and _range(29, 6) in [m for m, _ in tables["straddle_adjacent"]["boxes"]]
    assert trees["tri64"][1] == 64 and n["tri64"] == (5, 4) and any(m >> 63 for m, _ in tables["tri64"]["boxes"])
    assert [m for m, _ in tables["tri64_one_box"]["boxes"]] == [(1 << 64) - 1]
    for k in ("straddle", "straddle_adjacent", "tri64"):                             # a record with bits in both mask words
        assert any(m & 0xffffffff and m >> 32 for m, _ in tables[k]["boxes"]), k


def test_the_scenes_of_the_gpu_test_are_what_they_are_there_for(api, scene_dir, tmp_path_factory):
    """tests/test_pair_boxes.py's fuzz seeds and its scene without a shell, through the same driver and the same checks."""
    d = tmp_path_factory.mktemp("box_table_fuzz")
    t = {"fuzz%d" % s: BT.pnodes_from_bvh(api.HostScene(BT.fuzz_config(scene_dir, s)).array("bvh")) for s in BT.FUZZ}
    t["open_floor"] = BT.pnodes_from_bvh(api.HostScene(BT.open_floor(scene_dir)).array("bvh"))
    r = BT.run_driver(BT.build_driver(d), d, t)
    for k in t:
        check_table(r[k], t[k][1])
    assert {s: (r["fuzz%d" % s]["n_leaves"], r["fuzz%d" % s]["n_boxes"]) for s in BT.FUZZ} == {s: v[:2] for s, v in BT.FUZZ.items()}
    assert (r["open_floor"]["n_leaves"], r["open_floor"]["n_boxes"]) == (14, 14) and t["open_floor"][1] == 28      # no duplicate box
    assert (r["open_floor"]["axis"], sorted(g[0] for g in r["open_floor"]["groups"])) == (0, [1, 1, 1, 2, 2, 3, 4])
    # every axis is some scene's grouped one, and there are groups of one record and of more than two
    assert {s: (r["fuzz%d" % s]["axis"], sorted(g[0] for g in r["fuzz%d" % s]["groups"])) for s in BT.FUZZ} == BT.FUZZ_GROUPS
    assert {a for a, _ in BT.FUZZ_GROUPS.values()} == {0, 1, 2}
    shared = lambda k: [m for m, b in r[k]["boxes"] if sum(1 for _, _, lb in r[k]["leaves"] if lb == b) > 1]
    assert any(m & 0xffffffff and m >> 32 for m in shared("fuzz3")) and len([m for m in shared("fuzz86") if m & 0xffffffff and m >> 32]) == 2
    assert t["fuzz110"][1] == 63 and any(m >> 62 for m, _ in r["fuzz110"]["boxes"])
    assert r["fuzz3"]["n_boxes"] % 2 == 0 and r["fuzz6"]["n_boxes"] % 2 == 1


def test_no_box_table_beyond_64_triangles_and_no_table_for_a_loose_tree(trees, tables):
    r = tables["tri65"]
    assert trees["tri65"][1] == 65 and r["nested"] == 1 and (r["n_leaves"], r["n_boxes"]) == (5, 0)      # the leaf table stays (128-bit masks)
    for k in ("not_nested", "not_finite"):
        assert (tables[k]["nested"], tables[k]["n_leaves"], tables[k]["n_boxes"]) == (0, 0, 0), k


def test_the_driver_runs_clean_under_address_and_undefined_behaviour_sanitizers(trees, tables, tmp_path_factory):
    d = tmp_path_factory.mktemp("box_table_san")
    assert BT.run_driver(BT.build_driver(d, sanitize=True), d, trees) == tables
