"""Build-time pins on the register moves of the pair kernels' bounce loop, read from the gfx950 assembly as
tools/pair_census.py reads it: v_mov_b32 / v_mov_b64 by source in the loop that holds one logic step and one pair pass, the runs of
constant fills in its logic step, and the machine code of every kernel the change must not touch.

The parent's bounce loops (profiles/r10_pair_census_before.txt), from_vgpr / from_const / total:
    headline (megakernel_flat2<0, true, false>)   105 /  79 / 207
    LEAN     (megakernel_flat2<0, false, true>)   182 / 132 / 339
This work reaches (profiles/r10_pair_census_after.txt):
    headline                                      102 /  37 / 162
    LEAN                                          179 /  80 / 284
The fills that went were of values only one arm of a split defines (pt_path.h: s2l, A, B, Cc in bounce_core; path_bounce's NeeRecord)."""
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import pair_census as PC  # noqa: E402
import roofline as RF  # noqa: E402

CHANGED = {"pt::megakernel_flat2<0, true, false>", "pt::megakernel_flat2<0, false, true>",
           "pt::megakernel_flat2_moments<0, true, false>", "pt::megakernel_flat2_moments<0, false, true>"}
PARENT = {"c2": dict(from_vgpr=105, from_const=79, v_mov=207), "mixed": dict(from_vgpr=182, from_const=132, v_mov=339)}
REACHED = {"c2": dict(from_vgpr=102, from_const=37, v_mov=162), "mixed": dict(from_vgpr=179, from_const=80, v_mov=284)}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return PC.compile_asm(str(tmp_path_factory.mktemp("moves") / "pt_mk_lds.s"))


@pytest.fixture(scope="module")
def moves(asm):
    return {k: PC.move_regions(PC.function(asm, name)) for k, name in PC.KERNELS.items()}


@pytest.mark.parametrize("kernel", sorted(PC.KERNELS))
def test_the_bounce_loop_issues_fewer_moves(moves, kernel):
    m = moves[kernel]["bounce_loop"]
    print(kernel, {k: m[k] for k in ("total", "valu", "v_mov", "from_vgpr", "from_const", "from_sgpr", "runs")})
    assert m["from_vgpr"] + m["from_const"] + m["from_sgpr"] == m["v_mov"]
    for k, bound in REACHED[kernel].items():
        assert m[k] <= bound <= PARENT[kernel][k], (kernel, k, m[k], bound)
    assert m["from_const"] < PARENT[kernel]["from_const"] and m["v_mov"] < PARENT[kernel]["v_mov"]


@pytest.mark.parametrize("kernel", sorted(PC.KERNELS))
def test_no_run_of_zero_fills_is_left_in_the_logic_step(moves, kernel):
    """The parent had one run of ten `v_mov_b32 vN, 0` per bounce arm (the fresh NeeRecord) and nine more in front of the merged light
    pdf (s2l, A, B, Cc). None of four or more is kept."""
    m = moves[kernel]["logic"]
    assert m["zero_fill_runs"] == [] and m["const_runs"] == [], (kernel, m["run_list"])
    # Nor four in a row inside a longer run of moves (the parent had 10 in both kernels), with one exception kept on purpose: the six
    # zeros with which the LEAN kernel's regeneration loop starts a new path (path_begin: depth, guard, prevPoint, woLocal; inside its
    # run of 15 moves). depth and guard are read by every lane of the new path; prevPoint indeterminate compiled to the same code
    # (DESIGN.md §6 round 10, step 3b): the compiler picks the 0 itself. The headline, which has no live woLocal, has three.
    assert m["longest_zero_fill"] <= {"c2": 3, "mixed": 6}[kernel], (kernel, m["longest_zero_fill"])


def test_registers_scratch_and_the_pair_pass_are_within_their_bounds(asm):
    """tests/test_isa_pair_boxes.py's totals, tests/test_isa_logic_arms.py's registers and regions, tests/test_isa.py's private segment of
    the LEAN kernel (28 B at the parent: a form that costs it scratch is not taken)."""
    for k, name in PC.KERNELS.items():
        lines = PC.function(asm, name)
        md, total, r = PC.metadata(asm, name), PC.census(lines)["total"], PC.regions(lines)
        print(k, md, total)
        if k == "c2":
            assert total <= 3655 and md["vgpr_count"] <= 128 and md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, (md, total)
            assert r["setup"]["total"] <= 230 and r["setup"]["lds"] <= 18, r["setup"]
        else:
            assert total <= 5746 and md["vgpr_count"] <= 128 and md["private_segment_fixed_size"] <= 28, (md, total)
        assert r["leaf_loop"]["total"] <= 122 and r["leaf_loop"]["v_readlane"] == 0, (k, r["leaf_loop"])
        t = r["trip_loop"]
        assert t["total"] <= 88 and t["salu"] <= 10 and t["branch"] <= 5 and t["lds"] <= 8 and t["s_waitcnt"] <= 4, (k, t)
        assert t["inner_back_edges"] == 0 and t["exec_splits"] == 0 and t["ds_min_u64"] == 2, (k, t)


def test_only_the_four_pair_kernels_differ_from_the_parent(api):
    """tests/golden/logic_moves_parent_hashes.json: tools/roofline.py: kernel_code_hashes of the parent commit's library."""
    with open(os.path.join(GOLDEN, "logic_moves_parent_hashes.json")) as f:
        parent = json.load(f)["hashes"]
    now = RF.kernel_code_hashes(api.LIB_PATH)
    assert len(parent) >= 30 and set(now) == set(parent)
    differ = {k for k in parent if now[k] != parent[k]}
    assert differ <= CHANGED, sorted(differ - CHANGED)
    assert differ == CHANGED, sorted(CHANGED - differ)
