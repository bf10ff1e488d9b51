"""Build-time pins on the pair kernels' leaf loop after the empty mask word left it, read from the gfx950
assembly as tools/pair_census.py reads it (leaf_record_path: the loop's blocks by the compiler's own annotations, walked from the
header through every fall-through to the back edge).

A record's 64-bit triangle mask arrives as two SGPRs. The parent folded both dwords into both rays' sets for every record: two
v_mov_b32 out of the SGPRs, four v_cndmask_b32, four v_or_b32. Now a ray's hit is an all-ones / zero VGPR (one v_cndmask_b32 per ray)
and a word's fold one v_and_or_b32 per ray with the SGPR as its operand; and the high dword, non-zero only for records that cover
triangles 32..63, is folded in a block of its own behind a scalar compare of that SGPR with 0 and a scalar branch. The loop steps a
32-bit byte offset (the s_load's SGPR offset): an add and a compare where a counter beside a 64-bit pointer was three adds and a compare.

Per record, headline (megakernel_flat2<0, true, false>) and LEAN (megakernel_flat2<0, false, true>) alike:
                 always executed: total / VALU / scalar / branches / s_nop     v_mov  v_cndmask  v_or  v_and_or    skipped block
    parent       47 / 40 / 5 / 1 / 0                                            2      4          4     0           -
    this work    44 / 34 / 4 / 2 / 3                                            0      2          0     2           8 (4 VALU and a copy of the loop tail)
Whole kernels 3610 / 5692 -> 3611 / 5693 instructions (bounds 3655 / 5746, tests/test_isa_logic_moves.py); bounce-loop moves
162 -> 159 and 284 -> 281 (profiles/r11_pair_census_before.txt, profiles/r11_pair_census_after.txt)."""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import pair_census as PC  # noqa: E402

PARENT_VALU, BOUND_VALU = 40, 35


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    asm = PC.compile_asm(str(tmp_path_factory.mktemp("mask_words") / "pt_mk_lds.s"))
    return {k: PC.leaf_record_path(PC.function(asm, name)) for k, name in PC.KERNELS.items()}


@pytest.mark.parametrize("kernel", sorted(PC.KERNELS))
def test_a_record_with_an_empty_high_word_issues_at_most_35_vector_instructions(paths, kernel):
    p = paths[kernel]
    print(kernel, p)
    assert p["always"]["valu"] <= BOUND_VALU < PARENT_VALU, p["always"]
    assert p["always"]["total"] <= 47, p["always"]                  # (the parent's whole loop: the compare and the branch cost less than they save)
    # one word's fold on the always-executed path, the other word's in the block a record without it skips
    assert p["v_cndmask"] <= 2 and p["v_or"] + p["v_and_or"] <= 2 and p["v_mov"] <= 1, p
    assert 0 < p["skipped"]["valu"] <= 5, p["skipped"]


@pytest.mark.parametrize("kernel", sorted(PC.KERNELS))
def test_the_skip_is_a_scalar_compare_and_a_scalar_branch_on_the_mask_dword(paths, kernel):
    p = paths[kernel]
    assert len(p["mask_branches"]) >= 1, p
    for cmp_, br in p["mask_branches"]:
        assert re.match(r"s_cmp_(eq|lg)_u32 s\d+, 0$", cmp_) and re.match(r"s_cbranch_scc[01] \.LBB", br), (cmp_, br)


@pytest.mark.parametrize("kernel", sorted(PC.KERNELS))
def test_no_exec_mask_split_and_no_readlane_in_the_leaf_loop(paths, kernel):
    p = paths[kernel]
    assert p["exec_splits"] == 0 and p["v_readlane"] == 0, p
    assert p["always"]["v_readlane"] == 0 and p["skipped"]["v_readlane"] == 0
