"""Build-time pins on the leaf stage of the pair pass (pt_trace.h: trace_pair_flat under ARMS) in the gfx950
code of both timed pair kernels, read with tools/pair_census.py. The stage runs over the table of distinct boxes (pt_box_table.h):
an outer loop per group of records that share their interval on one axis, which computes that axis once per ray, and an inner loop
per record — what the census takes as the leaf loop: the innermost loop in front of the trip loop that reads an eight-dword record —
which computes the other two axes and takes the record's triangle mask as it comes.

                              parent (two leaves per trip)          now (one record per trip)
  leaf loop, total            122                                   47
  leaf loop, VALU             108                                   40
  leaf loop, SALU             12: two s_load_dwordx8, and per       5: one s_load_dwordx8, the counter, the pointer's two
                              leaf s_bfm_b64 / s_lshl_b64 for       halves, the compare
                              the mask from (first, count)
  64-bit scalar shifts in it  4                                     0
  a group's own part          -                                     33 (16 VALU: the shared axis of both rays; 15 SALU)
  whole kernel                3724 (headline) / 5791 (LEAN)         3655 / 5746

Per pass the headline scene has 15 records in 5 groups where it had 16 leaves: 15 x 47 + 5 x 33 = 870 against 8 x 122 = 976. The other pins on
these kernels (tests/test_isa_logic_arms.py, tests/test_isa_pair_pass.py, tests/test_isa_pair_slots.py,
tests/test_isa_pair_cursor.py) hold unchanged."""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import pair_census as PC  # noqa: E402

WHOLE = {"c2": 3655, "mixed": 5746}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    text = PC.compile_asm(str(tmp_path_factory.mktemp("pair_boxes") / "pt_mk_lds.s"))
    return {k: PC.function(text, name) for k, name in PC.KERNELS.items()}


def _leaf_loop(lines):
    """The lines of what tools/pair_census.py takes as the leaf loop (its own rule, restated on its own loop finder)."""
    lp = PC.loops(lines)
    trip = [(h, e) for h, e in lp if all(any(op in lines[k] for k in range(h, e + 1)) for op in ("ds_min_u64", "v_ffbl_b32"))]
    th, _ = min(trip, key=lambda x: x[1] - x[0])
    leaf = [(h, e) for h, e in lp if e < th and any("s_load_dwordx8" in lines[k] for k in range(h, e + 1))]
    assert leaf, "no loop in front of the trip loop reads an eight-dword record"
    lh, le = min(leaf, key=lambda x: x[1] - x[0])
    return lines[lh:le + 1]


def test_the_leaf_loop_takes_its_masks_from_the_records(kernels):
    for k, lines in kernels.items():
        loop = _leaf_loop(lines)
        c = PC.census(loop)
        assert c == PC.regions(lines)["leaf_loop"], k
        print(k, c)
        assert c["salu"] <= 5 and c["total"] <= 47 and c["valu"] <= 40 and c["s_waitcnt"] <= 1 and c["v_readlane"] == 0, (k, c)
        assert sum(1 for ln in loop if "s_load_dwordx8" in ln) == 1 and sum(1 for ln in loop if PC.is_insn(ln) and ln.strip().startswith("s_load")) == 1, k
        shifts = [ln.strip() for ln in loop if PC.is_insn(ln) and re.match(r"s_(lshl|lshr|ashr|bfm|bfe)_[bui]64", ln.strip())]
        assert not shifts, (k, shifts)


def test_the_whole_kernels_are_no_longer_than_measured(kernels):
    for k, lines in kernels.items():
        total = PC.census(lines)["total"]
        print(k, total)
        assert total <= WHOLE[k], (k, total)
