"""Build-time pins on the pair pass's slot records (pt_trace.h: trace_pair_flat) in the gfx950 code of both FLAT pair kernels.
A slot is one 32-byte record read by two ds_read_b128 plus its bound, and the trip's `t > 0 && t < max_t` is one unsigned
compare. What tools/pair_census.py reports for the committed code is
profiles/r05_pair_census_after.txt; the limits below are what the change was measured with."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import pair_census as PC  # noqa: E402


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    text = PC.compile_asm(str(tmp_path_factory.mktemp("pair_slots") / "pt_mk_lds.s"))
    return {k: (PC.metadata(text, name), PC.regions(PC.function(text, name))) for k, name in PC.KERNELS.items()}


def test_trip_loop_fetches_a_slot_in_three_reads(census):
    """Three LDS reads for the next slot and three for the triangle (8 LDS instructions with the two ds_min_u64; 10 before), at
    most four waits (8 before), and the loop no longer than 88 instructions (96 before)."""
    for k, (_, r) in census.items():
        t = r["trip_loop"]
        assert t["lds"] <= 8 and t["ds_min_u64"] == 2, (k, t)
        assert t["s_waitcnt"] <= 4, (k, t)
        assert t["total"] <= 88 and t["salu"] <= 10 and t["branch"] <= 5, (k, t)


def test_headline_setup_writes_slots_wide(census):
    """The headline's set-up writes each slot with two ds_write_b128 and two ds_write_b32 (ten ds_write_b32 before): at most 230
    static instructions (250 before), and no scratch."""
    md, r = census["c2"]
    assert r["setup"]["total"] <= 230 and r["setup"]["lds"] <= 18, r["setup"]
    assert md.get("private_segment_fixed_size") == 0 and md.get("vgpr_spill_count") == 0, md
