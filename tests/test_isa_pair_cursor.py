"""Build-time pins on the pair pass's cursor (pt_trace.h: trace_pair_flat, BOUND and ONEB) in the gfx950
code of both timed pair kernels, read as tools/pair_census.py reads it. The trips know no range bound and a slot's second minimum
lies 1024 bytes behind its first, so the block that moves a lane to its next slot is two ds_read_b128 and two adds: the parent's
trip loop was 87 (headline) and 88 (LEAN) instructions with 8 LDS instructions, its set-up 229. What the committed code measures
is profiles/r08_pair_census_after.txt."""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import pair_census as PC  # noqa: E402

TRIP_TOTAL = {"c2": 83, "mixed": 84}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return PC.compile_asm(str(tmp_path_factory.mktemp("pair_cursor") / "pt_mk_lds.s"))


def _trip_lines(lines):
    """The trip loop's lines, found as tools/pair_census.py: regions finds it."""
    lp = PC.loops(lines)
    trip = [(h, e) for h, e in lp if all(any(op in lines[k] for k in range(h, e + 1)) for op in ("ds_min_u64", "v_ffbl_b32"))]
    th, te = min(trip, key=lambda x: x[1] - x[0])
    return lines[th:te + 1]


@pytest.mark.parametrize("kernel", sorted(PC.KERNELS))
def test_the_trip_loop_moves_to_the_next_slot_with_two_registers(asm, kernel):
    lines = PC.function(asm, PC.KERNELS[kernel])
    t = PC.regions(lines)["trip_loop"]
    print(kernel, "trip loop:", t)
    assert t["total"] <= TRIP_TOTAL[kernel] and t["lds"] <= 7, t
    assert t["ds_min_u64"] == 2 and t["s_waitcnt"] <= 4 and t["branch"] <= 5 and t["inner_back_edges"] == 0, t
    mins = [ln.split(";")[0].split() for ln in _trip_lines(lines) if ln.strip().startswith("ds_min_u64")]
    addr = [m[1].rstrip(",") for m in mins]
    print(kernel, "minima:", [" ".join(m) for m in mins])
    assert len(addr) == 2 and addr[0] == addr[1] and re.fullmatch(r"v\d+", addr[0]), mins      # one address register ...
    offs = sorted(int(re.search(r"offset:(\d+)", " ".join(m)).group(1)) if "offset:" in " ".join(m) else 0 for m in mins)
    assert offs[1] - offs[0] == 1024, mins                                                         # ... the second minimum 1024 bytes on


def test_the_headline_kernel_as_a_whole(asm):
    lines = PC.function(asm, PC.KERNELS["c2"])
    r, md, whole = PC.regions(lines), PC.metadata(asm, PC.KERNELS["c2"]), PC.census(lines)
    count = lambda op: sum(1 for ln in lines if PC.is_insn(ln) and ln.strip().startswith(op))      # noqa: E731
    sqrt, div = count("v_sqrt_f32"), count("v_div_scale_f32")
    print("headline: set-up %d, leaf loop %d, whole %d, v_sqrt_f32 %d, v_div_scale_f32 %d, %s" % (r["setup"]["total"], r["leaf_loop"]["total"], whole["total"], sqrt, div, md))
    assert r["setup"]["total"] <= 226, r["setup"]
    assert whole["total"] < 3783
    assert sqrt == 8 and div == 60
    assert md["vgpr_count"] <= 128 and md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
