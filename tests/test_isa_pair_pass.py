"""Build-time pins on the pair pass (pt_trace.h: trace_pair_flat) in the gfx950 code of both FLAT pair kernels — the C2
headline (megakernel_flat2<0, true, false>) and the mixed Cornell row (<0, false, true>). The headline runs at the CU's
instruction-issue ceiling, and the trip loop (one dealt ray-triangle test per trip, ~20 trips per wave and bounce) is
where a few instructions more per trip show up as a slower frame. tools/pair_census.py finds the
regions in the code; what it reports for the committed code is profiles/r04_pair_census_after.txt."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import pair_census as PC  # noqa: E402


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    text = PC.compile_asm(str(tmp_path_factory.mktemp("pair") / "pt_mk_lds.s"))
    return {k: PC.regions(PC.function(text, name)) for k, name in PC.KERNELS.items()}


def test_trip_loop_is_one_straight_pass_per_test(census):
    """No loop inside the trip loop (the next ray with tests is always the next slot: one conditional fetch, no search), no
    exec-mask split of the hit update (an extension ray's and a shadow ray's hit take the same two ds_min_u64), and the static
    length of the loop no longer than it was measured with (100 before the change)."""
    for k, r in census.items():
        t = r["trip_loop"]
        assert t["inner_back_edges"] == 0, (k, t)
        assert t["exec_splits"] == 0, (k, t)
        assert t["ds_min_u64"] == 2, (k, t)
        assert t["total"] <= 96 and t["salu"] <= 11 and t["branch"] <= 5, (k, t)


def test_the_leaf_loop_is_untouched(census):
    """The lockstep leaf loop (unrolled twice) stays as lean as round 3 left it."""
    for k, r in census.items():
        assert r["leaf_loop"]["total"] <= 122 and r["leaf_loop"]["v_readlane"] == 0, (k, r["leaf_loop"])
