"""Build-time pins on the logic step of the headline kernel (megakernel_flat2<0, true, false>) after its duplicate arms were merged
(pt_megakernel.h: the ARMS switch), read from the gfx950 assembly as tools/pair_census.py reads it, and the machine
code of every kernel the change must not touch.

The parent's headline kernel: 3879 static instructions, 11 v_sqrt_f32, 70 v_div_scale_f32. Steps 1 to 4 are kept. Step 5 (the dead
`o` arm of the SIMPLE bounce) is NOT: eight static instructions less, and 0.3 % slower in both A/B forms
(profiles/r07_ab_logic_arms.log), so nothing here pins its "at least 6 fewer". Steps 2, 3 and 4 each drop one normalise, so one
v_sqrt_f32 each: 11 -> 8. v_div_scale_f32 comes in pairs, one pair per IEEE division, and a normalise holds one too — the division
behind rcp_exact's wave-uniform range test — which the estimate of 66 did not count: step 2 drops one division (70 -> 68), step 3
one normalise and the two divisions of the emitter arm (-> 62), step 4 one normalise (-> 60). Total with steps 1 to 4: 3783."""
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


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return PC.compile_asm(str(tmp_path_factory.mktemp("arms") / "pt_mk_lds.s"))


def _count(lines, op):
    return sum(1 for ln in lines if PC.is_insn(ln) and ln.strip().startswith(op))


def test_the_headline_kernel_lost_three_normalises_and_the_emitter_arms_divisions(asm):
    lines = PC.function(asm, PC.KERNELS["c2"])
    total = PC.census(lines)["total"]
    sqrt, div = _count(lines, "v_sqrt_f32"), _count(lines, "v_div_scale_f32")
    print("headline: total %d, v_sqrt_f32 %d, v_div_scale_f32 %d" % (total, sqrt, div))
    assert sqrt == 8
    assert div <= 66 and div == 60
    assert total < 3879 and total <= 3783


def test_the_pair_kernels_keep_their_registers(asm):
    md = PC.metadata(asm, PC.KERNELS["c2"])
    assert md["vgpr_count"] <= 128 and md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
    md = PC.metadata(asm, PC.KERNELS["mixed"])        # the LEAN pair kernel has the switch too: its pin (tests/test_isa.py) holds
    assert md["vgpr_count"] <= 128 and md["private_segment_fixed_size"] <= 52, md


def test_the_pair_pass_regions_are_what_they_were(asm):
    """The bounds of tests/test_isa_pair_pass.py and tests/test_isa_pair_slots.py's set-up, on the same regions."""
    for k, name in PC.KERNELS.items():
        r = PC.regions(PC.function(asm, name))
        assert r["leaf_loop"]["total"] <= 122 and r["leaf_loop"]["v_readlane"] == 0, (k, r["leaf_loop"])
        if k == "c2":
            assert r["setup"]["total"] <= 230 and r["setup"]["lds"] <= 18, r["setup"]
        t = r["trip_loop"]
        assert t["total"] <= 88 and t["salu"] <= 10 and t["branch"] <= 5 and t["lds"] <= 8 and t["s_waitcnt"] <= 4, (k, t)
        assert t["inner_back_edges"] == 0 and t["exec_splits"] == 0 and t["ds_min_u64"] == 2, (k, t)


def test_every_other_kernel_keeps_its_machine_code(api):
    """tests/golden/logic_arms_parent_hashes.json: tools/roofline.py: kernel_code_hashes of the parent commit's library. Only the two
    timed pair kernels and their moments twins may differ from it."""
    with open(os.path.join(GOLDEN, "logic_arms_parent_hashes.json")) as f:
        parent = json.load(f)["hashes"]
    now = RF.kernel_code_hashes(api.LIB_PATH)
    assert len(parent) >= 30 and set(now) == set(parent)
    differ = {k for k in parent if now[k] != parent[k]}
    assert differ <= CHANGED, sorted(differ - CHANGED)
    assert differ == CHANGED, sorted(CHANGED - differ)       # (and the switch is on where it should be)
