"""Option "moments_fused" and pt_last_moments_launches without a device: the option's name and range as pt_set_option /
pt_get_option see them, and the accessor as declared, exported and bound. What the option renders: tests/test_moments_fused.py."""
import os
import re

from conftest import ROOT


def _err(api):
    return api.lib().pt_last_error().decode(errors="replace")


def test_the_option_is_known_with_values_0_and_1(api):
    L = api.lib()
    # the name and the value are checked before the scene: with a NULL scene an accepted pair gets as far as the scene check
    for v in (0, 1):
        assert L.pt_set_option(None, b"moments_fused", v) == -1 and "null scene" in _err(api), (v, _err(api))
    for v in (2, -1):
        assert L.pt_set_option(None, b"moments_fused", v) == -1 and "moments_fused = %d is outside [0, 1]" % v in _err(api), (v, _err(api))
    assert L.pt_set_option(None, b"moments_fuse", 1) == -1 and "unknown option" in _err(api)
    assert L.pt_get_option(None, b"moments_fused", None) == -1 and "null argument" in _err(api), _err(api)
    assert L.pt_get_option(None, b"moments_fuse", None) == -1 and "unknown option" in _err(api)
    # ... and for an option that was there before, the same order
    assert L.pt_set_option(None, b"flat", 3) == -1 and "outside" in _err(api)
    assert L.pt_set_option(None, b"flat", 1) == -1 and "null scene" in _err(api)


def test_the_accessor_is_declared_exported_and_bound(api):
    header = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    assert re.search(r"^int pt_last_moments_launches\(pt_scene\* scene\);", header, flags=re.M)
    assert '"moments_fused" 0|1' in header
    fn = api.lib().pt_last_moments_launches                      # AttributeError if the library does not export it
    assert fn.argtypes is not None and len(fn.argtypes) == 1
    assert callable(getattr(api.Scene, "last_moments_launches"))


def test_a_null_scene_has_made_no_launches(api):
    assert api.lib().pt_last_moments_launches(None) == -1


def test_the_table_keeps_its_25_names_and_has_no_positions():
    """Every option is one row of kOptions that says where its value lives; pt_set_option / pt_get_option look the row up by name
    and never by position, so a new row may go anywhere."""
    src = open(os.path.join(ROOT, "cudapathtracer_amd", "csrc", "pt_api.hip")).read()
    table = re.search(r"const Option kOptions\[\] = \{(.*?)\n\};", src, flags=re.S).group(1)
    names = re.findall(r'\{"(\w+)", -?\d', table)
    assert sorted(names) == sorted(["flat", "onchip", "waves_hbm", "refill", "refill_keep", "node_keep", "tri_keep", "defer_shadow", "slice_iters", "slice_always",
                                    "sched_mask", "lpt_prio", "persistent", "xcd_bands", "culling", "spec", "simple", "flat2", "leaf_boxes", "wide", "compact",
                                    "wf_wide_wg", "lean", "queue_timeout_ms", "moments_fused"]), names
    for fn in ("pt_set_option", "pt_get_option"):
        body = re.search(r"^int %s\(.*?^}" % fn, src, flags=re.S | re.M).group(0)
        assert "switch" not in body and not re.search(r"\b(k|i) == \d", body) and not re.search(r"kOptions\[\d", body), body
