"""The HIP BSDF probes at edge directions and on material tables of their own.

Every case set of tests/bsdf_cases.py goes through pt_probe_bsdf_sample / pt_probe_bsdf_eval in one launch each and is held
  - to the CPU oracle bit for bit (a NaN equal to any NaN), with nothing left out, and
  - to the float64 restatement of the reference's formulas (tests/bsdf_ref.py) under its tolerance and exclusion rules, so that
    the kernels stay pinned to the formulas even if the oracle library were rebuilt wrongly.
The synthetic table is installed twice: at creation (Scene.from_arrays) and on a live scene by pt_scene_update_materials; the
probes must not tell the two apart. No scene carrying the synthetic table is rendered.
"""
import numpy as np
import pytest

import bsdf_cases as BC
import bsdf_ref as R
from util import assert_bits_equal_nan_class

pytestmark = pytest.mark.gpu

SETS = ["%s/eta_i=%g" % (t, e) for t in ("reference", "synthetic") for e in BC.ETA_I]


@pytest.fixture(scope="module")
def scenes(api, oracle, gpu_ready):
    table = BC.synthetic_table()[0]
    n = len(table) // 176
    live = api.Scene.from_arrays(BC.scene_arrays(oracle, BC.placeholder_table(n)))
    live.update_materials(table)
    return {"reference": (api.Scene(api.HostScene(BC.SCENES + "/mixed32.rendertron")), oracle.OracleScene(BC.SCENES + "/mixed32.rendertron")),
            "synthetic": (api.Scene.from_arrays(BC.scene_arrays(oracle, table)), oracle.OracleScene(arrays=BC.scene_arrays(oracle, table))),
            "live": (live, None)}


def test_the_reference_table_is_the_one_the_device_scene_carries(api, oracle, gpu_ready):
    assert np.array_equal(api.HostScene(BC.SCENES + "/mixed32.rendertron").array("materials"), BC.reference_table(oracle))


@pytest.mark.parametrize("kind", ["eval", "sample"])
@pytest.mark.parametrize("name", SETS)
def test_probes_at_edges(api, oracle, scenes, name, kind):
    cs = next(c for c in BC.all_sets(oracle) if c.name == name)
    gs, osc = scenes[cs.table_name]
    assert 0 <= cs.material.min() and cs.material.max() < len(cs.table) // 176      # the kernels index the table unchecked

    def probe(scene):
        if kind == "eval":
            return scene.bsdf_eval(cs.material, cs.wi, cs.wo, eta_i=cs.eta_i)
        return scene.bsdf_sample(cs.material, cs.wi, cs.backface, cs.subseq, eta_i=cs.eta_i)

    g = probe(gs)
    o = osc.bsdf_eval_n(cs.material, cs.wi, cs.wo, eta_i=cs.eta_i) if kind == "eval" else \
        osc.bsdf_sample_n(cs.material, cs.wi, cs.backface, cs.subseq, eta_i=cs.eta_i)
    assert_bits_equal_nan_class(g, o, "%s %s: probe against the oracle" % (name, kind))
    if cs.table_name == "synthetic":
        assert_bits_equal_nan_class(probe(scenes["live"][0]), g, "%s %s: table installed by pt_scene_update_materials" % (name, kind))
    got = BC.unpack_eval(g, cs.wo) if kind == "eval" else BC.unpack_sample(g)
    res = R.check(BC.restate(cs, kind), got, cs.exact, "%s %s (HIP probe)" % (name, kind), ref32=BC.restate(cs, kind, np.float32), cls=cs.cls)
    BC.assert_caps(res, name, kind)
