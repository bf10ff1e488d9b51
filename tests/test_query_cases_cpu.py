"""The ray sets of the query tests (tests/query_cases.py) hold every class of result the GPU comparisons rely on, checked on the CPU
oracle alone. The floors are conditions on the INPUT, not tolerances: tests/test_query.py leaves no ray out of any comparison, so a
class that is missing here would go untested there.

Every set: closest hits, misses, hits seen from the back, hits on a light; shadow rays that are occluded and that are clear. A
partially attenuated shadow ray (0 < throughput < 1) needs a leaf material, which only scenes.textured() has: its set holds them.

Counts at the seeds of query_cases (hit, miss, backface, light, occluded, clear, partial):
  cornell          644 353 106 9 314 683 0
  cornell_outside  455 542 130 5 241 756 0
  glass_mirror     597 400 101 8 296 701 0
  textured         631 366 109 8 321 666 10   (9 of the 10 lie in (0, 1); one, along an unnormalised direction, exceeds 1)"""
import numpy as np
import pytest

import query_cases as QC

FLOOR = {"hit": 100, "miss": 50, "backface": 20, "light": 5, "occluded": 50, "clear": 50}


@pytest.fixture(scope="module")
def sets(api, oracle, scene_dir):
    out = {}
    for name in QC.SCENES:
        hs = QC.host(api, scene_dir, name, "query_cpu_")
        a = QC.arrays(hs)
        osc = oracle.OracleScene(arrays=a)
        rays = QC.ray_set(oracle, QC.camera(api, hs, name), a, name)
        oi, of, _ = osc.trace_closest(rays)
        thr, _ = osc.trace_shadow(rays, QC.shadow_max_t(oi, of))
        out[name] = {"rays": rays, "oi": oi, "of": of, "thr": thr, "lights": QC.lights_of_triangles(a)}
    return out


@pytest.mark.parametrize("name", QC.SCENES)
def test_a_set_holds_every_class(sets, name):
    s = sets[name]
    assert s["rays"].shape == (QC.N, 6) and QC.N % 64 != 0 and np.isfinite(s["rays"]).all()
    got = QC.classes(s["oi"], s["of"], s["thr"], s["lights"])
    print(name, got)
    for cls, floor in FLOOR.items():
        assert got[cls] >= floor, (name, cls, got)
    if name == "textured":
        frac = ((s["thr"] > 0) & (s["thr"] < 1)).all(1)
        assert got["partial"] >= 5 and frac.sum() >= 5, (got, int(frac.sum()))
    assert got["occluded"] + got["clear"] + got["partial"] == QC.N


@pytest.mark.parametrize("name", QC.SCENES)
def test_every_kind_of_ray_hits_and_misses(sets, name):
    s = sets[name]
    hit = s["oi"][:, 0] == 1
    d = s["rays"][:, 3:]
    for kind, sl in QC.KIND_SLICES.items():
        assert hit[sl].sum() >= 20 and (~hit[sl]).sum() >= 5, (name, kind, int(hit[sl].sum()))
    length = np.linalg.norm(d.astype(np.float64), axis=1)
    assert np.allclose(length[QC.KIND_SLICES["centre"]], 1, atol=1e-6) and np.allclose(length[QC.KIND_SLICES["inside"]], 1, atol=1e-6)
    un = length[QC.KIND_SLICES["unnormalised"]]
    assert un.min() < 0.5 and un.max() > 5.0
    ax = d[QC.KIND_SLICES["axis"]]
    assert ((ax == 0).sum(1) == 2).sum() >= 100 and ((ax == 0).sum(1) == 1).sum() >= 100


def test_the_sets_are_reproducible(api, oracle, scene_dir, sets):
    hs = QC.host(api, scene_dir, "cornell", "query_cpu2_")
    again = QC.ray_set(oracle, QC.camera(api, hs, "cornell"), QC.arrays(hs), "cornell")
    assert np.array_equal(again.view(np.uint32), sets["cornell"]["rays"].view(np.uint32))
    r = QC.records(again[:5], np.arange(5, dtype=np.float32))
    assert r.shape == (5, 8) and np.array_equal(r[:, 3], np.arange(5)) and not r[:, 7].any() and np.array_equal(r[:, 4:7], again[:5, 3:])
