"""Which megakernel a launch gets, with how much dynamic LDS: the table and the choice against what the if-ladders did.

tests/golden/mk_choice_parent.json records the last commit that dispatched by ladders (launch_megakernel, launch_megakernel_lds,
launch_megakernel_hbm; default build): the same driver as tests/mk_choice_driver.hip was built against those three functions, and for
every input of the cross product it noted which kernel they launched, with how many bytes of dynamic LDS at two parameter sets (every
family below 64 KB at the first and above it at the second) and whether hipFuncSetAttribute was called, or that they refused, and what
megakernel_has_moments_twin said. Here the driver is built, host code only and without a GPU, against megakernel_choose,
launch_megakernel and the two tables, and compared input by input:

  * where the ladders launched kernel K with L bytes, the new code launches K with L bytes, or refuses — but only an input that breaks
    an invariant of render_tiles (pt_render.hip), `invariants` below; what the ladders refused stays refused;
  * the LDS attribute is raised exactly when L > 65536, for every row. The ladders raised it under that condition on the arms that
    had PT_LDS_OK and never on the 4-wave general kernel's; wherever they raised it, it is still raised;
  * L follows from the launched row's own stack entries, medium stacks and attribute cache, and the row's name is the kernel that
    was launched;
  * a moments twin exists exactly when the choice with moments on returns a row that is dispatched, and that equals the ladders'
    megakernel_has_moments_twin on every input that keeps the invariants. An input that breaks them may be refused, and a refused
    launch has no twin; so there the new predicate is the recorded one or false. (The ladders ignored flat, simple or lean where an
    arm did not read them, and sized the LDS of a 4-wave kernel for the pair form's 24 rows at flat == 3 without onchip: inputs
    render_tiles never produces. 136 of the 2048 selector combinations have a recorded twin that is now refused, none of them
    invariant-keeping.)
"""
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "cudapathtracer_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "mk_choice_driver.hip")


def invariants(i, parent_twin, experimental=False):
    """What render_tiles guarantees about the selector fields of every launch it makes (read off pt_render.hip; pt_set_option
    refuses "refill" 2, "defer_shadow", "xcd_bands", "wide" and "compact": the record's inputs carry none of the last three)."""
    imp = lambda a, b: (not a) or b
    wide, compact, bands = i.get("wide", 0), i.get("compact", 0), i.get("xcdBands", 0)
    ok = imp(i["hbm"], not i["onchip"])
    ok = ok and imp(i["flat"] != 0, i["onchip"] and not i["refill"] and i["syncShadow"])
    ok = ok and imp(i["flat"] == 3, i["integrator"] == 0 and not i["count"])
    ok = ok and imp(i["simple"], i["flat"] != 0 or (not i["onchip"] and i["refill"] and not i["cull"] and not i["count"]))
    ok = ok and imp(i["lean"], not i["simple"] and not i["count"] and not i["cull"] and (i["flat"] == 3 or (not i["onchip"] and i["refill"])))
    ok = ok and imp(i["cull"], i["hbm"] and not i["refill"])
    ok = ok and imp((i["onchip"] and i["refill"]) or not i["syncShadow"] or wide or compact or bands, experimental)
    ok = ok and imp(wide or compact, i["hbm"] and i["simple"] and i["refill"] and not i["count"] and not (wide and compact))
    ok = ok and imp(not i["syncShadow"], not (i["onchip"] or i["hbm"] or i["flat"] or i["refill"] or i["simple"] or i["lean"]))
    ok = ok and imp(i.get("moments", 0), parent_twin)
    return bool(ok)


def _outcome(text):
    text = text.strip()
    if text == "refused":
        return None
    k, lds, attr = [x.strip() for x in text.split(";")]
    return k, int(lds), int(attr)


def _inputs(axes):
    rows = [{}]
    for name, values in axes:
        rows = [dict(r, **{name: v}) for r in rows for v in values]
    return rows


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLDEN, "mk_choice_parent.json")) as f:
        fx = json.load(f)
    inputs = _inputs(fx["axes"])
    assert len(inputs) == len(fx["index"]) == 4096
    parent = []
    for k in fx["index"]:
        a, b, twin = fx["outcomes"][k].split("|")
        parent.append((_outcome(a), _outcome(b), int(twin)))
    return fx, inputs, parent


@pytest.fixture(scope="module")
def head(tmp_path_factory):
    """The driver's output against the tables and the choice as they are now: [(set 0, set 1, twin, row)] in input order."""
    d = tmp_path_factory.mktemp("mk_choice")
    flags = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "--cuda-host-only", "-I" + CSRC]
    objs, procs = [], []
    for src in (os.path.join(CSRC, "pt_kernels.hip"), os.path.join(CSRC, "pt_mk_lds.hip"), os.path.join(CSRC, "pt_mk_hbm.hip"), DRIVER):
        obj = str(d / (os.path.basename(src) + ".o"))
        objs.append(obj)
        procs.append((src, subprocess.Popen(["hipcc"] + flags + ["-c", "-o", obj, src], stderr=subprocess.PIPE)))
    for src, pr in procs:
        err = pr.communicate()[1]
        assert pr.returncode == 0, (src, err.decode()[-2000:])
    exe = str(d / "mk_choice_driver")
    # (host-only objects name a device binary that is never built: the registration calls that would read it end in the driver's stubs)
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-rdynamic", "-Wl,--unresolved-symbols=ignore-all", "-o", exe] + objs + ["-ldl"])
    out = subprocess.check_output([exe]).decode().strip().split("\n")
    rows = []
    for ln in out:
        a, b, twin, row = ln.split("|")
        row = row.strip()
        if row != "none":
            name, *facts = [x.strip() for x in row.split(";")]
            row = (name,) + tuple(int(x) for x in facts)                # stack entries, medium stacks, attribute cache, waves per workgroup / SIMD
        rows.append((_outcome(a), _outcome(b), int(twin), None if row == "none" else row))
    return rows


def test_the_choice_launches_what_the_ladders_launched(record, head):
    fx, inputs, parent = record
    assert len(head) == len(inputs)
    launched = refused_now = 0
    for i, p, n in zip(inputs, parent, head):
        keeps = invariants(i, p[2] == 1)
        for k in (0, 1):
            if n[k] is None:
                assert p[k] is None or not keeps, ("an input that keeps the invariants is refused", i, p[k])
                refused_now += p[k] is not None
                continue
            assert p[k] is not None, ("launched what the ladders refused", i, n[k])
            assert n[k][:2] == p[k][:2], (i, p[k], n[k])
            assert n[k][2] == (1 if n[k][1] > 65536 else 0), ("the LDS attribute is raised exactly above 64 KB", i, n[k])
            assert p[k][2] <= n[k][2], (i, p[k], n[k])
            launched += 1
    # (the record holds launches that keep the invariants and launches that break them: both branches above were taken)
    keeping = sum(1 for i, p in zip(inputs, parent) for k in (0, 1) if p[k] is not None and invariants(i, p[2] == 1))
    assert launched >= keeping == 2 * 75 and refused_now > 0, (launched, keeping, refused_now)


def test_every_family_crosses_64k_in_the_record(record):
    fx, inputs, parent = record
    below = {p[0][0] for p in parent if p[0] is not None and p[0][1] <= 65536}
    above = {p[1][0] for p in parent if p[1] is not None and p[1][1] > 65536}
    kernels = {p[0][0] for p in parent if p[0] is not None}
    assert len(kernels) == 67 and below == kernels and above == kernels      # the 68 built, less the SIMPLE pair kernel's twin: out of the dispatch


def test_the_lds_size_follows_from_the_rows_facts(record, head):
    fx, inputs, parent = record
    seen = {}
    for i, p, n in zip(inputs, parent, head):
        for k in (0, 1):
            if n[k] is None:
                continue
            name, stack, med, attr = n[3][:4]
            assert name == n[k][0], ("the row's name is not the kernel its address launches", n[3], n[k])
            s = fx["sets"][k]
            lds = s["cacheNodes"] * 64 + s["cacheTris"] * 48 + s["wgWaves"] * (stack * 256 + (1024 if med else 0))
            if attr:
                lds += s["cacheAttrs"] * 80 + s["cacheMats"] * 96 + s["cacheLights"] * 64
            assert lds == p[k][1], (i, n[3], lds, p[k])
            assert seen.setdefault(name, n[3]) == n[3]
    assert len(seen) == 67


def test_a_twin_exists_exactly_when_the_choice_with_moments_returns_a_dispatched_row(record, head):
    fx, inputs, parent = record
    by_selectors = {}
    differ = 0
    for i, p, n in zip(inputs, parent, head):
        if i["moments"]:
            assert n[2] == (1 if n[0] is not None else 0), (i, n)
            if n[0] is None and n[3] is not None:
                assert n[3][0] == "megakernel_flat2_moments<0, true, false>", n[3]      # the one row that is built and not dispatched
        key = tuple(sorted((k, v) for k, v in i.items() if k != "moments"))
        assert by_selectors.setdefault(key, n[2]) == n[2]                                 # (the predicate does not read `moments`)
        if invariants(dict(i, moments=0), False):
            assert n[2] == p[2], ("has_moments_twin changed on an input render_tiles can produce", i, p[2], n[2])
        else:
            assert n[2] in (0, p[2]), (i, p[2], n[2])
            differ += n[2] != p[2]
    assert differ == 2 * 136, differ
    # render_tiles sizes the launch by the counterpart's row and then launches the twin: their facts must agree
    twins = 0
    for k in range(0, len(inputs), 2):                                  # (moments is the innermost axis)
        assert not inputs[k]["moments"] and inputs[k + 1]["moments"]
        if head[k + 1][3] is not None:
            assert head[k][3] is not None and head[k][3][1:] == head[k + 1][3][1:], (inputs[k], head[k][3], head[k + 1][3])
            twins += 1
    assert twins >= 27
