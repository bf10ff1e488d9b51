"""Which megakernel a launch gets, with how much dynamic LDS: the table and the choice against what the if-ladders did.

tests/golden/mk_choice_parent.json records the last commit that dispatched by ladders (launch_megakernel, launch_megakernel_lds,
launch_megakernel_hbm; default build): the same driver as tests/mk_choice_driver.hip was built against those three functions, and for
every input of the cross product it noted which kernel they launched, with how many bytes of dynamic LDS at two parameter sets (every
family below 64 KB at the first and above it at the second) and whether hipFuncSetAttribute was called, or that they refused, and what
megakernel_has_moments_twin said. Here the driver is built, host code only and without a GPU, against megakernel_choose,
launch_megakernel and the two tables, and compared input by input:

  * where the ladders launched kernel K with L bytes, the new code launches K with L bytes, or refuses — but only an input that breaks
    an invariant of render_tiles (pt_plan.hip: plan_launch), `invariants` below; what the ladders refused stays refused;
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

One step earlier on the launch path, tests/launch_plan_driver.hip walks plan_launch and size_launch (pt_plan.hip) as render_tiles calls
them, over scene shapes x fact flags x options x requests. tests/golden/launch_plan_parent.json records what the last commit with the
decision inside render_tiles decided and sized for the same inputs; the plan, the chosen row, the sized fields and the dynamic LDS are
compared input by input, and every plan is put to `invariants`.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "cudapathtracer_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "mk_choice_driver.hip")
PLAN_DRIVER = os.path.join(ROOT, "tests", "launch_plan_driver.hip")


def invariants(i, parent_twin, experimental=False):
    """What render_tiles guarantees about the selector fields of every launch it makes: a restatement by hand of plan_launch
    (pt_plan.hip), which test_the_invariants_hold_for_every_plan checks against every plan the second driver produces (pt_set_option
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
def drivers(tmp_path_factory):
    """The two host-only drivers, built against the tables, the choice and the plan as they are now: (directory, {source: executable})."""
    d = tmp_path_factory.mktemp("mk_choice")
    flags = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "--cuda-host-only", "-I" + CSRC]
    units = [os.path.join(CSRC, n) for n in ("pt_kernels.hip", "pt_mk_lds.hip", "pt_mk_hbm.hip", "pt_plan.hip")]
    objs, procs = {}, []
    for src in units + [DRIVER, PLAN_DRIVER]:
        objs[src] = str(d / (os.path.basename(src) + ".o"))
        procs.append((src, subprocess.Popen(["hipcc"] + flags + ["-c", "-o", objs[src], src], stderr=subprocess.PIPE)))
    for src, pr in procs:
        err = pr.communicate()[1]
        assert pr.returncode == 0, (src, err.decode()[-2000:])
    exes = {}
    for drv, n in ((DRIVER, 3), (PLAN_DRIVER, 4)):                      # (only the plan's driver links pt_plan.hip)
        exes[drv] = str(d / os.path.basename(drv)[:-4])
        # (host-only objects name a device binary that is never built: the registration calls that would read it end in the driver's stubs)
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-rdynamic", "-Wl,--unresolved-symbols=ignore-all", "-o", exes[drv]] +
                              [objs[u] for u in units[:n]] + [objs[drv], "-ldl"])
    return d, exes


@pytest.fixture(scope="module")
def head(drivers):
    """The driver's output against the tables and the choice as they are now: [(set 0, set 1, twin, row)] in input order."""
    exe = drivers[1][DRIVER]
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


# ---- the plan and the sizes (pt_plan.hip) against what render_tiles decided before the decision moved there ----
PARTS = ("plan", "row", "scene", "grid")


def _fields(text):
    w = text.split()
    return {w[k]: int(w[k + 1]) for k in range(0, len(w), 2)}


def _expand(levels, axes):
    """A part's index (the record's index_format) as one array of text ids, an entry per input."""
    cur = None
    for (name, values), level in zip(reversed(axes), levels):
        t = np.array(level, dtype=np.int64)
        assert t.shape[1] == len(values), name
        cur = t if cur is None else cur[t].reshape(len(t), -1)
    assert len(cur) == 1
    return cur[0]


def _input(axes, k):
    i = {}
    for name, values in reversed(axes):
        i[name] = values[k % len(values)]
        k //= len(values)
    return i


@pytest.fixture(scope="module")
def plan_record():
    with open(os.path.join(GOLDEN, "launch_plan_parent.json")) as f:
        fx = json.load(f)
    return fx, {p: _expand(fx["index"][p], fx["axes"]) for p in PARTS}


@pytest.fixture(scope="module")
def plans(drivers):
    """The second driver's output: per part its distinct texts and, per input, which of them."""
    d, exes = drivers
    ids = str(d / "launch_plan.idx")
    out = subprocess.check_output([exes[PLAN_DRIVER], ids]).decode().strip().split("\n")
    texts = {p: [] for p in PARTS}
    axes = json.loads(out[0][2:])
    for ln in out[1:]:
        tag, k, text = ln.split(" ", 2)
        part = {"P": "plan", "R": "row", "S": "scene", "G": "grid"}[tag]
        assert int(k) == len(texts[part])
        texts[part].append(text)
    index = np.fromfile(ids, dtype=np.int32).reshape(-1, 4)
    return texts, {p: index[:, k] for k, p in enumerate(PARTS)}, axes


def test_the_plan_and_the_sizes_are_what_render_tiles_decided(plan_record, plans):
    fx, parent = plan_record
    texts, now, axes = plans
    assert all(dict(fx["axes"])[a] == axes[a] for a in ("shape", "options", "live")), "the driver's inputs are not the record's"
    n = len(parent["plan"])
    assert n == 9 * 32 * 90 * 96 and all(len(now[p]) == n == len(parent[p]) for p in PARTS)
    for p in PARTS:
        was = {t: k for k, t in enumerate(fx["parts"][p])}                 # this run's text ids as the record's (-1: a text it has not)
        differ = np.nonzero(np.array([was.get(t, -1) for t in texts[p]])[now[p]] != parent[p])[0]
        if len(differ):
            k = int(differ[0])
            both = lambda t, idx: {q: t[q][int(idx[q][k])] for q in PARTS}
            assert False, ("%d inputs differ in '%s'; the first:" % (len(differ), p), _input(fx["axes"], k), "parent", both(fx["parts"], parent),
                           "now", both(texts, now))


def test_the_record_has_every_case_it_is_to_have(plan_record):
    fx, parent = plan_record
    axes = dict(fx["axes"])
    assert [name for name, values in fx["axes"]] == ["shape", "flags", "options", "live", "listed", "integrator", "count", "useMIS"]
    shapes, sets = axes["shape"], axes["options"]
    per_shape = len(parent["plan"]) // len(shapes)
    plan = lambda shape, flags: _fields(fx["parts"]["plan"][parent["plan"][shape * per_shape + flags * (per_shape // 32)]])     # (defaults, first request)
    # every return of scene_onchip_wg at the defaults, and the shape that the per-wave area of the medium stacks pushes to the next size
    wg = [(plan(k, 0)["wg"], plan(k, 2)["wg"]) for k in range(len(shapes))]             # generic, SIMPLE (flags bit 1: simpleOk)
    assert {w for pair in wg for w in pair} == {0, 4, 8, 16} and (8, 4) in wg, wg
    assert any(sh[4] > 16 for sh in shapes) and any(sh[5] == 0 for sh in shapes) and any(sh[5] > 0 for sh in shapes)    # stackSpill != 0; nLeaves
    assert {64, 65, 128, 129} <= {sh[0] for sh in shapes} and {64, 65, 128, 129} <= {sh[1] for sh in shapes}
    # scenes in HBM whose triangles are not cached (the tree alone exceeds the 12 KB cache), below, between and above the two copies of
    # the tree top that the kernels for scenes in HBM hold: 512 nodes, 768 with the SIMPLE bounce, as the record's sized launches say
    hbm = [sh[0] for k, sh in enumerate(shapes) if wg[k] == (0, 0) and sh[0] * 64 > 12288]
    assert any(n < 512 for n in hbm) and any(512 < n < 768 for n in hbm) and any(n > 768 for n in hbm), hbm
    cached = {(_fields(fx["parts"]["plan"][int(p)])["simple"], _fields(fx["parts"]["scene"][int(s)])["cacheNodes"])
              for p, s in zip(parent["plan"][-per_shape:], parent["scene"][-per_shape:]) if fx["parts"]["scene"][int(s)] != "-" and _fields(fx["parts"]["plan"][int(p)])["hbm"]}
    assert cached == {(0, 512), (1, 768)}, cached
    # the options: the defaults, each setting alone, each pair of settings of different options
    single = [s[0] for s in sets if len(s) == 1]
    assert sets[0] == [] and {tuple(s) for s in single} == {("onchip", 0), ("waves_hbm", 0), ("waves_hbm", 2), ("refill", 0), ("culling", 1), ("flat", 0),
                                                               ("flat", 2), ("flat2", 0), ("simple", 0), ("lean", 0), ("leaf_boxes", 0), ("refill_keep", 3),
                                                               ("persistent", 0)}
    pairs = [s for s in sets if len(s) == 2]
    assert len(sets) == 1 + len(single) + len(pairs) and sorted(map(json.dumps, pairs)) == sorted(
        json.dumps([a, b]) for k, a in enumerate(single) for b in single[k + 1:] if a[0] != b[0])
    assert axes["flags"] == list(range(32)) and axes["live"] == [1, 6143, 6144, 7679, 7680, 32400]
    assert [axes[a] for a in ("listed", "integrator", "count", "useMIS")] == [[0, 1], [0, 2], [0, 1], [0, 1]]


def test_the_invariants_hold_for_every_plan(plan_record, plans):
    fx, parent = plan_record
    texts, now, axes = plans
    # integrator and count are the third- and second-innermost axes; a plan's text does not carry them
    k = np.arange(len(now["plan"]))
    planned = 0
    for key in np.unique(now["plan"].astype(np.int64) * 4 + ((k >> 1) & 3)):
        p, integ, count = int(key) >> 2, (int(key) >> 1) & 1, int(key) & 1
        if texts["plan"][p] == "-":
            continue                                                    # (a counting launch with a tile list: refused before it is planned)
        f = _fields(texts["plan"][p])
        i = dict(f, onchip=int(f["wg"] > 0), integrator=(0, 2)[integ], count=int(count), syncShadow=1)
        assert invariants(i, False), i
        planned += 1
    assert planned > 100
    # "render_tiles: no megakernel is built for this launch": no planned launch of the parent's lacked a row, and none does now
    assert "none" not in fx["parts"]["row"] and "none" not in texts["row"]
    # a workgroup may take all of its CU's LDS, and no more
    lds = [_fields(t)["lds"] for t in texts["scene"] if t != "-"]
    assert len(lds) > 100 and max(lds) <= 160 * 1024, max(lds)
