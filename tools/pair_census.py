#!/usr/bin/env python3
"""Static instruction census of the pair pass (pt_trace.h: trace_pair_flat) inside the FLAT pair megakernels, read from the
gfx950 device code with the Makefile's flags (hipcc -S, no GPU needed):

    python tools/pair_census.py [--asm FILE.s] [--json] [--runs]

Regions of the kernel's bounce loop, found from the code itself:
  leaf loop   the loop that reads the leaf table through the scalar cache (s_load_dwordx8 of a leaf's box)
  set-up      from the first DPP prefix-sum step after the leaf loop up to the trip loop's header
  trip loop   the loop that folds hits into the LDS minima (ds_min_u64), one dealt test per trip
Counts per region by class: VALU, SALU (without s_nop / s_waitcnt / branches), branch, LDS, s_nop, s_waitcnt, v_readlane;
and the trip loop's inner back edges (a loop inside the trip loop: the old "next ray" search), its exec-mask splits, and the
longest chain of LDS reads in the set-up that each wait for the one before (lgkmcnt(0) between a ds_read and the next).

Register moves (v_mov_b32 / v_mov_b64), under the key "moves" of a kernel, for the regions above and two more:
  bounce_loop the loop that holds the leaf loop and the trip loop: one logic step and one pair pass
  logic       the bounce loop's head up to the leaf loop: scheduling check, logic step, regeneration, the pair pass's head
split by source (from_vgpr, from_const, from_sgpr), and the lengths of the runs of four or more consecutive moves (const_runs:
those of them that load constants only). "leaf_path" (leaf_record_path): what the leaf loop issues per record on the path every
record takes and in the blocks that a record with an empty mask word skips, and the scalar branches on a mask dword. --runs lists every run with the first source line it maps to; for that the census
compiles with line tables (-gline-tables-only), which the library's build never has.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudapathtracer_amd", "csrc")
KERNELS = {"c2": "_ZN2pt16megakernel_flat2ILi0ELb1ELb0EEEvNS_7KParamsE",        # megakernel_flat2<0, true, false>: the headline
           "mixed": "_ZN2pt16megakernel_flat2ILi0ELb0ELb1EEEvNS_7KParamsE"}     # megakernel_flat2<0, false, true>: the mixed Cornell row


def compile_asm(out, lines=False):
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]
    if lines:
        flags.append("-gline-tables-only")
    subprocess.check_call(["hipcc"] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "pt_mk_lds.hip")], stderr=subprocess.DEVNULL)
    return open(out).read()


def function(text, name):
    m = re.search(r"^%s:.*?^\s*s_endpgm" % re.escape(name), text, flags=re.S | re.M)
    assert m, name
    return m.group(0).split("\n")


def metadata(text, name):
    m = re.search(r"\.name:\s+%s\n(.*?)(?:\n\s+- \.|\Z)" % re.escape(name), text, flags=re.S)
    md = {}
    if m:
        for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size"):
            mm = re.search(r"\.%s:\s+(\d+)" % k, m.group(1))
            if mm:
                md[k] = int(mm.group(1))
    return md


def is_insn(ln):
    s = ln.strip()
    return bool(s) and not s.startswith((";", ".")) and not s.endswith(":")


def classify(s):
    op = s.split()[0]
    if op.startswith(("s_branch", "s_cbranch")):
        return "branch"
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return "other"


def census(lines):
    c = {"total": 0, "valu": 0, "salu": 0, "branch": 0, "lds": 0, "s_nop": 0, "s_waitcnt": 0, "other": 0, "v_readlane": 0}
    for ln in lines:
        if is_insn(ln):
            s = ln.strip()
            c["total"] += 1
            c[classify(s)] += 1
            if s.startswith("v_readlane"):
                c["v_readlane"] += 1
    return c


def loops(lines):
    """(header index, back-edge index) of every backward branch."""
    pos = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            pos[m.group(1)] = i
    out = []
    for i, ln in enumerate(lines):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(1) in pos and pos[m.group(1)] < i:
            out.append((pos[m.group(1)], i))
    return out


def dependent_lds_chain(lines):
    """Longest run of ds_read -> s_waitcnt lgkmcnt(0) -> ds_read ... in which each read waits for the one before."""
    best = run = 0
    pending = False
    for ln in lines:
        if not is_insn(ln):
            continue
        s = ln.strip()
        if s.startswith("ds_read"):
            if not pending:
                run = run + 1 if run else 1
            pending = True
        elif s.startswith("s_waitcnt") and "lgkmcnt(0)" in s:
            pending = False
        elif s.startswith(("ds_write", "ds_min", "s_branch", "s_cbranch")) or re.match(r"^\.LBB", s):
            run = 0
            pending = False
        best = max(best, run)
    return best


def regions(lines):
    lp = loops(lines)
    trip = [(h, e) for h, e in lp if all(any(op in lines[k] for k in range(h, e + 1)) for op in ("ds_min_u64", "v_ffbl_b32"))]
    assert trip, "no trip loop (ds_min_u64) found"
    th, te = min(trip, key=lambda x: x[1] - x[0])             # the innermost loop that picks a triangle (ctz) and folds its hit
    leaf = [(h, e) for h, e in lp if e < th and any("s_load_dwordx8" in lines[k] for k in range(h, e + 1))]
    # the innermost of them: a cold block the compiler lays out behind the loop (the IEEE divisions of inv3_uniform) branches back to
    # code in front of it, which makes an enclosing "loop" of this kind that is no loop of the source
    lh, le = min(leaf, key=lambda x: x[1] - x[0]) if leaf else (th, th)
    s0 = next(k for k in range(le, th) if "row_shr:1 " in lines[k] or lines[k].rstrip().endswith("row_shr:1"))
    trip_lines = lines[th:te + 1]
    inner = [(h, e) for h, e in lp if th < h and e <= te]                 # (branches back to the header itself are the loop's own)
    out = {"leaf_loop": census(lines[lh:le + 1]), "setup": census(lines[s0:th]), "trip_loop": census(trip_lines)}
    out["trip_loop"]["inner_back_edges"] = len(inner)
    out["trip_loop"]["exec_splits"] = sum(1 for ln in trip_lines if re.search(r"s_(xor|andn2_saveexec)_b64", ln))
    out["trip_loop"]["ds_min_u64"] = sum(1 for ln in trip_lines if "ds_min_u64" in ln)
    out["setup"]["dependent_lds_chain"] = dependent_lds_chain(lines[s0:th])
    return out


def leaf_record_path(lines):
    """The leaf loop per record, for a loop whose body branches on a record's mask dword. The loop is the
    innermost one around the s_load_dwordx8 in front of the trip loop; its blocks are walked from the header, falling through every
    forward conditional branch that leaves a block for one inside the loop, until the back edge:
      always      census of the blocks on that walk: what every record issues
      skipped     census of the loop's other blocks: what only a record with a non-empty word issues
      v_cndmask, v_or, v_and_or, v_mov   counts on the always-executed walk
      mask_branches   [(compare, branch)] of the s_cmp_*_u32 of an SGPR of the record against 0 with the s_cbranch_scc* behind it
      exec_splits     s_and_saveexec / s_or_saveexec / s_andn2_saveexec in the loop
    The loop's blocks are the ones the compiler's annotations name as its own, wherever it lays them out."""
    lp = loops(lines)
    trip = [(h, e) for h, e in lp if all(any(op in lines[k] for k in range(h, e + 1)) for op in ("ds_min_u64", "v_ffbl_b32"))]
    th, _ = min(trip, key=lambda x: x[1] - x[0])
    leaf = [(h, e) for h, e in lp if e < th and any("s_load_dwordx8" in lines[k] for k in range(h, e + 1))]
    lh = min(leaf, key=lambda x: x[1] - x[0])[0]
    head = re.match(r"^\.L(BB\d+_\d+):", lines[lh]).group(1)
    rotated = re.search(r"in Loop: Header=(BB\d+_\d+)", lines[lh])     # the branch goes back to a block laid out in front of the header it falls into
    if rotated:
        head = rotated.group(1)
    bl = blocks(lines)
    member = [n for n, (i, _, lab, note) in enumerate(bl) if lab == head or re.search(r"in Loop: Header=%s\b" % head, note)]
    at = {bl[n][2]: n for n in member if bl[n][2]}
    inside = [k for n in member for k in range(bl[n][0], bl[n][1])]
    # the record's SGPRs: the destination of the loop's s_load_dwordx8
    m = next(re.search(r"s_load_dwordx8 s\[(\d+):(\d+)\]", lines[k]) for k in inside if "s_load_dwordx8" in lines[k])
    rec = {"s%d" % i for i in range(int(m.group(1)), int(m.group(2)) + 1)}
    walk, n, seen = [], at[head], set()
    while n is not None and n in member and n not in seen:
        seen.add(n)
        nxt = n + 1                                                # a conditional branch that is not the back edge: fall through
        for k in range(bl[n][0], bl[n][1]):
            walk.append(k)
            mm = re.match(r"\s+s_c?branch\w*\s+\.L(BB\d+_\d+)", lines[k])
            if mm and (mm.group(1) == head or lines[k].strip().startswith("s_branch")):
                nxt = None if mm.group(1) == head else at.get(mm.group(1))
                break
        n = nxt
    always = [lines[k] for k in walk]
    skipped = [lines[k] for n in member if n not in seen for k in range(bl[n][0], bl[n][1])]      # (whole blocks: not the exit branch behind the back edge)
    out = {"always": census(always), "skipped": census(skipped)}
    for op in ("v_cndmask", "v_or", "v_and_or", "v_mov"):
        out[op] = sum(1 for ln in always if is_insn(ln) and ln.strip().startswith(op + "_"))
    pairs, cmp_ = [], None
    for k in inside:
        if not is_insn(lines[k]):
            continue
        s = lines[k].strip().split(";")[0].strip()
        mm = re.match(r"s_cmp_(?:eq|lg)_u32 (s\d+), 0$", s)
        if mm and mm.group(1) in rec:
            cmp_ = s
        elif s.startswith("s_cmp"):
            cmp_ = None
        elif cmp_ and re.match(r"s_cbranch_scc[01] ", s):
            pairs.append((cmp_, s))
            cmp_ = None
    out["mask_branches"] = pairs
    out["exec_splits"] = sum(1 for k in inside if re.search(r"s_(and|or|andn2|xor)_saveexec_b64", lines[k]))
    out["v_readlane"] = sum(1 for k in inside if is_insn(lines[k]) and lines[k].strip().startswith("v_readlane"))
    return out


def move_source(s):
    """"from_vgpr" / "from_const" / "from_sgpr" for a v_mov_b32 / v_mov_b64 (DPP and SDWA forms are cross-lane or partial: no moves), else None."""
    t = s.split(None, 1)
    if len(t) < 2 or t[0] not in ("v_mov_b32_e32", "v_mov_b64_e32", "v_mov_b32", "v_mov_b64", "v_mov_b32_e64", "v_mov_b64_e64"):
        return None
    src = t[1].split(";")[0].split(",", 1)[1].strip()
    if src.startswith("v"):
        return "from_vgpr"
    if re.match(r"^(s\d|s\[|vcc|exec|ttmp|m0)", src):
        return "from_sgpr"
    return "from_const"


def move_census(lines):
    """Moves of a region by source, and its runs of four or more consecutive moves: (index of the first, [source, ...]).
    zero_fill_runs: the runs that are `v_mov vN, 0` throughout; longest_zero_fill: the most such fills in a row anywhere."""
    c = {"valu": 0, "v_mov": 0, "from_vgpr": 0, "from_const": 0, "from_sgpr": 0}
    runs, zero, cur, text, start = [], [], [], [], 0
    fills = longest = 0                                    # consecutive `v_mov vN, 0`, inside a longer run of moves or not
    for i, ln in enumerate(list(lines) + ["\ts_endpgm"]):
        if not is_insn(ln):
            continue
        s = ln.strip()
        k = move_source(s)
        if classify(s) == "valu":
            c["valu"] += 1
        fills = fills + 1 if k and re.search(r",\s*0$", s.split(";")[0].strip()) else 0
        longest = max(longest, fills)
        if k:
            c["v_mov"] += 1
            c[k] += 1
            if not cur:
                start = i
            cur.append(k)
            text.append(s.split(";")[0].strip())
        else:
            if len(cur) >= 4:
                runs.append((start, cur))
                if all(re.search(r",\s*0$", t) for t in text):
                    zero.append(len(cur))
            cur, text = [], []
    c["runs"] = [len(r) for _, r in runs]
    c["const_runs"] = [len(r) for _, r in runs if all(k == "from_const" for k in r)]
    c["zero_fill_runs"] = zero
    c["longest_zero_fill"] = longest
    return c, runs


def blocks(lines):
    """[(first line, end line, label or None, annotation)] of the basic blocks: a block starts at a .LBB label or at the
    compiler's `; %bb.N:` comment, and its annotation is what the compiler says there about the loops it is in."""
    starts = [i for i, ln in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:", ln) or re.match(r"^; %bb\.\d+:", ln)]
    out = []
    for n, i in enumerate(starts):
        end = starts[n + 1] if n + 1 < len(starts) else len(lines)
        note = lines[i].split(";", 1)[1] if ";" in lines[i] else ""
        k = i + 1
        while k < end and lines[k].strip().startswith(";") and not lines[k].startswith("; %bb."):
            note += " " + lines[k]
            k += 1
        m = re.match(r"^\.L(BB\d+_\d+):", lines[i])
        out.append((i, end, m.group(1) if m else None, note))
    return out


def bounce_loop(lines):
    """(member line indices, leaf loop's header line) of the bounce loop: the innermost loop that holds both the leaf loop and
    the trip loop, by the compiler's own loop annotations, so that blocks it lays out behind the back edge count as well."""
    lp = loops(lines)
    trip = [(h, e) for h, e in lp if all(any(op in lines[k] for k in range(h, e + 1)) for op in ("ds_min_u64", "v_ffbl_b32"))]
    th, te = min(trip, key=lambda x: x[1] - x[0])
    leaf = [(h, e) for h, e in lp if e < th and any("s_load_dwordx8" in lines[k] for k in range(h, e + 1))]
    lh, le = min(leaf, key=lambda x: x[1] - x[0]) if leaf else (th, th)
    bl = blocks(lines)
    parents = {lab: [h for h, _ in re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", note)] for _, _, lab, note in bl if lab}

    def enclosing(lab, note):
        """Headers of the loops a block is in, outermost first."""
        hd = re.search(r"Header=(BB\d+_\d+)", note)
        if hd:
            return parents.get(hd.group(1), []) + [hd.group(1)]
        return parents.get(lab, []) + [lab] if "Loop Header" in note else []

    enc = {i: enclosing(lab, note) for i, _, lab, note in bl}
    common = [h for h in enc[th] if h in enc[lh]]
    assert common, "no loop around the leaf loop and the trip loop"
    head = common[-1]
    member = []
    for i, end, lab, note in bl:
        if head in enc[i]:
            member.extend(range(i, end))
    return member, lh


def source_of(lines, i):
    """The last .loc in front of line i (its comment: file:line:col and the inlining chain), or None without line tables."""
    for k in range(i, -1, -1):
        m = re.match(r"\s+\.loc\s.*?;\s*(.*)", lines[k])
        if m:
            return m.group(1).strip()
    return None


def move_regions(lines):
    """{"bounce_loop": ..., "logic": ...}: move_census of the two regions, plus "run_list" (line, length, sources, first source line).
    logic: the bounce loop's blocks laid out in front of the leaf loop."""
    member, lh = bounce_loop(lines)
    out = {}
    for reg, idx in (("bounce_loop", member), ("logic", [i for i in member if i < lh])):
        sub = [lines[i] for i in idx]
        c, runs = move_census(sub)
        c["total"] = census(sub)["total"]
        c["run_list"] = [{"at": idx[st], "len": len(r), "from_const": r.count("from_const"), "from_vgpr": r.count("from_vgpr"),
                          "from_sgpr": r.count("from_sgpr"), "first": sub[st].strip().split(";")[0].strip(), "source": source_of(lines, idx[st])}
                         for st, r in runs]
        out[reg] = c
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="device assembly of pt_mk_lds.hip (default: compile it now)")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--runs", action="store_true", help="list the runs of four or more consecutive moves with their first source line (compiles with line tables)")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            text = compile_asm(os.path.join(d, "pt_mk_lds.s"), lines=a.runs)
    res = {}
    for key, name in KERNELS.items():
        lines = function(text, name)
        res[key] = {"kernel": name, "metadata": metadata(text, name), "whole": census(lines), "regions": regions(lines), "moves": move_regions(lines)}
        res[key]["moves"]["whole"] = move_census(lines)[0]
        res[key]["leaf_path"] = leaf_record_path(lines)
    if a.json:
        json.dump(res, sys.stdout, indent=1)
        print()
        return
    for key, r in res.items():
        print("%s  %s  %s" % (key, r["kernel"], " ".join("%s=%s" % kv for kv in r["metadata"].items())))
        for reg, c in [("whole", r["whole"])] + list(r["regions"].items()):
            print("  %-10s %s" % (reg, " ".join("%s=%d" % kv for kv in c.items())))
        p = r["leaf_path"]
        print("  leaf path  per record, always executed: %s; %s" % (" ".join("%s=%d" % (k, p["always"][k]) for k in ("total", "valu", "salu", "branch", "s_nop")),
                                                                     " ".join("%s=%d" % (k, p[k]) for k in ("v_mov", "v_cndmask", "v_or", "v_and_or"))))
        print("             skipped by a record with an empty mask word: total=%d valu=%d; branches on a mask dword: %s; exec_splits=%d v_readlane=%d"
              % (p["skipped"]["total"], p["skipped"]["valu"], ", ".join("%s / %s" % b for b in p["mask_branches"]) or "none", p["exec_splits"], p["v_readlane"]))
        for reg in ("whole", "bounce_loop", "logic"):
            m = r["moves"][reg]
            print("  moves %-11s %s runs=%s const_runs=%s zero_fill_runs=%s" % (reg, " ".join("%s=%d" % (k, m[k]) for k in ("total", "valu", "v_mov", "from_vgpr", "from_const", "from_sgpr", "longest_zero_fill") if k in m),
                                                              m["runs"], m["const_runs"], m["zero_fill_runs"]))
            if a.runs:
                for x in m.get("run_list", []):
                    print("    run of %2d (const %d, vgpr %d, sgpr %d) at line %d: %-28s %s" % (x["len"], x["from_const"], x["from_vgpr"], x["from_sgpr"], x["at"], x["first"], x["source"] or "-"))


if __name__ == "__main__":
    main()
