#!/usr/bin/env python3
"""Static instruction census of the pair pass (pt_trace.h: trace_pair_flat) inside the FLAT pair megakernels, read from the
gfx950 device code with the Makefile's flags (hipcc -S, no GPU needed):

    python tools/pair_census.py [--asm FILE.s] [--json]

Regions of the kernel's bounce loop, found from the code itself:
  leaf loop   the loop that reads the leaf table through the scalar cache (s_load_dwordx8 of a leaf's box)
  set-up      from the first DPP prefix-sum step after the leaf loop up to the trip loop's header
  trip loop   the loop that folds hits into the LDS minima (ds_min_u64), one dealt test per trip
Counts per region by class: VALU, SALU (without s_nop / s_waitcnt / branches), branch, LDS, s_nop, s_waitcnt, v_readlane;
and the trip loop's inner back edges (a loop inside the trip loop: the old "next ray" search), its exec-mask splits, and the
longest chain of LDS reads in the set-up that each wait for the one before (lgkmcnt(0) between a ds_read and the next).
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


def compile_asm(out):
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="device assembly of pt_mk_lds.hip (default: compile it now)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            text = compile_asm(os.path.join(d, "pt_mk_lds.s"))
    res = {}
    for key, name in KERNELS.items():
        lines = function(text, name)
        res[key] = {"kernel": name, "metadata": metadata(text, name), "whole": census(lines), "regions": regions(lines)}
    if a.json:
        json.dump(res, sys.stdout, indent=1)
        print()
        return
    for key, r in res.items():
        print("%s  %s  %s" % (key, r["kernel"], " ".join("%s=%s" % kv for kv in r["metadata"].items())))
        for reg, c in [("whole", r["whole"])] + list(r["regions"].items()):
            print("  %-10s %s" % (reg, " ".join("%s=%d" % kv for kv in c.items())))


if __name__ == "__main__":
    main()
