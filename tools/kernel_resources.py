r"""Registers, scratch and LDS of a translation unit's kernels, from the code-object notes of a device-only compile. No GPU needed.

    python tools/kernel_resources.py pt_aov '(aov\w*?_kernel)'
    python tools/kernel_resources.py pt_temporal '(temporal_kernel)'
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudapathtracer_amd", "csrc")
FLAGS = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math")     # the Makefile's FLAGS
KEYS = "vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size"


def kernel_resources(translation_unit, name_regex):
    """{kernel: {vgpr_count, vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size (scratch bytes per lane),
    group_segment_fixed_size (LDS bytes per workgroup)}} of the kernels pt::<name> of csrc/<translation_unit>.hip whose name matches
    name_regex in full; the key is the regex's first group, and for an instantiation of a template kernel the whole mangled name
    (it carries the template arguments: pt_temporal 'temporal_kernel' lists nine)."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, translation_unit + ".s")
        subprocess.check_call(["hipcc", *FLAGS, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, translation_unit + ".hip")],
                              stderr=subprocess.DEVNULL)
        text = open(out).read()
    res = {}
    notes = text[text.index("amdhsa.kernels:"):]
    for block in re.split(r"^  - ", notes, flags=re.M)[1:]:            # one list item per kernel; its keys come in alphabetical order
        name = re.search(r"^\s*\.name:\s+(_ZN2pt\d+%s(E|I)\S*)" % name_regex, block, flags=re.M)
        if name:
            res[name.group(1) if name.group(3) == "I" else name.group(2)] = {k: int(v) for k, v in re.findall(r"\.(%s):\s+(\d+)$" % KEYS, block, flags=re.M)}
    return res


if __name__ == "__main__":
    print(json.dumps(kernel_resources(sys.argv[1], sys.argv[2])))
