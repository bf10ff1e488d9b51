"""CPU only. tools/repack_check.hip — the makers of the packed records (csrc/pt_pack.h) on exactly representable values, the area
ranking with a tie and a non-finite area, and the host re-pack of a caller's own tree — built as a stand-alone program (its own
main, --cuda-host-only: no device code, no library, no GPU) and run: plain, and with -fsanitize=address,undefined. Every case prints
one line; a case that came out wrong prints FAILED and the program returns 1."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "repack_check.hip")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-fno-omit-frame-pointer"]
CASES = ("make_light", "make_tri", "make_attr", "make_node", "order_area", "rank_by_area", "number_nodes", "stack_need", "pack_triangles", "pack_lights")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_pack_rules_hold_on_the_host(tmp_path, sanitize):
    exe = str(tmp_path / "repack_check")
    flags = ["--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "--cuda-host-only"] + (SANITIZE if sanitize else [])
    subprocess.check_call(["hipcc"] + flags + ["-o", exe, TOOL])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    assert "FAILED" not in p.stdout
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert lines and all(ln.endswith(" ok") for ln in lines)
    for c in CASES:
        assert any(ln.startswith(c) for ln in lines), c
