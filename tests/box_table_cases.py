"""Trees for the box table's tests (pt_box_table.h), as the 64-byte PNode records derive_layout (pt_scene.hip) hands its builders —
the children's triangle counts in the spare words — and the host-only driver tests/box_table_driver.hip built and run on them.

  pnodes_from_bvh     a loaded scene's reference tree (48-byte nodes), packed as number_nodes packs it: internal nodes breadth-first
  chain               a left-deep tree over given leaf boxes and counts, every parent box the float-wise min / max of its children's
  FUZZ, fuzz_config   the scenes.fuzz seeds of tests/test_pair_boxes.py and what each is there for; open_floor: a scene without a shell
  run_driver          build the driver once per directory (optionally with -fsanitize=address,undefined) and parse what it prints
"""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudapathtracer_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "box_table_driver.hip")
BVH = np.dtype([("mn", "<f4", 4), ("mx", "<f4", 4), ("left", "<i4"), ("right", "<i4"), ("first", "<i4"), ("count", "<i4")])
PNODE = np.dtype([("lmin", "<f4", 3), ("lmax", "<f4", 3), ("rmin", "<f4", 3), ("rmax", "<f4", 3), ("left", "<i4"), ("right", "<i4"),
                  ("pad0", "<i4"), ("pad1", "<i4")])
assert BVH.itemsize == 48 and PNODE.itemsize == 64


# scenes.fuzz seeds the timed pair kernels run (3: the SIMPLE one; 6, 86, 110: the LEAN one; seen in the launches' flags on the GPU),
# chosen with the driver: seed -> (leaves, records, what it covers). Every fuzz scene stands in the Cornell shell, whose wall leaves
# share the whole-scene box: none of 700 seeds gives a tree without a duplicate, and none a box that three leaves share. The
# duplicate-free case is open_floor below; the largest sharing is the two leaves of these scenes.
FUZZ = {3: (14, 12, "an even record count; a shared box's mask with bits on both sides of bit 32; grouped on y: three groups of 3, three of 1"),
        6: (12, 11, "an odd record count; grouped on x: 8 groups, five of them of one record"),
        86: (25, 22, "three shared boxes, two of them with bits in both mask words, and a leaf whose own range crosses bit 32; on y: 15 groups, one of 5"),
        110: (31, 29, "63 triangles: mask bits up to 62, an odd count; grouped on z: 19 groups")}
FUZZ_GROUPS = {3: (1, [1, 1, 1, 3, 3, 3]), 6: (0, [1, 1, 1, 1, 1, 2, 2, 2]), 86: (1, [1] * 12 + [2, 3, 5]), 110: (2, [1] * 13 + [2, 2, 2, 3, 3, 4])}      # axis, group sizes


def fuzz_config(outdir, seed):
    from cudapathtracer_amd import scenes
    return scenes.fuzz(os.path.join(str(outdir), "boxes_fuzz%d" % seed), seed, name="boxes_fuzz%d" % seed)["config"]


def open_floor(outdir, w=32, h=24, spp=4, depth=8):
    """A floor, a light and two boxes standing apart, no walls: 28 triangles in 14 leaves with 14 distinct boxes (an even count), grouped on
    x: 7 groups of 1 to 4."""
    from cudapathtracer_amd import scenes
    rng = np.random.RandomState(0)
    zf = scenes._FRONT_Z
    zc, hh = zf - 1.25, 0.35
    floor = scenes.Mesh("floor", 2)
    floor.quad((-1.2, -1, zf), (1.2, -1, zf), (1.2, -1, zf - 2.5), (-1.2, -1, zf - 2.5), (0, 1, 0))
    light = scenes.Mesh("light", 2, 10.0, (1.0, 0.92, 0.8))
    light.quad((-hh, 0.995, zc - hh), (hh, 0.995, zc - hh), (hh, 0.995, zc + hh), (-hh, 0.995, zc + hh), (0, -1, 0))
    meshes = [floor, light]
    for k in range(2):
        b = scenes.Mesh("box%d" % k, (6, 23)[k])
        scenes._box(b, -0.8 + 1.6 * rng.rand(), zc - 0.8 + 1.6 * rng.rand(), 0.1 + 0.2 * rng.rand(), 0.3 + rng.rand(), 0.1 + 0.2 * rng.rand(), -1.0 + 1e-3,
                    90 * rng.rand())
        meshes.append(b)
    return scenes._emit(os.path.join(str(outdir), "boxes_open_floor"), "boxes_open_floor", meshes, w, h, spp, depth)["config"]


def pnodes_from_bvh(raw):
    """(PNode records, number of triangles) of the 48-byte reference nodes in `raw` (uint8)."""
    n = np.frombuffer(np.ascontiguousarray(raw).tobytes(), BVH)
    assert n[0]["count"] <= 0, "the root is a leaf: no internal node, no table"
    order, ids = [0], {0: 0}
    for node in order:                                            # (grows while it is walked: breadth-first)
        for c in (int(n[node]["left"]), int(n[node]["right"])):
            if n[c]["count"] <= 0:
                ids[c] = len(order)
                order.append(c)

    def below(c):
        return int(n[c]["count"]) if n[c]["count"] > 0 else below(int(n[c]["left"])) + below(int(n[c]["right"]))
    pn = np.zeros(len(order), PNODE)
    for k, node in enumerate(order):
        for side, c in (("l", int(n[node]["left"])), ("r", int(n[node]["right"]))):
            pn[k][side + "min"], pn[k][side + "max"] = n[c]["mn"][:3], n[c]["mx"][:3]
            pn[k]["left" if side == "l" else "right"] = ~int(n[c]["first"]) if n[c]["count"] > 0 else ids[c]
            pn[k]["pad0" if side == "l" else "pad1"] = below(c)
    return pn, below(0)


def chain(boxes, counts):
    """Node i: left child leaf i, right child node i + 1 (the last node: leaf i + 1). boxes: [(mn, mx)] per leaf, float32 triples."""
    assert len(boxes) == len(counts) >= 2
    m = len(boxes) - 1
    pn = np.zeros(m, PNODE)
    first = np.concatenate([[0], np.cumsum(counts)])
    mn = [np.asarray(b[0], np.float32) for b in boxes]
    mx = [np.asarray(b[1], np.float32) for b in boxes]
    umn, umx = mn[m], mx[m]                                       # the box of everything from leaf i + 1 on
    for i in range(m - 1, -1, -1):
        pn[i]["lmin"], pn[i]["lmax"], pn[i]["left"], pn[i]["pad0"] = mn[i], mx[i], ~int(first[i]), counts[i]
        pn[i]["rmin"], pn[i]["rmax"] = umn, umx
        pn[i]["right"] = ~int(first[m]) if i == m - 1 else i + 1
        pn[i]["pad1"] = int(first[-1] - first[i + 1])
        umn, umx = np.minimum(umn, mn[i]), np.maximum(umx, mx[i])
    return pn, int(first[-1])


def build_driver(outdir, sanitize=False):
    exe = os.path.join(str(outdir), "box_table_driver" + ("_san" if sanitize else ""))
    if not os.path.exists(exe):
        flags = ["--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "--cuda-host-only", "-I" + CSRC]
        if sanitize:
            flags += ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-fno-omit-frame-pointer"]
        subprocess.check_call(["hipcc"] + flags + ["-o", exe, DRIVER])
    return exe


def run_driver(exe, outdir, trees):
    """trees: {name: (PNode records, triangles)} -> {name: dict(nested, leaves [(first, count, box)], boxes [(mask, box)], axis,
    records [(mask, rotated box)], groups [(count, lo, hi)])}; box: 6 uint32, mn x y z then mx x y z."""
    args, names = [], []
    for name, (pn, nt) in trees.items():
        path = os.path.join(str(outdir), name + ".pnodes")
        np.ascontiguousarray(pn).tofile(path)
        args += [path, str(nt)]
        names.append(name)
    p = subprocess.run([exe] + args, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-3000:]
    out, cur = {}, None
    for ln in p.stdout.splitlines():
        w = ln.split()
        if w[0] == "tree":
            cur = dict(nodes=int(w[3]), nested=int(w[5]), n_leaves=int(w[7]), n_boxes=int(w[9]), leaves=[], boxes=[], axis=None, records=[], groups=[])
            out[names[len(out)]] = cur
        elif w[0] == "L":
            cur["leaves"].append((int(w[1]), int(w[2]), tuple(int(x, 16) for x in w[3:9])))
        elif w[0] == "B":
            cur["boxes"].append((int(w[1], 16), tuple(int(x, 16) for x in w[2:8])))
        elif w[0] == "groups":
            cur["axis"], cur["n_groups"] = int(w[2]), int(w[4])
        elif w[0] == "R":
            cur["records"].append((int(w[1], 16), tuple(int(x, 16) for x in w[2:8])))
        elif w[0] == "G":
            cur["groups"].append((int(w[1]), int(w[2], 16), int(w[3], 16)))
    assert len(out) == len(names)
    for r in out.values():
        assert len(r["leaves"]) == r["n_leaves"] and len(r["boxes"]) == r["n_boxes"] == len(r["records"]) and len(r["groups"]) == r["n_groups"]
    return out
