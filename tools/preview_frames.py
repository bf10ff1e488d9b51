"""What the pt_preview session computes over its whole option matrix, as digests: for a change to the session that must change no frame.

    python tools/preview_frames.py --run OUT.json                          # one library (PT_LIB_PATH or the built one): write its record
    python tools/preview_frames.py --against OTHER.so --out-dir DIR [--summary FILE]
                                                                            # both libraries in fresh child processes, then compare
    python tools/preview_frames.py --compare A.json B.json [--summary FILE]

One session per combination of temporal {1, 0}, filter {1, 0}, scale {1, 2}, guide chain {0, 2}, centre guides {0, 1}, motion {0, 1},
respond {off, defaults} and converge {off, on}: 256 sessions at 40 x 24 on the Cornell scene of tests/motion_cases.py, 4 spp in 2
batches, depth 4. Converge is on with threshold 100 and min_history 2 (as tests/test_converge.py): a resting frame then renders only
the tiles that still hold a pixel the moving camera uncovered, and the next one none. Every
session runs: 3 frames of a moving camera, 2 of a resting one, a vertex update announced with keep_history 1 and a frame, a resting
frame, a frame with a camera of another size (it must fail), one more good frame. After every call the record holds the digests of
rgba8, mean, hist and hist_len where the session has them, guide_passes, last_live and stats()["frames"]; for the failed frame also
the error's code and text. --against runs the record once with OTHER.so (through PT_LIB_PATH) and once with the built library, each in
a fresh child process, and compares: every entry must be equal. Exit status 0: it is; 1: it is not; 3: a run did not finish."""
import argparse
import hashlib
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SPP, BATCHES, DEPTH = 4, 2, 4
OPTIONS = ("temporal", "filter", "scale", "chain", "centre", "motion", "respond", "converge")
VALUES = ((1, 0), (1, 0), (1, 2), (0, 2), (0, 1), (0, 1), (0, 1), (0, 1))
CHILD_TIMEOUT_S = 420


def _digest(a):
    return hashlib.sha256(a.tobytes()).hexdigest()[:16]


def _state(pv):
    out = {k: _digest(v) for k, v in pv.read().items()}
    out.update(guide_passes=pv.guide_passes, last_live=list(pv.last_live()), frames=pv.stats()["frames"])
    return out


def _session(api, MC, Q, host, moved, opt):
    W, H = MC.W, MC.H
    sc = api.Scene.from_mesh(host)
    pv = api.Preview(sc, W, H, spp=SPP, batches=BATCHES, max_depth=DEPTH, temporal=opt["temporal"], filter=opt["filter"])
    pv.set_scale(opt["scale"]).set_guide_chain(opt["chain"]).set_guide_centre(opt["centre"]).set_motion(opt["motion"])
    if opt["respond"]:
        pv.set_respond()
    if opt["converge"]:
        pv.set_converge(100.0, 2)
    rest = Q.camera(api, 2, True, W, H)
    steps = [("moving", Q.camera(api, t, True, W, H)) for t in range(3)] + [("resting", rest)] * 2
    steps += [("update", None), ("after_update", rest), ("resting", rest), ("wrong_size", Q.camera(api, 2, True, W + 8, H)), ("good", rest)]
    calls, seed = [], 100
    for what, cam in steps:
        entry = {"call": what}
        if what == "update":
            sc.update_vertices(moved)
            pv.scene_changed(True)
        else:
            seed += 1
            try:
                pv.frame(cam, seed)
            except api.PtError as e:
                entry["error"] = str(e)
            if (what == "wrong_size") != ("error" in entry):
                raise SystemExit("preview_frames: %s: the %s frame %s" % (opt, what, "did not fail" if what == "wrong_size" else "failed: " + entry["error"]))
        entry.update(_state(pv))
        calls.append(entry)
    pv.close(); sc.close()
    return calls


def run(out):
    import torch
    import motion_cases as MC
    import temporal_seq as Q
    from cudapathtracer_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("preview_frames.py needs a HIP device")
    torch.cuda.set_device(0)
    host = MC.cornell_host(api, tempfile.mkdtemp(), "preview_frames")
    moved = MC.moved_arrays(host)["points"]
    record = {}
    for n, values in enumerate(itertools.product(*VALUES)):
        opt = dict(zip(OPTIONS, values))
        record[" ".join("%s=%d" % kv for kv in opt.items())] = _session(api, MC, Q, host, moved, opt)
        if n % 32 == 31:
            print("%d sessions" % (n + 1), flush=True)
    with open(out, "w") as f:
        json.dump({"library": api.LIB_PATH, "sessions": record}, f, indent=0)


def compare(a, b, summary):
    A, B = (json.load(open(p))["sessions"] for p in (a, b))
    mismatches, entries = [], 0
    if sorted(A) != sorted(B):
        mismatches.append("the two records hold different sessions")
    for key in sorted(set(A) & set(B)):
        if len(A[key]) != len(B[key]):
            mismatches.append("%s: %d and %d calls" % (key, len(A[key]), len(B[key])))
        for t, (x, y) in enumerate(zip(A[key], B[key])):
            for k in sorted(set(x) | set(y)):
                entries += 1
                if x.get(k) != y.get(k):
                    mismatches.append("%s call %d (%s) %s: %r and %r" % (key, t, x["call"], k, x.get(k), y.get(k)))
    res = {"size": [40, 24], "spp": SPP, "batches": BATCHES, "max_depth": DEPTH, "sessions": len(A), "calls_per_session": len(next(iter(A.values()))),
           "frames": sum(1 for s in A.values() for c in s if c["call"] != "update"), "entries_compared": entries, "mismatches": len(mismatches)}
    for m in mismatches[:40]:
        print(m)
    print(json.dumps(res))
    if summary:
        with open(summary, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 1 if mismatches else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run")
    ap.add_argument("--against")
    ap.add_argument("--out-dir")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--summary")
    a = ap.parse_args()
    if a.run:
        return run(a.run)
    if a.compare:
        return compare(a.compare[0], a.compare[1], a.summary)
    if not (a.against and a.out_dir):
        ap.error("one of --run, --compare, or --against with --out-dir")
    os.makedirs(a.out_dir, exist_ok=True)
    outs = []
    for name, lib in (("other", os.path.abspath(a.against)), ("built", None)):
        env = dict(os.environ)
        env.pop("PT_LIB_PATH", None)
        if lib:
            env["PT_LIB_PATH"] = lib
        outs.append(os.path.join(a.out_dir, "preview_frames_%s.json" % name))
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--run", outs[-1]], env=env, timeout=CHILD_TIMEOUT_S).returncode
        except subprocess.TimeoutExpired:
            rc = "its time limit"
        if rc != 0:                                           # nothing more starts on the device after a failed run
            print("preview_frames: the run with the %s library ended with %s" % (name, rc), file=sys.stderr)
            return 3
    return compare(outs[0], outs[1], a.summary)


if __name__ == "__main__":
    sys.exit(main())
