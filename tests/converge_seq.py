"""The frame sequences of the converge checks, and the sweep behind pt_converge_defaults' threshold.

tests/test_converge.py runs these sequences on the GPU. Run as a script, this file renders the same frames with the CPU reference
in oracle/ (they equal the GPU's bit for bit), runs the numpy restatements (tests/converge_ref.py, tests/temporal_ref.py) over
them and prints what DESIGN.md §14 records and what the GPU test expects:

    python tests/converge_seq.py [--cache DIR] [--sweep-converge]

1. QUALITY: the still sequence of tests/temporal_seq.py (128 x 128 Cornell, depth 8, 4 spp in 2 batches, seeds SEED0 + t) extended
   to N_FRAMES frames. min_history is 8, so frame 8 is the first whose select may stop a tile; 24 frames leave sixteen frames in
   which tiles are actually carried, twice the history a tile needs to stop, and stay a few seconds of CPU rendering. The error is
   the last frame's history + filter against REF_SPP samples, as in temporal_seq.
2. SESSION: the 64 x 48 Cornell (depth 4) sequence that the session test steps through, and the live count of each of its
   converging frames at SESSION_THRESHOLD."""
import os
import sys

import numpy as np

import temporal_seq as Q

N_FRAMES = 24
MIN_HISTORY = 8
SWEEP = (0.0, 0.04, 0.08, 0.12, 0.16, 0.20, 0.24, 0.28, 0.32, 0.40, 0.50, 0.65, 0.80, 1.0)

# the session test: frames 0..11 rest at the scene's camera, frame 12 moves to a pose of the moving sequence, 13 and 14 rest there
SW, SH, SDEPTH = 64, 48, 4
S_STILL, S_AFTER = 12, 2
S_MOVED_POSE = 2                  # of the moving sequence's poses, the first whose reprojection has no fragile decision here
SESSION_THRESHOLD = 0.5


def session_cameras(api, w=SW, h=SH):
    a, b = Q.camera(api, 0, False, w, h), Q.camera(api, S_MOVED_POSE, True, w, h)
    return [a] * S_STILL + [b] * (1 + S_AFTER)


def session_seeds():
    return [Q.SEED0 + t for t in range(S_STILL + 1 + S_AFTER)]


def run_converging(api_cams, frames, threshold, min_history=MIN_HISTORY, params=None):
    """The session's rule in numpy: a frame converges when a history exists and the camera's bytes equal the previous frame's.
    Returns (hist, hist_len, per-frame live counts, per-frame (tile_err, tile_live) or None)."""
    import converge_ref as C
    import temporal_ref as T
    params = T.DEFAULTS if params is None else params
    hist = ln = prev_n = prev_cam = None
    counts, maps = [], []
    for (S, Qm, A, N), cam in zip(frames, api_cams):
        h, w = S.shape[:2]
        total = ((h + 7) // 8) * ((w + 7) // 8)
        rests = threshold > 0 and hist is not None and prev_cam is not None and prev_cam.tobytes() == cam.tobytes()
        if rests:
            err, live, lst = C.select(hist, ln, threshold, min_history)
            S2, Q2 = C.moments_tiles(S, Qm, live)
            hist, ln = C.accumulate_live(cam, S2, Q2, Q.SPP, Q.BATCHES, A, N, prev_n, hist, ln, live, **params)
            counts.append(int(lst.size)); maps.append((err, live))
        else:
            hist, ln, _ = T.accumulate(cam, prev_cam, S, Qm, Q.SPP, Q.BATCHES, A, N, prev_n, hist, ln, **params)
            counts.append(total); maps.append(None)
        prev_n, prev_cam = N, cam
    return hist, ln, counts, maps


def pixel_samples_saved(counts, h, w, tile_counts=None):
    """Share of the tile-frames that were not rendered (tiles weigh the same here: a partial tile renders all 64 lanes)."""
    total = ((h + 7) // 8) * ((w + 7) // 8)
    return 1.0 - sum(counts) / float(total * len(counts))


def oracle_frames(api, O, cfg, cams, seeds, w, h, depth, cache=None, tag="seq", ref=None):
    """[(S, Q, A, N)] of the CPU reference for the given cameras and seeds, and optionally the REF_SPP reference of the last camera."""
    from denoise_ref import aovs_from_hits
    from denoise_var_ref import moments_from_partial_sums
    from test_aov import _oracle_hits
    key = os.path.join(cache, "converge_%s_%dx%d_%d.npz" % (tag, w, h, len(cams))) if cache else None
    if key and os.path.exists(key):
        z = np.load(key)
        return [tuple(z["f%d_%s" % (t, k)] for k in "SQAN") for t in range(len(cams))], (z["ref"] if "ref" in z else None)
    osc = O.OracleScene(cfg)
    frames = []
    c = Q.SPP // Q.BATCHES
    for cam, seed in zip(cams, seeds):
        cb = np.frombuffer(cam.tobytes(), np.uint8).copy()
        sums = [osc.render(camera=cb, width=w, height=h, spp=(j + 1) * c, max_depth=depth, integrator=0, seed=seed, threads=16)[0]
                for j in range(Q.BATCHES)]
        hits = [_oracle_hits(O, osc, cam, w, h, seed)]
        A, N = aovs_from_hits([(v, a, n, d) for v, _, a, n, d, _ in hits], 1)
        frames.append((sums[-1], moments_from_partial_sums(sums), A.reshape(h, w, 4), N.reshape(h, w, 4)))
    refsum = None
    if ref:
        cb = np.frombuffer(cams[-1].tobytes(), np.uint8).copy()
        refsum = osc.render(camera=cb, width=w, height=h, spp=Q.REF_SPP, max_depth=depth, integrator=0, seed=Q.REF_SEED, threads=16)[0]
    if key:
        os.makedirs(cache, exist_ok=True)
        extra = {"ref": refsum} if refsum is not None else {}
        np.savez(key, **extra, **{"f%d_%s" % (t, k): a for t, f in enumerate(frames) for k, a in zip("SQAN", f)})
    return frames, refsum


def quality(frames, ref, cams, threshold):
    """(errors dict of temporal_seq.errors, live counts) of the converging restatement at `threshold` (0: it never converges)."""
    import temporal_ref as T
    hist, ln, counts, _ = run_converging(cams, frames, threshold)
    S, Qm, A, N = frames[-1]
    filt, _, _ = T.denoise_hist(hist, A, N)
    return Q.errors(frames, ref, hist, filt), counts


def main(argv):
    import argparse
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    from cudapathtracer_amd import api, scenes
    from oracle import oracle_py as O
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=None, help="keep the rendered frames here")
    ap.add_argument("--sweep-converge", action="store_true")
    a = ap.parse_args(argv)
    O.build()
    tmp = tempfile.mkdtemp()
    # 1. quality
    cfg = scenes.cornell(tmp, width=Q.W, height=Q.H, spp=Q.SPP, max_depth=Q.DEPTH, name="cq")["config"]
    cams = [Q.camera(api, 0, False)] * N_FRAMES
    frames, ref = oracle_frames(api, O, cfg, cams, [Q.SEED0 + t for t in range(N_FRAMES)], Q.W, Q.H, Q.DEPTH, a.cache, "quality", ref=True)
    import converge_ref as C
    base, _ = quality(frames, ref, cams, 0.0)
    print("quality, %d still frames of %d x %d: raw mse %.5g; not converging: history + filter %.5g (ratio to raw %.4f)" % (
        N_FRAMES, Q.W, Q.H, base["raw"], base["hist_filter"], base["hist_filter"] / base["raw"]))
    rows = []
    for thr in (SWEEP if a.sweep_converge else (C.DEFAULTS["threshold"],)):
        m, counts = quality(frames, ref, cams, thr)
        rows.append((thr, m["hist_filter"], m["hist_filter"] / base["hist_filter"], m["hist_filter"] / base["raw"], counts[-1],
                     pixel_samples_saved(counts, Q.H, Q.W)))
        print("threshold %.3f: history + filter mse %.5g = %.4f x not converging (ratio to raw %.4f); live tiles on the last frame %d of %d; "
              "tile-frames saved %.1f %%" % (thr, m["hist_filter"], rows[-1][2], rows[-1][3], counts[-1], 256, 100 * rows[-1][5]), flush=True)
    if a.sweep_converge:
        ok = [r for r in rows if r[2] <= 1.10]
        print("the largest threshold within 10 %% of the non-converging error: %.3f" % max(r[0] for r in ok))
    # 2. the session test's sequence
    cfg = scenes.cornell(tmp, width=SW, height=SH, spp=Q.SPP, max_depth=SDEPTH, name="cs")["config"]
    cams = session_cameras(api)
    frames, _ = oracle_frames(api, O, cfg, cams, session_seeds(), SW, SH, SDEPTH, a.cache, "session")
    for thr in ((0.16, 0.20, 0.24, 0.28, 0.32, 0.40, 0.50, 0.65) if a.sweep_converge else (SESSION_THRESHOLD,)):
        _, _, counts, _ = run_converging(cams, frames, thr)
        print("session %d x %d, threshold %.3f, min_history %d: live counts per frame %s" % (SW, SH, thr, MIN_HISTORY, counts))
    import temporal_ref as T
    hh = ll = pn = pc = None
    for f, cam in zip(frames[:S_STILL + 1], cams):
        hh, ll, fr = T.accumulate(cam, pc, f[0], f[1], Q.SPP, Q.BATCHES, f[2], f[3], pn, hh, ll, **T.DEFAULTS)
        pn, pc = f[3], cam
    print("fragile pixels of the moved frame (non-converging history): %d" % int(fr.sum()))


if __name__ == "__main__":
    main(sys.argv[1:])
