"""The frame sequences of the temporal-accumulation quality checks, and the sweep behind the library's defaults.

tests/test_temporal.py renders these sequences on the GPU. Run as a script, this file renders the same frames with the CPU
reference in oracle/ (they equal the GPU's bit for bit), runs the numpy restatement (tests/temporal_ref.py) over them and prints
the tables of DESIGN.md §11: the restatement's error ratios, which the GPU test holds the kernels to, and the parameter sweep.

    python tests/temporal_seq.py [--cache DIR] [--sweep]

A sequence is N_FRAMES frames of a 128 x 128 Cornell box (depth 8, MIS), SPP samples each in BATCHES batches, beauty and feature
buffers seeded SEED0 + t; the error is measured on the last frame against REF_SPP samples with another seed."""
import os
import sys

import numpy as np

W = H = 128
N_FRAMES = 8
SPP, BATCHES, DEPTH = 4, 2, 8
SEED0 = 2000
REF_SPP, REF_SEED = 2048, 777
FOV = 60.0


def camera_pose(t, moving):
    """Position and rotation (degrees) of frame t: the scene's own camera, or a drift of 0.03 / 0.01 units and 0.8 degrees of yaw
    per frame."""
    if not moving:
        return (0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
    return (0.03 * t, 0.01 * t, 1.0), (0.0, 0.8 * t, 0.0)


def camera(api, t, moving, w=W, h=H):
    pos, rot = camera_pose(t, moving)
    return api.make_camera(True, pos, rot, FOV, w, h)


def run_restatement(frames, cams, params, iterations=None):
    """The history after the last frame and its filtered mean, by tests/temporal_ref.py. frames: list of (S, Q, A, N)."""
    import temporal_ref as T
    hist = ln = prev_n = prev_cam = None
    for (S, Q, A, N), cam in zip(frames, cams):
        hist, ln, _ = T.accumulate(cam, prev_cam, S, Q, SPP, BATCHES, A, N, prev_n, hist, ln, **params)
        prev_n, prev_cam = N, cam
    S, Q, A, N = frames[-1]
    kw = {} if iterations is None else {"iterations": iterations}
    filt, _, _ = T.denoise_hist(hist, A, N, **kw)
    return hist, ln, filt


def errors(frames, ref_sum, hist, filt):
    """MSE against the reference mean of: the raw last frame, pt_denoise_var on it alone (restated), the history, history + filter."""
    import temporal_ref as T
    from denoise_ref import mse, passthrough_mask
    from denoise_var_ref import demod_albedo, denoise_var
    S, Q, A, N = frames[-1]
    mask = ~passthrough_mask(S, SPP, A) & ~passthrough_mask(ref_sum, REF_SPP, A) & ~T.hist_passthrough(hist)
    refm = ref_sum / np.float32(REF_SPP)
    var = denoise_var(S, Q, SPP, BATCHES, A, N)[0] / SPP
    mean_hist = hist.astype(np.float64).copy()
    mean_hist[..., :3] *= demod_albedo(A)
    return {"raw": mse(S / np.float32(SPP), refm, mask), "var": mse(var, refm, mask), "hist": mse(mean_hist, refm, mask),
            "hist_filter": mse(filt, refm, mask)}


# ---- the CPU side: frames from the reference implementation in oracle/ ----------------------------------------------------------
def _oracle_frames(api, O, cfg, moving, aov_spp, cache):
    from denoise_ref import aovs_from_hits
    from denoise_var_ref import moments_from_partial_sums
    from test_aov import _oracle_hits
    key = os.path.join(cache, "seq_%s_aov%d.npz" % ("moving" if moving else "still", aov_spp)) if cache else None
    if key and os.path.exists(key):
        z = np.load(key)
        return [tuple(z["f%d_%s" % (t, k)] for k in "SQAN") for t in range(N_FRAMES)], z["ref"]
    osc = O.OracleScene(cfg)
    frames = []
    for t in range(N_FRAMES):
        cam = camera(api, t, moving)
        cb = np.frombuffer(cam.tobytes(), np.uint8).copy()
        c = SPP // BATCHES
        sums = [osc.render(camera=cb, width=W, height=H, spp=(j + 1) * c, max_depth=DEPTH, integrator=0, seed=SEED0 + t, threads=16)[0]
                for j in range(BATCHES)]
        hits = [_oracle_hits(O, osc, cam, W, H, SEED0 + t + k) for k in range(aov_spp)]
        A, N = aovs_from_hits([(v, a, n, d) for v, _, a, n, d, _ in hits], aov_spp)
        frames.append((sums[-1], moments_from_partial_sums(sums), A.reshape(H, W, 4), N.reshape(H, W, 4)))
    cb = np.frombuffer(camera(api, N_FRAMES - 1, moving).tobytes(), np.uint8).copy()
    ref = osc.render(camera=cb, width=W, height=H, spp=REF_SPP, max_depth=DEPTH, integrator=0, seed=REF_SEED, threads=16)[0]
    if key:
        os.makedirs(cache, exist_ok=True)
        np.savez(key, ref=ref, **{"f%d_%s" % (t, k): a for t, f in enumerate(frames) for k, a in zip("SQAN", f)})
    return frames, ref


def main(argv):
    import argparse
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    import temporal_ref as T
    from cudapathtracer_amd import api, scenes
    from oracle import oracle_py as O
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=None, help="keep the rendered frames here")
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args(argv)
    O.build()
    cfg = scenes.cornell(tempfile.mkdtemp(), width=W, height=H, spp=SPP, max_depth=DEPTH, name="tq")["config"]
    data = {(mv, k): _oracle_frames(api, O, cfg, mv, k, a.cache) for mv in (False, True) for k in ((1, 4) if a.sweep else (1,))}
    for mv in (False, True):
        frames, ref = data[(mv, 1)]
        cams = [camera(api, t, mv) for t in range(N_FRAMES)]
        hist, ln, filt = run_restatement(frames, cams, T.DEFAULTS)
        m = errors(frames, ref, hist, filt)
        frag = []
        hh = ll = pn = pc = None
        for f, cam in zip(frames, cams):
            hh, ll, fr = T.accumulate(cam, pc, f[0], f[1], SPP, BATCHES, f[2], f[3], pn, hh, ll, **T.DEFAULTS)
            pn, pc = f[3], cam
            frag.append(fr.mean())
        print("%s: mse raw %.5g; ratios to raw: denoise_var alone %.4f, history %.4f, history + filter %.4f; mean length %.2f; "
              "fragile share max %.4f %%" % ("moving" if mv else "still", m["raw"], m["var"] / m["raw"], m["hist"] / m["raw"],
                                             m["hist_filter"] / m["raw"], ln.mean(), 100 * max(frag)))
    if not a.sweep:
        return
    print("aov_spp depth_tol normal_tol max_history | still: hist hist+filter | moving: hist hist+filter   (ratios to raw)")
    rows = []
    for k in (1, 4):
        for dt in (0.02, 0.05, 0.1, 0.2):
            for nt in (0.8, 0.9, 0.99):
                for mh in (4, 8, 16, 32, 64):
                    r = []
                    for mv in (False, True):
                        frames, ref = data[(mv, k)]
                        cams = [camera(api, t, mv) for t in range(N_FRAMES)]
                        hist, ln, filt = run_restatement(frames, cams, {"max_history": mh, "depth_tol": dt, "normal_tol": nt})
                        m = errors(frames, ref, hist, filt)
                        r += [m["hist"] / m["raw"], m["hist_filter"] / m["raw"]]
                    rows.append((k, dt, nt, mh, *r))
                    print("%d %.2f %.2f %2d | %.4f %.4f | %.4f %.4f" % rows[-1], flush=True)
    for k in (1, 4):
        mine = [r for r in rows if r[0] == k]
        best_still = min(r[5] for r in mine)
        ok = [r for r in mine if r[5] <= 1.1 * best_still]
        pick = min(ok, key=lambda r: r[7])
        print("aov_spp %d: best still history + filter %.4f; among settings within 10 %% of it the smallest moving error is at "
              "depth_tol %.2f normal_tol %.2f max_history %d: still %.4f, moving %.4f" % (k, best_still, pick[1], pick[2], pick[3], pick[5], pick[7]))


if __name__ == "__main__":
    main(sys.argv[1:])
