"""What pixel-centre guides do to the preview stack's error: the sequences of tests/temporal_seq.py with each frame's feature
buffers traced through pixel centres (pt_render_aovs_centre's ray: the oracle's camera_ray of the camera with jitter and aperture
0) in place of the jittered ray.

tests/test_temporal_centre.py renders both kinds of sequence on the GPU. Run as a script, this file takes temporal_seq's CPU
reference frames (and its cache), replaces their (A, N) by the oracle's hits along the centre rays, runs the numpy restatement
(tests/temporal_ref.py) over both and prints the tables of DESIGN.md §17: the restatement's error ratios, which the GPU test holds
the library to, and the depth_tol sweep.

    python tests/temporal_centre_seq.py [--cache DIR]"""
import os
import sys

import numpy as np

import temporal_seq as Q

DEPTH_TOLS = (0.10, 0.03, 0.01)


def cam0(cam):
    """The camera with antiAliasJitterDist = 0 and aperture = 0."""
    from cudapathtracer_amd import api
    c = api.Camera.frombytes(cam.tobytes())
    c.antiAliasJitterDist = 0.0
    c.aperture = 0.0
    return c


def centre_frames(api, O, osc, frames, moving):
    """frames with each (A, N) replaced by the first-hit buffers along the centre rays (aov_spp 1: the hit itself)."""
    from denoise_ref import aovs_from_hits
    from test_aov import _oracle_hits
    out = []
    for t, (S, Qs, _, _) in enumerate(frames):
        v, _, a, n, d, _ = _oracle_hits(O, osc, cam0(Q.camera(api, t, moving)), Q.W, Q.H, 0)
        A, N = aovs_from_hits([(v, a, n, d)], 1)
        out.append((S, Qs, A.reshape(Q.H, Q.W, 4), N.reshape(Q.H, Q.W, 4)))
    return out


def measure(api, frames, ref, moving, params):
    """Q.errors' ratios to the raw last frame, and the mean history length, of the restatement over `frames`."""
    cams = [Q.camera(api, t, moving) for t in range(Q.N_FRAMES)]
    hist, ln, filt = Q.run_restatement(frames, cams, params)
    m = Q.errors(frames, ref, hist, filt)
    return {"var": m["var"] / m["raw"], "hist": m["hist"] / m["raw"], "hist_filter": m["hist_filter"] / m["raw"], "len": float(ln.mean())}


def main(argv):
    import argparse
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    import temporal_ref as T
    from cudapathtracer_amd import api, scenes
    from oracle import oracle_py as O
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=None, help="temporal_seq.py's cache of rendered frames")
    a = ap.parse_args(argv)
    O.build()
    cfg = scenes.cornell(tempfile.mkdtemp(), width=Q.W, height=Q.H, spp=Q.SPP, max_depth=Q.DEPTH, name="tq")["config"]
    osc = O.OracleScene(cfg)
    print("ratios to the raw last frame's MSE: pt_denoise_var alone | history | history + filter | mean history length")
    for mv in (False, True):
        name = "moving" if mv else "still"
        jit, ref = Q._oracle_frames(api, O, cfg, mv, 1, a.cache)
        cen = centre_frames(api, O, osc, jit, mv)
        rows = {}
        for kind, frames in (("jittered", jit), ("centre", cen)):
            for dt in DEPTH_TOLS:
                r = rows[(kind, dt)] = measure(api, frames, ref, mv, dict(T.DEFAULTS, depth_tol=dt))
                print("%s, %s guide, depth_tol %.2f: %.4f | %.4f | %.4f | %.2f" % (name, kind, dt, r["var"], r["hist"], r["hist_filter"], r["len"]),
                      flush=True)
        d = T.DEFAULTS["depth_tol"]
        print("%s: centre / jittered, history + filter at the default depth_tol %.2f: %.3f" % (
            name, d, rows[("centre", d)]["hist_filter"] / rows[("jittered", d)]["hist_filter"]))


if __name__ == "__main__":
    main(sys.argv[1:])
