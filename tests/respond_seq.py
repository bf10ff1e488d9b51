"""The frame sequences of the responsive-history quality checks, and the sweep behind pt_respond_defaults.

A CHANGED-SCENE sequence is N_FRAMES frames of a 64 x 64 Cornell box (depth 6, MIS) from a resting camera, SPP samples each in
BATCHES batches, seeds SEED0 + t, centre guides; before frame CHANGE the geometry changes once ("box": the tall box, vertices 48..71,
moves by (0.25, 0, 0.15); "light": the light quad, vertices 20..23, moves by (0.3, 0, 0)). The reference of a frame is REF_SPP samples
(REF_SEED) of its own geometry. The error is DESIGN §19's relMSE, mean of (x - ref)^2 / (ref^2 + 0.01), of history + pt_denoise_hist,
divided by the raw frame's; over the whole frame, and over the CHANGED pixels: static pixels (the same centre guide before and
after) whose reference luminance changed by more than a quarter of the old one.

tests/test_respond.py renders the sequences on the GPU. Run as a script, this file renders them with the CPU reference in oracle/
(the frames equal the GPU's bit for bit), runs the numpy restatement (tests/respond_ref.py) and prints the tables of DESIGN.md §20;
with --sweep also the grid over radius, power and threshold on these two sequences and on the two unchanged 8-frame sequences of
tests/temporal_centre_seq.py (still camera; moving camera, nothing changing), and the pick of §11's selection rule.

    python tests/respond_seq.py [--cache DIR] [--sweep]"""
import os
import sys

import numpy as np

W = H = 64
N_FRAMES, CHANGE = 14, 7
SPP, BATCHES, DEPTH = 4, 2, 6
SEED0 = 2000
REF_SPP, REF_SEED = 1024, 777
EXPERIMENTS = {"box": (48, 72, (0.25, 0.0, 0.15)), "light": (20, 24, (0.3, 0.0, 0.0))}
LUMA = np.array([0.2126, 0.7152, 0.0722])
RADII, POWERS, THRESHOLDS = (1, 2, 3), (1, 2, 4), (1.5, 2.0, 3.0, 4.0, 6.0)
# The restatement's ratios (changed pixels, history + filter over raw) on frames 7..13 at the library's defaults, as this script
# prints them: what tests/test_respond.py holds the library to.
RECORDED = {"box": (0.0991, 0.1841, 0.1066, 0.1224, 0.1096, 0.0731, 0.0788), "light": (0.3336, 0.2719, 0.2942, 0.2189, 0.1228, 0.1644, 0.1371)}


def host(api, scene_dir, name="respond_seq"):
    from cudapathtracer_amd import scenes
    cfg = scenes.cornell(os.path.join(scene_dir, name), width=W, height=H, name=name, spp=SPP, max_depth=DEPTH)["config"]
    hs = api.HostScene(cfg)
    assert hs.info["n_tris"] == 36 and hs.info["n_points"] == 72
    return hs


def camera(api):
    import temporal_seq as Q
    return Q.camera(api, 0, False, W, H)


def relmse(x, ref, mask):
    x = np.asarray(x, np.float64)[..., :3]; ref = np.asarray(ref, np.float64)[..., :3]
    err = ((x - ref) ** 2 / (ref ** 2 + 1e-2)).mean(-1)
    ok = mask & np.isfinite(err)
    return float(err[ok].mean())


def changed_mask(ref_old, ref_new, guide_old, guide_new):
    """Static pixels (the centre guides' bits agree before and after) whose reference luminance changed by more than a quarter."""
    static = (guide_old[0].view(np.uint32) == guide_new[0].view(np.uint32)).all(-1) & (guide_old[1].view(np.uint32) == guide_new[1].view(np.uint32)).all(-1)
    lo, ln = ref_old[..., :3].astype(np.float64) @ LUMA, ref_new[..., :3].astype(np.float64) @ LUMA
    return static & (np.abs(ln - lo) > 0.25 * lo)


def run(seq, cam, accumulate, filt, respond, keep=True):
    """The sequence through a history stage and the history filter. accumulate(cam, S, Q, A, N, prev_n, hist, ln, respond) ->
    (hist, ln, lambda or None), filt(hist, A, N) -> the filtered mean [h,w,>=3]. respond None: the base function. keep False: the
    history is dropped at the change. Returns per frame (filtered mean, lambda or None)."""
    out = []
    hist = ln = prev_n = None
    for t, (S, Qs, A, N) in enumerate(seq["frames"]):
        if t == CHANGE and not keep:
            hist = ln = prev_n = None
        hist, ln, lam = accumulate(cam, S, Qs, A, N, prev_n, hist, ln, respond)
        prev_n = N
        out.append((filt(hist, A, N), lam))
    return out


def ratios(seq, result):
    """Per frame: (changed-pixel error ratio to the raw frame's, whole-frame ratio, share of pixels with lambda < 1)."""
    rows = []
    every = np.ones((H, W), bool)
    for t, ((S, _, _, _), (mean, lam)) in enumerate(zip(seq["frames"], result)):
        ref = seq["ref"][t >= CHANGE] / np.float32(REF_SPP)
        raw = S / np.float32(SPP)
        ch = seq["changed"]
        rows.append((relmse(mean, ref, ch) / relmse(raw, ref, ch), relmse(mean, ref, every) / relmse(raw, ref, every),
                     float((lam < 1).mean()) if lam is not None else 0.0))
    return rows


# ---- the restatement as run()'s stages ---------------------------------------------------------------------------------------------
def ref_accumulate(cam, S, Qs, A, N, prev_n, hist, ln, respond):
    import respond_ref as R
    import temporal_ref as T
    if respond is None or hist is None:
        h, l, _ = T.accumulate(cam, None, S, Qs, SPP, BATCHES, A, N, prev_n, hist, ln, **T.DEFAULTS)
        return h, l, None
    h, l, lam, _ = R.accumulate(cam, None, S, Qs, SPP, BATCHES, A, N, prev_n, hist, ln, **T.DEFAULTS, **respond)
    return h, l, lam


def ref_filter(hist, A, N):
    import temporal_ref as T
    return T.denoise_hist(hist, A, N)[0]


# ---- the CPU side: frames from the reference implementation in oracle/ -------------------------------------------------------------
def oracle_sequence(api, O, hs, which, cache=None):
    import motion_cases as MC
    from denoise_var_ref import moments_from_partial_sums
    key = os.path.join(cache, "respond_%s.npz" % which) if cache else None
    if key and os.path.exists(key):
        z = np.load(key)
        seq = {"frames": [tuple(z["f%d_%s" % (t, k)] for k in "SQAN") for t in range(N_FRAMES)], "ref": (z["ref0"], z["ref1"])}
    else:
        first, last, shift = EXPERIMENTS[which]
        cam = camera(api)
        cb = np.frombuffer(cam.tobytes(), np.uint8).copy()
        leaf = hs.info["leaf_size"]
        geo = [MC.oracle_scene(O, MC.arrays(hs), leaf), MC.oracle_scene(O, MC.moved_arrays(hs, first, last, shift), leaf)]
        guides = [MC.oracle_centre_hits(O, g, cam, W, H)[1:] for g in geo]
        frames = []
        for t in range(N_FRAMES):
            g = geo[t >= CHANGE]
            c = SPP // BATCHES
            sums = [g.render(camera=cb, width=W, height=H, spp=(j + 1) * c, max_depth=DEPTH, integrator=0, seed=SEED0 + t, threads=16)[0]
                    for j in range(BATCHES)]
            frames.append((sums[-1], moments_from_partial_sums(sums), *guides[t >= CHANGE]))
        ref = tuple(g.render(camera=cb, width=W, height=H, spp=REF_SPP, max_depth=DEPTH, integrator=0, seed=REF_SEED, threads=16)[0] for g in geo)
        seq = {"frames": frames, "ref": ref}
        if key:
            os.makedirs(cache, exist_ok=True)
            np.savez(key, ref0=ref[0], ref1=ref[1], **{"f%d_%s" % (t, k): a for t, f in enumerate(frames) for k, a in zip("SQAN", f)})
    seq["changed"] = changed_mask(seq["ref"][0], seq["ref"][1], seq["frames"][0][2:], seq["frames"][-1][2:])
    return seq


def unchanged_ratio(api, Q, frames, ref, moving, respond):
    """History + filter over raw on the last frame of one of temporal_centre_seq's sequences, and the share of lambda < 1 over its
    frames with a history."""
    import respond_ref as R
    import temporal_ref as T
    hist = ln = prev_n = prev_cam = None
    short = []
    for t, (S, Qs, A, N) in enumerate(frames):
        cam = Q.camera(api, t, moving)
        if respond is None or hist is None:
            hist, ln, _ = T.accumulate(cam, prev_cam, S, Qs, Q.SPP, Q.BATCHES, A, N, prev_n, hist, ln, **T.DEFAULTS)
        else:
            hist, ln, lam, _ = R.accumulate(cam, prev_cam, S, Qs, Q.SPP, Q.BATCHES, A, N, prev_n, hist, ln, **T.DEFAULTS, **respond)
            short.append(float((lam < 1).mean()))
        prev_n, prev_cam = N, cam
    S, Qs, A, N = frames[-1]
    m = Q.errors(frames, ref, hist, T.denoise_hist(hist, A, N)[0])
    return m["hist_filter"] / m["raw"], (float(np.mean(short)) if short else 0.0)


def main(argv):
    import argparse
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    import respond_ref as R
    import temporal_centre_seq as CS
    import temporal_seq as Q
    from cudapathtracer_amd import api, scenes
    from oracle import oracle_py as O
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=None, help="keep the rendered frames here")
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args(argv)
    O.build()
    hs = host(api, tempfile.mkdtemp())
    cam = camera(api)
    seqs = {w: oracle_sequence(api, O, hs, w, a.cache) for w in EXPERIMENTS}
    defaults = api.respond_defaults()
    shown = (7, 8, 9, 13)
    for which, seq in seqs.items():
        print("%s: changed pixels %.1f %% of the frame" % (which, 100 * seq["changed"].mean()))
        print("   (history + filter over the raw frame, relMSE)  changed pixels at frame %s | whole frame 7 | whole frame 13 | sum 7..13" % (shown,))
        base = None
        for name, respond, keep in (("keep_history 1, respond off", None, True), ("keep_history 0", None, False),
                                    ("respond r %(radius)d k %(threshold)g power %(power)d" % defaults, defaults, True)):
            r = ratios(seq, run(seq, cam, ref_accumulate, ref_filter, respond, keep))
            print("   %-32s %s | %.3f | %.3f | %.3f" % (name, "  ".join("%.3f" % r[t][0] for t in shown), r[7][1], r[13][1], sum(x[0] for x in r[CHANGE:])))
            if respond is None and keep:
                base = r
            if respond is not None:
                print("   static frames 1..6: whole-frame ratio respond on / off %s; share of lambda < 1: %.3f %%" % (
                    "  ".join("%.4f" % (r[t][1] / base[t][1]) for t in range(1, CHANGE)), 100 * np.mean([r[t][2] for t in range(1, CHANGE)])))
                print("   share of lambda < 1 at frames 7..13: %s" % "  ".join("%.3f" % r[t][2] for t in range(CHANGE, N_FRAMES)))
                print("   RECORDED[%r] = (%s)" % (which, ", ".join("%.4f" % r[t][0] for t in range(CHANGE, N_FRAMES))))
    cfg = scenes.cornell(tempfile.mkdtemp(), width=Q.W, height=Q.H, spp=Q.SPP, max_depth=Q.DEPTH, name="tq")["config"]
    osc = O.OracleScene(cfg)
    un = {}
    for mv in (False, True):
        jit, ref = Q._oracle_frames(api, O, cfg, mv, 1, a.cache)
        un[mv] = (CS.centre_frames(api, O, osc, jit, mv), ref)
    off = {mv: unchanged_ratio(api, Q, *un[mv], mv, None)[0] for mv in un}
    on = {mv: unchanged_ratio(api, Q, *un[mv], mv, defaults) for mv in un}
    for mv in un:
        print("unchanged, %s camera: history + filter over raw: respond off %.4f, on %.4f (%.3f x); share of lambda < 1: %.3f %%" % (
            "moving" if mv else "still", off[mv], on[mv][0], on[mv][0] / off[mv], 100 * on[mv][1]))
    if not a.sweep:
        return
    print("radius power threshold | still: ratio to off, share | moving: ratio to off, share | changed 7..13: box, light, sum")
    rows = []
    for rad in RADII:
        for pw in POWERS:
            for k in THRESHOLDS:
                p = {"radius": rad, "power": pw, "threshold": k}
                u = {mv: unchanged_ratio(api, Q, *un[mv], mv, p) for mv in un}
                ch = {w: sum(x[0] for x in ratios(s, run(s, cam, ref_accumulate, ref_filter, p))[CHANGE:]) for w, s in seqs.items()}
                rows.append((rad, pw, k, u[False][0] / off[False], u[False][1], u[True][0] / off[True], u[True][1], ch["box"], ch["light"],
                             ch["box"] + ch["light"]))
                print("%d %d %.1f | %.4f %.4f | %.4f %.4f | %.3f %.3f %.3f" % rows[-1], flush=True)
    for label, ok in (("both unchanged sequences", [r for r in rows if r[3] <= 1.1 and r[5] <= 1.1]),
                      ("the still sequence alone", [r for r in rows if r[3] <= 1.1])):
        if not ok:
            print("no setting stays within 10 %% of respond-off on %s" % label)
            continue
        pick = min(ok, key=lambda r: (round(r[9], 3), r[0], -r[2]))
        print("within 10 %% on %s: %d settings; the smallest changed-pixel sum is at radius %d power %d threshold %.1f: %.3f" % (
            label, len(ok), pick[0], pick[1], pick[2], pick[9]))


if __name__ == "__main__":
    main(sys.argv[1:])
