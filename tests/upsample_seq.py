"""The frames of the render scale's quality check, its error measures, and the sweep behind pt_upsample's defaults.

tests/test_upsample.py renders these frames on the GPU. Run as a script, this file renders the same frames with the CPU reference
in oracle/ (they equal the GPU's bit for bit), runs the numpy restatement (tests/upsample_ref.py, tests/temporal_ref.py) over them
and prints the tables of DESIGN.md §13: the restatement's errors, which the GPU test holds the kernels to, and the parameter sweep.

    python tests/upsample_seq.py [--cache DIR] [--sweep]

A 128 x 128 Cornell box (depth 8, MIS) from the scene's own camera: SPP samples in BATCHES batches at 1 / s of the size in each
axis, feature buffers at both sizes, all seeded SEED; the error is measured against REF_SPP samples at full size with another
seed, over all pixels and over those more than 4 pixels from the emitter (the reference pixels whose mean exceeds 2, dilated 4
times): a low-res pixel that straddles the light's silhouette holds a mixture that depth and normal cannot separate."""
import os
import sys

import numpy as np

W = H = 128
SPP, BATCHES, DEPTH = 4, 2, 8
SEED = 2000
REF_SPP, REF_SEED = 1024, 777
SCALES = (2, 4)
ITERATIONS = 3
SWEEP = [(sn, sd) for sd in (0.02, 0.05, 0.10) for sn in (64.0, 16.0)]


def camera(api, w=W, h=H):
    import temporal_seq as Q
    return Q.camera(api, 0, False, w, h)


def nearest(rgba_sum_lo, s):
    """The low-res mean, every pixel replicated s x s times."""
    m = (np.asarray(rgba_sum_lo, np.float32) / np.float32(SPP)).astype(np.float32)
    return np.repeat(np.repeat(m, s, 0), s, 1)


def far_from_emitter(ref_mean):
    """Pixels more than 4 pixels (3 x 3 dilations) from a reference pixel whose mean over rgb exceeds 2."""
    near = ref_mean[..., :3].mean(-1) > 2
    for _ in range(4):
        p = np.pad(near, 1)
        near = np.logical_or.reduce([p[1 + dy:p.shape[0] - 1 + dy, 1 + dx:p.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    return ~near


def errors(s, lo, guides, ref_sum, upsample, denoise_hist, **params):
    """MSE against the reference mean, over all pixels and far from the emitter, of: nearest replication, the upsampled frame, the
    upsampled frame after ITERATIONS iterations of the history filter. lo = (S, Q, albedo_lo, normal_depth_lo), guides = (albedo,
    normal_depth); upsample and denoise_hist are the library's functions or the restatement's."""
    from denoise_ref import mse
    ref = (np.asarray(ref_sum, np.float32) / np.float32(REF_SPP)).astype(np.float32)
    everywhere = np.isfinite(ref[..., :3]).all(-1)
    far = everywhere & far_from_emitter(ref)
    cur = upsample(s, lo[0], lo[1], SPP, BATCHES, lo[2], lo[3], guides[0], guides[1], **params)
    cur = cur[0] if isinstance(cur, tuple) else cur
    images = {"nearest": nearest(lo[0], s)}
    for name, it in (("up", 0), ("up_filter", ITERATIONS)):
        out = denoise_hist(cur, guides[0], guides[1], iterations=it)
        images[name] = np.asarray(out[0] if isinstance(out, tuple) else out)
    res = {}
    for name, img in images.items():
        res[name] = mse(img, ref, everywhere); res[name + "_far"] = mse(img, ref, far)
    res["pass_share"] = float((cur[..., 3] < 0).mean())
    return res


def full_res_errors(full, guides, ref_sum):
    """The full-resolution frame next to it (restated): raw SPP samples, and pt_denoise_var on them."""
    from denoise_ref import mse
    from denoise_var_ref import denoise_var
    ref = (np.asarray(ref_sum, np.float32) / np.float32(REF_SPP)).astype(np.float32)
    everywhere = np.isfinite(ref[..., :3]).all(-1)
    far = everywhere & far_from_emitter(ref)
    raw = full[0] / np.float32(SPP)
    var = denoise_var(full[0], full[1], SPP, BATCHES, guides[0], guides[1])[0] / SPP
    return {"raw": mse(raw, ref, everywhere), "raw_far": mse(raw, ref, far), "var": mse(var, ref, everywhere), "var_far": mse(var, ref, far)}


# ---- the CPU side: frames from the reference implementation in oracle/ ----------------------------------------------------------
def _oracle_frame(api, O, osc, s):
    """(S, Q, albedo, normal_depth) of the camera scaled by s, as pt_render_moments and pt_render_aovs(aov_spp = 1) write them."""
    from denoise_ref import aovs_from_hits
    from denoise_var_ref import moments_from_partial_sums
    from test_aov import _oracle_hits
    cam = api.scaled_camera(camera(api), s)
    w, h = W // s, H // s
    cb = np.frombuffer(cam.tobytes(), np.uint8).copy()
    c = SPP // BATCHES
    sums = [osc.render(camera=cb, width=w, height=h, spp=(j + 1) * c, max_depth=DEPTH, integrator=0, seed=SEED, threads=16)[0] for j in range(BATCHES)]
    v, _, a, n, d, _ = _oracle_hits(O, osc, cam, w, h, SEED)
    A, N = aovs_from_hits([(v, a, n, d)], 1)
    return sums[-1], moments_from_partial_sums(sums), A.reshape(h, w, 4), N.reshape(h, w, 4)


def oracle_data(api, O, cfg, cache=None):
    key = os.path.join(cache, "upsample_seq.npz") if cache else None
    if key and os.path.exists(key):
        z = np.load(key)
        return {s: tuple(z["s%d_%s" % (s, k)] for k in "SQAN") for s in (1,) + SCALES}, z["ref"]
    osc = O.OracleScene(cfg)
    frames = {s: _oracle_frame(api, O, osc, s) for s in (1,) + SCALES}
    cb = np.frombuffer(camera(api).tobytes(), np.uint8).copy()
    ref = osc.render(camera=cb, width=W, height=H, spp=REF_SPP, max_depth=DEPTH, integrator=0, seed=REF_SEED, threads=16)[0]
    if key:
        os.makedirs(cache, exist_ok=True)
        np.savez(key, ref=ref, **{"s%d_%s" % (s, k): a for s, f in frames.items() for k, a in zip("SQAN", f)})
    return frames, ref


def main(argv):
    import argparse
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    import temporal_ref as T
    import upsample_ref as U
    from cudapathtracer_amd import api, scenes
    from oracle import oracle_py as O
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=None, help="keep the rendered frames here")
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args(argv)
    O.build()
    cfg = scenes.cornell(tempfile.mkdtemp(), width=W, height=H, spp=SPP, max_depth=DEPTH, name="uq")["config"]
    frames, ref = oracle_data(api, O, cfg, a.cache)
    guides = frames[1][2:]
    m = full_res_errors(frames[1], guides, ref)
    print("full res: raw %d spp %.5g (far from the emitter %.5g); pt_denoise_var %.5g (%.5g)" % (SPP, m["raw"], m["raw_far"], m["var"], m["var_far"]))
    for s in SCALES:
        m = errors(s, frames[s], guides, ref, U.upsample, T.denoise_hist, **U.DEFAULTS)
        _, kind, fragile = U.upsample(s, *frames[s][:2], SPP, BATCHES, *frames[s][2:], *guides, **U.DEFAULTS)
        print("scale %d: nearest %.5g (%.5g); upsampled %.5g (%.5g); upsampled + %d iterations %.5g (%.5g); pass-through %.2f %%, fallback "
              "%.2f %%, fragile %.4f %%" % (s, m["nearest"], m["nearest_far"], m["up"], m["up_far"], ITERATIONS, m["up_filter"], m["up_filter_far"],
                                           100 * (kind == U.PASS).mean(), 100 * (kind == U.FALLBACK).mean(), 100 * fragile.mean()))
    if not a.sweep:
        return
    print("sigma_normal sigma_depth | scale 2: upsampled + %d iterations, all pixels / far from the emitter | fallback share" % ITERATIONS)
    rows = []
    for sn, sd in SWEEP:
        m = errors(2, frames[2], guides, ref, U.upsample, T.denoise_hist, sigma_normal=sn, sigma_depth=sd)
        _, kind, _ = U.upsample(2, *frames[2][:2], SPP, BATCHES, *frames[2][2:], *guides, sigma_normal=sn, sigma_depth=sd)
        rows.append((sn, sd, m["up_filter"], m["up_filter_far"], float((kind == U.FALLBACK).mean())))
        print("%4.0f %.2f | %.6g / %.6g | %.2f %%" % (rows[-1][:4] + (100 * rows[-1][4],)), flush=True)
    # errors within a relative 1e-4 of the smallest count as equal (the kernels' own rounding moves a pixel by up to 1e-3 of its
    # value); among equals the filters' own 64 / 0.02 is preferred: sigma_normal 64 first, then the smaller sigma_depth
    low = min(r[2] for r in rows)
    best = min((r for r in rows if r[2] <= low * (1 + 1e-4)), key=lambda r: (r[0] != 64.0, r[1]))
    print("smallest all-pixel error (ties settled): sigma_normal %.0f, sigma_depth %.2f" % best[:2])


if __name__ == "__main__":
    main(sys.argv[1:])
