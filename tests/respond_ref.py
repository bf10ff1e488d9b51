"""numpy restatement of the responsive history stage (include/pt_api.h, "RESPOND": pt_temporal_accumulate_respond). Independent of
the kernels; tests/test_respond_ref_cpu.py checks it without a GPU, tests/test_respond.py and tests/test_preview_respond.py hold the
library to it bit for bit.

Everything is float32, one rounding per operation, in the header's order. gather() is the base function's steps 1-4 from
temporal_ref's and motion_ref's own pieces (frame_ev, unit_normals, reproject, project), stated once more because their accumulate()
does not hand out the gathered history; with threshold inf accumulate() must equal theirs exactly, which the CPU test checks.
accumulate() also returns a FRAGILE mask: the base function's, a window-membership comparison within 1e-3 relative of its
threshold, or a T within 1e-3 relative of lim."""
import numpy as np

import motion_ref as M
import temporal_ref as T

f32 = np.float32
DEFAULTS = {"radius": 3, "power": 4, "threshold": 2.0}


def gather(cam, cam_prev, normal_depth, prev_normal_depth, hist, hist_len, motion=None, depth_tol=0.10, normal_tol=0.9):
    """Steps 2-4 of pt_temporal_accumulate[_motion] for every pixel: (has [h,w] bool: W >= 0.01, e_h [h,w,3], V_h, N_h, fragile)."""
    N = np.asarray(normal_depth, f32)
    h, w = N.shape[:2]
    depth_tol, normal_tol = f32(depth_tol), f32(normal_tol)
    hist = np.asarray(hist, f32); hist_len = np.asarray(hist_len, f32)
    fragile = np.zeros((h, w), bool)
    moved = np.zeros((h, w), bool)
    n_cur, zero_cur = T.unit_normals(N)
    n_prev, zero_prev = T.unit_normals(prev_normal_depth)
    z_prev = np.asarray(prev_normal_depth, f32)[..., 3]
    xp, yp, zexp, ok = T.reproject(cam, cam_prev, N[..., 3])
    identity = cam_prev is None or T.camera_fields(cam_prev)["bytes"] == T.camera_fields(cam)["bytes"]
    if motion is not None:
        motion = np.asarray(motion, f32)
        moved = motion[..., 3] == f32(1)
        mx, my, mz, mok = M.project(motion[..., :3], cam if cam_prev is None else cam_prev, w, h)
        xp = np.where(moved, mx, xp); yp = np.where(moved, my, yp); zexp = np.where(moved, mz, zexp); ok = np.where(moved, mok, ok)
    single = ~moved if identity else np.zeros((h, w), bool)               # the identity tap: (x, y) itself with weight 1
    with np.errstate(invalid="ignore"):
        ok = ok & ~zero_cur & (xp >= -1) & (xp < w) & (yp >= -1) & (yp < h)
    xq = np.where(ok, xp, f32(0)); yq = np.where(ok, yp, f32(0))
    x0 = np.floor(xq).astype(f32); y0 = np.floor(yq).astype(f32)
    ax = (xq - x0).astype(f32); ay = (yq - y0).astype(f32)
    one = f32(1)
    taps = [(0, 0, ((one - ax).astype(f32) * (one - ay).astype(f32)).astype(f32)), (1, 0, (ax * (one - ay).astype(f32)).astype(f32)),
            (0, 1, ((one - ax).astype(f32) * ay).astype(f32)), (1, 1, (ax * ay).astype(f32))]
    se = np.zeros((h, w, 3), f32); sv = np.zeros((h, w), f32); sn = np.zeros((h, w), f32); sw = np.zeros((h, w), f32)
    for k, (dx, dy, wt) in enumerate(taps):
        wt = np.where(single, one, wt) if k == 0 else wt
        xi = x0.astype(np.int64) + dx; yi = y0.astype(np.int64) + dy
        inside = ok & (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        if k > 0:
            inside = inside & ~single
        xc, yc = np.clip(xi, 0, w - 1), np.clip(yi, 0, h - 1)
        hq = hist[yc, xc]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            live = inside & (hq[..., 3] >= 0)
            dz = np.abs((z_prev[yc, xc] - zexp).astype(f32))
            lim = (depth_tol * zexp).astype(f32)
            cs = T._dot(n_cur, n_prev[yc, xc])
            valid = live & (dz <= lim) & ~zero_prev[yc, xc] & (cs >= normal_tol)
            matters = live & (wt > 1e-3)
            fragile |= matters & (np.abs(dz.astype(np.float64) / lim.astype(np.float64) - 1.0) < 1e-3)
            fragile |= matters & ~zero_prev[yc, xc] & (np.abs(cs.astype(np.float64) - float(normal_tol)) < 1e-4)
            se = np.where(valid[..., None], (se + (wt[..., None] * hq[..., :3]).astype(f32)).astype(f32), se)
            sv = np.where(valid, (sv + (wt * hq[..., 3]).astype(f32)).astype(f32), sv)
            sn = np.where(valid, (sn + (wt * hist_len[yc, xc]).astype(f32)).astype(f32), sn)
            sw = np.where(valid, (sw + wt).astype(f32), sw)
    fragile |= np.abs(sw.astype(np.float64) - 0.01) < 1e-3
    has = sw >= f32(0.01)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        swd = np.where(has, sw, one)
        eh = (se / swd[..., None]).astype(f32); vh = (sv / swd).astype(f32); nh = (sn / swd).astype(f32)
    return has, eh, vh, nh, fragile


def scale(e, V, skip, has, eh, vh, normal_depth, radius, power, threshold, depth_tol=0.10, normal_tol=0.9):
    """lambda of every pixel (1 where no test runs) and the mask of the pixels whose test is fragile."""
    h, w = V.shape
    depth_tol, normal_tol = f32(depth_tol), f32(normal_tol)
    n_cur, zero_cur = T.unit_normals(normal_depth)
    z = np.asarray(normal_depth, f32)[..., 3]
    witness = has & ~skip
    with np.errstate(invalid="ignore", over="ignore"):
        d = (e - eh).astype(f32)
        v = (V + vh).astype(f32)
        counts = witness & np.isfinite(d).all(-1) & np.isfinite(v) & ~zero_cur          # what a pixel needs to count in any window
    D = np.zeros((h, w, 3), f32); Vs = np.zeros((h, w), f32)
    fragile = np.zeros((h, w), bool)
    ys, xs = np.mgrid[0:h, 0:w]
    zlim = (depth_tol * z).astype(f32)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            yq, xq = ys + dy, xs + dx
            inside = (yq >= 0) & (yq < h) & (xq >= 0) & (xq < w)
            yc, xc = np.clip(yq, 0, h - 1), np.clip(xq, 0, w - 1)
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                cand = inside & counts[yc, xc] & counts
                dz = np.abs((z[yc, xc] - z).astype(f32))
                cs = T._dot(n_cur, n_cur[yc, xc])
                member = cand & (dz <= zlim) & (cs >= normal_tol)
                fragile |= cand & (np.abs(dz.astype(np.float64) / zlim.astype(np.float64) - 1.0) < 1e-3)
                fragile |= cand & (np.abs(cs.astype(np.float64) / float(normal_tol) - 1.0) < 1e-3)
                D = np.where(member[..., None], (D + d[yc, xc]).astype(f32), D)
                Vs = np.where(member, (Vs + v[yc, xc]).astype(f32), Vs)
    k = f32(threshold)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Tt = (((D[..., 0] * D[..., 0]).astype(f32) + (D[..., 1] * D[..., 1]).astype(f32)).astype(f32) + (D[..., 2] * D[..., 2]).astype(f32)).astype(f32)
        lim = (f32(k * k) * Vs).astype(f32)
        over = counts & (Tt > lim)
        rho = (lim / np.where(over, Tt, f32(1))).astype(f32)
        r2 = (rho * rho).astype(f32)
        lam = rho if power == 1 else (r2 if power == 2 else (r2 * r2).astype(f32))
        fragile |= counts & np.isfinite(lim) & (np.abs(Tt.astype(np.float64) - lim.astype(np.float64)) < 1e-3 * np.abs(lim.astype(np.float64)))
    assert power in (1, 2, 4) and 1 <= radius <= 3
    return np.where(over, lam, f32(1)).astype(f32), fragile & counts


def _accumulate(cam, cam_prev, m, e, V, skip, normal_depth, prev_normal_depth, hist, hist_len, motion, max_history, depth_tol, normal_tol,
                radius, power, threshold):
    h, w = V.shape
    out = np.concatenate([e, V[..., None]], -1).astype(f32)
    out_len = np.ones((h, w), f32)
    lam = np.ones((h, w), f32)
    fragile = np.zeros((h, w), bool)
    if hist is not None:
        has, eh, vh, nh, fragile = gather(cam, cam_prev, normal_depth, prev_normal_depth, hist, hist_len, motion, depth_tol, normal_tol)
        lam, fr = scale(e, V, skip, has, eh, vh, normal_depth, radius, power, threshold, depth_tol, normal_tol)
        fragile = fragile | fr
        one = f32(1)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            N = np.minimum(((lam * nh).astype(f32) + one).astype(f32), f32(max_history))
            alpha = (one / N).astype(f32); keep = (one - alpha).astype(f32)
            eb = (eh + (alpha[..., None] * (e - eh).astype(f32)).astype(f32)).astype(f32)
            vb = (((keep * keep).astype(f32) * vh).astype(f32) + ((alpha * alpha).astype(f32) * V).astype(f32)).astype(f32)
        out[..., :3] = np.where(has[..., None], eb, e)
        out[..., 3] = np.where(has, vb, V)
        out_len = np.where(has, N, one).astype(f32)
    out[skip, :3] = m[skip]
    out[skip, 3] = -1
    out_len[skip] = 0
    lam = lam.copy(); lam[skip] = 1
    fragile &= ~skip
    return out, out_len, lam, fragile


def accumulate(cam, cam_prev, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, prev_normal_depth=None, hist=None, hist_len=None,
               motion=None, max_history=32, depth_tol=0.10, normal_tol=0.9, radius=3, power=4, threshold=2.0):
    """pt_temporal_accumulate_respond, the frame as sums. Returns (out_hist [h,w,4], out_hist_len [h,w], lambda [h,w], fragile [h,w])."""
    m, e, V, skip = T.frame_ev(rgba_sum, sq_sum, spp, batches, albedo)
    return _accumulate(cam, cam_prev, m, e, V, skip, normal_depth, prev_normal_depth, hist, hist_len, motion, max_history, depth_tol, normal_tol,
                       radius, power, threshold)


def accumulate_cur(cam, cam_prev, cur, normal_depth, prev_normal_depth=None, hist=None, hist_len=None, motion=None, max_history=32,
                   depth_tol=0.10, normal_tol=0.9, radius=3, power=4, threshold=2.0):
    """pt_temporal_accumulate_respond, the frame as working pixels: !(cur.w >= 0) passes through with (cur.rgb, -1)."""
    cur = np.asarray(cur, f32)
    with np.errstate(invalid="ignore"):
        skip = ~(cur[..., 3] >= 0)
    return _accumulate(cam, cam_prev, cur[..., :3], cur[..., :3], cur[..., 3], skip, normal_depth, prev_normal_depth, hist, hist_len, motion,
                       max_history, depth_tol, normal_tol, radius, power, threshold)
