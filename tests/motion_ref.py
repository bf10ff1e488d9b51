"""numpy restatement of the motion pass and of the history stage with motion (include/pt_api.h: pt_render_motion,
pt_temporal_accumulate_motion, pt_temporal_accumulate_cur_motion). Independent of the kernels; tests/test_motion_ref_cpu.py checks
it without a GPU, tests/test_motion.py and tests/test_preview_motion.py hold the library to it bit for bit.

Everything is float32, one rounding per operation, in the header's order. accumulate() is temporal_ref.accumulate's arithmetic
from temporal_ref's own pieces (frame_ev, unit_normals, reproject, camera_fields) with the reprojected point replaced for the
pixels that moved: such a pixel projects motion.xyz and never takes the identity tap."""
import numpy as np

import temporal_ref as T

f32 = np.float32


def _f4(a):
    return np.ascontiguousarray(a).view(f32).reshape(-1, 4)


def triangle_vertices(mesh):
    """aInd, bInd, cInd of every pt_triangle (80 bytes each): int32 [n, 3]."""
    return np.ascontiguousarray(mesh).view(np.uint8).reshape(-1, 80)[:, :12].copy().view(np.int32)


def motion(points_cur, points_prev, mesh, hits):
    """pt_render_motion's out_motion over closest-hit records. hits = (valid bool [n], u [n], v [n], tri [n]): the barycentrics and the
    ORIGINAL triangle index of each ray's closest hit (pt_probe_trace_closest's, or the oracle's). points_prev None: the scene has no
    previous positions. Returns float32 [n, 4]."""
    valid, u, v, tri = hits
    valid = np.asarray(valid, bool); u = np.asarray(u, f32); v = np.asarray(v, f32)
    out = np.zeros((len(valid), 4), f32)
    if points_prev is None:
        return out
    cur, prev = _f4(points_cur)[:, :3], _f4(points_prev)[:, :3]
    idx = triangle_vertices(mesh)[np.where(valid, tri, 0)]                 # [n, 3]
    A, B, Cc = cur[idx[:, 0]], cur[idx[:, 1]], cur[idx[:, 2]]
    Ap, Bp, Cp = prev[idx[:, 0]], prev[idx[:, 1]], prev[idx[:, 2]]
    still = (A == Ap).all(-1) & (B == Bp).all(-1) & (Cc == Cp).all(-1)
    bz = ((f32(1) - u).astype(f32) - v).astype(f32)
    P = (((Ap * bz[:, None]).astype(f32) + (Bp * u[:, None]).astype(f32)).astype(f32) + (Cp * v[:, None]).astype(f32)).astype(f32)
    moved = valid & ~still
    out[moved, :3] = P[moved]
    out[moved, 3] = 1
    return out


def project(P, cam_prev, w, h):
    """The second half of step 3 for given world points P [h,w,3]: (x', y', z', z_c > 0) seen from cam_prev, float32."""
    p = T.camera_fields(cam_prev)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = (np.asarray(P, f32) - p["origin"]).astype(f32)
        zc = T._dot(q, np.broadcast_to(p["forward"], q.shape))
        ok = zc > 0
        fs = f32(f32(f32(p["w"]) / f32(p["h"])) * p["fovScale"])
        xp = ((((T._dot(q, np.broadcast_to(p["right"], q.shape)) / zc).astype(f32) / fs).astype(f32) + f32(1)).astype(f32) * f32(w)).astype(f32) / f32(2)
        yp = ((((T._dot(q, np.broadcast_to(p["up"], q.shape)) / zc).astype(f32) / p["fovScale"]).astype(f32) + f32(1)).astype(f32) * f32(h)).astype(f32) / f32(2)
        zexp = np.sqrt(T._dot(q, q)).astype(f32)
    return xp.astype(f32), yp.astype(f32), zexp, ok


def _blend(cam, cam_prev, m, e, V, skip, normal_depth, prev_normal_depth, hist, hist_len, motion, max_history, depth_tol, normal_tol):
    """Steps 2-5 for the working pixels (e, V), pass-through mask `skip` with raw means m."""
    h, w = V.shape
    out = np.concatenate([e, V[..., None]], -1).astype(f32)
    out_len = np.ones((h, w), f32)
    fragile = np.zeros((h, w), bool)
    moved = np.zeros((h, w), bool)
    if hist is not None:
        depth_tol, normal_tol = f32(depth_tol), f32(normal_tol)
        hist = np.asarray(hist, f32); hist_len = np.asarray(hist_len, f32)
        n_cur, zero_cur = T.unit_normals(normal_depth)
        n_prev, zero_prev = T.unit_normals(prev_normal_depth)
        z_prev = np.asarray(prev_normal_depth, f32)[..., 3]
        xp, yp, zexp, ok = T.reproject(cam, cam_prev, np.asarray(normal_depth, f32)[..., 3])
        identity = cam_prev is None or T.camera_fields(cam_prev)["bytes"] == T.camera_fields(cam)["bytes"]
        if motion is not None:
            motion = np.asarray(motion, f32)
            moved = motion[..., 3] == f32(1)
            mx, my, mz, mok = project(motion[..., :3], cam if cam_prev is None else cam_prev, w, h)
            xp = np.where(moved, mx, xp); yp = np.where(moved, my, yp); zexp = np.where(moved, mz, zexp); ok = np.where(moved, mok, ok)
        single = ~moved if identity else np.zeros((h, w), bool)           # the identity tap: (x, y) itself with weight 1
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
            N = np.minimum((nh + one).astype(f32), f32(max_history))
            alpha = (one / N).astype(f32); keep = (one - alpha).astype(f32)
            eb = (eh + (alpha[..., None] * (e - eh).astype(f32)).astype(f32)).astype(f32)
            vb = (((keep * keep).astype(f32) * vh).astype(f32) + ((alpha * alpha).astype(f32) * V).astype(f32)).astype(f32)
        out[..., :3] = np.where(has[..., None], eb, e)
        out[..., 3] = np.where(has, vb, V)
        out_len = np.where(has, N, one).astype(f32)
    out[skip, :3] = m[skip]
    out[skip, 3] = -1
    out_len[skip] = 0
    fragile &= ~skip
    return out, out_len, fragile


def accumulate(cam, cam_prev, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, prev_normal_depth=None, hist=None, hist_len=None,
               motion=None, max_history=32, depth_tol=0.10, normal_tol=0.9):
    """pt_temporal_accumulate_motion. Returns (out_hist [h,w,4] float32, out_hist_len [h,w] float32, fragile mask [h,w]); with
    motion None (or all zeros) it is temporal_ref.accumulate."""
    m, e, V, skip = T.frame_ev(rgba_sum, sq_sum, spp, batches, albedo)
    return _blend(cam, cam_prev, m, e, V, skip, normal_depth, prev_normal_depth, hist, hist_len, motion, max_history, depth_tol, normal_tol)


def accumulate_cur(cam, cam_prev, cur, normal_depth, prev_normal_depth=None, hist=None, hist_len=None, motion=None, max_history=32,
                   depth_tol=0.10, normal_tol=0.9):
    """pt_temporal_accumulate_cur_motion: this frame's working pixels are given; !(cur.w >= 0) passes through with (cur.rgb, -1)."""
    cur = np.asarray(cur, f32)
    with np.errstate(invalid="ignore"):
        skip = ~(cur[..., 3] >= 0)
    return _blend(cam, cam_prev, cur[..., :3], cur[..., :3], cur[..., 3], skip, normal_depth, prev_normal_depth, hist, hist_len, motion,
                  max_history, depth_tol, normal_tol)


def rescued(cam, normal_depth, prev_normal_depth, motion, depth_tol=0.10, normal_tol=0.9):
    """For a STILL camera: the pixels that moved, whose same-pixel tap is invalid against the previous guide, and whose motion
    reprojection finds a valid tap there (W >= 0.01), on a previous history without a pass-through pixel: bool [h,w]."""
    N = np.asarray(normal_depth, f32)
    h, w = N.shape[:2]
    cur = np.ones((h, w, 4), f32)                                          # any working pixels: only the lengths are read
    hist, ln = np.ones((h, w, 4), f32), np.full((h, w), 2, f32)
    base = _blend(cam, None, cur[..., :3], cur[..., :3], cur[..., 3], np.zeros((h, w), bool), N, prev_normal_depth, hist, ln, None, 32, depth_tol,
                  normal_tol)[1]
    with_m = _blend(cam, None, cur[..., :3], cur[..., :3], cur[..., 3], np.zeros((h, w), bool), N, prev_normal_depth, hist, ln, motion, 32,
                    depth_tol, normal_tol)[1]
    return (np.asarray(motion, f32)[..., 3] == 1) & (base == 1) & (with_m > 1)
