"""numpy restatement of temporal accumulation and of the history filter (include/pt_api.h: pt_temporal_accumulate,
pt_denoise_hist). Independent of the kernels; used by tests/test_temporal_api.py (without a GPU) and tests/test_temporal.py.

This frame's e and V are denoise_var_ref's float32 statements. Projection, tap tests and the blend run in float32 in the header's
order, one rounding per operation, as the kernel does: the tap decisions are comparisons, and a float64 restatement would decide
differently where the kernel's rounding matters. accumulate() also returns a FRAGILE mask: pixels where a decision sits so close
to its threshold that one ulp may flip it. The filter of denoise_hist runs in float64 from (e, V) on, as denoise_var_ref does."""
import numpy as np

from denoise_ref import H5, LUMA, passthrough_mask
from denoise_var_ref import binomial3, demod_albedo, variance_of_mean

f32 = np.float32
DEFAULTS = {"max_history": 32, "depth_tol": 0.10, "normal_tol": 0.9}


def camera_fields(cam):
    """origin, forward, right, up (float32 [3] each), fovScale, w, h from a pt_camera (an api.Camera, or its 112 bytes)."""
    b = cam.tobytes() if hasattr(cam, "tobytes") and not isinstance(cam, np.ndarray) else np.ascontiguousarray(cam).tobytes()
    assert len(b) == 112
    f = np.frombuffer(b, f32)
    i = np.frombuffer(b, np.int32)
    return {"origin": f[0:3], "w": int(i[4]), "h": int(i[5]), "fovScale": f[11], "forward": f[16:19], "right": f[20:23], "up": f[24:27], "bytes": b}


def frame_ev(rgba_sum, sq_sum, spp, batches, albedo):
    """pt_denoise_var's per-pixel working values: (m [h,w,3], e [h,w,3], V [h,w], pass-through mask), float32."""
    S = np.asarray(rgba_sum, f32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = (S[..., :3] / f32(spp)).astype(f32)
        e = (m / demod_albedo(albedo)).astype(f32)
    V = variance_of_mean(S, sq_sum, spp, batches, albedo)
    skip = passthrough_mask(S, spp, albedo) | ~np.isfinite(V)
    return m, e, V, skip


def unit_normals(normal_depth):
    """The guide's normals as the kernels normalise them, float32: n / sqrtf(x x + y y + z z), or 0 for a zero normal."""
    n = np.asarray(normal_depth, f32)[..., :3]
    ln = np.sqrt(((n[..., 0] * n[..., 0]).astype(f32) + (n[..., 1] * n[..., 1]).astype(f32)).astype(f32) + (n[..., 2] * n[..., 2]).astype(f32)).astype(f32)
    zero = ~(ln > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (n / np.where(zero, f32(1), ln)[..., None]).astype(f32)
    out[zero] = 0
    return out, zero


def _dot(a, b):
    """a . b over the last axis, float32, left to right."""
    return ((a[..., 0] * b[..., 0]).astype(f32) + (a[..., 1] * b[..., 1]).astype(f32) + (a[..., 2] * b[..., 2]).astype(f32)).astype(f32)


def reproject(cam, cam_prev, depth):
    """Step 3 of the contract: (x', y', z', has_projection), float32 [h,w]. Identity (cam_prev None or the same bytes) returns the
    pixel's own coordinates and depth exactly."""
    c = camera_fields(cam)
    w, h = c["w"], c["h"]
    ys, xs = np.mgrid[0:h, 0:w]
    z = np.asarray(depth, f32)
    if cam_prev is None or camera_fields(cam_prev)["bytes"] == c["bytes"]:
        return xs.astype(f32), ys.astype(f32), z, np.ones((h, w), bool)
    p = camera_fields(cam_prev)
    aspect = f32(f32(w) / f32(h))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = ((((f32(2) * (xs.astype(f32) / f32(w)).astype(f32)).astype(f32) - f32(1)).astype(f32) * aspect).astype(f32) * c["fovScale"]).astype(f32)
        v = (((f32(2) * (ys.astype(f32) / f32(h)).astype(f32)).astype(f32) - f32(1)).astype(f32) * c["fovScale"]).astype(f32)
        t = np.stack([(((c["right"][k] * u).astype(f32) + (c["up"][k] * v).astype(f32)).astype(f32) + c["forward"][k]).astype(f32) for k in range(3)], -1)
        tl = np.sqrt(_dot(t, t)).astype(f32)
        P = np.stack([(c["origin"][k] + ((t[..., k] / tl).astype(f32) * z).astype(f32)).astype(f32) for k in range(3)], -1)
        q = (P - p["origin"]).astype(f32)
        zc = _dot(q, np.broadcast_to(p["forward"], q.shape))
        ok = zc > 0
        paspect = f32(f32(p["w"]) / f32(p["h"]))
        fs = f32(paspect * p["fovScale"])
        xp = ((((_dot(q, np.broadcast_to(p["right"], q.shape)) / zc).astype(f32) / fs).astype(f32) + f32(1)).astype(f32) * f32(w)).astype(f32) / f32(2)
        yp = ((((_dot(q, np.broadcast_to(p["up"], q.shape)) / zc).astype(f32) / p["fovScale"]).astype(f32) + f32(1)).astype(f32) * f32(h)).astype(f32) / f32(2)
        zexp = np.sqrt(_dot(q, q)).astype(f32)
    return xp.astype(f32), yp.astype(f32), zexp, ok


def accumulate(cam, cam_prev, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, prev_normal_depth=None, hist=None, hist_len=None,
               max_history=32, depth_tol=0.10, normal_tol=0.9):
    """pt_temporal_accumulate. Returns (out_hist [h,w,4] float32, out_hist_len [h,w] float32, fragile mask [h,w])."""
    m, e, V, skip = frame_ev(rgba_sum, sq_sum, spp, batches, albedo)
    h, w = V.shape
    out = np.concatenate([e, V[..., None]], -1).astype(f32)
    out_len = np.ones((h, w), f32)
    fragile = np.zeros((h, w), bool)
    if hist is not None:
        depth_tol, normal_tol = f32(depth_tol), f32(normal_tol)
        hist = np.asarray(hist, f32); hist_len = np.asarray(hist_len, f32)
        n_cur, zero_cur = unit_normals(normal_depth)
        n_prev, zero_prev = unit_normals(prev_normal_depth)
        z_prev = np.asarray(prev_normal_depth, f32)[..., 3]
        xp, yp, zexp, ok = reproject(cam, cam_prev, np.asarray(normal_depth, f32)[..., 3])
        identity = cam_prev is None or camera_fields(cam_prev)["bytes"] == camera_fields(cam)["bytes"]
        with np.errstate(invalid="ignore"):
            ok = ok & ~zero_cur & (xp >= -1) & (xp < w) & (yp >= -1) & (yp < h)
        xq = np.where(ok, xp, f32(0)); yq = np.where(ok, yp, f32(0))
        x0 = np.floor(xq).astype(f32); y0 = np.floor(yq).astype(f32)
        ax = (xq - x0).astype(f32); ay = (yq - y0).astype(f32)
        one = f32(1)
        taps = [(0, 0, ((one - ax).astype(f32) * (one - ay).astype(f32)).astype(f32)), (1, 0, (ax * (one - ay).astype(f32)).astype(f32)),
                (0, 1, ((one - ax).astype(f32) * ay).astype(f32)), (1, 1, (ax * ay).astype(f32))]
        if identity:
            taps = [(0, 0, np.ones((h, w), f32))]
        se = np.zeros((h, w, 3), f32); sv = np.zeros((h, w), f32); sn = np.zeros((h, w), f32); sw = np.zeros((h, w), f32)
        for dx, dy, wt in taps:
            xi = x0.astype(np.int64) + dx; yi = y0.astype(np.int64) + dy
            inside = ok & (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            xc, yc = np.clip(xi, 0, w - 1), np.clip(yi, 0, h - 1)
            hq = hist[yc, xc]
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                live = inside & (hq[..., 3] >= 0)
                dz = np.abs((z_prev[yc, xc] - zexp).astype(f32))
                lim = (depth_tol * zexp).astype(f32)
                cs = _dot(n_cur, n_prev[yc, xc])
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


def hist_passthrough(hist):
    hist = np.asarray(hist, f32)
    with np.errstate(invalid="ignore"):
        return ~((hist[..., 3] >= 0) & np.isfinite(hist).all(-1))


def denoise_hist(hist, albedo, normal_depth, iterations=3, sigma_var=6.0, sigma_normal=64.0, sigma_depth=0.02):
    """pt_denoise_hist: denoise_var_ref.denoise_var's loop on (e, V) read from hist. Returns (out float64 [h,w,4] = the radiance
    mean, pass-through mask, L)."""
    hist = np.asarray(hist, f32)
    h, w = hist.shape[:2]
    skip = hist_passthrough(hist)
    use = ~skip
    a = demod_albedo(albedo).astype(np.float64)
    e = np.where(use[..., None], hist[..., :3].astype(np.float64), 0.0)
    v = np.where(use, hist[..., 3].astype(np.float64), 0.0)
    L = float((e[use] @ LUMA).mean()) if use.any() else 0.0
    n = normal_depth[..., :3].astype(np.float64)
    ln = np.linalg.norm(n, axis=-1)
    nzero = ln == 0
    nh = np.where(nzero[..., None], 0.0, n / np.where(nzero, 1.0, ln)[..., None])
    z = normal_depth[..., 3].astype(np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    for i in range(iterations):
        s = 1 << i
        den = sigma_var * np.sqrt(binomial3(v, use)) + 1e-3 * L + 1e-20
        num = (H5[2] ** 2) * e
        wsum = np.full((h, w), H5[2] ** 2)
        vnum = (H5[2] ** 4) * v
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dx == 0 and dy == 0:
                    continue
                yq, xq = ys + dy * s, xs + dx * s
                inside = (yq >= 0) & (yq < h) & (xq >= 0) & (xq < w)
                yc, xc = np.clip(yq, 0, h - 1), np.clip(xq, 0, w - 1)
                ok = inside & use[yc, xc] & use
                eq = e[yc, xc]
                wc = np.exp(-np.sqrt(((e - eq) ** 2).sum(-1)) / den)
                cos = (nh * nh[yc, xc]).sum(-1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    wn = np.where(nzero | nzero[yc, xc], 0.0, np.maximum(0.0, cos) ** sigma_normal)
                    wz = np.exp(-np.abs(z - z[yc, xc]) / (sigma_depth * z))
                wt = np.where(ok, H5[dx + 2] * H5[dy + 2] * wc * wn * wz, 0.0)
                num += wt[..., None] * eq
                wsum += wt
                vnum += wt * wt * v[yc, xc]
        e = np.where(use[..., None], num / wsum[..., None], e)
        v = np.where(use, vnum / (wsum * wsum), v)
    out = np.zeros((h, w, 4), np.float64)
    out[..., :3] = np.where(use[..., None], a * e, hist[..., :3].astype(np.float64))
    return out, skip, L
