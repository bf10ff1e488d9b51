"""numpy restatement of the render scale's two stages (include/pt_api.h: pt_upsample, pt_temporal_accumulate_cur). Independent of
the kernels; used by tests/test_upsample_api.py (without a GPU), tests/test_upsample.py and tests/upsample_seq.py.

The low-res working pixels are temporal_ref.frame_ev's float32 statements. Positions, bilinear weights, the candidate / usable
decisions, the cosine and the W threshold run in float32 in the header's order: they are comparisons, and the kernel decides them
in float32. The tap weights' exp and pow and the sums run in float64, as denoise_var_ref runs its filter. upsample() also returns a
FRAGILE mask: the pixels whose W lies within a relative 1e-3 of the 1e-4 threshold, where rounding may pick the other branch."""
import numpy as np

import temporal_ref as T

f32 = np.float32
DEFAULTS = {"sigma_normal": 64.0, "sigma_depth": 0.10}
W_MIN = f32(1e-4)
PASS, FALLBACK, WEIGHTED = 0, 1, 2
TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))


def bilinear_weights(w, h, s):
    """Steps 1 and 2: X0, Y0 (int [h,w]) and the four b_k (float32 [h,w]) in tap order."""
    ys, xs = np.mgrid[0:h, 0:w]
    X0, Y0 = xs // s, ys // s
    fx = ((xs - s * X0).astype(f32) / f32(s)).astype(f32)
    fy = ((ys - s * Y0).astype(f32) / f32(s)).astype(f32)
    one = f32(1)
    gx, gy = (one - fx).astype(f32), (one - fy).astype(f32)
    return X0, Y0, [(gx * gy).astype(f32), (fx * gy).astype(f32), (gx * fy).astype(f32), (fx * fy).astype(f32)]


def upsample(scale, rgba_sum_lo, sq_sum_lo, spp, batches, albedo_lo, normal_depth_lo, albedo, normal_depth, sigma_normal=64.0, sigma_depth=0.10):
    """pt_upsample. Returns (cur [h,w,4] float32, kind [h,w] of PASS / FALLBACK / WEIGHTED, fragile mask [h,w])."""
    s = int(scale)
    A = np.asarray(albedo, f32); N = np.asarray(normal_depth, f32)
    h, w = A.shape[:2]
    hl, wl = h // s, w // s
    assert w % s == 0 and h % s == 0 and np.asarray(rgba_sum_lo).shape == (hl, wl, 4)
    m, e, V, skip = T.frame_ev(rgba_sum_lo, sq_sum_lo, spp, batches, albedo_lo)
    n_p, zero_p = T.unit_normals(N)
    n_lo, zero_lo = T.unit_normals(normal_depth_lo)
    z_p = N[..., 3]; z_lo = np.asarray(normal_depth_lo, f32)[..., 3]
    with np.errstate(invalid="ignore"):
        hit = A[..., 3] > 0
    X0, Y0, b = bilinear_weights(w, h, s)
    cand_b = np.zeros((h, w), f32); cand_m = np.zeros((h, w, 3), f32)
    use_b = np.zeros((h, w), f32); use_ev = np.zeros((h, w, 4), f32)
    num = np.zeros((h, w, 3)); vnum = np.zeros((h, w)); W64 = np.zeros((h, w)); W32 = np.zeros((h, w), f32)
    for (dx, dy), bk in zip(TAPS, b):
        xk, yk = X0 + dx, Y0 + dy
        cand = (bk > 0) & (xk < wl) & (yk < hl)
        xc, yc = np.minimum(xk, wl - 1), np.minimum(yk, hl - 1)
        nearer = cand & (bk > cand_b)                     # strictly: the first in tap order wins a tie
        cand_b = np.where(nearer, bk, cand_b); cand_m = np.where(nearer[..., None], m[yc, xc], cand_m)
        usable = cand & hit & ~skip[yc, xc]
        nearer = usable & (bk > use_b)
        use_b = np.where(nearer, bk, use_b)
        use_ev = np.where(nearer[..., None], np.concatenate([e[yc, xc], V[yc, xc][..., None]], -1), use_ev)
        cs = T._dot(n_p, n_lo[yc, xc])
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            wn = np.ones((h, w)) if sigma_normal == 0 else np.where(cs > 0, np.maximum(cs.astype(np.float64), 0.0) ** float(sigma_normal), 0.0)
            dz = np.abs((z_p - z_lo[yc, xc]).astype(f32)).astype(np.float64)
            wz = np.exp(-dz / (float(f32(sigma_depth)) * z_p.astype(np.float64)))
            wk = bk.astype(np.float64) * wn * wz
            wk = np.where(zero_p | zero_lo[yc, xc], 0.0, wk)
            taken = usable & (wk.astype(f32) > 0)         # 0 or NaN: skipped, never multiplied in
        wk = np.where(taken, wk, 0.0)
        ek = np.where(taken[..., None], e[yc, xc].astype(np.float64), 0.0)
        vk = np.where(taken, V[yc, xc].astype(np.float64), 0.0)
        num += wk[..., None] * ek; vnum += wk * wk * vk; W64 += wk
        W32 = (W32 + wk.astype(f32)).astype(f32)
    have = use_b > 0
    weighted = have & (W32 >= W_MIN)
    kind = np.where(weighted, WEIGHTED, np.where(have, FALLBACK, PASS))
    out = np.empty((h, w, 4), f32)
    out[..., :3] = cand_m; out[..., 3] = -1
    out[have] = use_ev[have]
    Wd = np.where(weighted, W64, 1.0)
    out[weighted, :3] = (num / Wd[..., None])[weighted].astype(f32)
    out[weighted, 3] = (vnum / (Wd * Wd))[weighted].astype(f32)
    fragile = have & (np.abs(W64 / float(W_MIN) - 1.0) < 1e-3)
    return out, kind, fragile


def accumulate_cur(cam, cam_prev, cur, normal_depth, prev_normal_depth=None, hist=None, hist_len=None, **params):
    """pt_temporal_accumulate_cur: temporal_ref.accumulate from its step 2 on, with this frame's working pixels read from `cur`
    (a pixel with !(cur.w >= 0) passes through as (cur.rgb, -1)). accumulate() takes its step 1 from temporal_ref.frame_ev, so
    that one function is stood in for while it runs; nothing of the blend is restated here."""
    cur = np.asarray(cur, f32)
    with np.errstate(invalid="ignore"):
        skip = ~(cur[..., 3] >= 0)
    given = (cur[..., :3], cur[..., :3], cur[..., 3], skip)          # (m, e, V, pass-through): a pass-through pixel keeps its rgb
    frame_ev = T.frame_ev
    T.frame_ev = lambda *a: given
    try:
        return T.accumulate(cam, cam_prev, None, None, 0, 0, None, normal_depth, prev_normal_depth, hist, hist_len, **params)
    finally:
        T.frame_ev = frame_ev


# ---- hand-made buffers with a known answer (tests/test_upsample_api.py on the restatement, tests/test_upsample.py on the kernel) ---
def synthetic(wl, hl, s, seed, spp=4, batches=2, albedo=0.5, depth_split=False):
    """A noisy low-res frame (S, Q, albedo_lo, normal_depth_lo) and display-size guides (albedo, normal_depth): flat albedo, coverage 1,
    normal (0, 0, 1), depth 1; with depth_split the right half lies at depth 2 (in both resolutions) and holds five times brighter samples
    (e in [0.18, 0.22] on the left, [0.9, 1.1] on the right)."""
    from denoise_var_ref import moments_from_partial_sums
    rng = np.random.default_rng(seed)
    w, h = wl * s, hl * s
    base = np.full((hl, wl, 1), 1.0 if not depth_split else 0.1, f32)
    if depth_split:
        base[:, wl // 2:] = 0.5
    acc = np.zeros((hl, wl, 4), f32); partial = []
    for _ in range(batches):
        acc = acc.copy()
        noise = rng.uniform(0.9, 1.1, (hl, wl, 3)).astype(f32) if depth_split else rng.uniform(0.2, 1.0, (hl, wl, 3)).astype(f32)
        acc[..., :3] = (acc[..., :3] + (base * noise).astype(f32) * f32(spp // batches)).astype(f32)
        partial.append(acc)

    def guides(hh, ww):
        A = np.zeros((hh, ww, 4), f32); A[..., :3] = albedo; A[..., 3] = 1.0
        N = np.zeros((hh, ww, 4), f32); N[..., 2] = 1.0; N[..., 3] = 1.0
        if depth_split:
            N[:, ww // 2:, 3] = 2.0
        return A, N
    Al, Nl = guides(hl, wl)
    A, N = guides(h, w)
    return partial[-1], moments_from_partial_sums(partial), Al, Nl, A, N


def bilinear_closed_form(s, e_lo, V_lo):
    """With constant guides every in-image tap has w_k = b_k: e = sum b e / sum b and V = sum b^2 V / (sum b)^2 over the taps
    inside the low-res image (float64). Away from the high edges sum b = 1: the plain bilinear interpolation."""
    hl, wl = V_lo.shape
    h, w = hl * s, wl * s
    X0, Y0, b = bilinear_weights(w, h, s)
    num = np.zeros((h, w, 3)); vnum = np.zeros((h, w)); W = np.zeros((h, w))
    for (dx, dy), bk in zip(TAPS, b):
        xk, yk = X0 + dx, Y0 + dy
        bk = np.where((xk < wl) & (yk < hl), bk.astype(np.float64), 0.0)
        xc, yc = np.minimum(xk, wl - 1), np.minimum(yk, hl - 1)
        num += bk[..., None] * e_lo[yc, xc]; vnum += bk * bk * V_lo[yc, xc]; W += bk
    return num / W[..., None], vnum / (W * W), W
