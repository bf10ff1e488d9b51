"""numpy restatement of the per-pixel moments and of the variance-guided denoiser (include/pt_api.h: pt_render_moments,
pt_denoise_var).

Used by tests/test_denoise_var_api.py (without a GPU), tests/test_moments.py and tests/test_denoise_var.py to pin the HIP
kernels. Q and V are computed in float32 in the header's order, as the kernels do: Q_c - S_c^2 / B cancels, and a float64
restatement of that one step would disagree on nearly noise-free pixels. From V on the filter runs in float64, as
denoise_ref.denoise does."""
import numpy as np

from denoise_ref import H5, LUMA, passthrough_mask

B3 = np.array([1.0, 2.0, 1.0]) / 4.0


def moments_from_partial_sums(partial_sums):
    """Q of pt_render_moments from S_1..S_B (each [..., 4] or [..., 3], float32): Q = Q + d d with d = S_j - S_{j-1}, S_0 = 0,
    every step rounded to float32 (the product before the add). Returns [..., 4] float32 with Q.w = B."""
    f = np.float32
    sums = [np.asarray(s, f) for s in partial_sums]
    prev = np.zeros_like(sums[0][..., :3])
    Q = np.zeros(sums[0].shape[:-1] + (4,), f)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in sums:
            d = (s[..., :3] - prev).astype(f)
            Q[..., :3] = (Q[..., :3] + (d * d).astype(f)).astype(f)
            prev = s[..., :3]
    Q[..., 3] = f(len(sums))
    return Q


def demod_albedo(albedo):
    return np.where(albedo[..., :3] >= np.float32(0.01), albedo[..., :3], np.float32(1.0)).astype(np.float32)


def variance_of_mean(rgba_sum, sq_sum, spp, batches, albedo):
    """V of pt_denoise_var, float32, in the header's order: var_c = max(0, Q_c - S_c S_c / B) / (B - 1) * B / (spp spp),
    V = var_r / a_r^2 + var_g / a_g^2 + var_b / a_b^2. max(0, NaN) stays NaN."""
    f = np.float32
    S = np.asarray(rgba_sum, f)[..., :3]
    Q = np.asarray(sq_sum, f)[..., :3]
    B, n = f(batches), f(spp)
    a = demod_albedo(albedo)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = (Q - ((S * S).astype(f) / B).astype(f)).astype(f)
        x = np.where(x < 0, f(0), x)
        var = (((x / (B - f(1))).astype(f) * B).astype(f) / (n * n)).astype(f)
        t = (var / (a * a).astype(f)).astype(f)
        return ((t[..., 0] + t[..., 1]).astype(f) + t[..., 2]).astype(f)


def passthrough_mask_var(rgba_sum, sq_sum, spp, batches, albedo):
    return passthrough_mask(rgba_sum, spp, albedo) | ~np.isfinite(variance_of_mean(rgba_sum, sq_sum, spp, batches, albedo))


def binomial3(v, use):
    """The 3x3 binomial of v around every pixel; a neighbour outside the image or not in `use` contributes the centre's v."""
    h, w = v.shape
    ys, xs = np.mgrid[0:h, 0:w]
    out = np.zeros_like(v)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            yq, xq = ys + dy, xs + dx
            inside = (yq >= 0) & (yq < h) & (xq >= 0) & (xq < w)
            yc, xc = np.clip(yq, 0, h - 1), np.clip(xq, 0, w - 1)
            out += B3[dx + 1] * B3[dy + 1] * np.where(inside & use[yc, xc], v[yc, xc], v)
    return out


def denoise_var(rgba_sum, sq_sum, spp, batches, albedo, normal_depth, iterations=3, sigma_var=6.0, sigma_normal=64.0, sigma_depth=0.02,
                return_variance=False):
    """pt_denoise_var. Returns (out float64 [h,w,4], pass-through mask, L) and, with return_variance, the filtered V as well."""
    S = np.asarray(rgba_sum, np.float32)
    h, w = S.shape[:2]
    m = (S / np.float32(spp)).astype(np.float64)
    V32 = variance_of_mean(S, sq_sum, spp, batches, albedo)
    skip = passthrough_mask(S, spp, albedo) | ~np.isfinite(V32)
    use = ~skip
    a32 = demod_albedo(albedo)
    a = a32.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = ((S[..., :3] / np.float32(spp)).astype(np.float32) / a32).astype(np.float64)     # e is stored in f32 by the kernel
    e[skip] = 0.0
    v = np.where(use, V32.astype(np.float64), 0.0)
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
    out = S.astype(np.float64).copy()
    out[..., :3] = np.where(use[..., None], spp * a * e, S[..., :3])
    if return_variance:
        return out, skip, L, v
    return out, skip, L
