"""numpy restatement of the feature buffers and of the denoiser (include/pt_api.h: pt_render_aovs, pt_denoise).

Used by tests/test_aov.py and tests/test_denoise.py to pin the HIP kernels."""
import numpy as np

H5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
LUMA = np.array([0.2126, 0.7152, 0.0722])


def aovs_from_hits(hits_per_k, aov_spp):
    """Compose the feature buffers from per-ray first hits.

    hits_per_k: list over k of (valid [n] bool, albedo [n,3] f32, normal [n,3] f32, t [n] f32), k in order.
    Returns (albedo [n,4], normal_depth [n,4]) float32: sums in k order in f32 (the first hit stored, not added to 0),
    one IEEE division by the hit count, coverage = hits / aov_spp; no hit -> zeros."""
    n = len(hits_per_k[0][0])
    sa = np.zeros((n, 3), np.float32); sn = np.zeros((n, 3), np.float32); st = np.zeros(n, np.float32)
    cnt = np.zeros(n, np.int32)
    for valid, alb, nrm, t in hits_per_k:
        first = valid & (cnt == 0)
        more = valid & (cnt > 0)
        sa[first] = alb[first]; sn[first] = nrm[first]; st[first] = t[first]
        sa[more] = sa[more] + alb[more]; sn[more] = sn[more] + nrm[more]; st[more] = st[more] + t[more]
        cnt += valid
    out_a = np.zeros((n, 4), np.float32); out_n = np.zeros((n, 4), np.float32)
    hit = cnt > 0
    c = cnt[hit].astype(np.float32)
    out_a[hit, :3] = sa[hit] / c[:, None]
    out_a[hit, 3] = c / np.float32(aov_spp)
    out_n[hit, :3] = sn[hit] / c[:, None]
    out_n[hit, 3] = st[hit] / c
    return out_a, out_n


def sample_texture(tex, start, width, height, uv):
    """reflectors.cuh bilinear lookup (pt_shade.h sample_texture) for one uv pair, in float32 steps."""
    f32 = np.float32
    if width <= 0 or height <= 0:
        return None
    fx = f32(uv[0]) * f32(width) - f32(0.5)
    fy = f32(uv[1]) * f32(height) - f32(0.5)
    flx, fly = np.floor(fx), np.floor(fy)
    xi, yi = int(flx), int(fly)
    sx, sy = f32(fx - flx), f32(fy - fly)
    x0, y0, x1, y1 = xi % width, yi % height, (xi + 1) % width, (yi + 1) % height
    c = lambda x, y: tex[start + y * width + x, :3].astype(np.float32)
    bottom = c(x0, y0) * (f32(1) - sx) + c(x1, y0) * sx
    top = c(x0, y1) * (f32(1) - sx) + c(x1, y1) * sx
    return (bottom * (f32(1) - sy) + top * sy).astype(np.float32)


def passthrough_mask(rgba_sum, spp, albedo):
    m = rgba_sum.astype(np.float32) / np.float32(spp)
    return (albedo[..., 3] <= 0) | ~np.isfinite(m[..., :3]).all(-1)


def denoise(rgba_sum, spp, albedo, normal_depth, iterations=5, sigma_color=1.0, sigma_normal=64.0, sigma_depth=0.02):
    """The a-trous filter of pt_denoise in float64 (after the f32 mean, as the kernel's first step)."""
    S = np.asarray(rgba_sum, np.float32)
    h, w = S.shape[:2]
    m = (S / np.float32(spp)).astype(np.float64)
    skip = passthrough_mask(S, spp, albedo)
    use = ~skip
    a = np.where(albedo[..., :3] >= np.float32(0.01), albedo[..., :3], np.float32(1.0)).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = m[..., :3] / a
    e[skip] = 0.0
    L = float((e[use] @ LUMA).mean()) if use.any() else 0.0
    n = normal_depth[..., :3].astype(np.float64)
    ln = np.linalg.norm(n, axis=-1)
    nzero = ln == 0
    nh = np.where(nzero[..., None], 0.0, n / np.where(nzero, 1.0, ln)[..., None])
    z = normal_depth[..., 3].astype(np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    for i in range(iterations):
        s = 1 << i
        den = sigma_color ** 2 * L * L * 2.0 ** -i + 1e-20
        num = (H5[2] ** 2) * e
        wsum = np.full((h, w), H5[2] ** 2)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dx == 0 and dy == 0:
                    continue
                yq, xq = ys + dy * s, xs + dx * s
                inside = (yq >= 0) & (yq < h) & (xq >= 0) & (xq < w)
                yc, xc = np.clip(yq, 0, h - 1), np.clip(xq, 0, w - 1)
                ok = inside & use[yc, xc] & use
                eq = e[yc, xc]
                wc = np.exp(-((e - eq) ** 2).sum(-1) / den)
                cos = (nh * nh[yc, xc]).sum(-1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    wn = np.where(nzero | nzero[yc, xc], 0.0, np.maximum(0.0, cos) ** sigma_normal)
                    wz = np.exp(-np.abs(z - z[yc, xc]) / (sigma_depth * z))
                wt = np.where(ok, H5[dx + 2] * H5[dy + 2] * wc * wn * wz, 0.0)
                num += wt[..., None] * eq
                wsum += wt
        e = np.where(use[..., None], num / wsum[..., None], e)
    out = S.astype(np.float64).copy()
    out[..., :3] = np.where(use[..., None], spp * a * e, S[..., :3])
    return out, skip, L


def mse(a, b, mask):
    d = (a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64))[mask]
    return float((d * d).mean())
