"""pt_grid_pack and pt_grid_irradiance (include/pt_api.h) restated in numpy f32, operation by operation in the header's order: every
array below is float32, so every numpy operation rounds once as the device's does; the only fused steps are the fma32 calls. min and
max are np.fmin / np.fmax, which drop a NaN operand as v_min_f32 / v_max_f32 do."""
import numpy as np

from irradiance_ref import fma32

F = np.float32
SH_C = tuple(F(c) for c in (0.2820948, 0.4886025, 1.0925484, 0.3153916, 0.5462742))
LOBE = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5).astype(F)


def packed_bytes(counts, res):
    n = int(counts[0]) * int(counts[1]) * int(counts[2])
    return n * 9 * 16 + (n * (res + 2) * (res + 2) * 8 if res else 0)


def border_source(res):
    """(sy, sx), both [R + 2, R + 2] ints: the interior texel each texel of the bordered map copies, by the header's rule."""
    sy, sx = np.meshgrid(np.arange(-1, res + 1), np.arange(-1, res + 1), indexing="ij")
    sy, sx = sy.copy(), sx.copy()
    left, right = sx < 0, sx > res - 1
    sx, sy = np.where(left, -1 - sx, np.where(right, 2 * res - 1 - sx, sx)), np.where(left | right, res - 1 - sy, sy)
    below, above = sy < 0, sy > res - 1
    sy, sx = np.where(below, -1 - sy, np.where(above, 2 * res - 1 - sy, sy)), np.where(below | above, res - 1 - sx, sx)
    return sy, sx


def pack(sh_samples, coeff_sums, maps=None, map_samples=1):
    """(coeff [n, 9, 4], texels [n, R + 2, R + 2, 2] or None), f32, from query_sh's sums [n, 9, 4] and query_distance's maps [n, R, R, 4]."""
    c = np.asarray(coeff_sums, F).reshape(-1, 9, 4)
    scale = F(4.0 * np.pi / sh_samples)
    coeff = np.zeros_like(c)
    coeff[..., :3] = ((c[..., :3] * scale).astype(F) * LOBE[None, :, None]).astype(F)
    if maps is None:
        return coeff, None
    m = np.asarray(maps, F)
    res = m.shape[-2]
    sy, sx = border_source(res)
    return coeff, (m[:, sy, sx, :2] / F(map_samples)).astype(F)


def packed_words(coeff, texels):
    """The packed buffer as float32 words: the coefficient rows, then the bordered maps."""
    return np.concatenate([coeff.ravel()] + ([texels.ravel()] if texels is not None else [])).astype(F)


def basis(nrm):
    x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    c0, c1, c2, c3, c4 = SH_C
    return np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c3 * (F(3) * (z * z) - F(1)), c2 * (x * z),
                     c4 * (x * x - y * y)], 1).astype(F)


def visibility(texels, res, power, j, v):
    """Step 5 from v = p - at on: [m] f32."""
    with np.errstate(all="ignore"):
        dist = np.sqrt(fma32(v[:, 2], v[:, 2], fma32(v[:, 1], v[:, 1], v[:, 0] * v[:, 0])))
        d = np.where((dist > 0)[:, None], v, np.array([0, 0, 1], F)[None, :]).astype(F)
        s = (np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])
        px, py = d[:, 0] / s, d[:, 1] / s
        one = np.ones_like(px)
        fold = d[:, 2] < 0
        qx = np.where(fold, (F(1) - np.abs(py)) * np.copysign(one, d[:, 0]), px)
        qy = np.where(fold, (F(1) - np.abs(px)) * np.copysign(one, d[:, 1]), py)
        r = F(res)
        gx, gy = ((qx + F(1)) * F(0.5)) * r + F(0.5), ((qy + F(1)) * F(0.5)) * r + F(0.5)
        ix, iy = np.fmin(np.fmax(np.floor(gx), F(0)), r), np.fmin(np.fmax(np.floor(gy), F(0)), r)
        wx, wy = (gx - ix)[:, None], (gy - iy)[:, None]
        ix, iy = ix.astype(np.int64), iy.astype(np.int64)
        t = texels[j]
        k = np.arange(len(j))
        t00, t10, t01, t11 = t[k, iy, ix], t[k, iy, ix + 1], t[k, iy + 1, ix], t[k, iy + 1, ix + 1]
        top = t00 + wx * (t10 - t00)
        bot = t01 + wx * (t11 - t01)
        m = top + wy * (bot - top)
        mean = m[:, 0]
        var = m[:, 1] - mean * mean
        var = np.where(var > 0, var, F(0))
        tt = dist - mean
        den = var + tt * tt
        ratio = np.where(den > 0, var / np.where(den > 0, den, F(1)), F(0)).astype(F)
        vis = ratio
        for _ in range(1, power):
            vis = vis * ratio
        out = np.where(dist <= mean, F(1), vis)
    assert out.dtype == F and m.dtype == F and gx.dtype == F
    return out


def lookup(lo, hi, counts, coeff, texels, power, records):
    """(out [m, 4] f32, fallback [m] bool): pt_grid_irradiance on [m, 8] records, and where step 6 took the plain mix with maps."""
    rec = np.ascontiguousarray(records, F).reshape(-1, 8)
    ok = np.isfinite(rec[:, [0, 1, 2, 4, 5, 6]]).all(1)
    p, nrm = np.where(ok[:, None], rec[:, 0:3], F(0)).astype(F), np.where(ok[:, None], rec[:, 4:7], F(0)).astype(F)
    m = len(rec)
    lo, hi, counts = [F(v) for v in lo], [F(v) for v in hi], [int(c) for c in counts]
    res = texels.shape[-2] - 2 if texels is not None else 0
    low, f, step = [], [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            if counts[a] > 1:
                span = float(hi[a]) - float(lo[a])
                inv, st = F((counts[a] - 1) / span), F(span / (counts[a] - 1))
                g = (p[:, a] - lo[a]) * inv
                lw = np.fmin(np.fmax(np.floor(g), F(0)), F(counts[a] - 2))
                low.append(lw.astype(np.int64)); f.append(np.fmin(np.fmax(g - lw, F(0)), F(1))); step.append(st)
            else:
                low.append(np.zeros(m, np.int64)); f.append(np.zeros(m, F)); step.append(F(0))
        y = basis(nrm)
        plain, num, W = np.zeros((m, 3), F), np.zeros((m, 3), F), np.zeros(m, F)
        for cz in (0, 1):
            for cy in (0, 1):
                for cx in (0, 1):
                    c = (cx, cy, cz)
                    i = [low[a] + (c[a] if counts[a] > 1 else 0) for a in range(3)]
                    w3 = [f[a] if c[a] else F(1) - f[a] for a in range(3)]
                    tri = (w3[0] * w3[1]) * w3[2]
                    j = (i[2] * counts[1] + i[1]) * counts[0] + i[0]
                    E = coeff[j]                                                   # [m, 9, 4]
                    e = E[:, 0, :3] * y[:, 0:1]
                    for k in range(1, 9):
                        e = np.stack([fma32(E[:, k, ch], y[:, k], e[:, ch]) for ch in range(3)], 1)
                    plain = np.stack([fma32(tri, e[:, ch], plain[:, ch]) for ch in range(3)], 1)
                    if texels is None:
                        W = W + tri
                        continue
                    at = np.stack([fma32(i[a].astype(F), step[a], lo[a]) for a in range(3)], 1)
                    w = tri * visibility(texels, res, power, j, (p - at).astype(F))
                    num = np.stack([fma32(w, e[:, ch], num[:, ch]) for ch in range(3)], 1)
                    W = W + w
        assert plain.dtype == F and num.dtype == F and W.dtype == F and tri.dtype == F
        use = (W >= F(1e-6)) if texels is not None else np.zeros(m, bool)
        rgb = np.where(use[:, None], num / np.where(use, W, F(1))[:, None], plain)
    out = np.concatenate([rgb, W[:, None]], 1).astype(F)
    out[~ok] = 0
    return out, ok & ~use & (texels is not None)
