"""pt_grid_relocate and pt_grid_irradiance_offsets (include/pt_api.h) restated in numpy f32, in the header's order, on grid_ref's and
grid_live_ref's pieces: every array is float32, so every numpy operation rounds once as the device's does; the only fused steps are
the fma32 calls. The texel-centre directions are distance_ref.oct_map's at u1 = u2 = 0.5."""
import numpy as np

import distance_ref as DR
import grid_live_ref as GL
import grid_ref as GR
from irradiance_ref import fma32

F = np.float32
KEPT, PUSHED_OUT, PUSHED_OFF = 0, 1, 2


def centre_direction(l, res):
    """c [3] f32 of texel l = ty * res + tx."""
    tx, ty = DR.texel_of_lane(l, res)
    return DR.oct_map(tx, ty, F(0.5), F(0.5), res)[0]


def chosen_texel(probe_map, map_samples, back_fraction):
    """(inside, l or None, m) of one probe's map [R, R, 4]: the header's candidate rule, the smallest (m, l)."""
    a = np.asarray(probe_map, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        m = (a[:, 0] / F(map_samples)).astype(F)
        H, K = a[:, 2], a[:, 3]
        back = (K + K).astype(F) > H
        front = (H > 0) & ~back
        hs, ks = F(H.astype(np.float64).sum()), F(K.astype(np.float64).sum())       # whole numbers below 2^22: every order gives this sum
        inside = bool(ks > F(back_fraction) * hs)
        cand = (m >= 0) & (back if inside else front)
    best = None
    for l in np.flatnonzero(cand):                                                  # ascending l: a strict < keeps the smaller l on a tie
        if best is None or m[l] < m[best]:
            best = int(l)
    return inside, best, (m[best] if best is not None else None)


def relocate(maps, map_samples, back_fraction, min_dist, max_offset, offsets, indices=None):
    """offsets [n, 4] f32 (a copy) after pt_grid_relocate on maps [k, R, R, 4]."""
    maps = np.asarray(maps, F)
    out = np.array(offsets, F).reshape(-1, 4)
    n, k, res = len(out), len(maps), maps.shape[-2]
    rows, probes = GL._list(indices, k, n)
    mn, mx = F(min_dist), np.asarray(max_offset, F).reshape(3)
    with np.errstate(all="ignore"):
        for row, j in zip(rows, probes):
            inside, l, m = chosen_texel(maps[row], map_samples, back_fraction)
            old = out[j, :3].copy()
            new, code = old, KEPT
            if l is not None and (inside or m < mn):
                c = centre_direction(l, res)
                if inside:
                    t = F(m + F(F(0.5) * mn))
                    new, code = fma32(c, np.full(3, t, F), old).reshape(3), PUSHED_OUT
                else:
                    t = F(mn - m)
                    new, code = fma32(-c, np.full(3, t, F), old).reshape(3), PUSHED_OFF
            out[j, :3] = np.fmin(np.fmax(new.astype(F), -mx), mx)
            out[j, 3] = code
    return out


def lookup(lo, hi, counts, coeff, texels, power, records, offsets, states=None):
    """(out [m, 4] f32, arm [m], T [m] f32): pt_grid_irradiance_offsets on [m, 8] records; grid_live_ref.lookup with the probe at
    fma(i, step, lo) + offset. states None: no probe is dead, and the arms are grid_ref.lookup's two."""
    assert texels is not None
    rec = np.ascontiguousarray(records, F).reshape(-1, 8)
    off = np.asarray(offsets, F).reshape(-1, 4)
    ok = np.isfinite(rec[:, [0, 1, 2, 4, 5, 6]]).all(1)
    p, nrm = np.where(ok[:, None], rec[:, 0:3], F(0)).astype(F), np.where(ok[:, None], rec[:, 4:7], F(0)).astype(F)
    m = len(rec)
    lo, hi, counts = [F(v) for v in lo], [F(v) for v in hi], [int(c) for c in counts]
    n = counts[0] * counts[1] * counts[2]
    dead_probe = (np.asarray(states).astype(np.int64) & 1) != 0 if states is not None else np.zeros(n, bool)
    res = texels.shape[-2] - 2
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
        y = GR.basis(nrm)
        plain, num, W, T = np.zeros((m, 3), F), np.zeros((m, 3), F), np.zeros(m, F), np.zeros(m, F)
        skipped = np.zeros(m, bool)
        for cz in (0, 1):
            for cy in (0, 1):
                for cx in (0, 1):
                    c = (cx, cy, cz)
                    i = [low[a] + (c[a] if counts[a] > 1 else 0) for a in range(3)]
                    w3 = [f[a] if c[a] else F(1) - f[a] for a in range(3)]
                    tri = (w3[0] * w3[1]) * w3[2]
                    j = (i[2] * counts[1] + i[1]) * counts[0] + i[0]
                    dead = dead_probe[j]
                    skipped |= dead
                    live = ~dead
                    E = coeff[j]
                    e = E[:, 0, :3] * y[:, 0:1]
                    for k in range(1, 9):
                        e = np.stack([fma32(E[:, k, ch], y[:, k], e[:, ch]) for ch in range(3)], 1)
                    plain = np.where(live[:, None], np.stack([fma32(tri, e[:, ch], plain[:, ch]) for ch in range(3)], 1), plain)
                    T = np.where(live, T + tri, T)
                    at = np.stack([fma32(i[a].astype(F), step[a], lo[a]).reshape(m) + off[j, a] for a in range(3)], 1)
                    assert at.dtype == F
                    w = tri * GR.visibility(texels, res, power, j, (p - at).astype(F))
                    num = np.where(live[:, None], np.stack([fma32(w, e[:, ch], num[:, ch]) for ch in range(3)], 1), num)
                    W = np.where(live, W + w, W)
        assert plain.dtype == F and num.dtype == F and W.dtype == F and T.dtype == F
        weighted = W >= F(1e-6)
        divided = ~weighted & skipped & (T > 0)
        gone = ~weighted & skipped & ~(T > 0)
        arm = np.where(weighted, GL.ARM_WEIGHTED, np.where(~skipped, GL.ARM_PLAIN, np.where(divided, GL.ARM_DIVIDED, GL.ARM_DEAD)))
        rgb = np.where(weighted[:, None], num / np.where(weighted, W, F(1))[:, None],
                       np.where(divided[:, None], plain / np.where(divided, T, F(1))[:, None], plain))
    out = np.concatenate([rgb, W[:, None]], 1).astype(F)
    out[gone] = 0
    out[~ok] = 0
    return out, np.where(ok, arm, GL.ARM_BAD), T


def fma_of_the_grid_is_never_minus_zero(lo, hi, counts):
    """The header's claim on the restatement: fma((float)i, step, lo) over every probe index of the grid has no -0."""
    for a in range(3):
        if int(counts[a]) > 1:
            st = F((float(F(hi[a])) - float(F(lo[a]))) / (int(counts[a]) - 1))
            v = fma32(np.arange(int(counts[a])).astype(F), np.full(int(counts[a]), st, F), np.full(int(counts[a]), F(lo[a]), F))
        else:
            v = fma32(np.zeros(1, F), np.zeros(1, F), np.full(1, F(lo[a]), F))
        if (np.signbit(v) & (v == 0)).any():
            return False
    return True
