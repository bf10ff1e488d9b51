"""pt_grid_classify, pt_grid_update and pt_grid_irradiance_states (include/pt_api.h) restated in numpy f32, in the header's order, on
grid_ref's pieces: every array is float32, so every numpy operation rounds once as the device's does; the only fused steps are the
fma32 calls."""
import numpy as np

import grid_ref as GR
from irradiance_ref import fma32

F = np.float32
INSIDE, IDLE = 1, 2
# which arm of the lookup's end answered a record: W >= 1e-6 with maps; the plain mix with no corner skipped; the plain mix over the
# live trilinear sum; zeros (every corner dead or the live ones weightless); a record that is not finite
ARM_WEIGHTED, ARM_PLAIN, ARM_DIVIDED, ARM_DEAD, ARM_BAD = 0, 1, 2, 3, 4


def _list(indices, k, n):
    """(rows, probes): the rows of the fresh data that touch something, and the probe each names."""
    idx = np.arange(k) if indices is None else np.asarray(indices).astype(np.int64).reshape(-1)
    assert len(idx) == k and (indices is not None or k == n)
    rows = np.flatnonzero((idx >= 0) & (idx < n))
    return rows, idx[rows]


def classify(maps, back_fraction, n, indices=None, states=None):
    """states [n] uint32 (a copy; zeros when None) with the listed probes' words from maps [k, R, R, 4]."""
    m = np.asarray(maps, F)
    k = len(m)
    out = np.zeros(n, np.uint32) if states is None else np.array(states, np.uint32)
    rows, probes = _list(indices, k, n)
    hs = m[..., 2].reshape(k, -1).astype(np.float64).sum(1).astype(F)       # whole numbers below 2^22: the f64 sum is the f32 sum of any order
    ks = m[..., 3].reshape(k, -1).astype(np.float64).sum(1).astype(F)
    with np.errstate(all="ignore"):
        word = np.where(ks > F(back_fraction) * hs, INSIDE, 0) | np.where(hs == 0, IDLE, 0)
    out[probes] = word[rows].astype(np.uint32)
    return out


def _blend(h, old, fresh):
    h = F(h)
    if h == 0:
        return fresh.copy()
    with np.errstate(all="ignore"):
        return fma32(np.full(fresh.shape, h, F), (old - fresh).astype(F), fresh).reshape(fresh.shape)


def update(coeff, texels, sh_samples, coeff_sums, maps, map_samples, hysteresis, indices=None):
    """(coeff, texels) after pt_grid_update: copies of grid_ref.pack's arrays with the listed probes' words blended."""
    n = len(coeff)
    fresh_c, fresh_t = GR.pack(sh_samples, coeff_sums, maps, map_samples)
    rows, probes = _list(indices, len(fresh_c), n)
    coeff = np.array(coeff, F)
    new = _blend(hysteresis, coeff[probes][..., :3], fresh_c[rows][..., :3])
    row = np.zeros((len(rows), 9, 4), F)
    row[..., :3] = new
    coeff[probes] = row
    if texels is not None:
        texels = np.array(texels, F)
        texels[probes] = _blend(hysteresis, texels[probes], fresh_t[rows])
    return coeff, texels


def lookup(lo, hi, counts, coeff, texels, power, records, states):
    """(out [m, 4] f32, arm [m], T [m] f32): pt_grid_irradiance_states on [m, 8] records, the ARM_* that answered each, and the
    live corners' trilinear sum."""
    rec = np.ascontiguousarray(records, F).reshape(-1, 8)
    ok = np.isfinite(rec[:, [0, 1, 2, 4, 5, 6]]).all(1)
    p, nrm = np.where(ok[:, None], rec[:, 0:3], F(0)).astype(F), np.where(ok[:, None], rec[:, 4:7], F(0)).astype(F)
    m = len(rec)
    lo, hi, counts = [F(v) for v in lo], [F(v) for v in hi], [int(c) for c in counts]
    dead_probe = (np.asarray(states).astype(np.int64) & 1) != 0
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
                    if texels is None:
                        continue
                    at = np.stack([fma32(i[a].astype(F), step[a], lo[a]) for a in range(3)], 1)
                    w = tri * GR.visibility(texels, res, power, j, (p - at).astype(F))
                    num = np.where(live[:, None], np.stack([fma32(w, e[:, ch], num[:, ch]) for ch in range(3)], 1), num)
                    W = np.where(live, W + w, W)
        if texels is None:
            W = T
        assert plain.dtype == F and num.dtype == F and W.dtype == F and T.dtype == F
        weighted = (W >= F(1e-6)) if texels is not None else np.zeros(m, bool)
        divided = ~weighted & skipped & (T > 0)
        gone = ~weighted & skipped & ~(T > 0)
        arm = np.where(weighted, ARM_WEIGHTED, np.where(~skipped, ARM_PLAIN, np.where(divided, ARM_DIVIDED, ARM_DEAD)))
        rgb = np.where(weighted[:, None], num / np.where(weighted, W, F(1))[:, None],
                       np.where(divided[:, None], plain / np.where(divided, T, F(1))[:, None], plain))
    out = np.concatenate([rgb, W[:, None]], 1).astype(F)
    out[gone] = 0
    out[~ok] = 0
    return out, np.where(ok, arm, ARM_BAD), T
