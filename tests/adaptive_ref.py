"""numpy restatement of pt_render_adaptive's schedule and error estimator (include/pt_api.h), in float32 with the header's
operation order. Its input is `frame_at(n)`: the frame sum ([h, w, 4] float32) after n samples per pixel, e.g. pt_render(spp = n)
or the CPU reference at n samples. A tile that stops after n samples holds exactly frame_at(n) over its pixels."""
import numpy as np

F = np.float32


def tile_max(e, w, h):
    """[h, w] -> [ceil(h/8), ceil(w/8)]: the max over each 8x8 tile's in-image pixels (pixels outside the image count as 0)."""
    ty, tx = (h + 7) // 8, (w + 7) // 8
    pad = np.zeros((ty * 8, tx * 8), F)
    pad[:h, :w] = e
    return pad.reshape(ty, 8, tx, 8).max(axis=(1, 3))


def pixel_error(S, H, n):
    """e per pixel for the sums S and the half sums H (rgb, [h, w, 3] float32) after n samples."""
    with np.errstate(all="ignore"):
        two = F(2)
        d = np.abs(S[..., 0] - two * H[..., 0]) + np.abs(S[..., 1] - two * H[..., 1])
        d = d + np.abs(S[..., 2] - two * H[..., 2])
        inv = F(1) / F(n)
        lum = (S[..., 0] + S[..., 1]) + S[..., 2]
        e = (d * inv) / (F(1e-4) + np.sqrt(lum * inv))
        bad = ~np.isfinite(S).all(-1) | ~np.isfinite(H).all(-1) | np.isnan(e)
    e = np.where(bad, F(0), e).astype(F)
    return e


def replay(frame_at, w, h, min_spp, max_spp, chunk_spp, threshold):
    """The schedule. Returns dict: tile_spp [ty, tx] int32, tile_err [ty, tx] float32, rounds, ns (n after each round),
    errs (per round: the E_T of every tile, NaN where the tile was not live) and colors (each tile's sums at its tile_spp)."""
    ty, tx = (h + 7) // 8, (w + 7) // 8
    live = np.ones((ty, tx), bool)
    H = np.zeros((h, w, 3), F)
    spp = np.zeros((ty, tx), np.int32)
    err = np.zeros((ty, tx), F)
    n, ns, errs = 0, [], []
    thr = F(threshold)
    while live.any():
        c = min(chunk_spp, (max_spp - n) // 2)
        if c == 0:
            break
        M = np.asarray(frame_at(n + c), F)[..., :3]
        S = np.asarray(frame_at(n + 2 * c), F)[..., :3]
        with np.errstate(all="ignore"):
            H = (H + (S - M)).astype(F)
        n += 2 * c
        E = np.maximum(tile_max(pixel_error(S, H, n), w, h), F(0))
        spp[live] = n
        err[live] = E[live]
        errs.append(np.where(live, E, F(np.nan)))
        ns.append(n)
        live &= ~((n >= min_spp) & (E < thr))
    colors = np.zeros((h, w, 4), F)
    for m in np.unique(spp):
        mask = np.repeat(np.repeat(spp == m, 8, axis=0), 8, axis=1)[:h, :w]
        colors[mask] = np.asarray(frame_at(int(m)), F)[mask]
    return {"tile_spp": spp, "tile_err": err, "rounds": len(ns), "ns": ns, "errs": errs, "colors": colors}


def stats(tile_spp, w, h, n_last):
    """pt_adaptive_stats' tiles_at_max and pixel_samples for a tile_spp grid."""
    ty, tx = tile_spp.shape
    px = np.zeros((ty, tx), np.int64)
    for j in range(ty):
        for i in range(tx):
            px[j, i] = min(8, w - 8 * i) * min(8, h - 8 * j)
    return int((tile_spp == n_last).sum()), int((px * tile_spp).sum())


def pick_threshold(frame_at, w, h, min_spp, max_spp, chunk_spp, want_rounds=3):
    """A threshold at which tiles stop in at least `want_rounds` different rounds (counting the tiles that run to the end as
    one). With threshold 0 nobody stops, so that replay gives every tile's E_T in every round; candidates are midpoints of
    those values. Returns the candidate with the most distinct stopping rounds, or None if none reaches want_rounds."""
    full = replay(frame_at, w, h, min_spp, max_spp, chunk_spp, 0.0)
    E = np.stack(full["errs"])                                      # [rounds, ty, tx], all live
    ok = np.array([m >= min_spp for m in full["ns"]])
    vals = np.unique(E[ok])
    vals = vals[np.isfinite(vals)]
    if vals.size < 2:
        return None
    cands = (vals[:-1] + (vals[1:] - vals[:-1]) / 2).astype(F)
    cands = cands[np.linspace(0, cands.size - 1, min(cands.size, 64)).astype(int)]
    best, best_k = None, 0
    for t in cands:
        stop = np.where(ok[:, None, None] & (E < t), np.arange(E.shape[0])[:, None, None], E.shape[0])
        k = np.unique(stop.min(axis=0)).size
        if k > best_k:
            best, best_k = float(t), k
    return best if best_k >= want_rounds else None
