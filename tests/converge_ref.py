"""numpy restatement of the converge stages (include/pt_api.h: pt_temporal_select, pt_temporal_accumulate_live, and what
pt_render_moments_tiles leaves of a full moments frame). Independent of the kernels; used by tests/test_converge_api.py
(without a GPU), tests/test_converge.py and tests/converge_seq.py.

select() runs in float32 in the header's order, one rounding per operation. A float maximum does not depend on its order, so the
tile error is exact, not approximate."""
import numpy as np

import temporal_ref as T

f32 = np.float32
DEFAULTS = {"threshold": 0.5, "min_history": 8}


def tile_grid(h, w):
    return (h + 7) // 8, (w + 7) // 8


def per_pixel(a, h, w):
    """A per-tile array [tilesY, tilesX] spread over the frame's pixels [h, w]."""
    return np.repeat(np.repeat(a, 8, axis=0), 8, axis=1)[:h, :w]


def pixel_error(hist):
    """(r [h,w] float32 with exempt pixels and NaN at 0, exempt mask)."""
    hist = np.asarray(hist, f32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        exempt = (hist[..., 3] < 0) | ~np.isfinite(hist).all(-1)
        lum = (((f32(0.2126) * hist[..., 0]).astype(f32) + (f32(0.7152) * hist[..., 1]).astype(f32)).astype(f32)
               + (f32(0.0722) * hist[..., 2]).astype(f32)).astype(f32)
        r = (np.sqrt(hist[..., 3]).astype(f32) / (f32(1e-4) + np.sqrt(lum).astype(f32)).astype(f32)).astype(f32)
        r = np.where(r > 0, r, f32(0)).astype(f32)         # max(0, r): NaN and -0 give +0
    r[exempt] = 0
    return r, exempt


def select(hist, hist_len, threshold=DEFAULTS["threshold"], min_history=DEFAULTS["min_history"]):
    """pt_temporal_select. Returns (tile_err float32 [tilesY, tilesX], tile_live int32 of that shape, the live tiles ascending)."""
    hist = np.asarray(hist, f32); hist_len = np.asarray(hist_len, f32)
    h, w = hist_len.shape
    ty, tx = tile_grid(h, w)
    r, exempt = pixel_error(hist)
    with np.errstate(invalid="ignore"):
        young = ~exempt & (hist_len < f32(min_history))
    R = np.zeros((ty * 8, tx * 8), f32); R[:h, :w] = r       # a pixel outside the image contributes 0 and is not young
    Y = np.zeros((ty * 8, tx * 8), bool); Y[:h, :w] = young
    err = R.reshape(ty, 8, tx, 8).max(axis=(1, 3)).astype(f32)
    any_young = Y.reshape(ty, 8, tx, 8).any(axis=(1, 3))
    live = (~((err < f32(threshold)) & ~any_young)).astype(np.int32)
    return err, live, np.flatnonzero(live.ravel()).astype(np.int32)


def moments_tiles(S, Q, tile_live):
    """What pt_render_moments_tiles writes, from the full frame's (S, Q): the listed tiles' pixels, S = 0 and Q.rgb = 0 elsewhere."""
    h, w = S.shape[:2]
    m = per_pixel(np.asarray(tile_live) != 0, h, w)
    So = np.where(m[..., None], S, f32(0)).astype(f32)
    Qo = np.where(m[..., None], Q, f32(0)).astype(f32)
    Qo[..., 3] = Q[..., 3]
    return So, Qo


def accumulate_live(cam, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, prev_normal_depth, hist, hist_len, tile_live, **params):
    """pt_temporal_accumulate_live on the identity path: temporal_ref.accumulate where the map is live, the input history and
    length where it is 0. Returns (out_hist, out_hist_len)."""
    out, out_len, _ = T.accumulate(cam, None, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, prev_normal_depth, hist, hist_len, **params)
    if tile_live is None:
        return out, out_len
    h, w = out_len.shape
    m = per_pixel(np.asarray(tile_live) != 0, h, w)
    return np.where(m[..., None], out, np.asarray(hist, f32)).astype(f32), np.where(m, out_len, np.asarray(hist_len, f32)).astype(f32)
