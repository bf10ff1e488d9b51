"""numpy restatement of pt_render_adaptive_moments and pt_denoise_var_tiles (include/pt_api.h), built on the restatements of
their halves: adaptive_ref.replay (the schedule) and denoise_var_ref (the moments and the variance-guided filter).

Used by tests/test_adaptive_moments_api.py (without a GPU) and tests/test_adaptive_moments.py to pin the HIP kernels."""
import numpy as np

import adaptive_ref
from denoise_var_ref import denoise_var, moments_from_partial_sums

F = np.float32


def pixel_map(tile_map, w, h):
    """[ceil(h/8), ceil(w/8)] per tile -> [h, w] per pixel: pixel (y, x) reads tile (y // 8, x // 8)."""
    return np.repeat(np.repeat(np.asarray(tile_map), 8, axis=0), 8, axis=1)[:h, :w]


def replay_moments(frame_at, w, h, min_spp, max_spp, chunk_spp, threshold):
    """adaptive_ref.replay plus "sq": every half-round is a batch of c = chunk_spp samples, so a tile that stops with
    tile_spp = n holds moments_from_partial_sums(frame_at(c), frame_at(2c), .., frame_at(n)) over its pixels, Q.w = n / c."""
    c = chunk_spp
    assert max_spp % (2 * c) == 0, "pt_render_adaptive_moments refuses a max_spp that is no multiple of 2 * chunk_spp"
    r = adaptive_ref.replay(frame_at, w, h, min_spp, max_spp, c, threshold)
    Q = np.zeros((h, w, 4), F)
    for n in np.unique(r["tile_spp"]):
        mask = pixel_map(r["tile_spp"] == n, w, h)
        Q[mask] = moments_from_partial_sums([np.asarray(frame_at(j * c), F) for j in range(1, int(n) // c + 1)])[mask]
    r["sq"] = Q
    return r


def denoise_var_tiles(rgba_sum, sq_sum, tile_spp, batch_spp, albedo, normal_depth, **kw):
    """pt_denoise_var_tiles: denoise_var_ref.denoise_var with spp and the batch count per pixel, from the tile map.
    denoise_var takes them as [h, w, 1] float32 arrays: every use of them there broadcasts over the channels
    (tests/test_adaptive_moments_api.py pins that a uniform map gives the scalar call bit for bit)."""
    h, w = np.asarray(rgba_sum).shape[:2]
    spp = pixel_map(tile_spp, w, h).astype(np.int64)
    return denoise_var(rgba_sum, sq_sum, spp.astype(F)[..., None], (spp // int(batch_spp)).astype(F)[..., None], albedo, normal_depth, **kw)
