"""The host side of the distance-probe tests, in numpy f32: the octahedral map from a texel and two uniforms to a unit direction, the
distance a sample counts with, and a lane's four sums, operation by operation in the order include/pt_api.h writes under
pt_query_distance. The fma is tests/irradiance_ref.py's. Nothing here calls the library."""
import numpy as np

from irradiance_ref import F, fma32


def texel_of_lane(lane, res):
    """(tx, ty) of lane l = ty * res + tx."""
    lane = np.asarray(lane, np.int64)
    return lane % res, lane // res


def oct_map(tx, ty, u1, u2, res):
    """d [n, 3] f32 of texel (tx, ty) of a res x res map at the uniforms (u1, u2): every operation rounded once, the dot fused as
    pt_device.h's dot() fuses it, the reciprocal of the f32 square root rounded on its own."""
    inv = F(1.0) / F(res)                                          # exact: res is a power of two
    tx, ty = np.atleast_1d(np.asarray(tx)).astype(F), np.atleast_1d(np.asarray(ty)).astype(F)
    u1, u2 = np.broadcast_to(np.asarray(u1, F), tx.shape), np.broadcast_to(np.asarray(u2, F), tx.shape)
    px, py = ((tx + u1).astype(F) * inv).astype(F), ((ty + u2).astype(F) * inv).astype(F)
    fx, fy = ((F(2.0) * px).astype(F) - F(1.0)).astype(F), ((F(2.0) * py).astype(F) - F(1.0)).astype(F)
    ax, ay = np.abs(fx), np.abs(fy)
    z = ((F(1.0) - ax).astype(F) - ay).astype(F)
    fold = z < 0
    x = np.where(fold, np.copysign((F(1.0) - ay).astype(F), fx), fx).astype(F)
    y = np.where(fold, np.copysign((F(1.0) - ax).astype(F), fy), fy).astype(F)
    dot = fma32(z, z, fma32(y, y, (x * x).astype(F)))
    il = (F(1.0) / np.sqrt(dot).astype(F)).astype(F)
    return np.stack([(x * il).astype(F), (y * il).astype(F), (z * il).astype(F)], 1)


def sample_r(t, tri, max_t):
    """r = hit ? t : max_t, [n] f32, from pt_query_closest's t and tri and the rays' max_t."""
    return np.where(np.asarray(tri) >= 0, np.asarray(t, F), np.asarray(max_t, F)).astype(F)


def texel_sums(samples):
    """[n, 4] f32 (A, B, H, K) from a list of per-sample (r, hit, back) triples of [n] arrays, in sample order:
    A = ((0 + r_0) + r_1) + ..., B likewise over r * r with the product rounded first, H and K the counts as floats."""
    n = len(samples[0][0])
    out = np.zeros((n, 4), F)
    for r, hit, back in samples:
        r = np.asarray(r, F)
        out[:, 0] = (out[:, 0] + r).astype(F)
        out[:, 1] = (out[:, 1] + (r * r).astype(F)).astype(F)
        out[:, 2] += np.asarray(hit, bool).astype(F)
        out[:, 3] += (np.asarray(hit, bool) & np.asarray(back, bool)).astype(F)
    return out


def from_closest(hits, surfaces, max_t):
    """One sample's (r, hit, back) from pt_query_closest's host-form records on the emitted rays."""
    hit = hits["tri"] >= 0
    return sample_r(hits["t"], hits["tri"], max_t), hit, surfaces["backface"] != 0
