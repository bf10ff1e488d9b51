"""The host side of the irradiance-query tests, in numpy f32: the adjacent-pair tree of S and Q over per-lane sums, the draw-offset
bookkeeping of a lane's samples, and the restatement of the world direction and the origin of a sample's ray from its local direction,
operation by operation in the order include/pt_api.h writes under pt_query_irradiance (as tests/aov_chain_ref.py restates the chain).
Nothing here calls the library."""
import numpy as np

F = np.float32
RAY_EPS = F(0.001)


def fma32(a, b, c):
    """a * b + c rounded once to f32. The product of two f32 is exact in f64; the f64 sum is then rounded to odd (TwoSum gives its
    error: where the sum is inexact and its last bit even, the neighbour on the error's side is the odd one), and a value rounded to
    odd at 53 bits rounds to f32 as the exact value does."""
    a, b, c = (np.atleast_1d(np.asarray(v, F)).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def tangent(nrm):
    """onb_tangent: [n, 3] f32."""
    nrm = np.asarray(nrm, F).reshape(-1, 3)
    x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    zero = np.zeros_like(x)
    x_arm = np.abs(x) > np.abs(z)                                  # the tie takes the second arm
    v = np.where(x_arm[:, None], np.stack([-y, x, zero], 1), np.stack([zero, -z, y], 1)).astype(F)
    d = fma32(v[:, 2], v[:, 2], fma32(v[:, 1], v[:, 1], v[:, 0] * v[:, 0]))
    il = F(1.0) / np.sqrt(d)                                       # f32 sqrt, then the f32 reciprocal: each rounded once
    return (v * il[:, None]).astype(F)


def cross(a, b):
    return np.stack([fma32(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1])), fma32(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2])),
                     fma32(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]))], 1)


def sample_ray(p, nrm, local):
    """(o, d), both [n, 3] f32, of a sample at points p with normals nrm whose local direction is `local`:
    d = (local.x * t + local.y * b) + local.z * nrm, o = p + nrm * RAY_EPS."""
    p, nrm, local = (np.asarray(v, F).reshape(-1, 3) for v in (p, nrm, local))
    t = tangent(nrm)
    b = cross(nrm, t)
    lx, ly, lz = local[:, 0:1], local[:, 1:2], local[:, 2:3]
    d = ((t * lx).astype(F) + (b * ly).astype(F)).astype(F) + (nrm * lz).astype(F)
    o = p + (nrm * RAY_EPS).astype(F)
    return o.astype(F), d.astype(F)


def tree(a):
    """The adjacent-pair tree over axis 1 of a, [n, L, ...] f32 with L a power of two: T_0 = a, T_(k+1)[l] = T_k[2l] + T_k[2l+1]."""
    t = np.asarray(a, F)
    assert t.shape[1] & (t.shape[1] - 1) == 0 and t.shape[1] >= 1
    while t.shape[1] > 1:
        t = (t[:, 0::2] + t[:, 1::2]).astype(F)
    return t[:, 0]


def sums(lane_sums):
    """(S, Q) as pt_query_irradiance writes them, both [n, 4] f32, from the lanes' sums a, [n, L, 3]: S = (tree(a), 0),
    Q = (tree(a * a), L), the product rounded before any sum."""
    a = np.asarray(lane_sums, F)
    n, lanes = a.shape[0], a.shape[1]
    s, q = np.zeros((n, 4), F), np.full((n, 4), F(lanes), F)
    s[:, :3] = tree(a[..., :3])
    q[:, :3] = tree((a[..., :3] * a[..., :3]).astype(F))
    return s, q


def lane_sum(li):
    """((0 + Li_0) + Li_1) + ...: li is a list of [m, >= 3] f32 arrays, one per sample, in sample order."""
    acc = np.zeros((len(li[0]), 3), F)
    for x in li:
        acc = (acc + np.asarray(x, F)[:, :3]).astype(F)
    return acc


def advance(offsets, hit):
    """The draw offsets of the lanes' next samples in the setting where Li reads no random number (integrator 2, max_depth 1, diffuse
    surfaces): a sample spends its two direction draws, and on a hit the two of the bounce's cosine_sample_f."""
    return (np.asarray(offsets, np.uint32) + np.uint32(2) + np.uint32(2) * np.asarray(hit, bool).astype(np.uint32)).astype(np.uint32)
