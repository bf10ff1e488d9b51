"""The host side of the SH-query tests, in numpy f32: the map from cosine_sample_f's local direction onto the sphere, the nine terms,
the term products, a lane's sum and the record's tree, operation by operation in the order include/pt_api.h writes under pt_query_sh.
The tree and the fma are tests/irradiance_ref.py's. Nothing here calls the library."""
import numpy as np

from irradiance_ref import F, fma32, tree          # noqa: F401  (fma32: for callers that restate a fused step beside these)

EPS = F(1e-5)
PI = F(3.141592)
C0, C1, C2, C3, C4 = F(0.2820948), F(0.4886025), F(1.0925484), F(0.3153916), F(0.5462742)


def local_direction(u1, u2):
    """cosine_sample_f's local direction [n, 3] f32 from the two uniforms, with numpy's f32 sine and cosine where the library has its
    own sincos_: good for the properties of the map, not for bits (the GPU tests take w from pt_probe_bsdf_sample)."""
    u1 = np.minimum(np.asarray(u1, F), F(1.0) - EPS)
    r = np.sqrt(u1)
    phi = ((F(2.0) * PI) * np.asarray(u2, F)).astype(F)
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(F(1.0) - u1)], 1).astype(F)


def sphere_map(w):
    """s = 2 w.z; d = (s w.x, s w.y, s w.z - 1): [n, 3] f32, every operation rounded once."""
    w = np.asarray(w, F).reshape(-1, 3)
    s = (F(2.0) * w[:, 2]).astype(F)
    return np.stack([s * w[:, 0], s * w[:, 1], (s * w[:, 2]).astype(F) - F(1.0)], 1).astype(F)


def basis(d):
    """Y_0 .. Y_8 at d [n, 3] f32: [n, 9] f32, every product and difference rounded once."""
    d = np.asarray(d, F).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    m = lambda a, b: (a * b).astype(F)
    return np.stack([np.full(len(d), C0, F), m(C1, y), m(C1, z), m(C1, x), m(C2, m(x, y)), m(C2, m(y, z)),
                     m(C3, (m(F(3.0), m(z, z)) - F(1.0)).astype(F)), m(C2, m(x, z)), m(C4, (m(x, x) - m(y, y)).astype(F))], 1).astype(F)


def terms(li, d):
    """t[k][c] = Li.c * Y_k(d): [n, 9, 3] f32 from li [n, >= 3] and d [n, 3]."""
    return (np.asarray(li, F)[:, None, :3] * basis(d)[:, :, None]).astype(F)


def lane_sum(ts):
    """((0 + t_0) + t_1) + ...: ts is a list of [m, 9, 3] f32 arrays, one per sample, in sample order."""
    acc = np.zeros_like(np.asarray(ts[0], F))
    for t in ts:
        acc = (acc + np.asarray(t, F)).astype(F)
    return acc


def coeffs(lane_sums):
    """pt_query_sh's output [n, 9, 4] f32 from the lanes' sums [n, L, 9, 3]: the adjacent-pair tree over the L lanes, and 0."""
    a = np.asarray(lane_sums, F)
    out = np.zeros((a.shape[0], 9, 4), F)
    out[:, :, :3] = tree(a)
    return out


def left_to_right(lane_sums):
    """What the tree is not: the same lanes added one after the other, [n, 9, 3] f32."""
    a = np.asarray(lane_sums, F)
    acc = np.zeros_like(a[:, 0])
    for l in range(a.shape[1]):
        acc = (acc + a[:, l]).astype(F)
    return acc
