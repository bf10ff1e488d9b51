"""Ray buffers for Scene.query_radiance / query_closest / query_shadow: camera models the library's own pt_camera (a pinhole or thin
lens on a pixel grid) does not have. Plain numpy, or torch when `device` is given; no library call. Every function returns an
[n, 8] float32 array of pt_ray records (ox, oy, oz, max_t, dx, dy, dz, pad), row-major over the image (ray y*w + x), with unit
directions and pad = 0: ray i then draws from stream first_stream + i.

    pano = sc.query_radiance(rays.panorama_rays((0, 0, 1.5), 2048, 1024), spp=16, max_depth=8).reshape(1024, 2048, 4) / 16

irradiance_records and records_from_surfaces make the records of Scene.query_irradiance in the same layout: a surface point where a
ray has its origin, the unit normal where it has its direction. sh_records and sh_grid make the records of Scene.query_sh (a probe
position; the direction words are not read); sh_basis and sh_irradiance evaluate what it returns.

distance_records makes the records of Scene.query_distance (sh_records' layout with a max_t chosen for the lookups; sh_grid lays them
out on the same grid as the SH probes). oct_decode and oct_encode are the call's octahedral map and its inverse, oct_border gives a
map the gutter a seamless bilinear lookup needs, distance_visibility is the Chebyshev test of a point against a probe's map, and
grid_irradiance mixes the eight probes around a point by trilinear weight times that visibility, so that a probe behind a wall
stops lighting the point:

    probes, near = rays.sh_grid(lo, hi, (8, 8, 8)), rays.sh_grid(lo, hi, (8, 8, 8), max_t=1.5 * cell_diagonal)
    sums, maps = sc.query_sh(probes, 256, 4, 8), sc.query_distance(near, 8, spp_lane=4)
    e = rays.grid_irradiance(lo, hi, (8, 8, 8), sums, 1024, points, normals, maps, 4)
"""
import numpy as np

from .api import QUERY_MAX_T


def _xp(device):
    if device is None:
        return np, {}
    import torch
    return torch, {"device": device}


def _records(xp, kw, o, d, n, max_t):
    out = xp.zeros((n, 8), dtype=xp.float32, **kw)
    out[:, 0:3] = o
    out[:, 3] = max_t
    out[:, 4:7] = d
    return out


def panorama_rays(origin, w, h, max_t=QUERY_MAX_T, device=None):
    """An equirectangular panorama from `origin`: column x is the azimuth (x + 0.5) / w * 2 pi about +y, counted from -z towards +x
    (the library's cameras look down -z), row y the elevation ((y + 0.5) / h - 0.5) * pi: the first row looks down, the last up."""
    xp, kw = _xp(device)
    az = (xp.arange(w, dtype=xp.float64, **kw) + 0.5) / w * (2.0 * np.pi)
    el = ((xp.arange(h, dtype=xp.float64, **kw) + 0.5) / h - 0.5) * np.pi
    ce, se = xp.cos(el)[:, None], xp.sin(el)[:, None]
    d = xp.stack([ce * xp.sin(az)[None, :], se * xp.ones_like(az)[None, :], -ce * xp.cos(az)[None, :]], -1).reshape(h * w, 3)
    d = d / xp.sqrt((d * d).sum(-1))[:, None]
    o = xp.asarray(np.asarray(origin, np.float64), **kw).reshape(1, 3)
    return _records(xp, kw, o.to(xp.float32) if xp is not np else o, d.to(xp.float32) if xp is not np else d, h * w, max_t)


def irradiance_records(points, normals, max_t=QUERY_MAX_T, device=None):
    """Records for Scene.query_irradiance: [n, 8] float32 (point, max_t, normal, pad = 0) from [n, 3] points and normals (numpy, or
    with `device` anything torch.as_tensor takes). The normals must be unit length and are copied as given: the library does not
    normalise them."""
    xp, kw = _xp(device)
    as_f32 = (lambda v: np.asarray(v, np.float32)) if xp is np else (lambda v: xp.as_tensor(v, dtype=xp.float32, **kw))
    p, nrm = as_f32(points).reshape(-1, 3), as_f32(normals).reshape(-1, 3)
    if len(p) != len(nrm):
        raise ValueError("irradiance_records: %d points but %d normals" % (len(p), len(nrm)))
    return _records(xp, kw, p, nrm, len(p), max_t)


def records_from_surfaces(surfaces, max_t=QUERY_MAX_T):
    """Records for Scene.query_irradiance from Scene.query_closest(..., surfaces=True)'s surfaces: a RAY_SURFACE_DTYPE array (numpy)
    or the [n, 12] float32 tensor of the device form, whose point and facing normal are copied bit for bit. A ray that missed
    (material -1) gives the record (0, 0, 0), max_t = 0, normal (0, 0, 1): no first segment hits anything below 0, so its sums are
    exact zeros."""
    if isinstance(surfaces, np.ndarray):
        s = np.ascontiguousarray(surfaces)
        f = s.view(np.float32).reshape(len(s), 12) if s.dtype.names else np.ascontiguousarray(s, np.float32).reshape(-1, 12)
        out = np.zeros((len(f), 8), np.float32)
        hit = f.view(np.int32)[:, 8] >= 0
    else:
        import torch
        f = surfaces.reshape(-1, 12)
        out = torch.zeros((f.shape[0], 8), dtype=torch.float32, device=f.device)
        hit = f.view(torch.int32)[:, 8] >= 0
    out[:, 0:3] = f[:, 0:3]
    out[:, 4:7] = f[:, 4:7]
    out[:, 3] = hit * np.float32(max_t)
    out[:, 6] += ~hit
    return out


def sh_records(points, max_t=QUERY_MAX_T, device=None):
    """Records for Scene.query_sh: [n, 8] float32 (probe position, max_t, three words the call does not read, pad = 0) from [n, 3]
    points (numpy, or with `device` anything torch.as_tensor takes)."""
    xp, kw = _xp(device)
    p = (np.asarray(points, np.float32) if xp is np else xp.as_tensor(points, dtype=xp.float32, **kw)).reshape(-1, 3)
    return _records(xp, kw, p, 0.0, len(p), max_t)


def sh_grid(lo, hi, counts, max_t=QUERY_MAX_T, device=None, offsets=None):
    """Records for Scene.query_sh on a regular grid of counts = (nx, ny, nz) probes from corner lo to corner hi, both included (a
    count of 1 puts the probe at lo's coordinate): probe (ix, iy, iz) is record (iz * ny + iy) * nx + ix, x fastest. With `offsets`
    [n, >= 3] (api.grid_relocate's; numpy or a tensor) probe j stands at its float32 grid position plus offsets[j, :3] as float32,
    added in float32."""
    ax = [np.linspace(float(a), float(b), int(c)) if int(c) > 1 else np.array([float(a)]) for a, b, c in zip(lo, hi, counts)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)
    if offsets is not None:
        off = offsets if isinstance(offsets, np.ndarray) or not hasattr(offsets, "cpu") else offsets.cpu().numpy()
        p = p + np.asarray(off, np.float32).reshape(len(p), -1)[:, :3]
    return sh_records(p, max_t, device)


SH_C = (0.2820948, 0.4886025, 1.0925484, 0.3153916, 0.5462742)      # the constants of include/pt_api.h, seven digits each
SH_LOBE = (np.pi, 2.0 * np.pi / 3.0, np.pi / 4.0)                    # the clamped cosine lobe's factor per band


def sh_basis(d):
    """The nine real spherical harmonics of bands 0..2 at directions d [..., 3], as pt_query_sh orders and writes them: [..., 9] in
    d's dtype (numpy or torch)."""
    xp = np if isinstance(d, np.ndarray) else __import__("torch")
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c0, c1, c2, c3, c4 = SH_C
    return xp.stack([c0 + 0 * x, c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c3 * (3 * (z * z) - 1), c2 * (x * z), c4 * (x * x - y * y)], -1)


def _sh_convolved(coeff_sums, samples):
    """Scene.query_sh's sums [..., 9, 4] as irradiance coefficients [..., 9, 3]: scaled by 4 pi / samples, band l times the cosine
    lobe's factor."""
    xp = np if isinstance(coeff_sums, np.ndarray) else __import__("torch")
    lobe = [SH_LOBE[0]] + [SH_LOBE[1]] * 3 + [SH_LOBE[2]] * 5
    lobe = np.asarray(lobe, coeff_sums.dtype) if xp is np else xp.tensor(lobe, dtype=coeff_sums.dtype, device=coeff_sums.device)
    return coeff_sums[..., :3] * (4.0 * np.pi / samples) * lobe[:, None]


def sh_irradiance(coeff_sums, samples, normals):
    """Irradiance at unit `normals` [m, 3] from Scene.query_sh's sums [n, 9, 4] of `samples` = lanes * spp_lane samples each: the
    sums scaled by 4 pi / samples are the radiance coefficients, band l is convolved with the cosine lobe (pi, 2 pi / 3, pi / 4), and
    the series is evaluated at the normals. Returns [n, m, 3] in the units of pi * S / N of Scene.query_irradiance."""
    xp = np if isinstance(coeff_sums, np.ndarray) else __import__("torch")
    e = _sh_convolved(coeff_sums, samples)                                             # [n, 9, 3]
    y = sh_basis(normals if xp is not np else np.asarray(normals, coeff_sums.dtype).reshape(-1, 3))     # [m, 9]
    return xp.einsum("nkc,mk->nmc", e, y.to(e.dtype) if xp is not np else y)


def distance_records(points, max_t, device=None):
    """Records for Scene.query_distance: sh_records' layout, [n, 8] float32 (probe position, max_t, three words the call does not
    read, pad = 0) from [n, 3] points; sh_grid(lo, hi, counts, max_t) makes the same records on a grid. max_t is the distance a miss
    counts with, and every hit beyond it clamps there: set it to the largest distance a lookup will ask about, for example 1.5
    diagonals of a grid cell. With QUERY_MAX_T's 999999 one miss swamps a texel's mean and variance."""
    return sh_records(points, max_t, device)


def _xp_of(a):
    return np if isinstance(a, np.ndarray) else __import__("torch")


def oct_decode(uv):
    """The octahedral map of pt_query_distance (include/pt_api.h) from points uv [..., 2] of the unit square to unit directions
    [..., 3], in uv's dtype (numpy or torch): z is the fold axis, the square's centre +z, its corners -z."""
    xp = _xp_of(uv)
    fx, fy = 2 * uv[..., 0] - 1, 2 * uv[..., 1] - 1
    ax, ay = xp.abs(fx), xp.abs(fy)
    z = (1 - ax) - ay
    x = xp.where(z < 0, xp.copysign(1 - ay, fx), fx)
    y = xp.where(z < 0, xp.copysign(1 - ax, fy), fy)
    il = 1 / xp.sqrt(x * x + y * y + z * z)
    return xp.stack([x * il, y * il, z * il], -1)


def oct_encode(d):
    """oct_decode's inverse, from directions d [..., 3] (any length but 0) to points [..., 2] of the unit square: p = d / (|x| + |y| +
    |z|); below the fold (z < 0) (x, y) = ((1 - |y|) sign x, (1 - |x|) sign y); uv = (p + 1) / 2. The sign of a zero is its sign
    bit, so -z itself goes to the corner its zeros name."""
    xp = _xp_of(d)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    s = xp.abs(x) + xp.abs(y) + xp.abs(z)
    px, py = x / s, y / s
    one = xp.ones_like(px)
    qx = xp.where(z < 0, (1 - xp.abs(py)) * xp.copysign(one, x), px)
    qy = xp.where(z < 0, (1 - xp.abs(px)) * xp.copysign(one, y), py)
    return xp.stack([(qx + 1) / 2, (qy + 1) / 2], -1)


def oct_border(maps):
    """Octahedral maps [..., R, R, C] (indexed [ty, tx], as Scene.query_distance returns them) with a gutter of one texel:
    [..., R + 2, R + 2, C]. Each gutter texel copies the interior texel the octahedral wrap of its centre reaches, so that a bilinear
    lookup is seamless across the square's edges: u < 0 goes to (-u, 1 - v), u > 1 to (2 - u, 1 - v), v < 0 to (1 - u, -v), v > 1 to
    (1 - u, 2 - v), and a corner, by both rules, to the diagonally opposite interior corner."""
    xp = _xp_of(maps)
    r = maps.shape[-2]
    ty, tx = np.meshgrid(np.arange(-1, r + 1), np.arange(-1, r + 1), indexing="ij")
    ty, tx = ty.copy(), tx.copy()
    for out, flip in ((tx < 0, -1 - tx), (tx > r - 1, 2 * r - 1 - tx)):         # u outside: u mirrored at its edge, v at the middle
        tx, ty = np.where(out, flip, tx), np.where(out, r - 1 - ty, ty)
    for out, flip in ((ty < 0, -1 - ty), (ty > r - 1, 2 * r - 1 - ty)):
        ty, tx = np.where(out, flip, ty), np.where(out, r - 1 - tx, tx)
    if xp is not np:
        ty, tx = xp.as_tensor(ty, device=maps.device), xp.as_tensor(tx, device=maps.device)
    return maps[..., ty, tx, :]


def distance_visibility(maps, samples, d, dist, power=3):
    """How much of a probe a point at distance `dist` [...] in direction `d` [..., 3] from it sees, by Chebyshev's inequality on the
    probe's map: maps [..., R, R, >= 2] are Scene.query_distance's sums of `samples` = spp_lane samples a texel, the leading shape
    that of dist. (A, B) / samples is looked up bilinearly at oct_encode(d) on the bordered map, texel centres at (i + 0.5) / R, which
    gives the mean distance m and the mean square; var = max(mean square - m * m, 0). The result is 1 where dist <= m, else
    (var / (var + (dist - m)^2)) ** power, with 0 / 0 as 0. In maps' dtype."""
    xp = _xp_of(maps)
    r = maps.shape[-2]
    lead = tuple(maps.shape[:-3])
    b = (oct_border(maps[..., :2]) / samples).reshape((-1, r + 2, r + 2, 2))
    uv = oct_encode(d).reshape((-1, 2))
    dist = dist.reshape((-1,)) if hasattr(dist, "reshape") else dist
    gx, gy = uv[:, 0] * r + 0.5, uv[:, 1] * r + 0.5                            # in texels of the bordered map, whose texel j has its centre at j
    fl = (lambda v: np.clip(np.floor(v), 0, r).astype(np.int64)) if xp is np else (lambda v: xp.clamp(xp.floor(v), 0, r).to(xp.int64))
    ix, iy = fl(gx), fl(gy)
    wx, wy = (gx - ix)[:, None], (gy - iy)[:, None]
    k = np.arange(len(ix)) if xp is np else xp.arange(len(ix), device=maps.device)
    top = b[k, iy, ix] + wx * (b[k, iy, ix + 1] - b[k, iy, ix])                  # a + w (b - a): equal texels interpolate to themselves
    bot = b[k, iy + 1, ix] + wx * (b[k, iy + 1, ix + 1] - b[k, iy + 1, ix])
    m = top + wy * (bot - top)
    mean, var = m[:, 0], m[:, 1] - m[:, 0] * m[:, 0]
    var = xp.where(var > 0, var, 0 * var)
    den = var + (dist - mean) * (dist - mean)
    ratio = xp.where(den > 0, var / xp.where(den > 0, den, 1 + 0 * den), 0 * den)
    return xp.where(dist <= mean, 1 + 0 * den, ratio ** power).reshape(lead)


def grid_irradiance(lo, hi, counts, coeff_sums, sh_samples, points, normals, maps=None, map_samples=None, power=3, states=None, offsets=None):
    """Irradiance at `points` [m, 3] with unit `normals` [m, 3] from the probes of an sh_grid(lo, hi, counts): coeff_sums [n, 9, 4]
    are Scene.query_sh's sums of sh_samples samples a probe, maps [n, R, R, >= 2] (optional) Scene.query_distance's of map_samples
    samples a texel, both in the grid's order (x fastest). Per point the eight probes around it (clamped at the grid's faces) are
    weighted trilinearly times distance_visibility of the point as seen from the probe, and the result is sum(w E_j(n)) / sum(w), E_j
    being probe j's sh_irradiance at the point's normal. Without maps, or where the weights sum to less than 1e-6, the plain
    trilinear mix. With `states` [n] (api.grid_classify's words; bit 0, api.PROBE_INSIDE, marks a dead probe) the dead corners are
    left out of every sum, and a point whose weights sum to less than 1e-6 (or a grid without maps) that lost a corner gets the plain
    mix of its live corners divided by their trilinear weights' sum, zeros where that sum is 0. With `offsets` [n, >= 3]
    (api.grid_relocate's) probe j stands at its grid position + offsets[j, :3] for the visibility test; the cell and the trilinear
    weights stay the regular grid's. Returns [m, 3] in coeff_sums' dtype (numpy or torch)."""
    xp = _xp_of(coeff_sums)
    dt = coeff_sums.dtype
    conv = (lambda v: np.asarray(v, dt)) if xp is np else (lambda v: xp.as_tensor(v, dtype=dt, device=coeff_sums.device))
    p, nrm = conv(points).reshape((-1, 3)), conv(normals).reshape((-1, 3))
    counts = [int(c) for c in counts]
    i0, i1, f, pos = [], [], [], []
    for a in range(3):
        step = (float(hi[a]) - float(lo[a])) / (counts[a] - 1) if counts[a] > 1 else 0.0
        g = (p[:, a] - float(lo[a])) / step if counts[a] > 1 else 0 * p[:, a]
        lowc = np.clip(np.floor(g), 0, max(counts[a] - 2, 0)) if xp is np else xp.clamp(xp.floor(g), 0, max(counts[a] - 2, 0))
        fa = np.clip(g - lowc, 0, 1) if xp is np else xp.clamp(g - lowc, 0, 1)
        lowi = lowc.astype(np.int64) if xp is np else lowc.to(xp.int64)
        i0.append(lowi); i1.append(lowi + 1 if counts[a] > 1 else lowi); f.append(fa); pos.append((float(lo[a]), step))
    y = sh_basis(nrm)                                                               # [m, 9]
    e = _sh_convolved(coeff_sums, sh_samples)                                       # [n, 9, 3]
    num, den, plain, live_sum, lost = 0, 0, 0, 0, False
    if states is not None:
        dead = (np.asarray(states).astype(np.int64) & 1) != 0 if xp is np else (xp.as_tensor(states, device=coeff_sums.device).to(xp.int64) & 1) != 0
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                ix, iy, iz = (i1[0] if cx else i0[0]), (i1[1] if cy else i0[1]), (i1[2] if cz else i0[2])
                tri = (f[0] if cx else 1 - f[0]) * (f[1] if cy else 1 - f[1]) * (f[2] if cz else 1 - f[2])
                j = (iz * counts[1] + iy) * counts[0] + ix
                ej = (e[j] * y[:, :, None]).sum(1)                                  # [m, 3]
                if states is not None:                                              # a dead corner adds exact zeros, whatever it holds
                    gone = dead[j]
                    tri, ej = xp.where(gone, 0 * tri, tri), xp.where(gone[:, None], 0 * ej, ej)
                    live_sum, lost = live_sum + tri, lost | gone
                plain = plain + tri[:, None] * ej
                if maps is not None:
                    at = xp.stack([pos[a][0] + pos[a][1] * (ix, iy, iz)[a] for a in range(3)], -1)      # the probe's position
                    if offsets is not None:
                        at = (at.astype(dt) if xp is np else at.to(dt)) + conv(offsets).reshape((len(e), -1))[j][:, :3]
                    v = p - (at.astype(dt) if xp is np else at.to(dt))
                    dist = xp.sqrt((v * v).sum(-1))
                    d = xp.where((dist > 0)[:, None], v, conv([0.0, 0.0, 1.0])[None, :] + 0 * v)
                    w = tri * distance_visibility(maps[j], map_samples, d, dist, power)
                    if states is not None:
                        w = xp.where(gone, 0 * w, w)
                    num, den = num + w[:, None] * ej, den + w
    if states is not None:
        some = live_sum > 0
        plain = xp.where(lost[:, None], xp.where(some[:, None], plain / xp.where(some, live_sum, 1 + 0 * live_sum)[:, None], 0 * plain), plain)
    if maps is None:
        return plain
    ok = den >= 1e-6
    return xp.where(ok[:, None], num / xp.where(ok, den, 1 + 0 * den)[:, None], plain)


def orthographic_rays(origin, forward, up, width, height, w, h, max_t=QUERY_MAX_T, device=None):
    """An orthographic sensor of width x height scene units centred at `origin`, looking along `forward` with `up` up: every ray has
    the direction forward / |forward|; ray y*w + x starts at the centre of cell (x, y) of the sensor, x to the right (forward x up),
    y upwards."""
    xp, kw = _xp(device)
    f = np.asarray(forward, np.float64); f = f / np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64)); r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    sx = ((xp.arange(w, dtype=xp.float64, **kw) + 0.5) / w - 0.5) * width
    sy = ((xp.arange(h, dtype=xp.float64, **kw) + 0.5) / h - 0.5) * height
    c = lambda v: xp.asarray(v, **kw).reshape(1, 1, 3)
    o = (c(np.asarray(origin, np.float64)) + sx[None, :, None] * c(r) + sy[:, None, None] * c(u)).reshape(h * w, 3)
    d = xp.asarray(f.astype(np.float32), **kw).reshape(1, 3)
    return _records(xp, kw, o.to(xp.float32) if xp is not np else o, d, h * w, max_t)
