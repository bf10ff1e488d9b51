"""Ray buffers for Scene.query_radiance / query_closest / query_shadow: camera models the library's own pt_camera (a pinhole or thin
lens on a pixel grid) does not have. Plain numpy, or torch when `device` is given; no library call. Every function returns an
[n, 8] float32 array of pt_ray records (ox, oy, oz, max_t, dx, dy, dz, pad), row-major over the image (ray y*w + x), with unit
directions and pad = 0: ray i then draws from stream first_stream + i.

    pano = sc.query_radiance(rays.panorama_rays((0, 0, 1.5), 2048, 1024), spp=16, max_depth=8).reshape(1024, 2048, 4) / 16

irradiance_records and records_from_surfaces make the records of Scene.query_irradiance in the same layout: a surface point where a
ray has its origin, the unit normal where it has its direction. sh_records and sh_grid make the records of Scene.query_sh (a probe
position; the direction words are not read); sh_basis and sh_irradiance evaluate what it returns.
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


def sh_grid(lo, hi, counts, max_t=QUERY_MAX_T, device=None):
    """Records for Scene.query_sh on a regular grid of counts = (nx, ny, nz) probes from corner lo to corner hi, both included (a
    count of 1 puts the probe at lo's coordinate): probe (ix, iy, iz) is record (iz * ny + iy) * nx + ix, x fastest."""
    ax = [np.linspace(float(a), float(b), int(c)) if int(c) > 1 else np.array([float(a)]) for a, b, c in zip(lo, hi, counts)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return sh_records(np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32), max_t, device)


SH_C = (0.2820948, 0.4886025, 1.0925484, 0.3153916, 0.5462742)      # the constants of include/pt_api.h, seven digits each
SH_LOBE = (np.pi, 2.0 * np.pi / 3.0, np.pi / 4.0)                    # the clamped cosine lobe's factor per band


def sh_basis(d):
    """The nine real spherical harmonics of bands 0..2 at directions d [..., 3], as pt_query_sh orders and writes them: [..., 9] in
    d's dtype (numpy or torch)."""
    xp = np if isinstance(d, np.ndarray) else __import__("torch")
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c0, c1, c2, c3, c4 = SH_C
    return xp.stack([c0 + 0 * x, c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c3 * (3 * (z * z) - 1), c2 * (x * z), c4 * (x * x - y * y)], -1)


def sh_irradiance(coeff_sums, samples, normals):
    """Irradiance at unit `normals` [m, 3] from Scene.query_sh's sums [n, 9, 4] of `samples` = lanes * spp_lane samples each: the
    sums scaled by 4 pi / samples are the radiance coefficients, band l is convolved with the cosine lobe (pi, 2 pi / 3, pi / 4), and
    the series is evaluated at the normals. Returns [n, m, 3] in the units of pi * S / N of Scene.query_irradiance."""
    xp = np if isinstance(coeff_sums, np.ndarray) else __import__("torch")
    lobe = [SH_LOBE[0]] + [SH_LOBE[1]] * 3 + [SH_LOBE[2]] * 5
    lobe = np.asarray(lobe, coeff_sums.dtype) if xp is np else xp.tensor(lobe, dtype=coeff_sums.dtype, device=coeff_sums.device)
    e = coeff_sums[..., :3] * (4.0 * np.pi / samples) * lobe[:, None]                  # [n, 9, 3]
    y = sh_basis(normals if xp is not np else np.asarray(normals, coeff_sums.dtype).reshape(-1, 3))     # [m, 9]
    return xp.einsum("nkc,mk->nmc", e, y.to(e.dtype) if xp is not np else y)


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
