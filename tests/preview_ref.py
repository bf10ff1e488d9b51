"""numpy restatement of pt_resolve, written from include/pt_api.h ("preview"): radiance sums to the bytes a viewer shows.

Every step is f32, one rounding per operation, in the header's order. The one exception is powf: the power is taken in f64 and
rounded to f32 once, which is what a correctly rounded powf returns; the host libm's and the device's powf are within an ulp or
two of that, which can only move a value that sits on a rounding boundary of the byte conversion."""
import numpy as np

f32 = np.float32


def tile_counts(tile_spp, h, w):
    """The per-pixel sample count [h, w] f32 of a per-8x8-tile map [ceil(h/8), ceil(w/8)] int32."""
    return np.repeat(np.repeat(tile_spp, 8, axis=0), 8, axis=1)[:h, :w].astype(f32)


def mean(rgba, spp=0, tile_spp=None):
    """Steps 1-4: the division and novum_finalise's paint. w passes through; painted pixels get w = 0."""
    rgba = np.asarray(rgba, f32)
    h, w = rgba.shape[:2]
    n = tile_counts(tile_spp, h, w)[..., None] if tile_spp is not None else f32(spp)
    m = rgba.copy()
    with np.errstate(all="ignore"):
        m[..., :3] = rgba[..., :3] / n
    nan = np.isnan(m[..., :3]).any(-1)
    m[nan] = (1.0, 0.0, 1.0, 0.0)
    inf = np.isinf(m[..., :3]).any(-1)
    m[inf] = (0.0, 1.0, 0.0, 0.0)
    return m


def clamp01(v):
    """v < 0 -> 0, v > 1 -> 1, anything else (a NaN included) stays."""
    return np.where(v < 0, f32(0), np.where(v > 1, f32(1), v)).astype(f32)


def aces(c):
    c = np.asarray(c, f32)
    with np.errstate(all="ignore"):
        num = c * (f32(2.51) * c + f32(0.03))
        den = c * (f32(2.43) * c + f32(0.59)) + f32(0.14)
        return clamp01(num / den)


def to_byte(c):
    with np.errstate(all="ignore"):
        v = clamp01(c) * f32(255.0) + f32(0.5)
        return np.where(np.isnan(v), 0, np.nan_to_num(v, nan=0.0).astype(np.int32)).astype(np.uint8)


def display(m, tonemap=True, exposure=1.0):
    """Steps 5-7 on a mean [h, w, 4]: returns [h, w, 4] uint8 = (r, g, b, 255)."""
    with np.errstate(all="ignore"):
        c = (np.asarray(m, f32)[..., :3] * f32(exposure)).astype(f32)
        if tonemap:
            ig = f32(1.0) / f32(2.2)
            c = np.power(aces(c).astype(np.float64), np.float64(ig)).astype(f32)
    out = np.empty(m.shape[:2] + (4,), np.uint8)
    out[..., :3] = to_byte(c)
    out[..., 3] = 255
    return out


def resolve(rgba, spp=0, tile_spp=None, tonemap=True, exposure=1.0):
    """pt_resolve: (rgba8, mean)."""
    m = mean(rgba, spp, tile_spp)
    return display(m, tonemap, exposure), m


def bmp_pixels(path, w, h):
    """The 24-bit pixels novum_save_bmp wrote, as [h, w, 3] uint8 in r, g, b order, row 0 first as it was handed to the writer."""
    raw = np.fromfile(path, np.uint8)
    row = (3 * w + 3) & ~3
    assert raw.size == 54 + row * h and bytes(raw[:2]) == b"BM"
    px = raw[54:].reshape(h, row)[:, :3 * w].reshape(h, w, 3)
    return px[..., ::-1]
