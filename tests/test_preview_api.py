"""pt_resolve and pt_preview without a GPU: the C ABI and the Python wrappers (symbols, struct layouts against the header,
defaults, argument checks that must fire before any HIP call), and the numpy restatement of the resolve (tests/preview_ref.py)
against the bytes novum_save_bmp writes."""
import ctypes
import os
import re

import numpy as np
import pytest

import preview_ref as R

NEW_SYMBOLS = ("pt_resolve_defaults", "pt_resolve", "pt_resolve_device", "pt_preview_defaults", "pt_preview_create", "pt_preview_frame",
               "pt_preview_reset", "pt_preview_read", "pt_preview_device_rgba8", "pt_preview_device_mean", "pt_preview_last_stats",
               "pt_preview_destroy")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pt_api.h")
f32 = np.float32


def _err(api):
    return api.lib().pt_last_error().decode()


def _header_fields(name):
    """Field names of `typedef struct NAME { ... } NAME;` in include/pt_api.h, in order (comments dropped)."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    names = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        names += words[1:]                                # the first word is the type
    return names


def _lognormal(w, h, seed):
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 4), f32)
    img[..., :3] = rng.lognormal(-1.0, 1.5, (h, w, 3)).astype(f32)
    return img


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported(api):
    L = api.lib()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    assert L.pt_api_version() == 1
    for name in ("ResolveParams", "PreviewParams", "PreviewStats", "Preview", "resolve", "resolve_device", "resolve_defaults", "preview_defaults",
                 "TemporalHistory"):
        assert hasattr(api, name), name


@pytest.mark.parametrize("cname,pyname,size", [("pt_resolve_params", "ResolveParams", 8), ("pt_preview_params", "PreviewParams", 68),
                                               ("pt_preview_stats", "PreviewStats", 28)])
def test_struct_layouts_match_the_header(api, cname, pyname, size):
    S = getattr(api, pyname)
    assert ctypes.sizeof(S) == size and ctypes.alignment(S) == 4
    assert [f for f, _ in S._fields_] == _header_fields(cname)
    offs = [getattr(S, f).offset for f, _ in S._fields_]
    assert offs == sorted(offs) and offs[0] == 0
    if cname == "pt_preview_params":                      # eight int32, then the three stages' structs back to back
        assert offs == [0, 4, 8, 12, 16, 20, 24, 28, 32, 44, 60]


def test_defaults(api):
    L = api.lib()
    buf = (ctypes.c_uint8 * 32)(*([0xAB] * 32))           # the C side writes exactly 8 bytes
    L.pt_resolve_defaults(ctypes.cast(buf, ctypes.POINTER(api.ResolveParams)))
    assert bytes(buf[8:]) == b"\xab" * 24
    p = api.ResolveParams.from_buffer_copy(bytes(buf[:8]))
    assert (p.tonemap, p.exposure) == (1, 1.0) and api.resolve_defaults() == {"tonemap": 1, "exposure": 1.0}
    buf = (ctypes.c_uint8 * 96)(*([0xAB] * 96))           # ... and exactly 68
    L.pt_preview_defaults(ctypes.cast(buf, ctypes.POINTER(api.PreviewParams)))
    assert bytes(buf[68:]) == b"\xab" * 28
    d = api.preview_defaults()
    assert [d[k] for k in ("spp", "batches", "max_depth", "integrator", "use_mis", "aov_spp", "temporal", "filter")] == [4, 2, 8, 0, 1, 1, 1, 1]
    assert d["temporal_params"] == api.temporal_defaults()
    assert d["filter_params"] == api.denoise_var_defaults()
    assert d["resolve_params"] == api.resolve_defaults()
    L.pt_resolve_defaults(None); L.pt_preview_defaults(None)          # ignored


def test_resolve_argument_checks(api):
    L = api.lib()
    w, h = 16, 8
    rgba = np.ones((h, w, 4), f32); out8 = np.zeros((h, w, 4), np.uint8); mean = np.zeros((h, w, 4), f32)
    tiles = np.full((1, 2), 4, np.int32)
    p, o, m, t = rgba.ctypes.data, out8.ctypes.data, mean.ctypes.data, tiles.ctypes.data

    def params(tonemap=1, exposure=1.0):
        return ctypes.byref(api.ResolveParams(tonemap, exposure))

    # (w, h, rgba, spp, tile_spp, params, rgba8, mean)
    cases = [
        ((0, h, p, 4, None, params(), o, m), "size"),
        ((w, -1, p, 4, None, params(), o, m), "size"),
        ((1 << 16, 1 << 16, p, 4, None, params(), o, m), "too large"),
        ((w, h, None, 4, None, params(), o, m), "null buffer"),
        ((w, h, p, 4, None, params(), None, m), "null output"),
        ((w, h, p, 0, None, params(), o, m), "spp 0 must be at least 1"),
        ((w, h, p, -2, None, params(), o, None), "spp -2 must be at least 1"),
        ((w, h, p, 4, None, params(tonemap=2), o, m), "tonemap 2"),
        ((w, h, p, 4, None, params(exposure=0.0), o, m), "exposure"),
        ((w, h, p, 4, None, params(exposure=-1.0), o, m), "exposure"),
        ((w, h, p, 4, None, params(exposure=float("nan")), o, m), "exposure"),
        ((w, h, p, 4, None, params(exposure=float("inf")), o, m), "exposure"),
        ((w, h, p, 4, None, params(), p, m), "alias"),
        ((w, h, p, 4, None, params(), o, p), "alias"),
        ((w, h, p, 4, None, params(), o, p + 64), "alias"),               # a partial overlap is one too
        ((w, h, p, 4, None, params(), m + 16, m), "alias"),               # the two outputs
        ((w, h, p, 4, t, params(), t, m), "alias"),                       # an output on the tile map
    ]
    for args, msg in cases:
        assert L.pt_resolve(*args) == -1, args
        assert msg in _err(api) and "pt_resolve" in _err(api), (args, _err(api))
        assert L.pt_resolve_device(*args, None) == -1, args
        assert msg in _err(api), (args, _err(api))
    # the host form reads its tile map: a count <= 0 is refused (the map overrides spp, so spp 0 is fine with a good map's check)
    for bad in (0, -3):
        tiles[0, 1] = bad
        assert L.pt_resolve(w, h, p, 0, t, params(), o, m) == -1
        assert "tile 1 has %d samples" % bad in _err(api)
    assert not out8.any() and not mean.any() and (rgba == 1).all()        # nothing ran
    with pytest.raises(api.PtError):
        api.resolve(np.zeros((h, w, 3), f32), 4)
    with pytest.raises(api.PtError):
        api.resolve(rgba, 4, tile_spp=np.ones((2, 2), np.int32))
    with pytest.raises(api.PtError):
        api.resolve(rgba, 4, tile_spp=np.ones((1, 2), np.int64))
    with pytest.raises(api.PtError, match="exposure"):
        api.resolve(rgba, 4, exposure=0.0)


def test_preview_null_arguments(api):
    L = api.lib()
    assert L.pt_preview_create(None, 64, 48, None) is None
    assert "pt_preview_create: null scene" in _err(api)
    with pytest.raises(api.PtError, match="null scene"):
        api.Preview(None, 64, 48)
    with pytest.raises(api.PtError, match="unknown parameter"):
        api.Preview(None, 64, 48, sigma_colour=1.0)
    cam = api.make_camera(True, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 60.0, 64, 48)
    out = api.PreviewStats()
    for rc, msg in ((L.pt_preview_frame(None, ctypes.byref(cam), 1), "pt_preview_frame"), (L.pt_preview_reset(None), "pt_preview_reset"),
                    (L.pt_preview_read(None, None, None, None, None), "pt_preview_read"),
                    (L.pt_preview_last_stats(None, ctypes.byref(out)), "pt_preview_last_stats")):
        assert rc == -1
    assert "pt_preview_last_stats" in _err(api)
    assert L.pt_preview_device_rgba8(None) is None and L.pt_preview_device_mean(None) is None
    L.pt_preview_destroy(None)                            # ignored


# ---- the restatement against the host's image writer -----------------------------------------------------------------------------
@pytest.mark.parametrize("post", [True, False])
def test_restatement_reproduces_save_bmp(api, tmp_path, post):
    w, h = 128, 96
    img = _lognormal(w, h, 5)
    img[3, 5, :3] = (-0.25, 0.0, 1e5)                     # below the clamp, exactly 0, far above it
    path = str(tmp_path / "a.bmp")
    api.save_bmp(path, img, post_process=post)
    want = R.bmp_pixels(path, w, h)
    got = R.display(img, tonemap=post)
    assert (got[..., 3] == 255).all()
    diff = got[..., :3] != want
    print("restatement vs novum_save_bmp, post %s: %d of %d bytes differ" % (post, diff.sum(), diff.size))
    assert not diff.any()
    assert len(np.unique(want)) > 200                     # the image exercises the whole byte range


def test_restatement_mean_is_finalise_and_adaptive_mean(api):
    w, h = 61, 43
    img = _lognormal(w, h, 6)
    img[..., 3] = 7.0
    img[2, 3, 1] = np.nan; img[4, 5, 0] = np.inf; img[4, 6, 2] = -np.inf; img[7, 7, :3] = (np.nan, np.inf, 1.0)
    m = R.mean(img, 3)
    assert np.array_equal(m.view(np.uint32), api.finalise(img, 3).view(np.uint32))
    assert tuple(m[2, 3]) == (1, 0, 1, 0) and tuple(m[4, 5]) == (0, 1, 0, 0) and tuple(m[4, 6]) == (0, 1, 0, 0) and tuple(m[7, 7]) == (1, 0, 1, 0)
    clean = _lognormal(w, h, 7)
    tiles = np.random.default_rng(8).integers(1, 9, ((h + 7) // 8, (w + 7) // 8)).astype(np.int32)
    assert np.array_equal(R.mean(clean, 0, tiles).view(np.uint32), api.adaptive_mean(clean, tiles).view(np.uint32))
    by = R.display(m, tonemap=False)
    assert tuple(by[2, 3]) == (255, 0, 255, 255) and tuple(by[4, 5]) == (0, 255, 0, 255)
    assert tuple(R.to_byte(np.array([np.nan, -1.0, 0.0, 0.5, 1.0, 2.0], f32))) == (0, 0, 0, 128, 255, 255)
