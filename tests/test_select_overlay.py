"""The selection overlay (pt_select_overlay) on the GPU against its integer numpy restatement (tests/ids_ref.py), byte for byte, on
synthetic ID buffers built to touch what the kernel distinguishes: every component and radius, selections on each border and in a
corner (no outline along the frame), one pixel, four overlapping entries, images smaller than, equal to and larger than one 16x16
workgroup tile, and the alpha byte."""
import numpy as np
import pytest

import ids_ref as IR

pytestmark = pytest.mark.gpu

SIZES = [(40, 24), (13, 11), (1, 1)]
GUARD = 64


def _ids(w, h, seed=11):
    """An ID buffer of blobs: tri in 0..59 by 3x2 blocks with holes of misses, material = tri // 7, light 0 / 1 on two blocks and -1
    elsewhere; its last row and column and a corner block carry ids of their own."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    tri = ((y // 2) * 5 + x // 3) % 60
    ids = np.stack([tri, tri // 7, np.where(tri % 11 == 0, tri % 2, -1), rng.integers(0, 2, (h, w)) | (rng.integers(0, 3, (h, w)) << 8)], -1).astype(np.int32)
    ids[rng.random((h, w)) < 0.05] = IR.MISS
    ids[0, :, 0] = 100; ids[-1, :, 0] = 101; ids[:, 0, 0] = 102; ids[:, -1, 0] = 103       # each border (the corners: the columns')
    ids[:min(5, h), :min(6, w), 1] = 50                                                          # a block in the corner
    return np.ascontiguousarray(ids)


def _rgba(w, h, seed=12):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _check(api, ids, rgba, entries, what):
    want = IR.overlay(ids, rgba, entries)
    got = api.select_overlay(ids, rgba, entries)
    bad = np.argwhere((got != want).any(-1))
    assert not len(bad), "%s: %d pixels differ, first at (y, x) = %s: %s vs %s" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(got[..., 3], rgba[..., 3]), what + ": the alpha byte"
    return got


@pytest.mark.parametrize("size", SIZES)
def test_each_component_and_radius(api, gpu_ready, size):
    w, h = size
    ids, rgba = _ids(w, h), _rgba(w, h)
    changed = 0
    for comp, lo, hi in ((0, 10, 25), (1, 2, 4), (2, 0, 0), (2, 0, 1), (0, 0, 2 ** 31 - 1)):
        for radius in (1, 2, 3, 4):
            out = _check(api, ids, rgba, [(comp, lo, hi, (255, 40, 10, 200), radius, 60)], "%dx%d comp %d radius %d" % (w, h, comp, radius))
            changed += int((out != rgba).any())
    assert changed >= (16 if w > 1 else 1)


@pytest.mark.parametrize("size", SIZES)
def test_borders_a_corner_and_one_pixel(api, gpu_ready, size):
    w, h = size
    ids, rgba = _ids(w, h), _rgba(w, h)
    for radius in (1, 4):
        for tri in (100, 101, 102, 103):
            _check(api, ids, rgba, [(0, tri, tri, (0, 255, 0, 255), radius, 0)], "border %d radius %d" % (tri, radius))
        out = _check(api, ids, rgba, [(1, 50, 50, (9, 9, 250, 255), radius, 0)], "corner radius %d" % radius)
        if (w, h) == (40, 24) and radius == 1:
            assert np.array_equal(out[:4, :5], rgba[:4, :5]) and (out[4, :6, :3] == (9, 9, 250)).all()       # no outline along the frame
    one = np.tile(np.array(IR.MISS, np.int32), (h, w, 1))
    one[h // 2, w // 2] = (7, 1, 0, 0)
    for comp, v in ((0, 7), (1, 1), (2, 0)):
        out = _check(api, one, rgba, [(comp, v, v, (1, 2, 3, 255), 2, 0)], "one pixel")
        if w > 1:
            assert (out[h // 2, w // 2, :3] == (1, 2, 3)).all() and (out != rgba).any(-1).sum() == 1
    whole = np.zeros((h, w, 4), np.int32)
    out = _check(api, whole, rgba, [(1, 0, 0, (1, 2, 3, 255), 4, 0)], "the whole image")
    assert np.array_equal(out, rgba)                            # fill only, at fill alpha 0 (also the 1 x 1 image's one pixel)
    assert np.array_equal(_check(api, ids, rgba, [], "n = 0"), rgba)
    assert np.array_equal(_check(api, ids, rgba, [(0, 2000, 3000, (1, 1, 1, 255), 3, 255)], "nothing selected"), rgba)


@pytest.mark.parametrize("size", SIZES)
def test_four_overlapping_entries_apply_in_order(api, gpu_ready, size):
    w, h = size
    ids, rgba = _ids(w, h), _rgba(w, h)
    entries = [(0, 0, 40, (255, 0, 0, 255), 4, 90), (1, 1, 3, (0, 255, 0, 128), 1, 255), (2, 0, 1, (0, 0, 255, 77), 3, 13),
               (0, 5, 2 ** 31 - 1, (200, 200, 0, 255), 2, 0)]
    out = _check(api, ids, rgba, entries, "four entries")
    if w > 1:
        assert not np.array_equal(out, _check(api, ids, rgba, entries[::-1], "four entries, reversed"))
    for n in (1, 2, 3):
        _check(api, ids, rgba, entries[:n], "%d entries" % n)


@pytest.mark.parametrize("size", SIZES)
def test_device_form_is_the_host_form(api, gpu_ready, size):
    torch = gpu_ready
    w, h = size
    ids, rgba = _ids(w, h), _rgba(w, h)
    entries = [(0, 0, 40, (255, 0, 0, 255), 4, 90), (1, 50, 50, (0, 255, 0, 128), 2, 30)]
    want = api.select_overlay(ids, rgba, entries)
    d_ids = torch.from_numpy(ids).cuda()
    buf = torch.full((GUARD + w * h * 4 + GUARD,), 0xa5, dtype=torch.uint8, device="cuda:0")
    buf[GUARD:GUARD + w * h * 4] = torch.from_numpy(rgba.reshape(-1)).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        api.select_overlay_device(w, h, d_ids.data_ptr(), entries, buf.data_ptr() + GUARD, stream=s.cuda_stream)
    s.synchronize()
    b = buf.cpu().numpy()
    assert (b[:GUARD] == 0xa5).all() and (b[GUARD + w * h * 4:] == 0xa5).all()
    assert np.array_equal(b[GUARD:GUARD + w * h * 4].reshape(h, w, 4), want)
    assert np.array_equal(d_ids.cpu().numpy(), ids)
