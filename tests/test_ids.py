"""The ID pass and the pick queries (pt_render_ids, pt_pick) on the GPU against their numpy restatement (tests/ids_ref.py), bit for
bit: the restatement reads the library's own closest hits, link by link (pt_probe_centre_rays + pt_probe_trace_closest), so what is
compared is the choice of the reported surface, its four words, its point and the summed path length. The inputs are
tests/ids_cases.py's, whose classes tests/test_ids_ref_cpu.py asserts without a GPU."""
import numpy as np
import pytest

import aov_chain_ref as AC
import ids_cases as IC
import ids_ref as IR
import motion_cases as MC
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

W, H = IC.W, IC.H
GUARD = 64                      # int32 words before and after a device buffer
SENTINEL = 0x5a5a5a5a


class _Arrays:
    """What aov_chain_ref.Materials reads, over a dict of arrays."""
    def __init__(self, a):
        self.a = a

    def array(self, k):
        return self.a[k]


@pytest.fixture(scope="module")
def hosts(api, gpu_ready, scene_dir):
    """scene -> (host scene, Materials, light index by triangle)"""
    out = {}
    for scene in ("cornell", "glass_mirror"):
        hs = IC.host(api, scene_dir, scene, "ids_gpu_" + scene)
        out[scene] = (hs, AC.Materials(hs), IR.light_of_triangle(api, IC.host_arrays(hs)))
    return out


def _want(api, sc, mats, lights, cam, w, h, max_links, xy=None):
    rays = IC.library_centre_rays(api, cam, w, h) if xy is None else api.probe_centre_rays(cam, xy)
    return IR.ids_chain(sc, mats, rays, max_links, lights)


def _guarded(torch, n_words):
    buf = torch.full((GUARD + n_words + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    return buf, buf.data_ptr() + 4 * GUARD


def _unguard(buf, n_words, what):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + n_words:] == SENTINEL).all(), what + ": the guard band was written"
    return b[GUARD:GUARD + n_words]


@pytest.mark.parametrize("max_links", IC.LINKS)
@pytest.mark.parametrize("name", list(IC.CAMERAS))
def test_ids_are_the_restatement(api, hosts, name, max_links):
    hs, mats, lights = hosts[IC.CAMERAS[name][0]]
    cam = IC.camera(api, hs, name)
    for make in (api.Scene, api.Scene.from_mesh):               # pt_scene_create (the host's tree) and pt_scene_create_from_mesh
        sc = make(hs)
        want = _want(api, sc, mats, lights, cam, W, H, max_links)
        got = sc.render_ids(cam, W, H, max_links)
        c = IR.classes(want)
        print(name, max_links, make.__name__, c)
        assert np.array_equal(got.reshape(-1, 4), want["ids"]), np.flatnonzero((got.reshape(-1, 4) != want["ids"]).any(1))[:8]
        assert c["miss"] >= 16 and (name != "cornell_outside" or c["backface"] >= 8)
        if max_links == 1 and name != "cornell_outside":
            assert c["capped"] >= 8 and c["left"] >= 4 and c["in_mirror"] >= 4
        if max_links == 4 and name != "cornell_outside":
            assert c["behind_glass"] >= 8 and c["in_mirror"] >= 4 and c["left"] >= 4 and c["light"] >= 2
        # the pick form over every pixel: the same words, the surface's point and the centre pass's depth, bit for bit
        ids, hit = sc.pick(cam, W, H, IC.pixels(W, H), max_links)
        assert np.array_equal(ids, want["ids"])
        assert_bits_equal(hit, want["hit"], "%s %d: (point, depth)" % (name, max_links))
        nd = sc.render_aovs_centre(cam, W, H, max_links)[1]
        assert_bits_equal(hit[:, 3].reshape(H, W), nd[..., 3], "depth against pt_render_aovs_centre's")
        sc.close()


@pytest.mark.parametrize("size", [(13, 11), (1, 1)])
@pytest.mark.parametrize("name", ["cornell_outside", "glass_mirror"])
def test_ragged_sizes_write_only_the_image_and_the_device_form_is_the_host_form(api, gpu_ready, hosts, name, size):
    torch = gpu_ready
    w, h = size
    hs, mats, lights = hosts[IC.CAMERAS[name][0]]
    cam = IC.camera(api, hs, name, w, h)
    sc = api.Scene(hs)
    s = torch.cuda.Stream()
    for max_links in IC.LINKS:
        want = _want(api, sc, mats, lights, cam, w, h, max_links)
        host = sc.render_ids(cam, w, h, max_links)
        assert np.array_equal(host.reshape(-1, 4), want["ids"])
        buf, ptr = _guarded(torch, w * h * 4)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            sc.render_ids_device(cam, w, h, max_links, ptr, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(_unguard(buf, w * h * 4, "%s %dx%d links %d" % (name, w, h, max_links)).reshape(h, w, 4), host)
    sc.close()


def test_device_form_is_the_host_form_at_the_full_size(api, gpu_ready, hosts):
    torch = gpu_ready
    hs, _, _ = hosts["cornell"]
    cam = IC.camera(api, hs, "cornell")
    sc = api.Scene.from_mesh(hs)
    for max_links in IC.LINKS:
        buf, ptr = _guarded(torch, W * H * 4)
        torch.cuda.synchronize()
        sc.render_ids_device(cam, W, H, max_links, ptr)
        torch.cuda.synchronize()
        assert np.array_equal(_unguard(buf, W * H * 4, "links %d" % max_links).reshape(H, W, 4), sc.render_ids(cam, W, H, max_links))
    sc.close()


def test_pick_is_the_id_pass_at_the_pixel(api, hosts):
    hs, mats, lights = hosts["cornell"]
    cam = IC.camera(api, hs, "cornell")
    sc = api.Scene(hs)
    for max_links in IC.LINKS:
        want = _want(api, sc, mats, lights, cam, W, H, max_links)
        img = sc.render_ids(cam, W, H, max_links)
        nd = sc.render_aovs_centre(cam, W, H, max_links)[1]
        first = lambda m: tuple(int(v) for v in IC.pixels(W, H)[np.flatnonzero(m)[0]])
        xy = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), first(~want["valid"]), first(want["ids"][:, 2] >= 0)]
        if max_links == 4:
            xy.append(first(want["refracted"]))
        xy = np.array(xy + xy[:1], np.int32)                     # (a repeated pixel)
        ids, hit = sc.pick(cam, W, H, xy, max_links)
        assert np.array_equal(ids, img[xy[:, 1], xy[:, 0]])
        assert_bits_equal(hit[:, 3], nd[xy[:, 1], xy[:, 0], 3], "depth")
        assert_bits_equal(hit, want["hit"].reshape(H, W, 4)[xy[:, 1], xy[:, 0]], "(point, depth)")
        assert (ids[4] == np.array(IR.MISS)).all() and not hit[4].any() and ids[5, 2] >= 0 and (hit[5, 3] > 0)
        if max_links == 4:
            assert ids[6, 3] >> 8 >= 2                          # through the glass box: in and out
        one_ids, one_hit = sc.pick(cam, W, H, xy[5:6], max_links)
        assert np.array_equal(one_ids, ids[5:6]) and np.array_equal(one_hit.view(np.uint32), hit[5:6].view(np.uint32))
    # more than one wave of queries, in an order of their own
    xy = IC.pixels(W, H)[np.random.default_rng(1).permutation(W * H)[:200]]
    ids, _ = sc.pick(cam, W, H, xy, 4)
    assert np.array_equal(ids, sc.render_ids(cam, W, H, 4)[xy[:, 1], xy[:, 0]])
    with pytest.raises(api.PtError, match=r"pt_pick: pixel 1 is \(40, 3\), outside the 40 x 24 image"):
        sc.pick(cam, W, H, [(0, 0), (40, 3)], 0)
    sc.close()


def test_ids_follow_a_vertex_update(api, hosts):
    """The tall box moved (motion_cases): the ids are the restatement's over the updated scene's hits, and those of a scene built
    from the moved arrays."""
    hs, mats, lights = hosts["cornell"]
    cam = IC.camera(api, hs, "cornell")
    new = MC.moved_arrays(hs)
    sc = api.Scene.from_mesh(hs)
    before = {ml: sc.render_ids(cam, W, H, ml) for ml in IC.LINKS}
    sc.update_vertices(new["points"])
    fresh = api.Scene.from_mesh(new, hs.info["leaf_size"])
    for ml in IC.LINKS:
        got = sc.render_ids(cam, W, H, ml)
        want = _want(api, sc, mats, lights, cam, W, H, ml)
        assert np.array_equal(got.reshape(-1, 4), want["ids"])
        assert np.array_equal(got, fresh.render_ids(cam, W, H, ml))
        assert (got != before[ml]).any(-1).sum() >= 16
    fresh.close(); sc.close()


def test_chain_ids_follow_a_material_edit(api, hosts):
    """The glass box becomes a mirror (row 19 copied over row 5): what was seen through it is now what it reflects."""
    hs, mats, lights = hosts["cornell"]
    cam = IC.camera(api, hs, "cornell")
    a = MC.arrays(hs)
    m = a["materials"].reshape(-1, 176).copy()
    m[5] = m[19]
    a["materials"] = m.reshape(-1)
    mats2 = AC.Materials(_Arrays(a))
    assert mats2.type[5] == AC.MAT_MIRROR and mats.type[5] == AC.MAT_DIELECTRIC
    for make in (api.Scene, api.Scene.from_mesh):
        sc = make(hs)
        before = sc.render_ids(cam, W, H, 4)
        sc.update_materials(a["materials"])
        got = sc.render_ids(cam, W, H, 4)
        want = _want(api, sc, mats2, lights, cam, W, H, 4)
        assert np.array_equal(got.reshape(-1, 4), want["ids"])
        changed = (got != before).any(-1)
        glass_first = sc.render_ids(cam, W, H, 0)[..., 1] == 5
        direct = ~want["first_spec"].reshape(H, W)               # pixels whose first hit starts no chain, before and after
        assert changed[glass_first].sum() >= 16 and not changed[direct].any()
        assert not want["refracted"].any() and want["reflected"].reshape(H, W)[glass_first].sum() >= 8
        sc.close()


def test_the_light_word_is_update_emissions_index(api, hosts):
    hs, _, lights = hosts["cornell"]
    cam = IC.camera(api, hs, "cornell")
    for make in (api.Scene, api.Scene.from_mesh):
        sc = make(hs)
        ids = sc.render_ids(cam, W, H, 0)
        on_lamp = np.argwhere(ids[..., 2] >= 0)
        assert len(on_lamp) >= 3
        y, x = on_lamp[0]
        one, _ = sc.pick(cam, W, H, [(x, y)], 0)
        light = int(one[0, 2])
        assert light == ids[y, x, 2] == lights[ids[y, x, 0]]
        L0, A0 = sc.packed("lights"), sc.packed("attrs")
        assert 0 <= light < len(L0)
        sc.update_emission([light], [(0.25, 3.0, 7.5)])
        L1, A1 = sc.packed("lights"), sc.packed("attrs")
        rows = np.flatnonzero((L0 != L1).any(1))
        assert list(rows) == [light], rows                     # exactly that light's record
        f = L1[light].view(np.float32)
        assert all(np.float32(v) in f for v in (0.25, 3.0, 7.5))
        tri = np.flatnonzero((A0 != A1).any(1))
        assert list(tri) == list(np.flatnonzero(lights == light)), (tri, light)     # and exactly its triangle's attributes
        assert np.array_equal(sc.render_ids(cam, W, H, 0), ids)   # the ids do not depend on what a light emits
        sc.close()
