"""numpy restatement of the ID pass, the pick queries and the selection overlay (include/pt_api.h: pt_render_ids, pt_pick,
pt_select_overlay). Independent of the kernels; tests/test_ids_ref_cpu.py checks it without a GPU over the oracle's hits,
tests/test_ids.py, tests/test_select_overlay.py and tests/test_preview_select.py hold the library to it bit for bit.

The chain walk is aov_chain_ref's (the link rule and the direction arithmetic: Materials, next_rays), operation by operation, keeping
the END SURFACE's words: the surface of the last hit with i == 0 or a non-specular material, which is the one whose albedo the chain
guide holds. The centre rays are the caller's (the oracle's camera_ray without jitter and aperture, or pt_probe_centre_rays). The
light index of a triangle comes from api.light_triangles. The overlay is integer numpy."""
import numpy as np

import aov_chain_ref as AC

f32 = np.float32
MISS = (-1, -1, -1, 0)


def light_of_triangle(api, a):
    """Per ORIGINAL triangle the index of the light it is (pt_scene_update_emission's), or -1. a: the scene's arrays with "bvh" and
    "indices" (a host scene's own, or the oracle's build_bvh): api.light_triangles names each light's triangle in leaf order.
    Cross-checked against the triangles' own lightInd field."""
    n_tris = a["mesh"].size // 80
    idx = np.ascontiguousarray(a["indices"]).view(np.int32)
    out = np.full(n_tris, -1, np.int32)
    for light, pos in enumerate(api.light_triangles(arrays=a)):
        assert pos >= 0, "light %d has no triangle among the first 63" % light
        out[idx[pos]] = light
    n_lights = a["lights"].size // 80
    own = a["mesh"].reshape(-1, 80)[:, 64:68].copy().view(np.int32)[:, 0]
    assert np.array_equal(out, np.where((own >= 0) & (own < n_lights), own, -1))
    return out


def ids_chain(tracer, mats, rays, max_links, light_of_tri):
    """pt_render_ids / pt_pick for the centre rays `rays` [n, 6]. tracer.trace_closest(rays) gives the closest hits, link by link: an
    oracle scene, or an api.Scene for the library's own hits. mats: aov_chain_ref.Materials. Returns a dict of per-ray arrays:
    ids [n,4] int32, hit [n,4] float32 (point, summed path length), and the classes valid, first_spec, links (the reported ones),
    refracted / reflected (the reported surface lies behind at least one such link), left (the chain left the scene after a specular
    hit) and capped (still on a specular surface after max_links links, max_links >= 1)."""
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 6)
    n = len(rays)
    oi, of, _ = tracer.trace_closest(rays)
    valid = oi[:, 0] == 1
    tri = np.where(valid, oi[:, 1], -1).astype(np.int32)
    mat = np.where(valid, oi[:, 2], -1).astype(np.int32)
    back = valid & (oi[:, 3] != 0)
    point = np.where(valid[:, None], of[:, 3:6], f32(0)).astype(f32)
    depth_out = np.where(valid, of[:, 0], f32(0)).astype(f32)
    links = np.zeros(n, np.int32)
    refracted = np.zeros(n, bool); reflected = np.zeros(n, bool); left = np.zeros(n, bool); capped = np.zeros(n, bool)
    n_refr = np.zeros(n, np.int32); n_refl = np.zeros(n, np.int32)
    first_spec = valid & mats.in_chain[np.maximum(oi[:, 2], 0)]
    live = np.flatnonzero(first_spec)
    depth = of[:, 0].copy()
    cur_i, cur_f, cur_d = oi[live], of[live], rays[live, 3:6]
    for link in range(1, max_links + 1):
        if live.size == 0:
            break
        m = cur_i[:, 2]
        o2, d2, refl, _ = AC.next_rays(cur_d, cur_f[:, 3:6], cur_f[:, 6:9], cur_i[:, 3] != 0, mats.type[m] == AC.MAT_DIELECTRIC, mats.ior[m])
        n_refl[live] += refl; n_refr[live] += ~refl
        oi2, of2, _ = tracer.trace_closest(np.concatenate([o2, d2], 1))
        hit = oi2[:, 0] == 1
        left[live[~hit]] = True
        depth[live[hit]] = (depth[live[hit]] + of2[hit, 0]).astype(f32)
        go_on = hit & mats.in_chain[np.maximum(oi2[:, 2], 0)]
        done = hit & ~go_on
        idx = live[done]
        tri[idx] = oi2[done, 1]; mat[idx] = oi2[done, 2]; back[idx] = oi2[done, 3] != 0
        point[idx] = of2[done, 3:6]; depth_out[idx] = depth[idx]; links[idx] = link
        refracted[idx] = n_refr[idx] > 0; reflected[idx] = n_refl[idx] > 0
        live, cur_i, cur_f, cur_d = live[go_on], oi2[go_on], of2[go_on], d2[go_on]
    if max_links >= 1:
        capped[live] = True
    light = np.where(valid, light_of_tri[np.maximum(tri, 0)], -1).astype(np.int32)
    info = (back.astype(np.int32) | (links << 8)).astype(np.int32)
    ids = np.stack([tri, mat, light, np.where(valid, info, 0)], 1).astype(np.int32)
    hit4 = np.concatenate([point, depth_out[:, None]], 1).astype(f32)
    return dict(ids=ids, hit=hit4, valid=valid, first_spec=first_spec, links=links, refracted=refracted, reflected=reflected, left=left,
                capped=capped, backface=back)


def classes(r):
    """How many rays fall into each class the tests want exercised."""
    ids = r["ids"]
    return dict(miss=int((~r["valid"]).sum()), light=int((ids[:, 2] >= 0).sum()), backface=int((ids[:, 3] & 1).sum()),
                behind_glass=int(r["refracted"].sum()), in_mirror=int(r["reflected"].sum()), left=int(r["left"].sum()), capped=int(r["capped"].sum()))


def overlay(ids, rgba8, entries):
    """pt_select_overlay: a copy of rgba8 [h,w,4] uint8 with `entries` drawn from ids [h,w,4] int32, in order. An entry is
    (component, lo, hi, (r, g, b, outline alpha), radius, fill_alpha). Integer arithmetic only."""
    out = rgba8.copy()
    h, w = ids.shape[:2]
    for comp, lo, hi, colour, radius, fill_alpha in entries:
        v = ids[..., comp]
        m = (v >= lo) & (v <= hi)
        pad = np.pad(m, radius, constant_values=True)              # beyond the image: does not count
        whole = np.ones((h, w), bool)                              # every pixel of the window inside the image is selected
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                whole &= pad[radius + dy:radius + dy + h, radius + dx:radius + dx + w]
        a = np.where(m & ~whole, int(colour[3]), int(fill_alpha)).astype(np.int64)
        for c in range(3):
            blended = (out[..., c].astype(np.int64) * (255 - a) + int(colour[c]) * a + 127) // 255
            out[..., c] = np.where(m, blended, out[..., c]).astype(np.uint8)
    return out
