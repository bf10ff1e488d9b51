"""numpy restatement of the motion pass through mirrors and glass (include/pt_api.h: pt_render_motion_chain). Independent of the
kernel; tests/test_motion_chain_ref_cpu.py checks it without a GPU over the oracle's hits, tests/test_motion_chain.py and
tests/test_preview_motion_chain.py hold the library to it bit for bit over the library's own hits.

Built on aov_chain_ref (the link rule and the direction arithmetic: Materials, next_rays) and motion_ref (the first-hit pixel and
the previous point: motion, triangle_vertices). Everything is float32, one rounding per operation, in the header's order. The
history stage is motion_ref.accumulate, unchanged: it takes this buffer as it takes pt_render_motion's."""
import numpy as np

import aov_chain_ref as AC
import motion_ref as MR

f32 = np.float32


def triangles_moved(points_cur, points_prev, mesh):
    """Per ORIGINAL triangle: some of the nine floats of its current positions differs from the previous ones (bool [n_tris])."""
    cur, prev = MR._f4(points_cur)[:, :3], MR._f4(points_prev)[:, :3]
    idx = MR.triangle_vertices(mesh)
    return ~((cur[idx] == prev[idx]).all(-1).all(-1))


def _dot3(a, b):
    return ((a[:, 0] * b[:, 0]).astype(f32) + (a[:, 1] * b[:, 1]).astype(f32)).astype(f32) + (a[:, 2] * b[:, 2]).astype(f32)


def motion_chain(tracer, mats, rays, max_links, points_cur, points_prev, mesh):
    """pt_render_motion_chain's out_motion for the centre rays `rays` [n, 6] (pt_probe_centre_rays', or the oracle's camera_ray of
    the camera without jitter and aperture). tracer.trace_closest(rays) gives the closest hits, link by link: an oracle scene, or
    an api.Scene for the library's own hits. mats: aov_chain_ref.Materials. points_prev None: the scene has no previous positions.
    Returns a dict of per-ray arrays: motion [n,4] float32, links (the reported ones: 0 after a fallback), valid, reflections (the
    links that reflected, of the rays with links >= 1), tir, link_moved (some link's triangle moved)."""
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 6)
    n = len(rays)
    oi, of, _ = tracer.trace_closest(rays)
    valid = oi[:, 0] == 1
    out = MR.motion(points_cur, points_prev, mesh, (valid, of[:, 1], of[:, 2], oi[:, 1]))       # every ray starts as its first hit's pixel
    links = np.zeros(n, np.int32)
    refl = np.zeros(n, np.int32); tir_any = np.zeros(n, bool); link_moved = np.zeros(n, bool)
    tri_moved = triangles_moved(points_cur, points_prev, mesh) if points_prev is not None else None
    M = np.tile(np.eye(3, dtype=f32), (n, 1, 1))                                          # rows M[:, r]
    mat = np.maximum(oi[:, 2], 0)
    live = np.flatnonzero(valid & mats.in_chain[mat])
    depth = of[:, 0].copy()
    cur_i, cur_f, cur_d = oi[live], of[live], rays[live, 3:6]
    for link in range(1, max_links + 1):
        if live.size == 0:
            break
        m = cur_i[:, 2]
        nrm = cur_f[:, 6:9].astype(f32)
        o2, d2, reflected, t = AC.next_rays(cur_d, cur_f[:, 3:6], nrm, cur_i[:, 3] != 0, mats.type[m] == AC.MAT_DIELECTRIC, mats.ior[m])
        if tri_moved is not None:
            link_moved[live] |= tri_moved[cur_i[:, 1]]
        tir_any[live] |= t
        refl[live] += reflected
        for r in range(3):                                                                # the unfolding, at the links that reflected
            row = M[live, r]
            s = (f32(2) * _dot3(row, nrm)).astype(f32)
            new = (row - (s[:, None] * nrm).astype(f32)).astype(f32)
            M[live, r] = np.where(reflected[:, None], new, row)
        oi2, of2, _ = tracer.trace_closest(np.concatenate([o2, d2], 1))
        hit = oi2[:, 0] == 1
        depth[live[hit]] = (depth[live[hit]] + of2[hit, 0]).astype(f32)
        go_on = hit & mats.in_chain[np.maximum(oi2[:, 2], 0)]
        done = hit & ~go_on
        idx = live[done]
        links[idx] = link
        px = np.zeros((len(idx), 4), f32)
        if tri_moved is not None and len(idx):
            first = MR.motion(points_cur, points_prev, mesh, (np.ones(len(idx), bool), of2[done, 1], of2[done, 2], oi2[done, 1]))
            moved = (first[:, 3] == 1) & ~link_moved[idx]
            D = (first[:, :3] - of2[done, 3:6]).astype(f32)                               # P' - P
            Du = np.stack([_dot3(M[idx, r], D) for r in range(3)], 1).astype(f32)
            V = (rays[idx, :3] + (rays[idx, 3:6] * depth[idx, None]).astype(f32)).astype(f32)
            px[moved, :3] = (V + Du).astype(f32)[moved]
            px[moved, 3] = 1
        out[idx] = px
        live, cur_i, cur_f, cur_d = live[go_on], oi2[go_on], of2[go_on], d2[go_on]
    return dict(motion=out, links=links, valid=valid, reflections=np.where(links > 0, refl, 0), tir=tir_any & (links > 0), link_moved=link_moved)
