"""numpy restatement of pt_render_aovs_chain (include/pt_api.h): feature buffers whose rays follow mirrors and glass.

Every closest hit (t, point, normal, material, backface, uv) is the ORACLE's trace_closest, the first rays are the oracle's
camera_ray, and material type, specular flag, ior, albedo and texture window are read from the oracle scene's 176-byte material
records. The direction arithmetic is the header's, one float32 rounding per operation, in the order written."""
import numpy as np

from denoise_ref import aovs_from_hits, sample_texture

F = np.float32
EPS = F(0.00001)
MAT_DIELECTRIC, MAT_MIRROR = 2, 6


class Materials:
    def __init__(self, osc):
        m = osc.array("materials").reshape(-1, 176)
        self.type = m[:, 32:36].copy().view(np.int32)[:, 0]
        self.albedo = m[:, 48:64].copy().view(np.float32)[:, :3]
        self.ior = m[:, 112:116].copy().view(np.float32)[:, 0]
        self.specular = m[:, 128] != 0
        self.has_tex = m[:, 0] != 0
        self.tex_info = m[:, 4:16].copy().view(np.int32)              # startInd, width, height
        self.in_chain = self.specular & ((self.type == MAT_MIRROR) | (self.type == MAT_DIELECTRIC))
        self.tex = osc.array("textures").view(np.float32).reshape(-1, 4) if self.has_tex.any() else None

    def albedo_at(self, mat, uv):
        """material_inputs' albedo at hits of materials `mat` [n] with uv [n, 2]: the material's, or the texture sample."""
        out = self.albedo[mat].astype(np.float32)
        for i in np.flatnonzero(self.has_tex[mat]):
            start, tw, th = (int(v) for v in self.tex_info[mat[i]])
            s = sample_texture(self.tex, start, tw, th, uv[i])
            if s is not None:
                out[i] = s
        return out


def next_rays(d, point, n, backface, is_dielectric, ior):
    """The header's direction arithmetic for a batch: returns (o', d', reflected [n] bool, tir [n] bool)."""
    d = d.astype(np.float32); n = n.astype(np.float32); point = point.astype(np.float32)
    dn = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    cos_i = np.minimum(np.maximum(-dn, EPS), F(1))
    eta = np.where(backface, ior, F(1) / ior).astype(np.float32)
    k = F(1) - (eta * eta) * (F(1) - cos_i * cos_i)
    refract = is_dielectric & ~(k < 0)
    tir = is_dielectric & (k < 0)
    with np.errstate(invalid="ignore"):
        cn = eta * cos_i - np.sqrt(np.where(refract, k, F(0)))
    s2 = F(2) * dn
    r = np.empty_like(d)
    for c in range(3):
        r[:, c] = np.where(refract, eta * d[:, c] + cn * n[:, c], d[:, c] - s2 * n[:, c])
    ln = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
    d2 = r / ln[:, None]
    off = n * EPS
    o2 = np.where(refract[:, None], point - off, point + off)
    return o2.astype(np.float32), d2.astype(np.float32), ~refract, tir


def chain_rays(osc, mats, rays, max_links):
    """Follow each ray of rays [n, 6]. Returns a dict of per-ray arrays: valid (the first ray hit), albedo [n,3], normal [n,3],
    depth, links (the reported ones: 0 after a fallback), and the classes first_spec, tir (some link was a total internal
    reflection), left (the chain left the scene) and out (still on a specular surface after max_links links)."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = len(rays)
    oi, of, _ = osc.trace_closest(rays)
    valid = oi[:, 0] == 1
    mat = np.maximum(oi[:, 2], 0)
    albedo = np.where(valid[:, None], mats.albedo_at(mat, of[:, 9:11]), F(0)).astype(np.float32)
    normal = of[:, 6:9].copy(); depth_out = of[:, 0].copy()
    links = np.zeros(n, np.int32)
    first_spec = valid & mats.in_chain[mat]
    tir = np.zeros(n, bool); left = np.zeros(n, bool); out = np.zeros(n, bool)
    live = np.flatnonzero(first_spec)
    depth = of[:, 0].copy()
    cur_i, cur_f, cur_d = oi[live], of[live], rays[live, 3:6]
    for link in range(1, max_links + 1):
        if live.size == 0:
            break
        m = cur_i[:, 2]
        o2, d2, _, t = next_rays(cur_d, cur_f[:, 3:6], cur_f[:, 6:9], cur_i[:, 3] != 0, mats.type[m] == MAT_DIELECTRIC, mats.ior[m])
        tir[live[t]] = True
        oi2, of2, _ = osc.trace_closest(np.concatenate([o2, d2], 1))
        hit = oi2[:, 0] == 1
        left[live[~hit]] = True
        depth[live[hit]] = depth[live[hit]] + of2[hit, 0]
        m2 = np.maximum(oi2[:, 2], 0)
        go_on = hit & mats.in_chain[m2]
        done = hit & ~go_on
        idx = live[done]
        albedo[idx] = mats.albedo_at(m2[done], of2[done, 9:11])
        normal[idx] = of2[done, 6:9]; depth_out[idx] = depth[idx]; links[idx] = link
        live, cur_i, cur_f, cur_d = live[go_on], oi2[go_on], of2[go_on], d2[go_on]
    out[live] = True
    tir &= ~(left | out)               # (a fallback reports the first hit: its TIR links are not in the result)
    return dict(valid=valid, albedo=albedo, normal=normal, depth=depth_out, links=links, first_spec=first_spec, tir=tir, left=left, out=out)


def camera_rays(O, cam, w, h, seed):
    cb = np.frombuffer(cam.tobytes() if hasattr(cam, "tobytes") else bytes(cam), np.uint8).copy()
    return np.array([O.camera_ray(cb, x, y, seed) for y in range(h) for x in range(w)], np.float32)


def chain_aovs(O, osc, cam, w, h, aov_spp, max_links, seed, mats=None):
    """pt_render_aovs_chain: (albedo [n,4], normal_depth [n,4], links [n], per-ray dicts over k), n = w*h scan-line."""
    mats = mats or Materials(osc)
    per_k = [chain_rays(osc, mats, camera_rays(O, cam, w, h, seed + k), max_links) for k in range(aov_spp)]
    a, nd = aovs_from_hits([(r["valid"], r["albedo"], r["normal"], r["depth"]) for r in per_k], aov_spp)
    cnt = sum(r["valid"].astype(np.int32) for r in per_k)
    lsum = sum(np.where(r["valid"], r["links"], 0).astype(np.int32) for r in per_k)
    links = np.zeros(w * h, np.float32)
    hit = cnt > 0
    links[hit] = lsum[hit].astype(np.float32) / cnt[hit].astype(np.float32)
    return a, nd, links, per_k


def classes(per_k):
    """How many rays of a case fall into each class the tests want exercised."""
    c = dict(diffuse_first=0, one_link=0, two_or_more=0, tir=0, fallback=0, miss=0)
    for r in per_k:
        fb = r["left"] | r["out"]
        c["diffuse_first"] += int((r["valid"] & ~r["first_spec"]).sum())
        c["one_link"] += int((r["links"] == 1).sum())
        c["two_or_more"] += int((r["links"] >= 2).sum())
        c["tir"] += int(r["tir"].sum())
        c["fallback"] += int(fb.sum())
        c["miss"] += int((~r["valid"]).sum())
    return c
