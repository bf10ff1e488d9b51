// pt_feature.h — what the feature kernels are assembled from (pt_aov.hip: aov_kernel, aov_chain_kernel, aov_centre_kernel,
// aov_centre_chain_kernel; pt_motion.hip: motion_kernel; pt_motion_chain.hip: motion_chain_kernel; pt_ids.hip: ids_kernel,
// ids_chain_kernel) and the ray-query kernels (pt_query.hip's trace kernels, pt_query_guides.hip, and pt_radiance.h's walk for
// pt_radiance.hip and pt_radiance_moments.hip: FeatureWave on 64 rays a tile). Every one of them is one wave per 8x8 tile
// (lane = ly*8+lx), four waves per workgroup, persistent over the tiles, with the non-counting trace_closest (max_t 999999, as
// pt_probe_trace_closest, or a caller's ray's own) on an LDS stack that overflows into the scene's spill area:
//   FeatureWave, tile_pixel   the wave's traversal state and the pixel of a lane in a tile
//   load_ray                  a caller's ray record (pt_query.hip, pt_query_guides.hip)
//   aov_stream                a XORWOW stream seeded in the kernel, into registers (the jittered aov kernels; pt_radiance.h)
//   first_hit_record          a resolved hit's (albedo, 1) and (normal, t)
//   follow_chain              a ray followed through mirrors and glass to the first non-specular surface; a kernel's ChainHook
//                             sees every surface and link on the way
//   MotionSrc                 what the motion kernels read beside the packed scene
//   FeatureSum                the sums over a pixel's rays and their division
// The __shared__ arrays stay declared in each kernel, so each kernel's LDS size is its own. pt_feature_host.h has the host's side.
#pragma once
#include "pt_path.h"
#include "pt_centre_ray.h"
#include "pt_feature_host.h"
#include "../../include/pt_api.h"

namespace pt {

// A wave's traversal state: its slice of the workgroup's LDS stack array and of the spill area ((gridDim.x * 4) waves x S.stackSpill
// entries x 64 lanes, the lane-interleaved layout of Stack), no scene cache, counters nobody reads. A kernel's tiles are
// gw, gw + gridDim.x * 4, ...; the stack is empty between traversals, so both slices serve every tile of the wave.
struct FeatureWave {
    Stack<kStackLds> st;
    SceneCache C;
    Ctr c;
    int wave, lane, gw;
    PT_DEV FeatureWave(int32_t (*ldsStack)[kStackLds][64], const DeviceScene& S, int32_t* spill) : c{} {
        wave = threadIdx.x >> 6;
        lane = threadIdx.x & 63;
        gw = blockIdx.x * 4 + wave;
        st.lds = (lds_i32*)&ldsStack[wave][0][0] + lane; st.sp = 0;
        st.spill = spill ? spill + (size_t)gw * S.stackSpill * 64 + lane : nullptr;
        C.nodes = nullptr; C.nNodes = 0; C.tris = nullptr; C.nTris = 0;
    }
};

// Ray `r` of a caller's buffer (pt_ray): (o, max_t), (d, pad).
struct QueryRay { V3 o, d; float maxT; };
PT_DEV QueryRay load_ray(const float4* __restrict__ rays, size_t r) {
    const float4 a = rays[2 * r], b = rays[2 * r + 1];
    return {v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), a.w};
}

// rng_init_kernel's per-lane body: stream `idx` of XORWOW(seed), via the 2^67-step jump matrices (row-image form).
PT_DEV Rng aov_stream(const uint32_t* __restrict__ jump, unsigned long long seed, uint32_t idx) {
    uint32_t s0 = (uint32_t)seed ^ 0xaad26b49u, s1 = (uint32_t)(seed >> 32) ^ 0xf7dcefddu;
    uint32_t t0 = 1099087573u * s0, t1 = 2591861531u * s1;
    uint32_t v[5] = {123456789u + t0, 362436069u ^ t0, 521288629u + t1, 88675123u ^ t1, 5783321u + t0};
    uint32_t d = 6615241u + t1 + t0;
    for (int k = 0; k < 32; k++) {
        if (!__ballot((idx >> k) & 1u)) continue;
        if ((idx >> k) & 1u) {
            const uint32_t* M = jump + (size_t)k * 800;
            uint32_t r[5] = {0, 0, 0, 0, 0};
            for (int i = 0; i < 5; i++) {
                uint32_t word = v[i];
#pragma unroll 4          // fully unrolled, the 800 row loads take 256 VGPRs (1 wave per SIMD); by 4: 76 VGPRs, 6 waves
                for (int j = 0; j < 32; j++) {
                    uint32_t m = 0u - ((word >> j) & 1u);
                    const uint32_t* row = M + (i * 32 + j) * 5;
                    r[0] ^= row[0] & m; r[1] ^= row[1] & m; r[2] ^= row[2] & m; r[3] ^= row[3] & m; r[4] ^= row[4] & m;
                }
            }
            for (int i = 0; i < 5; i++) v[i] = r[i];
        }
    }
    Rng rng = {v[0], v[1], v[2], v[3], v[4], d};
    return rng;
}

// The pixel of `lane` in tile `tile`; inside: the tile's last column and row may hang over the image.
struct TilePixel { int x, y; bool inside; };
PT_DEV TilePixel tile_pixel(int tile, int tilesX, int lane, int w, int h) {
    TilePixel p;
    p.x = (tile % tilesX) * 8 + (lane & 7); p.y = (tile / tilesX) * 8 + (lane >> 3);
    p.inside = p.x < w && p.y < h;
    return p;
}

// The record of a closest hit at distance t that resolve_hit has resolved into hi: (albedo, 1) and (normal, t), with material_inputs'
// albedo (the texture sample for textured materials), so t, the normal and the material are those of pt_probe_trace_closest.
// resolve_hit stays a call of the kernel's own: inside this function it costs the three first-hit kernels two VGPRs each (the
// vectorizer then packs the ray's direction before the traversal instead of after it), which takes aov_centre_kernel and motion_kernel
// from 63 to 65 and so from 8 waves per SIMD to 7.
PT_DEV void first_hit_record(const DeviceScene& S, const HitInfo& hi, float t, float4& oa, float4& on) {
    V3 a; float trans;
    material_inputs(S.mats[hi.material], S.textures, hi.uvx, hi.uvy, true, a, trans);
    oa = make_float4(a.x, a.y, a.z, 1.0f);
    on = make_float4(hi.normal.x, hi.normal.y, hi.normal.z, t);
}

// What a kernel does beside follow_chain's record at each step of its lane's chain: it passes a type with these two members. This
// one does nothing (aov_chain_kernel, aov_centre_chain_kernel).
struct ChainHook {
    // Hit i of the chain, resolved, at summed path length depth. With i == 0 or !spec its record is the chain's result unless a later
    // call says so too; with spec && i < maxLinks the chain goes on through it. (Plain arguments: with the two conditions formed at
    // the call the chain kernels of pt_aov.hip compile to other code, though this body is empty.)
    PT_DEV void surface(int i, const Hit& hit, const HitInfo& hi, bool spec, float depth) {}
    // The link through the surface just seen reflected (a mirror, or total internal reflection) or refracted, at normal n.
    PT_DEV void link(bool reflect, const V3& n) {}
};

// The ray (o, d) of a `live` lane followed through mirrors (type 6) and smooth dielectrics (type 2), deterministically, to the first
// non-specular surface or for maxLinks links. Returns the number of links followed, -1 if the ray hit nothing at all, and leaves in
// rec[j * 64], j = 0..6 (the lane's words of an LDS array float[7][64]) that surface's albedo and normal and the summed path length.
// One trace_closest call site serves the first ray (i = 0) and every link (i >= 1): lanes leave the loop at different links, the wave
// leaves it when one ballot finds no lane left, so every lane of the wave calls this, the ones without a ray with live = false.
// Live across a traversal: o, d, the running depth and the link count. The record lives in LDS, not in registers: it is written at the
// first hit, overwritten where the chain ends on a surface and simply stays when it does not (a miss after the first hit, or the cap),
// and the caller reads it once afterwards, so it need not be live across the traversals (7 VGPRs: 86 -> 6 waves per SIMD).
// The direction arithmetic is written out operation by operation (no dot(), normalize(), fmaf): tests/aov_chain_ref.py restates it.
// hook: the kernel's ChainHook; whatever it keeps is live across the traversals too. firstMaxT: the first ray's max_t (a caller's
// own ray, pt_query_guides.hip); every link's is 999999, and so is the first ray's in every kernel that passes none.
template <class Hook = ChainHook>
PT_DEV int follow_chain(const DeviceScene& S, const SceneCache& C, Stack<kStackLds>& st, Ctr& c, V3 o, V3 d, bool live, int maxLinks, float* rec,
                        Hook&& hook = Hook(), float firstMaxT = 999999.0f) {
    float depth = 0.0f;
    int links = -1;
    for (int i = 0; i <= maxLinks; i++) {
        if (!__ballot(live)) break;
        if (live) {
            Hit hit;
            trace_closest<false, kStackLds>(S, C, o, d, i == 0 ? firstMaxT : 999999.0f, st, hit, c);
            live = false;
            if (hit.tri >= 0) {                  // (a miss: no hit at all at i = 0, the first hit's record stands after that)
                HitInfo hi; resolve_hit(S, hit, o, d, hi);
                const PMat& m = S.mats[hi.material];
                const bool spec = (m.flags & kMatSpecular) && (m.type == 6 || m.type == 2);
                depth = i == 0 ? hit.t : depth + hit.t;
                hook.surface(i, hit, hi, spec, depth);
                if (i == 0 || !spec) {
                    V3 a; float trans;
                    material_inputs(m, S.textures, hi.uvx, hi.uvy, true, a, trans);
                    rec[0] = a.x; rec[64] = a.y; rec[128] = a.z;
                    rec[192] = hi.normal.x; rec[256] = hi.normal.y; rec[320] = hi.normal.z; rec[384] = depth;
                    links = i;
                }
                if (spec && i < maxLinks) {
                    const V3 n = hi.normal;
                    const float dn = d.x * n.x + d.y * n.y + d.z * n.z;
                    bool reflect = true;
                    V3 r = v3(0.0f);
                    if (m.type == 2) {
                        const float cosI = fminf_(fmaxf_(-dn, kEps), 1.0f);
                        const float eta = hi.backface ? m.ior : 1.0f / m.ior;
                        const float kk = 1.0f - (eta * eta) * (1.0f - cosI * cosI);
                        if (!(kk < 0.0f)) {
                            const float cn = eta * cosI - __builtin_sqrtf(kk);
                            r = v3(eta * d.x + cn * n.x, eta * d.y + cn * n.y, eta * d.z + cn * n.z);
                            reflect = false;
                        }
                    }
                    if (reflect) {
                        const float s2 = 2.0f * dn;
                        r = v3(d.x - s2 * n.x, d.y - s2 * n.y, d.z - s2 * n.z);
                    }
                    hook.link(reflect, n);
                    const float len = __builtin_sqrtf(r.x * r.x + r.y * r.y + r.z * r.z);
                    d = v3(r.x / len, r.y / len, r.z / len);
                    const V3 off = v3(n.x * kEps, n.y * kEps, n.z * kEps);
                    o = reflect ? v3(hi.point.x + off.x, hi.point.y + off.y, hi.point.z + off.z)
                                : v3(hi.point.x - off.x, hi.point.y - off.y, hi.point.z - off.z);
                    live = true;
                }
            }
        }
    }
    return links;
}

// What the motion passes read beside the packed scene, passed next to DeviceScene (which every megakernel takes and which stays as it
// is). prev NULL: the scene has no previous positions, every pixel is static.
struct MotionSrc {
    const pt_triangle* tris;    // original order: Hit::tri indexes it
    const float4* cur;          // nPos positions as of the last update (or creation)
    const float4* prev;         // ... and before it
    int nPos;
};

// The sums over the aov_spp rays of a pixel, in k order, and their division. The first contribution is stored, not added to 0, so
// that a -0 component survives (aov_spp = 1 is the hit itself: dividing by n = 1 changes no bit). Coverage is n / aov_spp.
struct FeatureSum {
    V3 a, n;
    float t;
    int hits;
    PT_DEV FeatureSum() : a(v3(0.0f)), n(v3(0.0f)), t(0.0f), hits(0) {}
    PT_DEV void add(V3 ra, V3 rn, float rt) {
        // (one branch around the additions, as the kernels had it: written as if / else it compiles to seven selects per ray,
        // which measured 0.3 to 0.5 % on the 82 k blob's jittered passes)
        if (hits != 0) { ra = a + ra; rn = n + rn; rt = t + rt; }
        a = ra; n = rn; t = rt;
        hits++;
    }
    PT_DEV void mean(int aovSpp, float4& oa, float4& on) const {
        oa = make_float4(0.0f, 0.0f, 0.0f, 0.0f); on = oa;
        if (hits > 0) {
            const float k = (float)hits;
            oa = make_float4(a.x / k, a.y / k, a.z / k, k / (float)aovSpp);
            on = make_float4(n.x / k, n.y / k, n.z / k, t / k);
        }
    }
};

}  // namespace pt
