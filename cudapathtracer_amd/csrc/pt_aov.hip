// pt_aov.hip — first-hit feature buffers (albedo, normal, depth) for denoisers (pt_render_aovs, include/pt_api.h).
//
// One wave per 8x8 tile (lane = ly*8+lx), four waves per workgroup, persistent over the tiles. Ray k of pixel (x, y) is
// camera_ray drawn from a FRESH XORWOW stream keyed (seed + k, y*w+x) — the seeding of rng_init_kernel, into registers
// — then the non-counting trace_closest (max_t 999999, as pt_probe_trace_closest) and resolve_hit, so t, the normal and
// the material are those of pt_probe_trace_closest. The albedo is material_inputs' (the texture sample for textured
// materials). First hit only: no specular chain is followed. The pass writes neither the scene's per-pixel RNG states nor
// its tile accumulator nor its counters, so it may run between the chunks of a progressive render.
// aov_chain_kernel (below, pt_render_aovs_chain) is the same pass with each ray followed through mirrors and glass.
#include "pt_path.h"
#include "pt_params.h"
#include "pt_centre_ray.h"

namespace pt {

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

// spill: (gridDim.x * 4) waves x S.stackSpill entries x 64 lanes, the lane-interleaved layout of Stack.
__global__ void __launch_bounds__(256) aov_kernel(DeviceScene S, CamK cam, const uint32_t* __restrict__ jump, unsigned long long seed,
                                                  int w, int h, int tilesX, int nTiles, int aovSpp, float4* __restrict__ albedo,
                                                  float4* __restrict__ normalDepth, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + wave;
    Stack<kStackLds> st; st.lds = (lds_i32*)&ldsStack[wave][0][0] + lane; st.sp = 0;
    st.spill = spill ? spill + (size_t)gw * S.stackSpill * 64 + lane : nullptr;
    SceneCache C; C.nodes = nullptr; C.nNodes = 0; C.tris = nullptr; C.nTris = 0;
    Ctr c = {};
    for (int tile = gw; tile < nTiles; tile += gridDim.x * 4) {
        const int x = (tile % tilesX) * 8 + (lane & 7), y = (tile / tilesX) * 8 + (lane >> 3);
        const bool inside = x < w && y < h;
        const uint32_t idx = inside ? (uint32_t)(y * w + x) : 0u;
        V3 sa = v3(0.0f), sn = v3(0.0f);
        float st_ = 0.0f;
        int hits = 0;
        for (int k = 0; k < aovSpp; k++) {
            Rng rng = aov_stream(jump, seed + (unsigned long long)k, idx);      // (every lane: the seeding ballots per bit)
            if (!inside) continue;
            V3 o, d;
            camera_ray<false>(cam, rng, x, y, o, d, c);
            Hit hit;
            trace_closest<false, kStackLds>(S, C, o, d, 999999.0f, st, hit, c);
            if (hit.tri < 0) continue;
            HitInfo hi; resolve_hit(S, hit, o, d, hi);
            V3 a; float trans;
            material_inputs(S.mats[hi.material], S.textures, hi.uvx, hi.uvy, true, a, trans);
            // sums in k order; the first hit is stored, not added to 0, so that a -0 component survives (aov_spp = 1 is the hit itself)
            if (hits == 0) { sa = a; sn = hi.normal; st_ = hit.t; }
            else { sa = sa + a; sn = sn + hi.normal; st_ = st_ + hit.t; }
            hits++;
        }
        if (!inside) continue;
        float4 oa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), on = oa;
        if (hits > 0) {
            const float n = (float)hits;
            oa = make_float4(sa.x / n, sa.y / n, sa.z / n, n / (float)aovSpp);
            on = make_float4(sn.x / n, sn.y / n, sn.z / n, st_ / n);
        }
        albedo[idx] = oa;
        normalDepth[idx] = on;
    }
}

// Workgroups of the AOV pass: persistent, as many as are resident at once (76 VGPRs: 6 waves per SIMD = 6 workgroups per CU).
int aov_blocks(int nTiles, int numCU) { return std::max(1, std::min((nTiles + 3) / 4, numCU * 6)); }

hipError_t launch_aov(const DeviceScene& S, const CamK& cam, const uint32_t* jump, unsigned long long seed, int w, int h, int aovSpp,
                      int blocks, float4* albedo, float4* normalDepth, int32_t* spill, hipStream_t stream) {
    const int tilesX = (w + 7) / 8, nTiles = tilesX * ((h + 7) / 8);
    hipLaunchKernelGGL(aov_kernel, dim3(blocks), dim3(256), 0, stream, S, cam, jump, seed, w, h, tilesX, nTiles, aovSpp, albedo, normalDepth, spill);
    return hipGetLastError();
}

// aov_chain_kernel — the feature buffers of pt_render_aovs_chain (include/pt_api.h states the contract): aov_kernel's tiling, rays,
// sums and division, but each ray follows mirrors (type 6) and smooth dielectrics (type 2) deterministically to the first
// non-specular surface and reports THAT surface's albedo and normal, the summed path length as depth and the number of links.
// One trace_closest call site serves the camera ray (i = 0) and every link (i >= 1): lanes leave the loop at different links,
// the wave leaves it when one ballot finds no lane left. Live across a traversal: o, d, the running depth and the link count; the
// first-hit record sits in LDS, becomes the result in place when the chain ends on a surface and simply stays when it does not.
// The direction arithmetic is written out operation by operation (no dot(), normalize(), fmaf): tests/aov_chain_ref.py restates it.
__global__ void __launch_bounds__(256) aov_chain_kernel(DeviceScene S, CamK cam, const uint32_t* __restrict__ jump, unsigned long long seed,
                                                        int w, int h, int tilesX, int nTiles, int aovSpp, int maxLinks,
                                                        float4* __restrict__ albedo, float4* __restrict__ normalDepth,
                                                        float* __restrict__ linksOut, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ float ldsRec[4][7][64];           // a ray's record (albedo, normal, depth), lane-interleaved: see below
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + wave;
    Stack<kStackLds> st; st.lds = (lds_i32*)&ldsStack[wave][0][0] + lane; st.sp = 0;
    st.spill = spill ? spill + (size_t)gw * S.stackSpill * 64 + lane : nullptr;
    float* rec = &ldsRec[wave][0][lane];          // rec[j * 64], j = 0..6; only this lane touches it
    SceneCache C; C.nodes = nullptr; C.nNodes = 0; C.tris = nullptr; C.nTris = 0;
    Ctr c = {};
    for (int tile = gw; tile < nTiles; tile += gridDim.x * 4) {
        const int x = (tile % tilesX) * 8 + (lane & 7), y = (tile / tilesX) * 8 + (lane >> 3);
        const bool inside = x < w && y < h;
        const uint32_t idx = inside ? (uint32_t)(y * w + x) : 0u;
        V3 sa = v3(0.0f), sn = v3(0.0f);
        float st_ = 0.0f;
        int hits = 0, linkSum = 0;
        for (int k = 0; k < aovSpp; k++) {
            Rng rng = aov_stream(jump, seed + (unsigned long long)k, idx);      // (every lane: the seeding ballots per bit)
            V3 o = v3(0.0f), d = v3(0.0f);
            if (inside) camera_ray<false>(cam, rng, x, y, o, d, c);
            // The ray's record lives in LDS, not in registers: it is written at the first hit, overwritten where the chain ends on a
            // surface and read once after the loop, so it need not be live across the traversals (7 VGPRs: 86 -> 6 waves per SIMD).
            float depth = 0.0f;
            int links = -1;                      // -1: no hit at all
            bool live = inside;
            for (int i = 0; i <= maxLinks; i++) {
                if (!__ballot(live)) break;
                if (live) {
                    Hit hit;
                    trace_closest<false, kStackLds>(S, C, o, d, 999999.0f, st, hit, c);
                    live = false;
                    if (hit.tri >= 0) {          // (a miss: no hit at all at i = 0, the first hit's record stands after that)
                        HitInfo hi; resolve_hit(S, hit, o, d, hi);
                        const PMat& m = S.mats[hi.material];
                        const bool spec = (m.flags & kMatSpecular) && (m.type == 6 || m.type == 2);
                        depth = i == 0 ? hit.t : depth + hit.t;
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
            if (links < 0) continue;
            const V3 ra = v3(rec[0], rec[64], rec[128]), rn = v3(rec[192], rec[256], rec[320]);
            const float rt = rec[384];
            // sums in k order; the first contributing ray is stored, not added to 0, so that a -0 component survives
            if (hits == 0) { sa = ra; sn = rn; st_ = rt; }
            else { sa = sa + ra; sn = sn + rn; st_ = st_ + rt; }
            linkSum += links;
            hits++;
        }
        if (!inside) continue;
        float4 oa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), on = oa;
        float ol = 0.0f;
        if (hits > 0) {
            const float n = (float)hits;
            oa = make_float4(sa.x / n, sa.y / n, sa.z / n, n / (float)aovSpp);
            on = make_float4(sn.x / n, sn.y / n, sn.z / n, st_ / n);
            ol = (float)linkSum / n;
        }
        albedo[idx] = oa;
        normalDepth[idx] = on;
        if (linksOut) linksOut[idx] = ol;
    }
}

// Workgroups of the chain pass: its own count, from its own resources (80 VGPRs, 23 KB of LDS per workgroup: 6 waves per SIMD =
// 6 workgroups per CU, 138 of the CU's 160 KB). aov_blocks is the first-hit kernel's.
constexpr int kAovChainWavesPerSimd = 6;
int aov_chain_blocks(int nTiles, int numCU) { return std::max(1, std::min((nTiles + 3) / 4, numCU * kAovChainWavesPerSimd)); }

hipError_t launch_aov_chain(const DeviceScene& S, const CamK& cam, const uint32_t* jump, unsigned long long seed, int w, int h, int aovSpp,
                            int maxLinks, int blocks, float4* albedo, float4* normalDepth, float* links, int32_t* spill, hipStream_t stream) {
    const int tilesX = (w + 7) / 8, nTiles = tilesX * ((h + 7) / 8);
    hipLaunchKernelGGL(aov_chain_kernel, dim3(blocks), dim3(256), 0, stream, S, cam, jump, seed, w, h, tilesX, nTiles, aovSpp, maxLinks, albedo,
                       normalDepth, links, spill);
    return hipGetLastError();
}

// ---- centre guides (pt_render_aovs_centre, pt_probe_centre_rays) -------------------------------------------------------------------
// (camera_ray_centre, the centre ray of pixel (x, y), is in pt_centre_ray.h: pt_motion.hip traces it too.)
__global__ void probe_centre_kernel(CamK cam, int n, const int* __restrict__ xy, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    V3 o, d;
    camera_ray_centre(cam, xy[2 * i], xy[2 * i + 1], o, d);
    out[6 * i] = o.x; out[6 * i + 1] = o.y; out[6 * i + 2] = o.z; out[6 * i + 3] = d.x; out[6 * i + 4] = d.y; out[6 * i + 5] = d.z;
}

hipError_t launch_probe_centre(const CamK& cam, int n, const int* xy, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(probe_centre_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, cam, n, xy, out);
    return hipGetLastError();
}

// aov_centre_kernel — aov_kernel for the one centre ray of each pixel: its tiling, traversal and record, without the stream seeding
// (no jump table, no Rng in registers) and without the sums over k: one ray, so the hit itself is the result (aov_kernel divides
// it by n = 1, which changes no bit, and writes coverage 1 / 1).
__global__ void __launch_bounds__(256) aov_centre_kernel(DeviceScene S, CamK cam, int w, int h, int tilesX, int nTiles,
                                                         float4* __restrict__ albedo, float4* __restrict__ normalDepth, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + wave;
    Stack<kStackLds> st; st.lds = (lds_i32*)&ldsStack[wave][0][0] + lane; st.sp = 0;
    st.spill = spill ? spill + (size_t)gw * S.stackSpill * 64 + lane : nullptr;
    SceneCache C; C.nodes = nullptr; C.nNodes = 0; C.tris = nullptr; C.nTris = 0;
    Ctr c = {};
    for (int tile = gw; tile < nTiles; tile += gridDim.x * 4) {
        const int x = (tile % tilesX) * 8 + (lane & 7), y = (tile / tilesX) * 8 + (lane >> 3);
        if (!(x < w && y < h)) continue;
        const size_t idx = (size_t)y * w + x;
        V3 o, d;
        camera_ray_centre(cam, x, y, o, d);
        Hit hit;
        trace_closest<false, kStackLds>(S, C, o, d, 999999.0f, st, hit, c);
        float4 oa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), on = oa;
        if (hit.tri >= 0) {
            HitInfo hi; resolve_hit(S, hit, o, d, hi);
            V3 a; float trans;
            material_inputs(S.mats[hi.material], S.textures, hi.uvx, hi.uvy, true, a, trans);
            oa = make_float4(a.x, a.y, a.z, 1.0f);
            on = make_float4(hi.normal.x, hi.normal.y, hi.normal.z, hit.t);
        }
        albedo[idx] = oa;
        normalDepth[idx] = on;
    }
}

// Workgroups of the centre first-hit pass: without the seeding the kernel needs 63 VGPRs, so 8 waves per SIMD = 8 workgroups per CU
// are resident (8 x 16 KB of LDS). The centre chain kernel (69 VGPRs, 23 KB) stays at aov_chain_blocks' 6: 7 would need 161 KB.
int aov_centre_blocks(int nTiles, int numCU) { return std::max(1, std::min((nTiles + 3) / 4, numCU * 8)); }

hipError_t launch_aov_centre(const DeviceScene& S, const CamK& cam, int w, int h, int blocks, float4* albedo, float4* normalDepth, int32_t* spill,
                             hipStream_t stream) {
    const int tilesX = (w + 7) / 8, nTiles = tilesX * ((h + 7) / 8);
    hipLaunchKernelGGL(aov_centre_kernel, dim3(blocks), dim3(256), 0, stream, S, cam, w, h, tilesX, nTiles, albedo, normalDepth, spill);
    return hipGetLastError();
}

// aov_centre_chain_kernel — aov_chain_kernel for the one centre ray of each pixel: the same link loop, link rule, fallback and LDS
// record (the arithmetic below is aov_chain_kernel's, operation for operation: tests/aov_chain_ref.py restates both), without the
// stream seeding and the sums over k.
__global__ void __launch_bounds__(256) aov_centre_chain_kernel(DeviceScene S, CamK cam, int w, int h, int tilesX, int nTiles, int maxLinks,
                                                               float4* __restrict__ albedo, float4* __restrict__ normalDepth,
                                                               float* __restrict__ linksOut, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ float ldsRec[4][7][64];           // the ray's record (albedo, normal, depth), lane-interleaved, as in aov_chain_kernel
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + wave;
    Stack<kStackLds> st; st.lds = (lds_i32*)&ldsStack[wave][0][0] + lane; st.sp = 0;
    st.spill = spill ? spill + (size_t)gw * S.stackSpill * 64 + lane : nullptr;
    float* rec = &ldsRec[wave][0][lane];          // rec[j * 64], j = 0..6; only this lane touches it
    SceneCache C; C.nodes = nullptr; C.nNodes = 0; C.tris = nullptr; C.nTris = 0;
    Ctr c = {};
    for (int tile = gw; tile < nTiles; tile += gridDim.x * 4) {
        const int x = (tile % tilesX) * 8 + (lane & 7), y = (tile / tilesX) * 8 + (lane >> 3);
        const bool inside = x < w && y < h;
        V3 o = v3(0.0f), d = v3(0.0f);
        if (inside) camera_ray_centre(cam, x, y, o, d);
        float depth = 0.0f;
        int links = -1;                          // -1: no hit at all
        bool live = inside;
        for (int i = 0; i <= maxLinks; i++) {
            if (!__ballot(live)) break;
            if (live) {
                Hit hit;
                trace_closest<false, kStackLds>(S, C, o, d, 999999.0f, st, hit, c);
                live = false;
                if (hit.tri >= 0) {              // (a miss: no hit at all at i = 0, the first hit's record stands after that)
                    HitInfo hi; resolve_hit(S, hit, o, d, hi);
                    const PMat& m = S.mats[hi.material];
                    const bool spec = (m.flags & kMatSpecular) && (m.type == 6 || m.type == 2);
                    depth = i == 0 ? hit.t : depth + hit.t;
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
        if (!inside) continue;
        const size_t idx = (size_t)y * w + x;
        float4 oa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), on = oa;
        float ol = 0.0f;
        if (links >= 0) {
            oa = make_float4(rec[0], rec[64], rec[128], 1.0f);
            on = make_float4(rec[192], rec[256], rec[320], rec[384]);
            ol = (float)links;
        }
        albedo[idx] = oa;
        normalDepth[idx] = on;
        if (linksOut) linksOut[idx] = ol;
    }
}

hipError_t launch_aov_centre_chain(const DeviceScene& S, const CamK& cam, int w, int h, int maxLinks, int blocks, float4* albedo, float4* normalDepth,
                                   float* links, int32_t* spill, hipStream_t stream) {
    const int tilesX = (w + 7) / 8, nTiles = tilesX * ((h + 7) / 8);
    hipLaunchKernelGGL(aov_centre_chain_kernel, dim3(blocks), dim3(256), 0, stream, S, cam, w, h, tilesX, nTiles, maxLinks, albedo, normalDepth, links,
                       spill);
    return hipGetLastError();
}

}  // namespace pt
