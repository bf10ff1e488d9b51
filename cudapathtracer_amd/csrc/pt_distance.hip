// pt_distance.hip — distance probes (pt_query_distance, pt_query_distance_rays_device; include/pt_api.h): per probe an
// octahedral map of R x R texels, each texel the sums of the hit distance and of its square over the texel's directions: what a
// probe volume's visibility test reads.
//   distance_kernel<CENTRE>   pt_query.hip's frame (pt_feature.h's FeatureWave, 64 lanes a tile, four waves per workgroup, persistent
//                             over the tiles): global lane g = 64 tile + lane is texel l = g & (R*R - 1) of record g >> 2 log2R. Per
//                             sample it makes a direction (oct_ray below), runs query_closest_kernel's trace_closest with the record's
//                             max_t, and adds to four sums of its own. A texel belongs to one lane: no tree, no workspace, no atomics.
//                             CENTRE: the texel's centre, one sample, no stream: the RNG-free kernel carries no stream registers
//   distance_rays_kernel      the ray a sample of such a lane starts from, one thread per lane: the tie to pt_query_closest
// Streams are pt_irradiance.hip's with log2L = 2 log2R (pt_radiance.h: irradiance_stream), seeded by aov_stream.
#include "pt_radiance.h"

namespace pt {

// The ray of a sample of texel (tx, ty) of an R x R map about p, invR = 1 / R, from the two uniforms: the point ((tx + u1) / R,
// (ty + u2) / R) of the unit square, unfolded onto the octahedron |x| + |y| + |z| = 1 about the world's z axis and normalised. Every
// operation rounded once, nothing fused but normalize()'s dot (include/pt_api.h; tests/distance_ref.py).
PT_DEV void oct_ray(int tx, int ty, float invR, float u1, float u2, V3 p, V3& o, V3& d) {
    const float px = ((float)tx + u1) * invR, py = ((float)ty + u2) * invR;
    const float fx = 2.0f * px - 1.0f, fy = 2.0f * py - 1.0f;
    const float ax = __builtin_fabsf(fx), ay = __builtin_fabsf(fy);
    const float z = (1.0f - ax) - ay;
    float x = fx, y = fy;
    if (z < 0.0f) { x = __builtin_copysignf(1.0f - ay, fx); y = __builtin_copysignf(1.0f - ax, fy); }
    d = normalize(v3(x, y, z));
    o = p;
}

// Every lane of a wave seeds (the seeding ballots per bit); the lanes past n * R * R then leave. A lane's samples run one after the
// other, every lane of a tile the same number of them: a sample draws u1, then u2, the trace draws nothing.
// out[g] = (A, B, H, K): A = ((0 + r_0) + r_1) + ..., B likewise over r_j * r_j (the product rounded first), r = the hit's t or, for a
// miss, max_t; H the samples that hit, K those of them whose surface record says backface (resolve_hit's test).
template <bool CENTRE>
__global__ void __launch_bounds__(256) distance_kernel(DeviceScene S, const float4* __restrict__ recs, int n, int nTiles, int log2R, float invR,
                                                       const uint32_t* __restrict__ jump, unsigned long long seed, uint32_t firstStream, int streamPad,
                                                       int sppLane, float4* __restrict__ out, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    FeatureWave W(ldsStack, S, spill);
    const int log2L = 2 * log2R;
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        const int g = tile * 64 + W.lane;
        const int i = g >> log2L;
        const bool live = i < n;
        const float4* rec = recs + 2 * (size_t)(live ? i : 0);
        Rng rng;
        if constexpr (!CENTRE) rng = aov_stream(jump, seed, live ? firstStream + irradiance_stream(__float_as_uint(rec[1].w), streamPad, g, log2L) : 0u);
        if (!live) continue;
        const float4 a = rec[0];
        const V3 p = v3(a.x, a.y, a.z);
        const int tx = g & ((1 << log2R) - 1), ty = (g >> log2R) & ((1 << log2R) - 1);
        float sumR = 0.0f, sumRR = 0.0f, hits = 0.0f, backs = 0.0f;
        for (int j = 0; j < (CENTRE ? 1 : sppLane); j++) {
            float u1 = 0.5f, u2 = 0.5f;
            if constexpr (!CENTRE) { u1 = rng_uniform(rng); u2 = rng_uniform(rng); }
            V3 o, d;
            oct_ray(tx, ty, invR, u1, u2, p, o, d);
            Hit hit;
            trace_closest<false, kStackLds>(S, W.C, o, d, a.w, W.st, hit, W.c);
            float r = a.w;
            if (hit.tri >= 0) {
                HitInfo hi; resolve_hit(S, hit, o, d, hi);
                r = hit.t;
                hits += 1.0f;
                backs += hi.backface ? 1.0f : 0.0f;
            }
            sumR = sumR + r;
            sumRR = sumRR + r * r;
        }
        out[g] = make_float4(sumR, sumRR, hits, backs);
    }
}

// Ray g = i * R * R + l: the (o, d) a sample of lane l of record i starts from when draws skip[g] and skip[g] + 1 of the lane's
// stream play u1 and u2 (skip NULL: 0), with the record's max_t and, in its pad word, what the lane adds to firstStream. centre: u1 =
// u2 = 0.5, no stream, skip is not read, and the pad word is g. Every lane of a wave seeds; the lanes past n * R * R then leave.
__global__ void __launch_bounds__(256)
distance_rays_kernel(const float4* __restrict__ recs, int n, int log2R, float invR, const uint32_t* __restrict__ jump, unsigned long long seed,
                     uint32_t firstStream, int streamPad, int centre, const uint32_t* __restrict__ skip, float4* __restrict__ rays) {
    const int log2L = 2 * log2R;
    const int g = blockIdx.x * 256 + threadIdx.x;
    const bool live = g < (n << log2L);
    const float4* rec = recs + 2 * (size_t)(live ? g >> log2L : 0);
    const float4 a = rec[0], b = rec[1];
    const uint32_t k = irradiance_stream(__float_as_uint(b.w), streamPad, g, log2L);
    float u1 = 0.5f, u2 = 0.5f;
    if (!centre) {
        Rng rng = aov_stream(jump, seed, live ? firstStream + k : 0u);
        if (!live) return;
        for (uint32_t left = skip ? skip[g] : 0u; left != 0u; left--) rng_next(rng);
        u1 = rng_uniform(rng); u2 = rng_uniform(rng);
    }
    if (!live) return;
    V3 o, d;
    oct_ray(g & ((1 << log2R) - 1), (g >> log2R) & ((1 << log2R) - 1), invR, u1, u2, v3(a.x, a.y, a.z), o, d);
    rays[2 * (size_t)g] = make_float4(o.x, o.y, o.z, a.w);
    rays[2 * (size_t)g + 1] = make_float4(d.x, d.y, d.z, __uint_as_float(k));
}

hipError_t launch_distance(const DeviceScene& S, int n, const void* recs, int log2R, const uint32_t* jump, unsigned long long seed, uint32_t firstStream,
                           bool streamPad, bool centre, int sppLane, int blocks, void* out, int32_t* spill, hipStream_t stream) {
    const int nTiles = irradiance_tiles(n, 2 * log2R);
    const float invR = 1.0f / (float)(1 << log2R);
    if (centre)
        hipLaunchKernelGGL(distance_kernel<true>, dim3(blocks), dim3(256), 0, stream, S, (const float4*)recs, n, nTiles, log2R, invR, jump, seed, firstStream,
                           0, 1, (float4*)out, spill);
    else
        hipLaunchKernelGGL(distance_kernel<false>, dim3(blocks), dim3(256), 0, stream, S, (const float4*)recs, n, nTiles, log2R, invR, jump, seed,
                           firstStream, streamPad ? 1 : 0, sppLane, (float4*)out, spill);
    return hipGetLastError();
}

hipError_t launch_distance_rays(int n, const void* recs, int log2R, const uint32_t* jump, unsigned long long seed, uint32_t firstStream, bool streamPad,
                                bool centre, const void* skip, void* rays, hipStream_t stream) {
    hipLaunchKernelGGL(distance_rays_kernel, dim3(((n << (2 * log2R)) + 255) / 256), dim3(256), 0, stream, (const float4*)recs, n, log2R,
                       1.0f / (float)(1 << log2R), jump, seed, firstStream, streamPad && !centre ? 1 : 0, centre ? 1 : 0, (const uint32_t*)skip,
                       (float4*)rays);
    return hipGetLastError();
}

}  // namespace pt
