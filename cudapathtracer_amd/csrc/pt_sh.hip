// pt_sh.hip — SH queries (pt_query_sh, pt_query_sh_rays_device, include/pt_api.h): the path tracer on uniformly
// distributed directions about a caller's points in free space, every sample projected onto the nine real spherical harmonics of
// bands 0..2: what a light probe stores.
//   sh_kernel<INTEG, SIMPLE, LEAN>   pt_radiance.h's walk with SphereBegin and ShSums: record i = (point, max_t, -, pad) is spread over
//                                    L = 1 << log2L lanes, 1 to 4096, each with a stream of its own; the lanes' 27 sums meet in the
//                                    adjacent-pair tree pt_irradiance.hip uses (pt_radiance.h: lane_tree), wave by wave
//   sh_reduce_kernel                 L > 64: the same tree, continued over the L / 64 partial sums the waves of a record left
//   sh_rays_kernel                   the ray a sample of lane l of record i starts from, one thread per lane: the tie to
//                                    pt_query_radiance
// Lanes, tiles and streams are pt_irradiance.hip's: lane g = 64 tile + lane works on record g >> log2L on stream firstStream + g
// (streamPad: firstStream + pad * L + l). A record of more than 64 lanes owns L / 64 whole tiles, which any waves of the launch may
// take: each leaves its tree's nine float4 in workspace[tile], and sh_reduce_kernel, launched behind the walk, adds them in tile order.
// L being a power of two, the two stages are one adjacent-pair tree of depth log2 L.
// A sample draws the two uniforms a radiance sample drops and makes its direction of them (sphere_ray below), then runs what a radiance
// sample runs from (o, d). At its end the sample's own Li, times each of the nine terms at its first direction, is added to the lane's
// 27 sums. Those and the direction are read and written at a sample's start and end only; they live in lane-interleaved LDS words of
// the kernel's own, as pt_radiance_moments.hip keeps its seven (the rule at the top of pt_radiance.h).
#include "pt_radiance.h"

namespace pt {

// The ray of a sample at point p, from the next two draws of rng: cosine_sample_f's local direction w (u1, then u2), and Archimedes'
// map of that hemisphere onto the sphere, s = 2 w.z, d = (s w.x, s w.y, s w.z - 1): d.z = 2 (1 - u1) - 1 is uniform in [-1, 1], the
// azimuth is w's. World axes, no basis, no offset, no normalise; every operation rounded once (include/pt_api.h; tests/sh_ref.py).
PT_DEV void sphere_ray(Rng& rng, V3 p, V3& o, V3& d, Ctr& c) {
    V3 w, f;
    float pdf;
    cosine_sample_f<false>(rng, v3(0.0f), w, f, pdf, c);
    const float s = 2.0f * w.z;
    d = v3(s * w.x, s * w.y, s * w.z - 1.0f);
    o = p;
}

// One lane's words m[j * 64], j = 0..29, of an LDS array float[30][64]: the sums a[k][c] at j = 3 k + c, the current sample's first
// direction at 27..29.
constexpr int kShWords = 30, kShDir = 27;

// The walk's begin policy: L lanes per record, a uniformly distributed ray per sample, its direction left for ShSums.
struct SphereBegin {
    int log2L;
    float* m;
    PT_DEV int record(int g) const { return g >> log2L; }
    PT_DEV uint32_t stream(const float4* __restrict__ rec, int streamPad, int g) const {
        return irradiance_stream(streamPad ? __float_as_uint(rec[1].w) : 0u, streamPad, g, log2L);
    }
    PT_DEV void sample(PathState& ps, float4 a, float4 b, Ctr& c) const {
        V3 o, d;
        sphere_ray(ps.rng, v3(a.x, a.y, a.z), o, d, c);
        m[(kShDir + 0) * 64] = d.x; m[(kShDir + 1) * 64] = d.y; m[(kShDir + 2) * 64] = d.z;
        radiance_state(ps, o, d);
    }
};

// The walk's sums policy. A sample's end: a[k][c] = a[k][c] + li.c * Y_k(d), the product rounded first (the unit is compiled without
// contraction), Y_k as include/pt_api.h writes them. The tile's end: lane_tree over each of the 27, within the wave; an
// idle lane holds 0. L <= 64: the record's first lane stores its nine float4. L > 64: lane 0 stores the tile's nine to
// workspace[tile], for sh_reduce_kernel.
struct ShSums {
    static constexpr bool kWave = true;
    int log2L;
    float* m;
    float4* __restrict__ out;
    float4* __restrict__ work;
    PT_DEV void reset() {
        for (int j = 0; j < kShDir; j++) m[j * 64] = 0.0f;
    }
    PT_DEV void sample(V3 acc, V3 li) {
        const float x = m[(kShDir + 0) * 64], y = m[(kShDir + 1) * 64], z = m[(kShDir + 2) * 64];
        const float C0 = 0.2820948f, C1 = 0.4886025f, C2 = 1.0925484f, C3 = 0.3153916f, C4 = 0.5462742f;
        const float Y[9] = {C0, C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), C3 * (3.0f * (z * z) - 1.0f), C2 * (x * z),
                            C4 * (x * x - y * y)};
#pragma unroll
        for (int k = 0; k < 9; k++) {
            m[(3 * k + 0) * 64] = m[(3 * k + 0) * 64] + li.x * Y[k];
            m[(3 * k + 1) * 64] = m[(3 * k + 1) * 64] + li.y * Y[k];
            m[(3 * k + 2) * 64] = m[(3 * k + 2) * 64] + li.z * Y[k];
        }
    }
    PT_DEV void store_wave(bool live, int i, int g, V3 acc) {
        const bool wide = log2L > 6;
        const int lanes = wide ? 64 : 1 << log2L;
        const bool first = live && (g & (lanes - 1)) == 0;
        float4* __restrict__ dst = wide ? work + 9 * (size_t)(g >> 6) : out + 9 * (size_t)i;
        for (int k = 0; k < 9; k++) {
            const V3 s = lane_tree(v3(m[(3 * k + 0) * 64], m[(3 * k + 1) * 64], m[(3 * k + 2) * 64]), lanes);
            if (first) dst[k] = make_float4(s.x, s.y, s.z, 0.0f);
        }
    }
};

// Compiled for sh_waves_per_simd (pt_feature_host.h): the 30 KB of ldsSh leave a CU three workgroups.
template <int INTEG, bool SIMPLE, bool LEAN>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(sh_waves_per_simd(INTEG, SIMPLE, LEAN), sh_waves_per_simd(INTEG, SIMPLE, LEAN))))
sh_kernel(DeviceScene S, const float4* __restrict__ recs, int n, int nTiles, int log2L, const uint32_t* __restrict__ jump, unsigned long long seed,
          uint32_t firstStream, int streamPad, int sppLane, int maxDepth, int useMIS, float4* __restrict__ out, float4* __restrict__ work,
          int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ uint8_t ldsMedium[SIMPLE ? 1 : 4][kMediumMax][64];
    __shared__ float ldsSh[4][kShWords][64];                             // the 27 sums and the sample's direction, lane-interleaved
    float* m = &ldsSh[threadIdx.x >> 6][0][threadIdx.x & 63];
    radiance_walk<INTEG, SIMPLE, LEAN>(S, ldsStack, ldsMedium, spill, recs, n, nTiles, jump, seed, firstStream, streamPad, sppLane, maxDepth, useMIS,
                                       ShSums{log2L, m, out, work}, SphereBegin{log2L, m});
}

// L > 64. Thread j = 9 i + k: out[j] = the adjacent-pair tree over work[9 (i W + w) + k], w = 0 .. W - 1, W = 1 << log2W tiles a
// record. Pairwise summation in tile order: partial w is added to the waiting sums of the levels at which w's low bits are ones
// (the left operand is the earlier one), and waits at the first level whose bit is 0; the last partial's chain ends in the tree's root.
__global__ void __launch_bounds__(256)
sh_reduce_kernel(const float4* __restrict__ work, int n, int log2W, float4* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= 9 * n) return;
    const int i = j / 9, k = j - 9 * i;
    const float4* __restrict__ src = work + 9 * ((size_t)i << log2W) + k;
    float sx[7] = {}, sy[7] = {}, sz[7] = {};
    float rx = 0.0f, ry = 0.0f, rz = 0.0f;
    for (int w = 0; w < (1 << log2W); w++) {
        const float4 p = src[9 * (size_t)w];
        float vx = p.x, vy = p.y, vz = p.z;
        bool carry = true;
#pragma unroll
        for (int lv = 0; lv < 7; lv++) {
            if (!carry) continue;
            if ((w >> lv) & 1) { vx = sx[lv] + vx; vy = sy[lv] + vy; vz = sz[lv] + vz; }
            else { sx[lv] = vx; sy[lv] = vy; sz[lv] = vz; carry = false; }
        }
        rx = vx; ry = vy; rz = vz;
    }
    out[j] = make_float4(rx, ry, rz, 0.0f);
}

// Ray g = i * L + l: the (o, d) a sample of lane l of record i starts from when draws skip[g] and skip[g] + 1 of the lane's stream
// play u1 and u2 (skip NULL: 0), with the record's max_t and, in its pad word, what the lane adds to firstStream. Every lane of a
// wave seeds (the seeding ballots per bit); the lanes past n * L then leave.
__global__ void __launch_bounds__(256)
sh_rays_kernel(const float4* __restrict__ recs, int n, int log2L, const uint32_t* __restrict__ jump, unsigned long long seed, uint32_t firstStream,
               int streamPad, const uint32_t* __restrict__ skip, float4* __restrict__ rays) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const bool live = g < (n << log2L);
    const float4* rec = recs + 2 * (size_t)(live ? g >> log2L : 0);
    const float4 a = rec[0], b = rec[1];
    const uint32_t k = irradiance_stream(__float_as_uint(b.w), streamPad, g, log2L);
    Rng rng = aov_stream(jump, seed, live ? firstStream + k : 0u);
    if (!live) return;
    for (uint32_t left = skip ? skip[g] : 0u; left != 0u; left--) rng_next(rng);
    Ctr c{};
    V3 o, d;
    sphere_ray(rng, v3(a.x, a.y, a.z), o, d, c);
    rays[2 * (size_t)g] = make_float4(o.x, o.y, o.z, a.w);
    rays[2 * (size_t)g + 1] = make_float4(d.x, d.y, d.z, __uint_as_float(k));
}

hipError_t launch_sh(const DeviceScene& S, int integrator, bool simple, bool lean, int n, const void* recs, int log2L, const uint32_t* jump,
                     unsigned long long seed, uint32_t firstStream, bool streamPad, int sppLane, int maxDepth, int useMIS, int blocks, void* out,
                     void* work, int32_t* spill, hipStream_t stream) {
    return radiance_dispatch(integrator, simple, lean, [&](auto integ, auto simp, auto ln) {
        hipLaunchKernelGGL((sh_kernel<decltype(integ)::value, decltype(simp)::value, decltype(ln)::value>), dim3(blocks), dim3(256), 0, stream, S,
                           (const float4*)recs, n, irradiance_tiles(n, log2L), log2L, jump, seed, firstStream, streamPad ? 1 : 0, sppLane, maxDepth, useMIS,
                           (float4*)out, (float4*)work, spill);
        return hipGetLastError();
    });
}

hipError_t launch_sh_reduce(int n, int log2L, const void* work, void* out, hipStream_t stream) {
    hipLaunchKernelGGL(sh_reduce_kernel, dim3((9 * n + 255) / 256), dim3(256), 0, stream, (const float4*)work, n, log2L - 6, (float4*)out);
    return hipGetLastError();
}

hipError_t launch_sh_rays(int n, const void* recs, int log2L, const uint32_t* jump, unsigned long long seed, uint32_t firstStream, bool streamPad,
                          const void* skip, void* rays, hipStream_t stream) {
    hipLaunchKernelGGL(sh_rays_kernel, dim3(((n << log2L) + 255) / 256), dim3(256), 0, stream, (const float4*)recs, n, log2L, jump, seed, firstStream,
                       streamPad ? 1 : 0, (const uint32_t*)skip, (float4*)rays);
    return hipGetLastError();
}

}  // namespace pt
