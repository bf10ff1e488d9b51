// pt_irradiance.hip — irradiance queries (pt_query_irradiance, pt_query_irradiance_rays_device, include/pt_api.h): the
// path tracer on cosine-distributed directions about a caller's surface points, for lightmap texels and light probes.
//   irradiance_kernel<INTEG, SIMPLE, LEAN>   pt_radiance.h's walk with CosineBegin and IrradianceSums: record i = (point, max_t,
//                                            normal, pad) is spread over L = 1 << log2L lanes, each with a stream of its own, and the
//                                            lanes' sums meet in an adjacent-pair tree after the walk
//   irradiance_rays_kernel                   the ray a sample of lane l of record i starts from, one thread per lane: the tie to
//                                            pt_query_radiance
// A 64-lane tile holds 64 / L records: lane g = 64 tile + lane of the launch works on record g >> log2L as its lane g & (L - 1), on
// stream firstStream + g (streamPad: firstStream + pad * L + l), and runs sppLane samples one after the other. Where a radiance sample
// draws two uniforms and drops them, a sample here draws the same two and makes its direction of them (cosine_ray below), then runs
// what a radiance sample runs from (o, d): radiance_state, the record's max_t on the first segment, the bounce. With sppLane = 1 a
// lane's sum is therefore pt_query_radiance's on the ray irradiance_rays_kernel emits for it, bit for bit.
// The record is read again at every sample, the normal with it: nothing of it is carried across a traversal. The tree runs once per
// tile, after the walk, in wave shuffles: it costs the walk no register and the kernel no LDS. Q, the tree over the squared lane
// sums, is formed there too, from the sums the lanes end with.
#include "pt_radiance.h"

namespace pt {

// The ray of a sample at point p with unit normal nrm, from the next two draws of rng: cosine_sample_f's local direction (u1, then u2;
// the reflectance it also returns is not read), turned to the world by the naive bounce's plain basis, and bounce_core's offset of a
// reflected ray. The order of operations is written out in include/pt_api.h and restated in tests/irradiance_ref.py.
PT_DEV void cosine_ray(Rng& rng, V3 p, V3 nrm, V3& o, V3& d, Ctr& c) {
    V3 local, f;
    float pdf;
    cosine_sample_f<false>(rng, v3(0.0f), local, f, pdf, c);
    d = to_world(local, onb_of(nrm));
    o = p + nrm * kRayEps;
}

// The walk's begin policy: L lanes per record, a cosine-distributed ray per sample.
struct CosineBegin {
    int log2L;
    PT_DEV int record(int g) const { return g >> log2L; }
    PT_DEV uint32_t stream(const float4* __restrict__ rec, int streamPad, int g) const {
        return irradiance_stream(streamPad ? __float_as_uint(rec[1].w) : 0u, streamPad, g, log2L);
    }
    PT_DEV void sample(PathState& ps, float4 a, float4 b, Ctr& c) const {
        V3 o, d;
        cosine_ray(ps.rng, v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), o, d, c);
        radiance_state(ps, o, d);
    }
};

// The walk's sums policy: nothing per sample; at the tile's end the record's lanes add up in the adjacent-pair tree (pt_radiance.h:
// lane_tree; the streams are its irradiance_stream's). A record's L lanes are one aligned group of the wave, live or idle together
// (an idle lane holds 0), so every lane of the wave takes every step. sq set: the same tree over a_l * a_l per channel, the product
// rounded first (the unit is compiled without contraction).
struct IrradianceSums {
    static constexpr bool kWave = true;
    int log2L;
    float4* __restrict__ out;
    float4* __restrict__ sq;
    PT_DEV void reset() {}
    PT_DEV void sample(V3 acc, V3 li) {}
    PT_DEV void store_wave(bool live, int i, int g, V3 acc) {
        const int lanes = 1 << log2L;
        const V3 s = lane_tree(acc, lanes);
        const bool first = live && (g & (lanes - 1)) == 0;
        if (first) out[i] = make_float4(s.x, s.y, s.z, 0.0f);
        if (sq) {
            const V3 q = lane_tree(v3(acc.x * acc.x, acc.y * acc.y, acc.z * acc.z), lanes);
            if (first) sq[i] = make_float4(q.x, q.y, q.z, (float)lanes);
        }
    }
};

// Compiled for radiance_kernel's waves per SIMD of the same material class (pt_feature_host.h: irradiance_waves_per_simd).
template <int INTEG, bool SIMPLE, bool LEAN>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(irradiance_waves_per_simd(INTEG, SIMPLE, LEAN), irradiance_waves_per_simd(INTEG, SIMPLE, LEAN))))
irradiance_kernel(DeviceScene S, const float4* __restrict__ recs, int n, int nTiles, int log2L, const uint32_t* __restrict__ jump,
                  unsigned long long seed, uint32_t firstStream, int streamPad, int sppLane, int maxDepth, int useMIS, float4* __restrict__ out,
                  float4* __restrict__ sq, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ uint8_t ldsMedium[SIMPLE ? 1 : 4][kMediumMax][64];
    radiance_walk<INTEG, SIMPLE, LEAN>(S, ldsStack, ldsMedium, spill, recs, n, nTiles, jump, seed, firstStream, streamPad, sppLane, maxDepth, useMIS,
                                       IrradianceSums{log2L, out, sq}, CosineBegin{log2L});
}

// Ray g = i * L + l: the (o, d) a sample of lane l of record i starts from when draws skip[g] and skip[g] + 1 of the lane's stream
// play u1 and u2 (skip NULL: 0), with the record's max_t and, in its pad word, what the lane adds to firstStream. Every lane of a
// wave seeds (the seeding ballots per bit); the lanes past n * L then leave.
__global__ void __launch_bounds__(256)
irradiance_rays_kernel(const float4* __restrict__ recs, int n, int log2L, const uint32_t* __restrict__ jump, unsigned long long seed,
                       uint32_t firstStream, int streamPad, const uint32_t* __restrict__ skip, float4* __restrict__ rays) {
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
    cosine_ray(rng, v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), o, d, c);
    rays[2 * (size_t)g] = make_float4(o.x, o.y, o.z, a.w);
    rays[2 * (size_t)g + 1] = make_float4(d.x, d.y, d.z, __uint_as_float(k));
}

hipError_t launch_irradiance(const DeviceScene& S, int integrator, bool simple, bool lean, int n, const void* recs, int log2L, const uint32_t* jump,
                             unsigned long long seed, uint32_t firstStream, bool streamPad, int sppLane, int maxDepth, int useMIS, int blocks, void* out,
                             void* sq, int32_t* spill, hipStream_t stream) {
    return radiance_dispatch(integrator, simple, lean, [&](auto integ, auto simp, auto ln) {
        hipLaunchKernelGGL((irradiance_kernel<decltype(integ)::value, decltype(simp)::value, decltype(ln)::value>), dim3(blocks), dim3(256), 0, stream,
                           S, (const float4*)recs, n, irradiance_tiles(n, log2L), log2L, jump, seed, firstStream, streamPad ? 1 : 0, sppLane, maxDepth,
                           useMIS, (float4*)out, (float4*)sq, spill);
        return hipGetLastError();
    });
}

hipError_t launch_irradiance_rays(int n, const void* recs, int log2L, const uint32_t* jump, unsigned long long seed, uint32_t firstStream,
                                  bool streamPad, const void* skip, void* rays, hipStream_t stream) {
    hipLaunchKernelGGL(irradiance_rays_kernel, dim3(((n << log2L) + 255) / 256), dim3(256), 0, stream, (const float4*)recs, n, log2L, jump, seed,
                       firstStream, streamPad ? 1 : 0, (const uint32_t*)skip, (float4*)rays);
    return hipGetLastError();
}

}  // namespace pt
