// pt_radiance.hip — radiance queries (pt_query_radiance, include/pt_api.h): the path tracer on a caller's own rays.
// The frame is pt_query.hip's: pt_feature.h's FeatureWave, "tile" t = rays 64 t .. 64 t + 63, one lane each, four waves per workgroup,
// persistent over the tiles, the LDS stack overflowing into the scene's feature spill area. What runs in it is the megakernel's SYNC
// logic step (pt_path.h: path_bounce with the shadow ray traced inside the bounce, path_exhausted) on a path that starts from the
// ray's record instead of camera_ray:
//   radiance_kernel<INTEG, SIMPLE, LEAN>   INTEG 0 = Li_unidirectional, 2 = Li_naive_unidirectional; SIMPLE and LEAN as the render
//                                          launch decides them from the scene's material class (pt_feature_api.hip)
// Per lane: the ray's XORWOW stream is seeded in the kernel (aov_stream: rng_init_kernel's stream k of `seed`) and runs on through the
// ray's spp samples. A sample draws two uniforms and drops them (the camera's jitter draws), starts path_begin's state at (o, d) as
// given, and walks: trace_closest (non-counting, Keep{0, 0}; the first segment with the ray's own max_t, every later one with 999999),
// then the bounce. A lane whose path ended starts its next sample in the same loop trip, so the wave traces with every lane that has
// work left; one ballot ends the tile. Nothing of a lane's arithmetic reads another lane: the seeding's ballots only skip jump
// matrices no lane needs, trace_closest's and trace_shadow's loop exits are off, and descend_node's wave-wide stack test chooses
// between two forms of the same push and pop. The sums: acc = ((0 + Li_0) + Li_1) + ..., one 16-byte store per ray. Lanes past n take
// no ray. No per-pixel RNG state, tile accumulator, counter or tile queue of the scene is read or written.
// PathState stays in scalars as pt_path.h demands: path_bounce copies the fields in and out, and the code here assigns whole values.
#include "pt_feature.h"

namespace pt {

// The start of a sample: path_begin without the camera. (SYNC: no flag of a previous path survives its end.)
PT_DEV void radiance_begin(PathState& ps, V3 o, V3 d, Ctr& c) {
    draw<false>(ps.rng, c); draw<false>(ps.rng, c);         // the two jitter draws of generateCameraRay; no lens numbers
    ps.o = o; ps.d = d;
    ps.beta = v3(1.0f); ps.Li = v3(0.0f); ps.prevPoint = v3(0.0f); ps.woLocal = v3(0.0f);
    ps.pdf = kEps; ps.etaI = kEps; ps.etaT = kEps;
    ps.depth = 0; ps.guard = 0; ps.msTop = 1;
    ps.flags = kInPath;
}

// amdgpu_waves_per_eu: each instantiation is compiled for the waves per SIMD it is launched at (pt_feature_host.h:
// radiance_waves_per_simd, from what the compile shows), so the register allocator works to that budget and to no tighter one.
template <int INTEG, bool SIMPLE, bool LEAN>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(radiance_waves_per_simd(INTEG, SIMPLE, LEAN), radiance_waves_per_simd(INTEG, SIMPLE, LEAN))))
radiance_kernel(DeviceScene S, const float4* __restrict__ rays, int n, int nTiles, const uint32_t* __restrict__ jump, unsigned long long seed,
                uint32_t firstStream, int streamPad, int spp, int maxDepth, int useMIS, float4* __restrict__ out, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ uint8_t ldsMedium[SIMPLE ? 1 : 4][kMediumMax][64];        // mediumStack[16] per lane, lane-interleaved; SIMPLE never names it
    FeatureWave W(ldsStack, S, spill);
    LdsMedium msLds;
    msLds.p = (LdsMedium::lds_u8*)&ldsMedium[SIMPLE ? 0 : W.wave][0][0] + W.lane;
    NoMedium msNone;
    auto& ms = [&]() -> auto& { if constexpr (SIMPLE) return msNone; else return msLds; }();
    auto shadowSync = [&](V3 ro, V3 wi, float maxt) { return trace_shadow<false, kStackLds, false, false, SIMPLE || LEAN>(S, W.C, ro, wi, maxt, W.st, W.c); };
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        const int i = tile * 64 + W.lane;
        const bool live = i < n;
        // (the record is read again at the start of every sample, from the cache, instead of living in seven VGPRs across every traversal)
        const float4* ray = rays + 2 * (size_t)(live ? i : 0);
        const uint32_t k = live ? firstStream + (streamPad ? __float_as_uint(ray[1].w) : (uint32_t)i) : 0u;
        PathState ps;
        ps.rng = aov_stream(jump, seed, k);                     // (every lane: the seeding ballots per bit)
        ps.o = v3(0.0f); ps.d = v3(0.0f); ps.beta = v3(1.0f); ps.Li = v3(0.0f); ps.prevPoint = v3(0.0f); ps.woLocal = v3(0.0f);
        ps.pdf = kEps; ps.etaI = kEps; ps.etaT = kEps; ps.depth = 0; ps.guard = 0; ps.msTop = 1; ps.flags = 0;
        ps.so = v3(0.0f); ps.sd = v3(0.0f); ps.smaxt = 0.0f; ps.neeRaw = v3(0.0f); ps.neeBeta = v3(0.0f); ps.neeW = 0.0f;
        V3 acc = v3(0.0f);
        int samplesLeft = live ? spp : 0;
        float maxT = 999999.0f;                                 // of the segment about to be traced
        Hit h; h.tri = -1; h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.material = 0;
        while (true) {
            if (ps.flags & kInPath) {
                bool done = path_bounce<INTEG, false, false, SIMPLE, LEAN>(S, ps, ms, h, maxDepth, useMIS, shadowSync, W.c);
                if (!done) done = path_exhausted<INTEG>(ps, maxDepth);
                if (done) { acc = acc + ps.Li; ps.flags &= ~kInPath; }          // colors[pixelIdx] += Li
                maxT = 999999.0f;
            }
            while (!(ps.flags & kInPath) && samplesLeft > 0) {
                samplesLeft--;
                const float4 a = ray[0], b = ray[1];
                radiance_begin(ps, v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), W.c);
                ms.set(0, 0);
                maxT = a.w;
                if (path_exhausted<INTEG>(ps, maxDepth)) { acc = acc + ps.Li; ps.flags &= ~kInPath; }
            }
            const bool hasExt = (ps.flags & kInPath) != 0;
            if (__ballot(hasExt) == 0ull) break;
            if (hasExt) trace_closest<false, kStackLds>(S, W.C, ps.o, ps.d, maxT, W.st, h, W.c);
        }
        if (live) out[i] = make_float4(acc.x, acc.y, acc.z, 0.0f);
    }
}

template <int INTEG, bool SIMPLE, bool LEAN>
static hipError_t launch_one(const DeviceScene& S, int n, const void* rays, const uint32_t* jump, unsigned long long seed, uint32_t firstStream,
                             bool streamPad, int spp, int maxDepth, int useMIS, int blocks, void* out, int32_t* spill, hipStream_t stream) {
    hipLaunchKernelGGL((radiance_kernel<INTEG, SIMPLE, LEAN>), dim3(blocks), dim3(256), 0, stream, S, (const float4*)rays, n, (n + 63) / 64, jump, seed,
                       firstStream, streamPad ? 1 : 0, spp, maxDepth, useMIS, (float4*)out, spill);
    return hipGetLastError();
}

hipError_t launch_radiance(const DeviceScene& S, int integrator, bool simple, bool lean, int n, const void* rays, const uint32_t* jump,
                           unsigned long long seed, uint32_t firstStream, bool streamPad, int spp, int maxDepth, int useMIS, int blocks, void* out,
                           int32_t* spill, hipStream_t stream) {
#define PT_RADIANCE_ARGS S, n, rays, jump, seed, firstStream, streamPad, spp, maxDepth, useMIS, blocks, out, spill, stream
    if (integrator == 2) {
        if (simple) return launch_one<2, true, false>(PT_RADIANCE_ARGS);
        if (lean) return launch_one<2, false, true>(PT_RADIANCE_ARGS);
        return launch_one<2, false, false>(PT_RADIANCE_ARGS);
    }
    if (simple) return launch_one<0, true, false>(PT_RADIANCE_ARGS);
    if (lean) return launch_one<0, false, true>(PT_RADIANCE_ARGS);
    return launch_one<0, false, false>(PT_RADIANCE_ARGS);
#undef PT_RADIANCE_ARGS
}

}  // namespace pt
