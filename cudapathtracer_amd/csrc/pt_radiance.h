// pt_radiance.h — the radiance walk, once, for the kernels of pt_radiance.hip and pt_radiance_moments.hip: the path
// tracer on a caller's own rays. The frame is pt_query.hip's: pt_feature.h's FeatureWave, "tile" t = rays 64 t .. 64 t + 63, one lane
// each, four waves per workgroup, persistent over the tiles, the LDS stack overflowing into the scene's feature spill area. What runs
// in it is the megakernel's SYNC logic step (pt_path.h: path_bounce with the shadow ray traced inside the bounce, path_exhausted) on a
// path that starts from the ray's record instead of camera_ray.
// Per lane: the ray's XORWOW stream is seeded in the kernel (aov_stream: rng_init_kernel's stream k of `seed`) and runs on through the
// ray's spp samples. A sample draws two uniforms and drops them (the camera's jitter draws), starts path_begin's state at (o, d) as
// given, and walks: trace_closest (non-counting, Keep{0, 0}; the first segment with the ray's own max_t, every later one with 999999),
// then the bounce. A lane whose path ended starts its next sample in the same loop trip, so the wave traces with every lane that has
// work left; one ballot ends the tile. Nothing of a lane's arithmetic reads another lane: the seeding's ballots only skip jump
// matrices no lane needs, trace_closest's and trace_shadow's loop exits are off, and descend_node's wave-wide stack test chooses
// between two forms of the same push and pop. The sums: acc = ((0 + Li_0) + Li_1) + ... Lanes past n take no ray. No per-pixel RNG
// state, tile accumulator, counter or tile queue of the scene is read or written.
// PathState stays in scalars as pt_path.h demands: path_bounce copies the fields in and out, and the code here assigns whole values.
//
// What a kernel does with the sums is its policy, a type with three members (RadianceSums is the plain kernel's; pt_radiance_moments.hip
// has MomentsLds, pt_irradiance.hip IrradianceSums, pt_sh.hip ShSums):
//   reset()          a tile begins: acc is 0
//   sample(acc, li)  a sample has ended: acc is the running sum after it, li the sample's own Li
//   store(i, acc)    the tile is over: ray i's sum is acc
// A policy keeps nothing per lane in registers. sample() runs between two traversals of a loop whose every value is live across
// trace_closest and the bounce, and the six plain kernels sit at the edge of their register budgets (tests/test_radiance_api.py pins
// them): one more live VGPR is scratch or a wave less. What is the same for the whole wave (pointers, batch_spp) is an SGPR and free;
// what a lane carries from sample to sample lives in LDS words of the kernel's own, read and written inside sample() only. The
// kernels declare their __shared__ arrays themselves and pass them in, so each kernel's LDS size stays its own.
#pragma once
#include <type_traits>
#include "pt_feature.h"

namespace pt {

// path_begin's state at (o, d), without the camera and without a draw. (SYNC: no flag of a previous path survives its end.)
PT_DEV void radiance_state(PathState& ps, V3 o, V3 d) {
    ps.o = o; ps.d = d;
    ps.beta = v3(1.0f); ps.Li = v3(0.0f); ps.prevPoint = v3(0.0f); ps.woLocal = v3(0.0f);
    ps.pdf = kEps; ps.etaI = kEps; ps.etaT = kEps;
    ps.depth = 0; ps.guard = 0; ps.msTop = 1;
    ps.flags = kInPath;
}

// The start of a sample of a caller's ray.
PT_DEV void radiance_begin(PathState& ps, V3 o, V3 d, Ctr& c) {
    draw<false>(ps.rng, c); draw<false>(ps.rng, c);         // the two jitter draws of generateCameraRay; no lens numbers
    radiance_state(ps, o, d);
}

// What a sample starts from and which record a lane works on is the walk's second policy, a type with three members (RayBegin is
// the radiance kernels'; pt_irradiance.hip has CosineBegin, pt_sh.hip SphereBegin):
//   record(g)                 the record of lane g = 64 tile + lane of the launch; the lane has work if it is below n
//   stream(rec, pad, g)       what the lane adds to firstStream: from the record's pad word (streamPad) or from g
//   sample(ps, a, b, c)       a sample begins: the draws it spends, and path_begin's state at its ray; (a, b) are the record's
//                             32 bytes, read again for every sample
// Like a sums policy it keeps nothing per lane in registers; what it holds is the same for the whole wave.
struct RayBegin {
    PT_DEV int record(int g) const { return g; }
    PT_DEV uint32_t stream(const float4* __restrict__ rec, int streamPad, int g) const { return streamPad ? __float_as_uint(rec[1].w) : (uint32_t)g; }
    PT_DEV void sample(PathState& ps, float4 a, float4 b, Ctr& c) const { radiance_begin(ps, v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), c); }
};

// For the begin policies that spread a record over L = 1 << log2L lanes (pt_irradiance.hip, pt_sh.hip): what lane g adds to
// firstStream, as lane l = g & (L - 1) of its record: g itself, or with streamPad (the record's pad word) * L + l.
PT_DEV uint32_t irradiance_stream(uint32_t padWord, int streamPad, int g, int log2L) {
    return streamPad ? (padWord << log2L) + ((uint32_t)g & ((1u << log2L) - 1u)) : (uint32_t)g;
}

// ... and for their sums policies the adjacent-pair tree T_0[l] = a_l, T_(k+1)[l] = T_k[2l] + T_k[2l+1] over aligned groups of
// `lanes` lanes of the wave, in shuffles. Step k leaves T_(k+1)[l] in lane l << (k + 1) of the group: every lane adds what the lane
// 1 << k above it holds, and the lanes that are multiples of 2 << k hold the tree's values. Every lane of the wave takes every step.
PT_DEV V3 lane_tree(V3 v, int lanes) {
    for (int s = 1; s < lanes; s <<= 1) v = v3(v.x + __shfl_down(v.x, s), v.y + __shfl_down(v.y, s), v.z + __shfl_down(v.z, s));
    return v;
}

// radiance_kernel's policy: one 16-byte store per ray, (acc, 0).
struct RadianceSums {
    static constexpr bool kWave = false;
    float4* __restrict__ out;
    PT_DEV void reset() {}
    PT_DEV void sample(V3 acc, V3 li) {}
    PT_DEV void store(int i, V3 acc) { out[i] = make_float4(acc.x, acc.y, acc.z, 0.0f); }
};

// The walk over the wave's tiles. ldsMedium: mediumStack[16] per lane, lane-interleaved, one slice per wave; SIMPLE never names it.
template <int INTEG, bool SIMPLE, bool LEAN, class Sums, class Begin = RayBegin>
PT_DEV void radiance_walk(const DeviceScene& S, int32_t (*ldsStack)[kStackLds][64], uint8_t (*ldsMedium)[kMediumMax][64], int32_t* spill,
                          const float4* __restrict__ rays, int n, int nTiles, const uint32_t* __restrict__ jump, unsigned long long seed,
                          uint32_t firstStream, int streamPad, int spp, int maxDepth, int useMIS, Sums sums, Begin begin = Begin()) {
    FeatureWave W(ldsStack, S, spill);
    LdsMedium msLds;
    msLds.p = (LdsMedium::lds_u8*)&ldsMedium[SIMPLE ? 0 : W.wave][0][0] + W.lane;
    NoMedium msNone;
    auto& ms = [&]() -> auto& { if constexpr (SIMPLE) return msNone; else return msLds; }();
    auto shadowSync = [&](V3 ro, V3 wi, float maxt) { return trace_shadow<false, kStackLds, false, false, SIMPLE || LEAN>(S, W.C, ro, wi, maxt, W.st, W.c); };
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        const int g = tile * 64 + W.lane;
        const int i = begin.record(g);
        const bool live = i < n;
        // (the record is read again at the start of every sample, from the cache, instead of living in seven VGPRs across every traversal)
        const float4* ray = rays + 2 * (size_t)(live ? i : 0);
        const uint32_t k = live ? firstStream + begin.stream(ray, streamPad, g) : 0u;
        PathState ps;
        ps.rng = aov_stream(jump, seed, k);                     // (every lane: the seeding ballots per bit)
        ps.o = v3(0.0f); ps.d = v3(0.0f); ps.beta = v3(1.0f); ps.Li = v3(0.0f); ps.prevPoint = v3(0.0f); ps.woLocal = v3(0.0f);
        ps.pdf = kEps; ps.etaI = kEps; ps.etaT = kEps; ps.depth = 0; ps.guard = 0; ps.msTop = 1; ps.flags = 0;
        ps.so = v3(0.0f); ps.sd = v3(0.0f); ps.smaxt = 0.0f; ps.neeRaw = v3(0.0f); ps.neeBeta = v3(0.0f); ps.neeW = 0.0f;
        V3 acc = v3(0.0f);
        sums.reset();
        int samplesLeft = live ? spp : 0;
        float maxT = 999999.0f;                                 // of the segment about to be traced
        Hit h; h.tri = -1; h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.material = 0;
        while (true) {
            if (ps.flags & kInPath) {
                bool done = path_bounce<INTEG, false, false, SIMPLE, LEAN>(S, ps, ms, h, maxDepth, useMIS, shadowSync, W.c);
                if (!done) done = path_exhausted<INTEG>(ps, maxDepth);
                if (done) { acc = acc + ps.Li; sums.sample(acc, ps.Li); ps.flags &= ~kInPath; }          // colors[pixelIdx] += Li
                maxT = 999999.0f;
            }
            while (!(ps.flags & kInPath) && samplesLeft > 0) {
                samplesLeft--;
                const float4 a = ray[0], b = ray[1];
                begin.sample(ps, a, b, W.c);
                ms.set(0, 0);
                maxT = a.w;
                if (path_exhausted<INTEG>(ps, maxDepth)) { acc = acc + ps.Li; sums.sample(acc, ps.Li); ps.flags &= ~kInPath; }
            }
            const bool hasExt = (ps.flags & kInPath) != 0;
            if (__ballot(hasExt) == 0ull) break;
            if (hasExt) trace_closest<false, kStackLds>(S, W.C, ps.o, ps.d, maxT, W.st, h, W.c);
        }
        if constexpr (Sums::kWave) sums.store_wave(live, i, g, acc);
        else if (live) sums.store(i, acc);
    }
}

// The six instantiations' dispatch: f(integrator, simple, lean) with the three as std::integral_constants; INTEG 0 =
// Li_unidirectional, 2 = Li_naive_unidirectional, SIMPLE and LEAN as the render launch decides them from the scene's material class
// (pt_feature_api.hip).
template <class F>
hipError_t radiance_dispatch(int integrator, bool simple, bool lean, F&& f) {
    auto klass = [&](auto integ) {
        if (simple) return f(integ, std::true_type(), std::false_type());
        if (lean) return f(integ, std::false_type(), std::true_type());
        return f(integ, std::false_type(), std::false_type());
    };
    return integrator == 2 ? klass(std::integral_constant<int, 2>()) : klass(std::integral_constant<int, 0>());
}

}  // namespace pt
