// pt_radiance_moments.hip — radiance queries that keep their variance (pt_query_radiance_moments, include/pt_api.h):
// radiance_kernel's walk (pt_radiance.hip) on a caller's own rays, and beside each ray's sample sum S the sum of its squared batch
// sums Q, pt_render_moments' pair, from one launch:
//   radiance_moments_kernel<INTEG, SIMPLE, LEAN>   INTEG, SIMPLE and LEAN as radiance_kernel has them
// The ray's spp samples are B = spp / batchSpp batches of c = batchSpp samples. Where radiance_kernel adds a finished sample
// (acc = acc + ps.Li) this one also counts the samples of the current batch, and at every c-th folds d = acc - prev into Q per
// channel (Q = Q + d * d: the product rounded, then the sum; the unit is compiled without contraction) and sets prev = acc. That is
// pt_render_moments' definition on the running f32 sum, so acc stays radiance_kernel's output bit for bit and Q is the render's.
// Two 16-byte stores per ray: (acc, 0) and (Q, B).
// The seven values the bookkeeping adds (prev, Q, the counter) are read and written at a sample's end only, never inside a traversal
// or a bounce. They live in lane-interleaved LDS words, as follow_chain keeps its record (7 KB per workgroup): in registers every
// instantiation compiled to more scratch than its radiance_kernel has, in LDS four of the six to the same and two to 8 and 4 bytes
// more (DESIGN.md §25's table).
// The tile loop is a second copy of radiance_kernel's 40 lines, not a shared header: the six kernels of pt_radiance.hip are pinned
// to their registers, scratch and LDS by name (tests/test_radiance_api.py) and to their code by hash, a hook or a template parameter
// in their loop is a change to them, and an empty hook is not free here (pt_feature.h: ChainHook::surface). A fix to one loop goes
// into the other.
#include "pt_feature.h"

namespace pt {

// The start of a sample, as pt_radiance.hip has it: path_begin without the camera.
PT_DEV void radiance_moments_begin(PathState& ps, V3 o, V3 d, Ctr& c) {
    draw<false>(ps.rng, c); draw<false>(ps.rng, c);         // the two jitter draws of generateCameraRay; no lens numbers
    ps.o = o; ps.d = d;
    ps.beta = v3(1.0f); ps.Li = v3(0.0f); ps.prevPoint = v3(0.0f); ps.woLocal = v3(0.0f);
    ps.pdf = kEps; ps.etaI = kEps; ps.etaT = kEps;
    ps.depth = 0; ps.guard = 0; ps.msTop = 1;
    ps.flags = kInPath;
}

// The batch bookkeeping of one lane, in its words m[j * 64], j = 0..6, of an LDS array float[7][64]: prev, Q, the counter's bits.
struct MomentsLds {
    float* m;
    PT_DEV void reset(int c) {
        m[0] = 0.0f; m[64] = 0.0f; m[128] = 0.0f; m[192] = 0.0f; m[256] = 0.0f; m[320] = 0.0f;
        m[384] = __int_as_float(c);
    }
    // a sample has been added: acc is the running sum after it
    PT_DEV void sample(V3 acc, int c) {
        const int left = __float_as_int(m[384]) - 1;
        if (left != 0) { m[384] = __int_as_float(left); return; }
        const V3 d = v3(acc.x - m[0], acc.y - m[64], acc.z - m[128]);
        const V3 dd = v3(d.x * d.x, d.y * d.y, d.z * d.z);
        m[192] = m[192] + dd.x; m[256] = m[256] + dd.y; m[320] = m[320] + dd.z;
        m[0] = acc.x; m[64] = acc.y; m[128] = acc.z;
        m[384] = __int_as_float(c);
    }
    PT_DEV V3 sum() const { return v3(m[192], m[256], m[320]); }
};

template <int INTEG, bool SIMPLE, bool LEAN>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(radiance_moments_waves_per_simd(INTEG, SIMPLE, LEAN), radiance_moments_waves_per_simd(INTEG, SIMPLE, LEAN))))
radiance_moments_kernel(DeviceScene S, const float4* __restrict__ rays, int n, int nTiles, const uint32_t* __restrict__ jump, unsigned long long seed,
                        uint32_t firstStream, int streamPad, int spp, int batchSpp, float batches, int maxDepth, int useMIS,
                        float4* __restrict__ out, float4* __restrict__ sq, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ uint8_t ldsMedium[SIMPLE ? 1 : 4][kMediumMax][64];        // mediumStack[16] per lane, lane-interleaved; SIMPLE never names it
    __shared__ float ldsMom[4][7][64];                                   // the batch bookkeeping, lane-interleaved
    FeatureWave W(ldsStack, S, spill);
    LdsMedium msLds;
    msLds.p = (LdsMedium::lds_u8*)&ldsMedium[SIMPLE ? 0 : W.wave][0][0] + W.lane;
    NoMedium msNone;
    auto& ms = [&]() -> auto& { if constexpr (SIMPLE) return msNone; else return msLds; }();
    MomentsLds mom;
    mom.m = &ldsMom[W.wave][0][W.lane];
    auto shadowSync = [&](V3 ro, V3 wi, float maxt) { return trace_shadow<false, kStackLds, false, false, SIMPLE || LEAN>(S, W.C, ro, wi, maxt, W.st, W.c); };
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        const int i = tile * 64 + W.lane;
        const bool live = i < n;
        const float4* ray = rays + 2 * (size_t)(live ? i : 0);
        const uint32_t k = live ? firstStream + (streamPad ? __float_as_uint(ray[1].w) : (uint32_t)i) : 0u;
        PathState ps;
        ps.rng = aov_stream(jump, seed, k);                     // (every lane: the seeding ballots per bit)
        ps.o = v3(0.0f); ps.d = v3(0.0f); ps.beta = v3(1.0f); ps.Li = v3(0.0f); ps.prevPoint = v3(0.0f); ps.woLocal = v3(0.0f);
        ps.pdf = kEps; ps.etaI = kEps; ps.etaT = kEps; ps.depth = 0; ps.guard = 0; ps.msTop = 1; ps.flags = 0;
        ps.so = v3(0.0f); ps.sd = v3(0.0f); ps.smaxt = 0.0f; ps.neeRaw = v3(0.0f); ps.neeBeta = v3(0.0f); ps.neeW = 0.0f;
        V3 acc = v3(0.0f);
        mom.reset(batchSpp);
        int samplesLeft = live ? spp : 0;
        float maxT = 999999.0f;                                 // of the segment about to be traced
        Hit h; h.tri = -1; h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.material = 0;
        while (true) {
            if (ps.flags & kInPath) {
                bool done = path_bounce<INTEG, false, false, SIMPLE, LEAN>(S, ps, ms, h, maxDepth, useMIS, shadowSync, W.c);
                if (!done) done = path_exhausted<INTEG>(ps, maxDepth);
                if (done) { acc = acc + ps.Li; mom.sample(acc, batchSpp); ps.flags &= ~kInPath; }
                maxT = 999999.0f;
            }
            while (!(ps.flags & kInPath) && samplesLeft > 0) {
                samplesLeft--;
                const float4 a = ray[0], b = ray[1];
                radiance_moments_begin(ps, v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), W.c);
                ms.set(0, 0);
                maxT = a.w;
                if (path_exhausted<INTEG>(ps, maxDepth)) { acc = acc + ps.Li; mom.sample(acc, batchSpp); ps.flags &= ~kInPath; }
            }
            const bool hasExt = (ps.flags & kInPath) != 0;
            if (__ballot(hasExt) == 0ull) break;
            if (hasExt) trace_closest<false, kStackLds>(S, W.C, ps.o, ps.d, maxT, W.st, h, W.c);
        }
        if (live) {
            const V3 q = mom.sum();
            out[i] = make_float4(acc.x, acc.y, acc.z, 0.0f);
            sq[i] = make_float4(q.x, q.y, q.z, batches);
        }
    }
}

template <int INTEG, bool SIMPLE, bool LEAN>
static hipError_t launch_one(const DeviceScene& S, int n, const void* rays, const uint32_t* jump, unsigned long long seed, uint32_t firstStream,
                             bool streamPad, int spp, int batchSpp, int maxDepth, int useMIS, int blocks, void* out, void* sq, int32_t* spill,
                             hipStream_t stream) {
    hipLaunchKernelGGL((radiance_moments_kernel<INTEG, SIMPLE, LEAN>), dim3(blocks), dim3(256), 0, stream, S, (const float4*)rays, n, (n + 63) / 64, jump,
                       seed, firstStream, streamPad ? 1 : 0, spp, batchSpp, (float)(spp / batchSpp), maxDepth, useMIS, (float4*)out, (float4*)sq, spill);
    return hipGetLastError();
}

hipError_t launch_radiance_moments(const DeviceScene& S, int integrator, bool simple, bool lean, int n, const void* rays, const uint32_t* jump,
                                   unsigned long long seed, uint32_t firstStream, bool streamPad, int spp, int batchSpp, int maxDepth, int useMIS,
                                   int blocks, void* out, void* sq, int32_t* spill, hipStream_t stream) {
#define PT_RADIANCE_ARGS S, n, rays, jump, seed, firstStream, streamPad, spp, batchSpp, maxDepth, useMIS, blocks, out, sq, spill, stream
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
