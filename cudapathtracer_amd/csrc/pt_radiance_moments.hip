// pt_radiance_moments.hip — radiance queries that keep their variance (pt_query_radiance_moments, include/pt_api.h):
// pt_radiance.h's walk on a caller's own rays, and beside each ray's sample sum S the sum of its squared batch sums Q,
// pt_render_moments' pair, from one launch:
//   radiance_moments_kernel<INTEG, SIMPLE, LEAN>   INTEG, SIMPLE and LEAN as radiance_kernel has them; the walk's policy is MomentsLds
// The ray's spp samples are B = spp / batchSpp batches of c = batchSpp samples. Where radiance_kernel adds a finished sample
// (acc = acc + ps.Li) this one also counts the samples of the current batch, and at every c-th folds d = acc - prev into Q per
// channel (Q = Q + d * d: the product rounded, then the sum; the unit is compiled without contraction) and sets prev = acc. That is
// pt_render_moments' definition on the running f32 sum, so acc stays radiance_kernel's output bit for bit and Q is the render's.
// Two 16-byte stores per ray: (acc, 0) and (Q, B).
// The seven values the bookkeeping adds (prev, Q, the counter) are read and written at a sample's end only, never inside a traversal
// or a bounce. They live in lane-interleaved LDS words, as follow_chain keeps its record (7 KB per workgroup): in registers every
// instantiation compiled to more scratch than its radiance_kernel has, in LDS four of the six to the same and two to 8 and 4 bytes
// more (DESIGN.md §25's table).
#include "pt_radiance.h"

namespace pt {

// The batch bookkeeping of one lane, in its words m[j * 64], j = 0..6, of an LDS array float[7][64]: prev, Q, the counter's bits.
struct MomentsLds {
    static constexpr bool kWave = false;
    float* m;
    int batchSpp;
    float batches;
    float4* __restrict__ out;
    float4* __restrict__ sq;
    PT_DEV void reset() {
        m[0] = 0.0f; m[64] = 0.0f; m[128] = 0.0f; m[192] = 0.0f; m[256] = 0.0f; m[320] = 0.0f;
        m[384] = __int_as_float(batchSpp);
    }
    // a sample has been added: acc is the running sum after it (its own Li is not read)
    PT_DEV void sample(V3 acc, V3 li) {
        const int left = __float_as_int(m[384]) - 1;
        if (left != 0) { m[384] = __int_as_float(left); return; }
        const V3 d = v3(acc.x - m[0], acc.y - m[64], acc.z - m[128]);
        const V3 dd = v3(d.x * d.x, d.y * d.y, d.z * d.z);
        m[192] = m[192] + dd.x; m[256] = m[256] + dd.y; m[320] = m[320] + dd.z;
        m[0] = acc.x; m[64] = acc.y; m[128] = acc.z;
        m[384] = __int_as_float(batchSpp);
    }
    PT_DEV void store(int i, V3 acc) {
        out[i] = make_float4(acc.x, acc.y, acc.z, 0.0f);
        sq[i] = make_float4(m[192], m[256], m[320], batches);
    }
};

template <int INTEG, bool SIMPLE, bool LEAN>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(radiance_moments_waves_per_simd(INTEG, SIMPLE, LEAN), radiance_moments_waves_per_simd(INTEG, SIMPLE, LEAN))))
radiance_moments_kernel(DeviceScene S, const float4* __restrict__ rays, int n, int nTiles, const uint32_t* __restrict__ jump, unsigned long long seed,
                        uint32_t firstStream, int streamPad, int spp, int batchSpp, float batches, int maxDepth, int useMIS,
                        float4* __restrict__ out, float4* __restrict__ sq, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ uint8_t ldsMedium[SIMPLE ? 1 : 4][kMediumMax][64];
    __shared__ float ldsMom[4][7][64];                                   // the batch bookkeeping, lane-interleaved
    radiance_walk<INTEG, SIMPLE, LEAN>(S, ldsStack, ldsMedium, spill, rays, n, nTiles, jump, seed, firstStream, streamPad, spp, maxDepth, useMIS,
                                       MomentsLds{&ldsMom[threadIdx.x >> 6][0][threadIdx.x & 63], batchSpp, batches, out, sq});
}

hipError_t launch_radiance_moments(const DeviceScene& S, int integrator, bool simple, bool lean, int n, const void* rays, const uint32_t* jump,
                                   unsigned long long seed, uint32_t firstStream, bool streamPad, int spp, int batchSpp, int maxDepth, int useMIS,
                                   int blocks, void* out, void* sq, int32_t* spill, hipStream_t stream) {
    return radiance_dispatch(integrator, simple, lean, [&](auto integ, auto simp, auto ln) {
        hipLaunchKernelGGL((radiance_moments_kernel<decltype(integ)::value, decltype(simp)::value, decltype(ln)::value>), dim3(blocks), dim3(256), 0,
                           stream, S, (const float4*)rays, n, (n + 63) / 64, jump, seed, firstStream, streamPad ? 1 : 0, spp, batchSpp,
                           (float)(spp / batchSpp), maxDepth, useMIS, (float4*)out, (float4*)sq, spill);
        return hipGetLastError();
    });
}

}  // namespace pt
