// pt_radiance.hip — radiance queries (pt_query_radiance, include/pt_api.h): the path tracer on a caller's own rays.
//   radiance_kernel<INTEG, SIMPLE, LEAN>   pt_radiance.h's walk with RadianceSums: one 16-byte store per ray, (the sum of its
//                                          samples' Li, 0)
// The unit holds the kernel's shell (its LDS, its waves per SIMD) and its launcher; the walk itself, what INTEG, SIMPLE and LEAN
// choose and the six-way dispatch are pt_radiance.h's.
#include "pt_radiance.h"

namespace pt {

// amdgpu_waves_per_eu: each instantiation is compiled for the waves per SIMD it is launched at (pt_feature_host.h:
// radiance_waves_per_simd, from what the compile shows), so the register allocator works to that budget and to no tighter one.
template <int INTEG, bool SIMPLE, bool LEAN>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(radiance_waves_per_simd(INTEG, SIMPLE, LEAN), radiance_waves_per_simd(INTEG, SIMPLE, LEAN))))
radiance_kernel(DeviceScene S, const float4* __restrict__ rays, int n, int nTiles, const uint32_t* __restrict__ jump, unsigned long long seed,
                uint32_t firstStream, int streamPad, int spp, int maxDepth, int useMIS, float4* __restrict__ out, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ uint8_t ldsMedium[SIMPLE ? 1 : 4][kMediumMax][64];
    radiance_walk<INTEG, SIMPLE, LEAN>(S, ldsStack, ldsMedium, spill, rays, n, nTiles, jump, seed, firstStream, streamPad, spp, maxDepth, useMIS,
                                       RadianceSums{out});
}

hipError_t launch_radiance(const DeviceScene& S, int integrator, bool simple, bool lean, int n, const void* rays, const uint32_t* jump,
                           unsigned long long seed, uint32_t firstStream, bool streamPad, int spp, int maxDepth, int useMIS, int blocks, void* out,
                           int32_t* spill, hipStream_t stream) {
    return radiance_dispatch(integrator, simple, lean, [&](auto integ, auto simp, auto ln) {
        hipLaunchKernelGGL((radiance_kernel<decltype(integ)::value, decltype(simp)::value, decltype(ln)::value>), dim3(blocks), dim3(256), 0, stream, S,
                           (const float4*)rays, n, (n + 63) / 64, jump, seed, firstStream, streamPad ? 1 : 0, spp, maxDepth, useMIS, (float4*)out, spill);
        return hipGetLastError();
    });
}

}  // namespace pt
