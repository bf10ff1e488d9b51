// pt_moments.hip — the per-batch bookkeeping kernel of pt_render_moments (include/pt_api.h).
//
// A moments render is B batches of c samples on the whole frame; the per-pixel streams continue across the batches, so after
// batch j the accumulator S holds exactly the sums of pt_render(spp = j c). After every batch
//   moments_update_kernel    d = S - P, Q = Q + d d per rgb channel, P = S (the first batch takes P = Q = 0 without reading them)
// so Q ends as the sum of the B squared batch sums. The renders are the ordinary launches of render_tiles (either variant): no
// megakernel knows about this. S, P and Q are tile-major over the whole frame ([tile][64] float4, lane = ly*8+lx), so a wave
// reads 1 KB coalesced per buffer; lanes outside the image carry zeros along. ~80 B per pixel and batch: cheap, not clever.
// Host side: pt_render.hip.
#include "pt_params.h"

namespace pt {

// One wave per tile, lane = pixel. The arithmetic is the header's, in its order (-ffp-contract=off: the product is rounded
// before the add). No special case for NaN / Inf: they propagate into Q.
__global__ void __launch_bounds__(256) moments_update_kernel(int nPixels, const float4* __restrict__ S, float4* __restrict__ P,
                                                             float4* __restrict__ Q, int first, float batches) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= nPixels) return;
    const float4 s = S[o];
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q = p;
    if (!first) { p = P[o]; q = Q[o]; }
    const float dx = s.x - p.x, dy = s.y - p.y, dz = s.z - p.z;
    q.x = q.x + dx * dx; q.y = q.y + dy * dy; q.z = q.z + dz * dz; q.w = batches;
    P[o] = s;
    Q[o] = q;
}

// nTiles * 64 float4 per buffer (nTiles * 64 fits an int: the callers check w * h).
hipError_t launch_moments_update(int nTiles, const float4* S, float4* P, float4* Q, bool first, int batches, hipStream_t stream) {
    if (nTiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(moments_update_kernel, dim3((nTiles + 3) / 4), dim3(256), 0, stream, nTiles * 64, S, P, Q, first ? 1 : 0, (float)batches);
    return hipGetLastError();
}

}  // namespace pt
