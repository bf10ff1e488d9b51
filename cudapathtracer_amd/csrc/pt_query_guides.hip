// pt_query_guides.hip — the denoisers' guides for a caller's own rays (pt_query_guides, include/pt_api.h): what
// pt_render_aovs_centre gives for the centre ray of a pixel, for a ray record instead. pt_query.hip's frame: pt_feature.h's FeatureWave,
// "tile" t = rays 64 t .. 64 t + 63, one lane each, four waves per workgroup, persistent over the tiles, the LDS stack overflowing
// into the scene's feature spill area. No camera, no RNG, no seed:
//   query_guides_kernel        trace_closest (non-counting) with the ray's own max_t, resolve_hit, first_hit_record: aov_centre_kernel's
//                              body
//   query_guides_chain_kernel  follow_chain with the ray's own max_t on the first segment and 999999 on every link:
//                              aov_centre_chain_kernel's body
// A ray is two 16-byte loads, its guides two 16-byte stores and, where the caller wants the links, one of 4 bytes. A miss is eight
// zeros and no links. Lanes past n take no ray and store nothing (in the chain kernel they call follow_chain with live = false, as
// its ballots want every lane of the wave).
#include "pt_feature.h"

namespace pt {

__global__ void __launch_bounds__(256) query_guides_kernel(DeviceScene S, const float4* __restrict__ rays, int n, int nTiles, float4* __restrict__ albedo,
                                                           float4* __restrict__ normalDepth, float* __restrict__ linksOut, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    FeatureWave W(ldsStack, S, spill);
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        const int i = tile * 64 + W.lane;
        if (i >= n) continue;
        const QueryRay q = load_ray(rays, (size_t)i);
        Hit hit;
        trace_closest<false, kStackLds>(S, W.C, q.o, q.d, q.maxT, W.st, hit, W.c);
        float4 oa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), on = oa;     // a miss: eight zeros
        if (hit.tri >= 0) { HitInfo hi; resolve_hit(S, hit, q.o, q.d, hi); first_hit_record(S, hi, hit.t, oa, on); }
        albedo[i] = oa;
        normalDepth[i] = on;
        if (linksOut) linksOut[i] = 0.0f;
    }
}

__global__ void __launch_bounds__(256) query_guides_chain_kernel(DeviceScene S, const float4* __restrict__ rays, int n, int nTiles, int maxLinks,
                                                                 float4* __restrict__ albedo, float4* __restrict__ normalDepth,
                                                                 float* __restrict__ linksOut, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ float ldsRec[4][7][64];           // follow_chain's record, lane-interleaved
    FeatureWave W(ldsStack, S, spill);
    float* rec = &ldsRec[W.wave][0][W.lane];
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        const int i = tile * 64 + W.lane;
        const bool live = i < n;
        QueryRay q = {v3(0.0f), v3(0.0f), 0.0f};
        if (live) q = load_ray(rays, (size_t)i);
        const int links = follow_chain(S, W.C, W.st, W.c, q.o, q.d, live, maxLinks, rec, ChainHook(), q.maxT);
        if (!live) continue;
        float4 oa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), on = oa;
        float ol = 0.0f;
        if (links >= 0) {
            oa = make_float4(rec[0], rec[64], rec[128], 1.0f);
            on = make_float4(rec[192], rec[256], rec[320], rec[384]);
            ol = (float)links;
        }
        albedo[i] = oa;
        normalDepth[i] = on;
        if (linksOut) linksOut[i] = ol;
    }
}

hipError_t launch_query_guides(const DeviceScene& S, int n, const void* rays, int maxLinks, int blocks, void* albedo, void* normalDepth, float* links,
                               int32_t* spill, hipStream_t stream) {
    const int nTiles = (n + 63) / 64;
    if (maxLinks > 0)
        hipLaunchKernelGGL(query_guides_chain_kernel, dim3(blocks), dim3(256), 0, stream, S, (const float4*)rays, n, nTiles, maxLinks, (float4*)albedo,
                           (float4*)normalDepth, links, spill);
    else
        hipLaunchKernelGGL(query_guides_kernel, dim3(blocks), dim3(256), 0, stream, S, (const float4*)rays, n, nTiles, (float4*)albedo,
                           (float4*)normalDepth, links, spill);
    return hipGetLastError();
}

}  // namespace pt
