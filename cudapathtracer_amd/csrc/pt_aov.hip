// pt_aov.hip — feature buffers (albedo, normal, depth) for denoisers and the preview (pt_render_aovs*, include/pt_api.h).
//
// Four kernels, each pt_feature.h's FeatureWave and tile loop around a choice of ray, record and sum:
//   aov_kernel               jittered rays   first_hit_record   FeatureSum over aov_spp rays
//   aov_chain_kernel         jittered rays   follow_chain       FeatureSum, and the mean number of links
//   aov_centre_kernel        the centre ray  first_hit_record   the record itself
//   aov_centre_chain_kernel  the centre ray  follow_chain       the record itself
// Jittered ray k of pixel (x, y) is camera_ray drawn from a FRESH XORWOW stream keyed (seed + k, y*w+x) — the seeding of
// rng_init_kernel, into registers; the centre ray (pt_centre_ray.h) has no seed. The first-hit kernels follow no specular chain; the
// chain kernels report the first non-specular surface behind mirrors and glass, the summed path length as depth and the number of
// links. No pass writes the scene's per-pixel RNG states, its tile accumulator or its counters, so each may run between the chunks of
// a progressive render. (aov_stream, the seeding, is in pt_feature.h: pt_radiance.hip seeds a ray's stream with it too.)
#include "pt_feature.h"

namespace pt {

__global__ void __launch_bounds__(256) aov_kernel(DeviceScene S, CamK cam, const uint32_t* __restrict__ jump, unsigned long long seed,
                                                  int w, int h, int tilesX, int nTiles, int aovSpp, float4* __restrict__ albedo,
                                                  float4* __restrict__ normalDepth, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    FeatureWave W(ldsStack, S, spill);
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        const TilePixel p = tile_pixel(tile, tilesX, W.lane, w, h);
        const uint32_t idx = p.inside ? (uint32_t)(p.y * w + p.x) : 0u;
        FeatureSum sum;
        for (int k = 0; k < aovSpp; k++) {
            Rng rng = aov_stream(jump, seed + (unsigned long long)k, idx);      // (every lane: the seeding ballots per bit)
            if (!p.inside) continue;
            V3 o, d;
            camera_ray<false>(cam, rng, p.x, p.y, o, d, W.c);
            Hit hit;
            trace_closest<false, kStackLds>(S, W.C, o, d, 999999.0f, W.st, hit, W.c);
            if (hit.tri < 0) continue;
            HitInfo hi; resolve_hit(S, hit, o, d, hi);
            float4 ra, rn;
            first_hit_record(S, hi, hit.t, ra, rn);
            sum.add(v3(ra.x, ra.y, ra.z), v3(rn.x, rn.y, rn.z), rn.w);
        }
        if (!p.inside) continue;
        float4 oa, on;
        sum.mean(aovSpp, oa, on);
        albedo[idx] = oa;
        normalDepth[idx] = on;
    }
}

hipError_t launch_aov(const DeviceScene& S, const CamK& cam, const uint32_t* jump, unsigned long long seed, int w, int h, int aovSpp,
                      int blocks, float4* albedo, float4* normalDepth, int32_t* spill, hipStream_t stream) {
    const FeatureTiles T = feature_tiles(w, h);
    hipLaunchKernelGGL(aov_kernel, dim3(blocks), dim3(256), 0, stream, S, cam, jump, seed, w, h, T.tilesX, T.nTiles, aovSpp, albedo, normalDepth, spill);
    return hipGetLastError();
}

// (pt_render_aovs_chain; include/pt_api.h states the contract.) Lanes outside the image call follow_chain too, with no ray.
__global__ void __launch_bounds__(256) aov_chain_kernel(DeviceScene S, CamK cam, const uint32_t* __restrict__ jump, unsigned long long seed,
                                                        int w, int h, int tilesX, int nTiles, int aovSpp, int maxLinks,
                                                        float4* __restrict__ albedo, float4* __restrict__ normalDepth,
                                                        float* __restrict__ linksOut, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ float ldsRec[4][7][64];           // follow_chain's record, lane-interleaved
    FeatureWave W(ldsStack, S, spill);
    float* rec = &ldsRec[W.wave][0][W.lane];
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        const TilePixel p = tile_pixel(tile, tilesX, W.lane, w, h);
        const uint32_t idx = p.inside ? (uint32_t)(p.y * w + p.x) : 0u;
        FeatureSum sum;
        int linkSum = 0;
        for (int k = 0; k < aovSpp; k++) {
            Rng rng = aov_stream(jump, seed + (unsigned long long)k, idx);      // (every lane: the seeding ballots per bit)
            V3 o = v3(0.0f), d = v3(0.0f);
            if (p.inside) camera_ray<false>(cam, rng, p.x, p.y, o, d, W.c);
            const int links = follow_chain(S, W.C, W.st, W.c, o, d, p.inside, maxLinks, rec);
            if (links < 0) continue;
            sum.add(v3(rec[0], rec[64], rec[128]), v3(rec[192], rec[256], rec[320]), rec[384]);
            linkSum += links;
        }
        if (!p.inside) continue;
        float4 oa, on;
        sum.mean(aovSpp, oa, on);
        albedo[idx] = oa;
        normalDepth[idx] = on;
        if (linksOut) linksOut[idx] = sum.hits > 0 ? (float)linkSum / (float)sum.hits : 0.0f;
    }
}

hipError_t launch_aov_chain(const DeviceScene& S, const CamK& cam, const uint32_t* jump, unsigned long long seed, int w, int h, int aovSpp,
                            int maxLinks, int blocks, float4* albedo, float4* normalDepth, float* links, int32_t* spill, hipStream_t stream) {
    const FeatureTiles T = feature_tiles(w, h);
    hipLaunchKernelGGL(aov_chain_kernel, dim3(blocks), dim3(256), 0, stream, S, cam, jump, seed, w, h, T.tilesX, T.nTiles, aovSpp, maxLinks, albedo,
                       normalDepth, links, spill);
    return hipGetLastError();
}

// ---- centre guides (pt_render_aovs_centre, pt_probe_centre_rays) -------------------------------------------------------------------
// (camera_ray_centre, the centre ray of pixel (x, y), is in pt_centre_ray.h: pt_motion.hip traces it too.)
__global__ void probe_centre_kernel(CamK cam, int n, const int* __restrict__ xy, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    V3 o, d;
    camera_ray_centre(cam, xy[2 * i], xy[2 * i + 1], o, d);
    out[6 * i] = o.x; out[6 * i + 1] = o.y; out[6 * i + 2] = o.z; out[6 * i + 3] = d.x; out[6 * i + 4] = d.y; out[6 * i + 5] = d.z;
}

hipError_t launch_probe_centre(const CamK& cam, int n, const int* xy, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(probe_centre_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, cam, n, xy, out);
    return hipGetLastError();
}

// No stream seeding (no jump table, no Rng in registers) and no sums over k: one ray, so the record itself is the result (aov_kernel
// divides it by n = 1, which changes no bit, and writes coverage 1 / 1).
__global__ void __launch_bounds__(256) aov_centre_kernel(DeviceScene S, CamK cam, int w, int h, int tilesX, int nTiles,
                                                         float4* __restrict__ albedo, float4* __restrict__ normalDepth, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    FeatureWave W(ldsStack, S, spill);
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        const TilePixel p = tile_pixel(tile, tilesX, W.lane, w, h);
        if (!p.inside) continue;
        const size_t idx = (size_t)p.y * w + p.x;
        V3 o, d;
        camera_ray_centre(cam, p.x, p.y, o, d);
        Hit hit;
        trace_closest<false, kStackLds>(S, W.C, o, d, 999999.0f, W.st, hit, W.c);
        float4 oa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), on = oa;     // a miss: eight zeros
        if (hit.tri >= 0) { HitInfo hi; resolve_hit(S, hit, o, d, hi); first_hit_record(S, hi, hit.t, oa, on); }
        albedo[idx] = oa;
        normalDepth[idx] = on;
    }
}

hipError_t launch_aov_centre(const DeviceScene& S, const CamK& cam, int w, int h, int blocks, float4* albedo, float4* normalDepth, int32_t* spill,
                             hipStream_t stream) {
    const FeatureTiles T = feature_tiles(w, h);
    hipLaunchKernelGGL(aov_centre_kernel, dim3(blocks), dim3(256), 0, stream, S, cam, w, h, T.tilesX, T.nTiles, albedo, normalDepth, spill);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) aov_centre_chain_kernel(DeviceScene S, CamK cam, int w, int h, int tilesX, int nTiles, int maxLinks,
                                                               float4* __restrict__ albedo, float4* __restrict__ normalDepth,
                                                               float* __restrict__ linksOut, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ float ldsRec[4][7][64];           // follow_chain's record, lane-interleaved
    FeatureWave W(ldsStack, S, spill);
    float* rec = &ldsRec[W.wave][0][W.lane];
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        const TilePixel p = tile_pixel(tile, tilesX, W.lane, w, h);
        V3 o = v3(0.0f), d = v3(0.0f);
        if (p.inside) camera_ray_centre(cam, p.x, p.y, o, d);
        const int links = follow_chain(S, W.C, W.st, W.c, o, d, p.inside, maxLinks, rec);
        if (!p.inside) continue;
        const size_t idx = (size_t)p.y * w + p.x;
        float4 oa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), on = oa;
        float ol = 0.0f;
        if (links >= 0) {
            oa = make_float4(rec[0], rec[64], rec[128], 1.0f);
            on = make_float4(rec[192], rec[256], rec[320], rec[384]);
            ol = (float)links;
        }
        albedo[idx] = oa;
        normalDepth[idx] = on;
        if (linksOut) linksOut[idx] = ol;
    }
}

hipError_t launch_aov_centre_chain(const DeviceScene& S, const CamK& cam, int w, int h, int maxLinks, int blocks, float4* albedo, float4* normalDepth,
                                   float* links, int32_t* spill, hipStream_t stream) {
    const FeatureTiles T = feature_tiles(w, h);
    hipLaunchKernelGGL(aov_centre_chain_kernel, dim3(blocks), dim3(256), 0, stream, S, cam, w, h, T.tilesX, T.nTiles, maxLinks, albedo, normalDepth, links,
                       spill);
    return hipGetLastError();
}

}  // namespace pt
