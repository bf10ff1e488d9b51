// pt_converge.hip — which 8x8 tiles of a resting viewer still need samples (pt_temporal_select, include/pt_api.h: "converge").
// tests/converge_ref.py restates the arithmetic in numpy.
//
//   converge_select_kernel   one wave per 8x8 tile, 16x16 pixels per workgroup as four tiles (the tiling of
//                            temporal_kernel, so a wave's loads fall into a few lines). Per lane one float4 of the
//                            history and one float of its length; r = sqrtf(V) / (1e-4 + sqrtf(lum)), the standard error of
//                            the pixel's mean over the root of the mean (the shape of pt_render_adaptive's estimator); a 64-lane
//                            max through cross-lane shuffles and a ballot for "some pixel is young"; lane 0 stores the tile's
//                            error and its live flag. No LDS, no atomics, no scratch.
// The ascending list of the live tiles and its length come from adaptive_compact_kernel (pt_adaptive.hip) over an iota list
// with the live flags as its keep flags. The other two stages of a converging frame live with what they extend: moments on a
// list in pt_render.hip (render_moments), the accumulation with a tile map in pt_temporal.hip.
#include <cmath>
#include <mutex>

#include <hip/hip_runtime.h>

#include "../../include/pt_api.h"
#include "pt_postfx_host.h"

namespace pt {

hipError_t launch_adaptive_iota(int n, int* list, hipStream_t stream);                                                   // pt_adaptive.hip
hipError_t launch_adaptive_compact(const int* list, const int32_t* keep, int nList, int* out, int* outCount, hipStream_t stream);

__global__ void __launch_bounds__(256) converge_select_kernel(int w, int h, int tilesX, int tilesY, const float4* __restrict__ hist,
                                                              const float* __restrict__ histLen, float threshold, float minHistory,
                                                              float* __restrict__ tileErr, int32_t* __restrict__ tileLive) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = blockIdx.x * 2 + (wave & 1), ty = blockIdx.y * 2 + (wave >> 1);
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    float e = 0.0f;                                        // a lane outside the image contributes 0 and is not young
    bool young = false;
    if (x < w && y < h) {
        const size_t p = (size_t)y * w + x;
        const float4 hq = hist[p];
        const float len = histLen[p];
        const bool exempt = hq.w < 0.0f || !(__builtin_isfinite(hq.x) && __builtin_isfinite(hq.y) && __builtin_isfinite(hq.z) && __builtin_isfinite(hq.w));
        if (!exempt) {
            const float lum = 0.2126f * hq.x + 0.7152f * hq.y + 0.0722f * hq.z;
            const float r = sqrtf(hq.w) / (1e-4f + sqrtf(lum));
            e = r > 0.0f ? r : 0.0f;                       // max(0, r): a NaN (lum < 0) and -0 give +0
            young = len < minHistory;
        }
    }
    for (int k = 32; k > 0; k >>= 1) {                     // E_T: every e here is >= +0 and not NaN
        const float other = __shfl_xor(e, k, 64);
        e = other > e ? other : e;
    }
    const bool anyYoung = __ballot(young) != 0ull;
    if (lane == 0 && tx < tilesX && ty < tilesY) {         // (the grid is rounded up to pairs of tiles)
        const int tile = ty * tilesX + tx;
        tileErr[tile] = e;
        tileLive[tile] = (e < threshold && !anyYoung) ? 0 : 1;
    }
}

int check_converge_params(const char* fn, const pt_converge_params& P) {
    if (!(P.threshold >= 0.0f) || !std::isfinite(P.threshold)) return postfx_fail_fn(-1, fn, "threshold must be a finite number >= 0");
    if (P.min_history < 1) return postfx_fail_fn(-1, fn, "min_history %d must be at least 1", P.min_history);
    return 0;
}

static int check_select_args(int w, int h, const void* hist, const void* histLen, const pt_converge_params& P, const void* tileErr,
                             const void* tileLive, const void* list, const void* count) {
    if (int r = postfx_check_size("pt_temporal_select", w, h)) return r;
    if (!hist || !histLen) return postfx_fail(-1, "pt_temporal_select: null buffer");
    if (!tileErr || !tileLive || !list || !count) return postfx_fail(-1, "pt_temporal_select: null output");
    if (int r = check_converge_params("pt_temporal_select", P)) return r;
    const size_t n = (size_t)w * h, tb = (size_t)((w + 7) / 8) * ((h + 7) / 8) * 4;
    const void* out[4] = {tileErr, tileLive, list, count};
    const size_t outBytes[4] = {tb, tb, tb, 4};
    for (int i = 0; i < 4; i++) {
        if (overlaps(out[i], outBytes[i], hist, n * 16) || overlaps(out[i], outBytes[i], histLen, n * 4))
            return postfx_fail(-1, "pt_temporal_select: the outputs must not alias the inputs or each other");
        for (int j = 0; j < i; j++)
            if (overlaps(out[i], outBytes[i], out[j], outBytes[j]))
                return postfx_fail(-1, "pt_temporal_select: the outputs must not alias the inputs or each other");
    }
    return 0;
}

// The list 0, 1, 2, ... that the compaction reads, one per HIP device and process, grown on demand. Its contents never change,
// so every stream may read it; it is filled on the caller's stream, which is waited for once, when it grows.
struct IotaList { int* p = nullptr; int n = 0; };
static std::mutex g_iotaMutex;
static IotaList g_iota[PT_MULTI_MAX_DEVICES];

static int iota_list(int n, hipStream_t stream, const int** out) {
    int dev = -1;
    POSTFX_HIP_OK(hipGetDevice(&dev));
    if (dev < 0 || dev >= PT_MULTI_MAX_DEVICES) return postfx_fail(-2, "pt_temporal_select: HIP device %d is out of range", dev);
    std::lock_guard<std::mutex> lock(g_iotaMutex);
    IotaList& L = g_iota[dev];
    if (L.n < n) {
        int cap = 4096;
        while (cap < n) cap <<= 1;
        int* p = nullptr;
        POSTFX_HIP_OK(hipMalloc(&p, (size_t)cap * sizeof(int)));
        hipError_t e = launch_adaptive_iota(cap, p, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { (void)hipFree(p); return postfx_fail(-2, "pt_temporal_select: could not fill the tile list"); }
        if (L.p) (void)hipFree(L.p);                       // (hipFree waits for whatever still reads it)
        L.p = p; L.n = cap;
    }
    *out = L.p;
    return 0;
}

static int select_launch(int w, int h, const float4* hist, const float* histLen, const pt_converge_params& P, float* tileErr, int32_t* tileLive,
                         int* list, int* count, hipStream_t stream) {
    const int tilesX = (w + 7) / 8, tilesY = (h + 7) / 8, T = tilesX * tilesY;
    const int* iota = nullptr;
    if (int r = iota_list(T, stream, &iota)) return r;
    hipLaunchKernelGGL(converge_select_kernel, dim3((w + 15) / 16, (h + 15) / 16), dim3(256), 0, stream, w, h, tilesX, tilesY, hist, histLen,
                       P.threshold, (float)P.min_history, tileErr, tileLive);
    POSTFX_HIP_OK(hipGetLastError());
    POSTFX_HIP_OK(launch_adaptive_compact(iota, tileLive, T, list, count, stream));
    return 0;
}

}  // namespace pt

using namespace pt;

extern "C" {

void pt_converge_defaults(pt_converge_params* out) {
    if (!out) return;
    out->threshold = 0.5f;
    out->min_history = 8;
}

int pt_temporal_select_device(int w, int h, const void* d_hist, const void* d_hist_len, const pt_converge_params* params, void* d_tile_err,
                              void* d_tile_live, void* d_list, void* d_count, void* stream) {
    pt_converge_params P;
    if (params) P = *params; else pt_converge_defaults(&P);
    if (int r = check_select_args(w, h, d_hist, d_hist_len, P, d_tile_err, d_tile_live, d_list, d_count)) return r;
    return select_launch(w, h, (const float4*)d_hist, (const float*)d_hist_len, P, (float*)d_tile_err, (int32_t*)d_tile_live, (int*)d_list,
                         (int*)d_count, (hipStream_t)stream);
}

int pt_temporal_select(int w, int h, const float* hist, const float* hist_len, const pt_converge_params* params, float* out_tile_err,
                       int32_t* out_tile_live, int32_t* out_list, int32_t* out_count) {
    pt_converge_params P;
    if (params) P = *params; else pt_converge_defaults(&P);
    if (int r = check_select_args(w, h, hist, hist_len, P, out_tile_err, out_tile_live, out_list, out_count)) return r;
    const size_t n = (size_t)w * h, tb = (size_t)((w + 7) / 8) * ((h + 7) / 8) * 4;
    const HostIn in[] = {{hist, n * 16}, {hist_len, n * 4}};
    const HostOut out[] = {{out_tile_err, tb}, {out_tile_live, tb}, {out_list, tb}, {out_count, 4}};
    return postfx_host_form("pt_temporal_select", 0, in, out, [&](char*, char** d, char** o) {
        if (hipMemset(o[2], 0, tb) != hipSuccess)          // the list's entries past the count read back as 0
            return postfx_fail(-2, "pt_temporal_select: upload failed");
        return select_launch(w, h, (const float4*)d[0], (const float*)d[1], P, (float*)o[0], (int32_t*)o[1], (int*)o[2], (int*)o[3], nullptr);
    });
}

}  // extern "C"
