// pt_preview.hip — what a viewer needs around the existing stages (include/pt_api.h, "preview"):
//
//   resolve_kernel      radiance sums to display bytes: the division of novum_finalise (or of an adaptive frame's tile map), its
//                       NaN / Inf paint, exposure, novum_save_bmp's tone map + gamma and its byte conversion. One thread per pixel,
//                       16x16 pixels per workgroup as four 8x8 tiles (one per wave, the tiling of temporal_kernel), so a
//                       wave's tile index is uniform and the tile's sample count is one scalar load. One float4 load, one dword
//                       store (plus the optional float4 mean); no LDS, no scratch. tests/preview_ref.py restates it in numpy.
//   pt_preview          a session that owns the device buffers of one w x h viewer and runs render_moments -> render_aovs ->
//                       temporal_accumulate -> denoise_hist -> resolve per frame on one stream through the public *_device entry
//                       points, ping-ponging history and guide. Nothing crosses PCIe unless pt_preview_read asks for it.
//                       With a render scale s > 1 (pt_preview_set_scale) the moments render runs at 1/s of the size in each axis and
//                       pt_upsample + pt_temporal_accumulate_cur bring it into the same display-size history.
//                       With converge on (pt_preview_set_converge) a frame whose camera rests selects the tiles that still need
//                       samples from the history, renders moments on that list alone and carries the other tiles' history forward.
//                       With a guide chain (pt_preview_set_guide_chain) every feature pass of a frame is pt_render_aovs_chain_device.
//                       With centre guides (pt_preview_set_guide_centre) every feature pass is pt_render_aovs_centre_device, the
//                       low-res guide of a scaled frame is pt_guide_subsample_device of the display guide, and a frame whose camera
//                       rests reuses the previous frame's guide: the guide has no seed, so nothing in it could have changed.
//                       With motion on (pt_preview_set_motion) the frame after an announced vertex update that keeps its history
//                       also runs pt_render_motion_device and accumulates through pt_temporal_accumulate[_cur]_motion_device.
//                       With respond on (pt_preview_set_respond) every frame with a history that is not a converging frame accumulates
//                       through pt_temporal_accumulate_respond_device, with the arguments of the form it would have taken.
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../include/pt_api.h"
#include "pt_postfx_host.h"

namespace pt {

int check_converge_params(const char* fn, const pt_converge_params& P);       // pt_converge.hip
int check_respond_params(const char* fn, const pt_respond_params& R);         // pt_temporal.hip

// novum_host.cpp's clamp01, aces and to_byte, operation for operation (-ffp-contract=off: nothing fuses).
__device__ inline float rs_clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
__device__ inline float rs_aces(float c) { return rs_clamp01((c * (2.51f * c + 0.03f)) / (c * (2.43f * c + 0.59f) + 0.14f)); }
__device__ inline uint32_t rs_byte(float c) {
    const float v = rs_clamp01(c) * 255.0f + 0.5f;
    return v != v ? 0u : (uint32_t)v;                     // v is NaN or in [0.5, 255.5]
}
__device__ inline float rs_display(float m, float exposure, bool tonemap) {
    const float c = m * exposure;
    return tonemap ? powf(rs_aces(c), 1.0f / 2.2f) : c;
}

__global__ void __launch_bounds__(256) resolve_kernel(int w, int h, const float4* __restrict__ in, float spp, const int32_t* __restrict__ tileSpp,
                                                      int tilesX, int tonemap, float exposure, uint32_t* __restrict__ out8,
                                                      float4* __restrict__ mean) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = blockIdx.x * 2 + (wave & 1), ty = blockIdx.y * 2 + (wave >> 1);
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    if (x >= w || y >= h) return;                             // (a tile outside the grid has no lane left: no read past the map)
    const float n = tileSpp ? (float)tileSpp[__builtin_amdgcn_readfirstlane(ty * tilesX + tx)] : spp;
    const size_t p = (size_t)y * w + x;
    const float4 s = in[p];
    float4 m = make_float4(s.x / n, s.y / n, s.z / n, s.w);
    if (m.x != m.x || m.y != m.y || m.z != m.z) m = make_float4(1.0f, 0.0f, 1.0f, 0.0f);
    if (__builtin_isinf(m.x) || __builtin_isinf(m.y) || __builtin_isinf(m.z)) m = make_float4(0.0f, 1.0f, 0.0f, 0.0f);
    if (mean) mean[p] = m;
    const uint32_t r = rs_byte(rs_display(m.x, exposure, tonemap != 0)), g = rs_byte(rs_display(m.y, exposure, tonemap != 0)),
                   b = rs_byte(rs_display(m.z, exposure, tonemap != 0));
    out8[p] = r | (g << 8) | (b << 16) | 0xff000000u;
}

static int check_resolve_params(const pt_resolve_params& P) {
    if (P.tonemap != 0 && P.tonemap != 1) return postfx_fail(-1, "pt_resolve: tonemap %d must be 0 or 1", P.tonemap);
    if (!(P.exposure > 0.0f) || !std::isfinite(P.exposure)) return postfx_fail(-1, "pt_resolve: exposure must be positive and finite");
    return 0;
}

static int check_resolve_args(int w, int h, const void* in, int spp, const void* tileSpp, const pt_resolve_params& P, const void* out8,
                              const void* mean) {
    if (int r = postfx_check_size("pt_resolve", w, h)) return r;
    if (!in) return postfx_fail(-1, "pt_resolve: null buffer");
    if (!out8) return postfx_fail(-1, "pt_resolve: null output");
    if (!tileSpp && spp < 1) return postfx_fail(-1, "pt_resolve: spp %d must be at least 1 (or give a tile map)", spp);
    if (int r = check_resolve_params(P)) return r;
    const size_t n = (size_t)w * h, tiles = (size_t)((w + 7) / 8) * ((h + 7) / 8);
    if (overlaps(out8, n * 4, in, n * 16) || (mean && (overlaps(mean, n * 16, in, n * 16) || overlaps(mean, n * 16, out8, n * 4))) ||
        (tileSpp && (overlaps(out8, n * 4, tileSpp, tiles * 4) || (mean && overlaps(mean, n * 16, tileSpp, tiles * 4)))))
        return postfx_fail(-1, "pt_resolve: the outputs must not alias the inputs or each other");
    return 0;
}

static int resolve_launch(int w, int h, const float4* in, int spp, const int32_t* tileSpp, const pt_resolve_params& P, uint32_t* out8, float4* mean,
                          hipStream_t stream) {
    hipLaunchKernelGGL(resolve_kernel, dim3((w + 15) / 16, (h + 15) / 16), dim3(256), 0, stream, w, h, in, (float)spp, tileSpp, (w + 7) / 8,
                       P.tonemap, P.exposure, out8, mean);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace pt

using namespace pt;

// One viewer: every buffer lives in `pool`. cur names the half of the ping-pong pairs that holds the history and the guide of the
// last good frame; a frame writes the other half and flips only when all of its stages succeeded.
struct pt_preview {
    pt_scene* scene;
    int w, h;
    pt_preview_params P;
    hipStream_t stream;
    hipEvent_t ev[6];                     // before the frame and after each of its five stages
    char* pool;
    char *S, *Q, *A, *N[2], *H[2], *L[2]; // sums, albedo; guide, history and history length twice (temporal 0: one guide only)
    char *ws, *filt, *mean, *rgba8;       // the filters' workspace, the filtered frame, the displayed mean and its bytes
    int scale;                            // render scale of the next frame; > 1 uses the buffers below (their own allocations)
    int guideChain;                       // max_links of the feature passes; 0: the first-hit pass (pt_preview_set_guide_chain)
    int guideCentre;                      // 1: the feature passes trace pixel centres (pt_preview_set_guide_centre)
    int curG;                             // the half of N that holds the last good frame's guide: cur's, until a frame reuses the guide
    bool guideFresh;                      // A and N[curG] are the guide of prevCam (no later frame has written A and then failed)
    int guidePasses, framePasses;         // feature-pass launches of all good frames / of the frame in flight (committed with the flip)
    char* lo;                             // four low-res float4 buffers of loCap pixels each: S, Q, albedo, guide
    size_t loCap;
    char* curEV;                          // w*h float4: pt_upsample's output
    int cur;
    bool haveHist, haveFrame;
    pt_camera prevCam;
    pt_preview_stats stats;
    // converge (pt_preview_set_converge): one allocation holding the tile error and the live map twice (a converging frame writes
    // the half that curT does not name and flips with the history), the live list and its count
    bool converge;
    pt_converge_params C;
    char* tiles;
    char *tErr[2], *tLive[2], *tList, *tCount;
    int curT;
    bool haveTiles;
    int lastLive;                         // live tiles of the last good frame (its total is the frame's tile count)
    int frameLive; bool frameConverged;   // what the frame in flight found; committed with the flip
    int sceneGen;                         // pt_scene_generation at the last good frame (at create before the first)
    bool sceneChanged;                    // pt_preview_scene_changed since the last good frame: the next frame counts as a moved camera
    int motion;                           // 1: MOTION FRAMES reproject moved surfaces (pt_preview_set_motion)
    char* M;                              // w*h float4: pt_render_motion's output (its own allocation, made when motion is first turned on)
    bool frameMotion;                     // the frame in flight is a motion frame
    bool respond;                         // frames with a history accumulate through pt_temporal_accumulate_respond_device
    pt_respond_params R;
    char* respondWs;                      // its workspace (its own allocation, made when respond is first turned on)
};

extern "C" {

void pt_resolve_defaults(pt_resolve_params* out) {
    if (!out) return;
    out->tonemap = 1;
    out->exposure = 1.0f;
}

int pt_resolve_device(int w, int h, const void* d_rgba, int spp, const void* d_tile_spp, const pt_resolve_params* params, void* d_rgba8, void* d_mean,
                      void* stream) {
    pt_resolve_params P;
    if (params) P = *params; else pt_resolve_defaults(&P);
    if (int r = check_resolve_args(w, h, d_rgba, spp, d_tile_spp, P, d_rgba8, d_mean)) return r;
    return resolve_launch(w, h, (const float4*)d_rgba, spp, (const int32_t*)d_tile_spp, P, (uint32_t*)d_rgba8, (float4*)d_mean, (hipStream_t)stream);
}

int pt_resolve(int w, int h, const float* rgba, int spp, const int32_t* tile_spp, const pt_resolve_params* params, uint8_t* rgba8, float* mean) {
    pt_resolve_params P;
    if (params) P = *params; else pt_resolve_defaults(&P);
    if (int r = check_resolve_args(w, h, rgba, spp, tile_spp, P, rgba8, mean)) return r;
    const size_t n = (size_t)w * h, tiles = (size_t)((w + 7) / 8) * ((h + 7) / 8);
    if (tile_spp)
        for (size_t t = 0; t < tiles; t++)
            if (tile_spp[t] <= 0) return postfx_fail(-1, "pt_resolve: tile %d has %d samples; every tile needs at least one", (int)t, tile_spp[t]);
    const HostIn in[] = {{rgba, n * 16}, {tile_spp, tiles * 4}};
    const HostOut out[] = {{rgba8, n * 4}, {mean, n * 16}};
    return postfx_host_form("pt_resolve", 0, in, out, [&](char*, char** d, char** o) {
        return resolve_launch(w, h, (const float4*)d[0], spp, (const int32_t*)d[1], P, (uint32_t*)o[0], (float4*)o[1], nullptr);
    });
}

void pt_preview_defaults(pt_preview_params* out) {
    if (!out) return;
    out->spp = 4; out->batches = 2; out->max_depth = 8; out->integrator = PT_UNIDIRECTIONAL; out->use_mis = 1; out->aov_spp = 1;
    out->temporal = 1; out->filter = 1;
    pt_temporal_defaults(&out->temporal_params);
    pt_denoise_var_defaults(&out->filter_params);
    pt_resolve_defaults(&out->resolve_params);
}

void pt_preview_destroy(pt_preview* p) {
    if (!p) return;
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    for (hipEvent_t e : p->ev)
        if (e) (void)hipEventDestroy(e);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    if (p->pool) (void)hipFree(p->pool);
    if (p->lo) (void)hipFree(p->lo);
    if (p->curEV) (void)hipFree(p->curEV);
    if (p->tiles) (void)hipFree(p->tiles);
    if (p->M) (void)hipFree(p->M);
    if (p->respondWs) (void)hipFree(p->respondWs);
    delete p;
}

pt_preview* pt_preview_create(pt_scene* scene, int w, int h, const pt_preview_params* params) {
    pt_preview_params P;
    if (params) P = *params; else pt_preview_defaults(&P);
    // what the stages would refuse on every frame is refused here, before any HIP call; the filters' and the history's own
    // parameters are checked by their stages
    int bad = 0;
    if (!scene) bad = postfx_fail(-1, "pt_preview_create: null scene");
    else if (w <= 0 || h <= 0) bad = postfx_fail(-1, "pt_preview_create: image size %d x %d must be positive", w, h);
    else if ((long long)((w + 7) / 8) * ((h + 7) / 8) * 64 > 0x7fffffffll) bad = postfx_fail(-1, "pt_preview_create: image of %d x %d pixels is too large", w, h);
    else if (P.spp <= 0) bad = postfx_fail(-1, "pt_preview_create: spp %d must be positive", P.spp);
    else if (P.batches < 2) bad = postfx_fail(-1, "pt_preview_create: batches %d must be at least 2", P.batches);
    else if (P.spp % P.batches != 0) bad = postfx_fail(-1, "pt_preview_create: batches %d must divide spp %d", P.batches, P.spp);
    else if (P.integrator != PT_UNIDIRECTIONAL && P.integrator != PT_NAIVE_UNIDIRECTIONAL)
        bad = postfx_fail(-3, "pt_preview_create: integrator %d is out of scope: only UNIDIRECTIONAL (0) and NAIVE_UNIDIRECTIONAL (2)", P.integrator);
    else if (P.aov_spp <= 0) bad = postfx_fail(-1, "pt_preview_create: aov_spp %d must be positive", P.aov_spp);
    else if ((P.temporal != 0 && P.temporal != 1) || (P.filter != 0 && P.filter != 1))
        bad = postfx_fail(-1, "pt_preview_create: temporal %d and filter %d must be 0 or 1", P.temporal, P.filter);
    else bad = check_resolve_params(P.resolve_params);
    if (bad) return nullptr;

    pt_preview* p = new pt_preview();      // zeroed
    p->scene = scene; p->w = w; p->h = h; p->P = P; p->scale = 1;
    p->sceneGen = pt_scene_generation(scene);
    const size_t n = (size_t)w * h, b16 = n * 16, b4 = (n * 4 + 15) & ~(size_t)15;
    const size_t ws = (pt_denoise_var_workspace_bytes(w, h) + 15) & ~(size_t)15;
    const int pairs = P.temporal ? 2 : 1;
    const size_t total = 3 * b16 + pairs * b16 + (P.temporal ? 2 * (b16 + b4) : 0) + ws + 2 * b16 + b4;
    bool ok = hipMalloc(&p->pool, total) == hipSuccess && hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i < 6; i++) ok = hipEventCreate(&p->ev[i]) == hipSuccess;
    if (!ok) {
        postfx_fail(-2, "pt_preview_create: could not allocate the session's buffers, stream and events (no usable HIP device, or out of memory)");
        pt_preview_destroy(p);
        return nullptr;
    }
    char* c = p->pool;
    auto take = [&c](size_t bytes) { char* r = c; c += bytes; return r; };
    p->S = take(b16); p->Q = take(b16); p->A = take(b16);
    for (int i = 0; i < pairs; i++) p->N[i] = take(b16);
    if (P.temporal)
        for (int i = 0; i < 2; i++) { p->H[i] = take(b16); p->L[i] = take(b4); }
    p->ws = take(ws); p->filt = take(b16); p->mean = take(b16); p->rgba8 = take(b4);
    return p;
}

int pt_preview_reset(pt_preview* p) {
    if (!p) return postfx_fail(-1, "pt_preview_reset: null session");
    p->haveHist = p->haveFrame = p->haveTiles = false;
    return 0;
}

int pt_preview_scene_changed(pt_preview* p, int keep_history) {
    if (!p) return postfx_fail(-1, "pt_preview_scene_changed: null session");
    if (keep_history != 0 && keep_history != 1) return postfx_fail(-1, "pt_preview_scene_changed: keep_history %d must be 0 or 1", keep_history);
    if (!keep_history) p->haveHist = p->haveFrame = p->haveTiles = false;
    p->sceneChanged = true;
    return 0;
}

int pt_preview_set_scale(pt_preview* p, int scale) {
    if (!p) return postfx_fail(-1, "pt_preview_set_scale: null session");
    if (scale < 1 || scale > 8) return postfx_fail(-1, "pt_preview_set_scale: scale %d must be 1..8", scale);
    if (p->w % scale != 0 || p->h % scale != 0)
        return postfx_fail(-1, "pt_preview_set_scale: scale %d must divide the session's size %d x %d", scale, p->w, p->h);
    if (scale > 1) {                      // (no frame is in flight: pt_preview_frame blocks)
        const size_t need = (size_t)(p->w / scale) * (p->h / scale);
        char* cur = p->curEV;
        char* lo = nullptr;
        bool ok = cur || hipMalloc(&cur, (size_t)p->w * p->h * 16) == hipSuccess;
        if (ok && need > p->loCap) ok = hipMalloc(&lo, 4 * need * 16) == hipSuccess;
        if (!ok) {
            if (cur && !p->curEV) (void)hipFree(cur);
            return postfx_fail(-2, "pt_preview_set_scale: could not allocate the buffers of scale %d", scale);
        }
        p->curEV = cur;
        if (lo) {
            if (p->lo) (void)hipFree(p->lo);
            p->lo = lo; p->loCap = need;
        }
    }
    p->scale = scale;
    return 0;
}

int pt_preview_scale(pt_preview* p) { return p ? p->scale : postfx_fail(-1, "pt_preview_scale: null session"); }

int pt_preview_set_guide_chain(pt_preview* p, int max_links) {
    if (!p) return postfx_fail(-1, "pt_preview_set_guide_chain: null session");
    if (max_links < 0 || max_links > 16) return postfx_fail(-1, "pt_preview_set_guide_chain: max_links %d must be 0..16", max_links);
    // guides from before and after a change do not validate against each other: the next frame is a first frame
    if (max_links != p->guideChain) p->haveHist = p->haveFrame = p->haveTiles = false;
    p->guideChain = max_links;
    return 0;
}

int pt_preview_guide_chain(pt_preview* p) { return p ? p->guideChain : postfx_fail(-1, "pt_preview_guide_chain: null session"); }

int pt_preview_set_guide_centre(pt_preview* p, int on) {
    if (on != 0 && on != 1) return postfx_fail(-1, "pt_preview_set_guide_centre: on %d must be 0 or 1", on);
    if (!p) return postfx_fail(-1, "pt_preview_set_guide_centre: null session");
    // jittered and centre guides do not validate against each other: the next frame is a first frame
    if (on != p->guideCentre) p->haveHist = p->haveFrame = p->haveTiles = false;
    p->guideCentre = on;
    return 0;
}

int pt_preview_guide_centre(pt_preview* p) { return p ? p->guideCentre : postfx_fail(-1, "pt_preview_guide_centre: null session"); }

int pt_preview_guide_passes(pt_preview* p) { return p ? p->guidePasses : postfx_fail(-1, "pt_preview_guide_passes: null session"); }

int pt_preview_set_motion(pt_preview* p, int on) {
    if (on != 0 && on != 1) return postfx_fail(-1, "pt_preview_set_motion: on %d must be 0 or 1", on);
    if (!p) return postfx_fail(-1, "pt_preview_set_motion: null session");
    if (on && !p->M) {                    // (no frame is in flight: pt_preview_frame blocks)
        if (hipMalloc(&p->M, (size_t)p->w * p->h * 16) != hipSuccess) {
            p->M = nullptr;
            return postfx_fail(-2, "pt_preview_set_motion: could not allocate the motion buffer");
        }
    }
    p->motion = on;                       // (no reset: the guides do not depend on it)
    return 0;
}

int pt_preview_motion(pt_preview* p) { return p ? p->motion : postfx_fail(-1, "pt_preview_motion: null session"); }

int pt_preview_set_respond(pt_preview* p, const pt_respond_params* params) {
    if (!p) return postfx_fail(-1, "pt_preview_set_respond: null session");
    if (!params) { p->respond = false; return 0; }
    if (int r = check_respond_params("pt_preview_set_respond", *params)) return r;
    if (!p->respondWs) {                  // (no frame is in flight: pt_preview_frame blocks)
        if (hipMalloc(&p->respondWs, pt_temporal_respond_workspace_bytes(p->w, p->h)) != hipSuccess) {
            p->respondWs = nullptr;
            return postfx_fail(-2, "pt_preview_set_respond: could not allocate the workspace");
        }
    }
    p->respond = true;                    // (no reset: neither the guides nor the history's format depend on it)
    p->R = *params;
    return 0;
}

int pt_preview_respond(pt_preview* p, pt_respond_params* out) {
    if (!p) return postfx_fail(-1, "pt_preview_respond: null session");
    if (p->respond && out) *out = p->R;
    return p->respond ? 1 : 0;
}

int pt_preview_set_converge(pt_preview* p, const pt_converge_params* params) {
    if (!p) return postfx_fail(-1, "pt_preview_set_converge: null session");
    if (!params || params->threshold == 0.0f) { p->converge = false; return 0; }
    if (int r = check_converge_params("pt_preview_set_converge", *params)) return r;
    if (!p->tiles) {                      // (no frame is in flight: pt_preview_frame blocks)
        const size_t tb = ((size_t)((p->w + 7) / 8) * ((p->h + 7) / 8) * 4 + 15) & ~(size_t)15;
        if (hipMalloc(&p->tiles, 5 * tb + 16) != hipSuccess) {
            p->tiles = nullptr;
            return postfx_fail(-2, "pt_preview_set_converge: could not allocate the tile buffers");
        }
        char* c = p->tiles;
        for (int i = 0; i < 2; i++) { p->tErr[i] = c; c += tb; p->tLive[i] = c; c += tb; }
        p->tList = c; c += tb; p->tCount = c;
    }
    p->converge = true;
    p->C = *params;
    return 0;
}

int pt_preview_last_live(pt_preview* p, int* live, int* total) {
    if (!p) return postfx_fail(-1, "pt_preview_last_live: null session");
    if (!p->haveFrame) return postfx_fail(-1, "pt_preview_last_live: no frame since the session was created or reset");
    if (live) *live = p->lastLive;
    if (total) *total = ((p->w + 7) / 8) * ((p->h + 7) / 8);
    return 0;
}

int pt_preview_read_tiles(pt_preview* p, float* tile_err, int32_t* tile_live) {
    if (!p) return postfx_fail(-1, "pt_preview_read_tiles: null session");
    if (!p->haveTiles) return postfx_fail(-1, "pt_preview_read_tiles: no converging frame since the session was created or reset");
    const size_t tb = (size_t)((p->w + 7) / 8) * ((p->h + 7) / 8) * 4;
    if (tile_err) POSTFX_HIP_OK(hipMemcpy(tile_err, p->tErr[p->curT], tb, hipMemcpyDeviceToHost));
    if (tile_live) POSTFX_HIP_OK(hipMemcpy(tile_live, p->tLive[p->curT], tb, hipMemcpyDeviceToHost));
    return 0;
}

// A feature pass of a frame: the first-hit pass, or the chain pass when the session has a guide chain; with centre guides the
// centre pass of either kind, which has no aov_spp and no seed.
static int preview_aovs(pt_preview* p, const pt_camera* cam, int w, int h, uint64_t seed, void* dA, void* dN) {
    p->framePasses++;
    if (p->guideCentre) return pt_render_aovs_centre_device(p->scene, cam, w, h, p->guideChain, dA, dN, nullptr, p->stream);
    if (p->guideChain > 0) return pt_render_aovs_chain_device(p->scene, cam, w, h, p->P.aov_spp, p->guideChain, seed, dA, dN, nullptr, p->stream);
    return pt_render_aovs_device(p->scene, cam, w, h, p->P.aov_spp, seed, dA, dN, p->stream);
}

// The display-size guide of a frame that traces one and, on a motion frame, the motion buffer: one fused pass where the guide is the
// centre first-hit pass (the motion pass writes that guide from its own trace), else the guide pass and then the motion pass.
static int preview_display_guide(pt_preview* p, const pt_camera* cam, uint64_t seed, int gn) {
    const int w = p->w, h = p->h;
    if (p->frameMotion && p->guideCentre && p->guideChain == 0) {
        p->framePasses++;
        return pt_render_motion_device(p->scene, cam, w, h, p->A, p->N[gn], p->M, p->stream);
    }
    if (int r = preview_aovs(p, cam, w, h, seed, p->A, p->N[gn])) return r;
    if (!p->frameMotion) return 0;
    p->framePasses++;
    return pt_render_motion_device(p->scene, cam, w, h, nullptr, nullptr, p->M, p->stream);
}

// A converging frame (the camera rests, a history exists, scale 1): the same five events around select + read-back + moments on
// the live list | the whole feature pass | the accumulation with the live map | filter | resolve.
static int preview_stages_converge(pt_preview* p, const pt_camera* cam, uint64_t seed, int nxt, int gn, bool reuse) {
    const pt_preview_params& P = p->P;
    const int w = p->w, h = p->h, T = ((w + 7) / 8) * ((h + 7) / 8), nt = p->curT ^ 1;
    hipStream_t st = p->stream;
    POSTFX_HIP_OK(hipEventRecord(p->ev[0], st));
    if (int r = pt_temporal_select_device(w, h, p->H[p->cur], p->L[p->cur], &p->C, p->tErr[nt], p->tLive[nt], p->tList, p->tCount, st)) return r;
    int count = -1;
    POSTFX_HIP_OK(hipMemcpyAsync(&count, p->tCount, sizeof(int), hipMemcpyDeviceToHost, st));
    POSTFX_HIP_OK(hipStreamSynchronize(st));
    if (count < 0 || count > T) return postfx_fail(-2, "pt_preview_frame: the live list holds %d of %d tiles", count, T);
    if (count > 0)
        if (int r = pt_render_moments_tiles_device(p->scene, cam, w, h, P.spp, P.spp / P.batches, P.max_depth, P.integrator, P.use_mis, seed, p->tList,
                                                   count, p->S, p->Q, st))
            return r;
    POSTFX_HIP_OK(hipEventRecord(p->ev[1], st));
    if (!reuse)
        if (int r = preview_aovs(p, cam, w, h, seed, p->A, p->N[gn])) return r;
    POSTFX_HIP_OK(hipEventRecord(p->ev[2], st));
    if (int r = pt_temporal_accumulate_live_device(w, h, cam, &p->prevCam, p->S, p->Q, P.spp, P.batches, p->A, p->N[gn], p->N[p->curG], p->H[p->cur],
                                                   p->L[p->cur], p->tLive[nt], &P.temporal_params, p->H[nxt], p->L[nxt], st))
        return r;
    POSTFX_HIP_OK(hipEventRecord(p->ev[3], st));
    pt_denoise_var_params F = P.filter_params;
    if (!P.filter) F.iterations = 0;
    if (int r = pt_denoise_hist_device(w, h, p->H[nxt], p->A, p->N[gn], &F, p->ws, p->filt, st)) return r;
    POSTFX_HIP_OK(hipEventRecord(p->ev[4], st));
    if (int r = pt_resolve_device(w, h, p->filt, 1, nullptr, &P.resolve_params, p->rgba8, p->mean, st)) return r;
    POSTFX_HIP_OK(hipEventRecord(p->ev[5], st));
    p->frameLive = count; p->frameConverged = true;
    return 0;
}

// A frame at render scale s > 1: the same five events around low-res moments | both feature passes | upsample + accumulate |
// filter | resolve. With centre guides the feature stage is the display pass (none when the guide is reused) and its subsample.
static int preview_stages_scaled(pt_preview* p, const pt_camera* cam, uint64_t seed, int nxt, int gn, bool reuse) {
    const pt_preview_params& P = p->P;
    const int w = p->w, h = p->h, s = p->scale, wl = w / s, hl = h / s;
    hipStream_t st = p->stream;
    if (cam->w != w || cam->h != h)       // (before the low-res camera is made: the stages would see a size that need not divide)
        return postfx_fail(-1, "pt_preview_frame: camera is %d x %d, the session %d x %d", cam->w, cam->h, w, h);
    pt_camera lowCam;
    if (int r = pt_camera_scaled(cam, s, &lowCam)) return r;
    const size_t lb = p->loCap * 16;
    char *S = p->lo, *Q = S + lb, *Al = Q + lb, *Nl = Al + lb;
    POSTFX_HIP_OK(hipEventRecord(p->ev[0], st));
    if (int r = pt_render_moments_device(p->scene, &lowCam, wl, hl, P.spp, P.spp / P.batches, P.max_depth, P.integrator, P.use_mis, seed, S, Q, st)) return r;
    POSTFX_HIP_OK(hipEventRecord(p->ev[1], st));
    if (p->guideCentre) {
        if (!reuse)
            if (int r = preview_display_guide(p, cam, seed, gn)) return r;
        // (also when the guide is reused: the scale may have changed since, and the copy is w * h / s^2 pixels)
        if (int r = pt_guide_subsample_device(w, h, s, p->A, p->N[gn], Al, Nl, st)) return r;
    } else {
        if (int r = preview_aovs(p, &lowCam, wl, hl, seed, Al, Nl)) return r;
        if (int r = preview_display_guide(p, cam, seed, gn)) return r;
    }
    POSTFX_HIP_OK(hipEventRecord(p->ev[2], st));
    if (int r = pt_upsample_device(w, h, s, S, Q, P.spp, P.batches, Al, Nl, p->A, p->N[gn], nullptr, p->curEV, st)) return r;
    const void* shown = p->curEV;         // the (e, V) buffer the filter reads
    if (P.temporal) {
        const bool hist = p->haveHist;
        if (p->respond && hist) {         // (the arguments of the form below that the frame would have taken)
            if (int r = pt_temporal_accumulate_respond_device(w, h, cam, &p->prevCam, nullptr, nullptr, 0, 0, nullptr, p->curEV, p->N[gn], p->N[p->curG],
                                                              p->H[p->cur], p->L[p->cur], p->frameMotion ? p->M : nullptr, &P.temporal_params, &p->R,
                                                              p->respondWs, p->H[nxt], p->L[nxt], nullptr, st))
                return r;
        } else if (p->frameMotion) {      // (a motion frame has a history)
            if (int r = pt_temporal_accumulate_cur_motion_device(w, h, cam, &p->prevCam, p->curEV, p->N[gn], p->N[p->curG], p->H[p->cur], p->L[p->cur],
                                                                 p->M, &P.temporal_params, p->H[nxt], p->L[nxt], st))
                return r;
        } else if (int r = pt_temporal_accumulate_cur_device(w, h, cam, hist ? &p->prevCam : nullptr, p->curEV, p->N[gn],
                                                             hist ? p->N[p->curG] : nullptr, hist ? p->H[p->cur] : nullptr,
                                                             hist ? p->L[p->cur] : nullptr, &P.temporal_params, p->H[nxt], p->L[nxt], st))
            return r;
        shown = p->H[nxt];
    }
    POSTFX_HIP_OK(hipEventRecord(p->ev[3], st));
    pt_denoise_var_params F = P.filter_params;
    if (!P.filter) F.iterations = 0;
    if (int r = pt_denoise_hist_device(w, h, shown, p->A, p->N[gn], &F, p->ws, p->filt, st)) return r;
    POSTFX_HIP_OK(hipEventRecord(p->ev[4], st));
    if (int r = pt_resolve_device(w, h, p->filt, 1, nullptr, &P.resolve_params, p->rgba8, p->mean, st)) return r;
    POSTFX_HIP_OK(hipEventRecord(p->ev[5], st));
    return 0;
}

// The five stages of a frame, enqueued on the session's stream with an event after each; the first error ends it. nxt: the half of
// the history pair this frame writes, gn: the half of the guide pair it writes, or, when it reuses the guide (centre guides, resting
// camera), the half it reads as this frame's guide and the previous frame's at once.
static int preview_stages(pt_preview* p, const pt_camera* cam, uint64_t seed, int nxt, int gn, bool reuse) {
    const pt_preview_params& P = p->P;
    const int w = p->w, h = p->h;
    hipStream_t st = p->stream;
    POSTFX_HIP_OK(hipEventRecord(p->ev[0], st));
    // (the first stage checks its arguments, the camera's size among them, before it enqueues anything)
    if (int r = pt_render_moments_device(p->scene, cam, w, h, P.spp, P.spp / P.batches, P.max_depth, P.integrator, P.use_mis, seed, p->S, p->Q, st)) return r;
    POSTFX_HIP_OK(hipEventRecord(p->ev[1], st));
    if (!reuse)
        if (int r = preview_display_guide(p, cam, seed, gn)) return r;
    POSTFX_HIP_OK(hipEventRecord(p->ev[2], st));
    const void* shown = p->S;             // what the resolve divides, and by what
    int shownSpp = P.spp;
    if (P.temporal) {
        const bool hist = p->haveHist;
        if (p->respond && hist) {         // (the arguments of the form below that the frame would have taken)
            if (int r = pt_temporal_accumulate_respond_device(w, h, cam, &p->prevCam, p->S, p->Q, P.spp, P.batches, p->A, nullptr, p->N[gn], p->N[p->curG],
                                                              p->H[p->cur], p->L[p->cur], p->frameMotion ? p->M : nullptr, &P.temporal_params, &p->R,
                                                              p->respondWs, p->H[nxt], p->L[nxt], nullptr, st))
                return r;
        } else if (p->frameMotion) {      // (a motion frame has a history)
            if (int r = pt_temporal_accumulate_motion_device(w, h, cam, &p->prevCam, p->S, p->Q, P.spp, P.batches, p->A, p->N[gn], p->N[p->curG],
                                                             p->H[p->cur], p->L[p->cur], p->M, &P.temporal_params, p->H[nxt], p->L[nxt], st))
                return r;
        } else if (int r = pt_temporal_accumulate_device(w, h, cam, hist ? &p->prevCam : nullptr, p->S, p->Q, P.spp, P.batches, p->A, p->N[gn],
                                                         hist ? p->N[p->curG] : nullptr, hist ? p->H[p->cur] : nullptr,
                                                         hist ? p->L[p->cur] : nullptr, &P.temporal_params, p->H[nxt], p->L[nxt], st))
            return r;
        POSTFX_HIP_OK(hipEventRecord(p->ev[3], st));
        pt_denoise_var_params F = P.filter_params;
        if (!P.filter) F.iterations = 0;  // no iteration: the history's mean a e, pass-through pixels as they are
        if (int r = pt_denoise_hist_device(w, h, p->H[nxt], p->A, p->N[gn], &F, p->ws, p->filt, st)) return r;
        shown = p->filt; shownSpp = 1;
    } else {
        POSTFX_HIP_OK(hipEventRecord(p->ev[3], st));
        if (P.filter) {
            if (int r = pt_denoise_var_device(w, h, p->S, p->Q, P.spp, P.batches, p->A, p->N[gn], &P.filter_params, p->ws, p->filt, st)) return r;
            shown = p->filt;
        }
    }
    POSTFX_HIP_OK(hipEventRecord(p->ev[4], st));
    if (int r = pt_resolve_device(w, h, shown, shownSpp, nullptr, &P.resolve_params, p->rgba8, p->mean, st)) return r;
    POSTFX_HIP_OK(hipEventRecord(p->ev[5], st));
    return 0;
}

int pt_preview_frame(pt_preview* p, const pt_camera* cam, uint64_t seed) {
    if (!p) return postfx_fail(-1, "pt_preview_frame: null session");
    if (!cam) return postfx_fail(-1, "pt_preview_frame: null camera");
    const int nxt = p->P.temporal ? p->cur ^ 1 : 0;
    p->frameLive = ((p->w + 7) / 8) * ((p->h + 7) / 8); p->frameConverged = false;
    // a scene updated behind the session's back: its history and guide are another geometry's, and nobody said to keep them
    const int gen = pt_scene_generation(p->scene);
    if (gen != p->sceneGen && !p->sceneChanged) { p->haveHist = p->haveFrame = p->haveTiles = false; p->sceneChanged = true; }
    // (a changed scene is a moved camera to the converge and guide-reuse decisions; the accumulation still sees the camera's bytes)
    const bool same = p->haveHist && !p->sceneChanged && memcmp(cam, &p->prevCam, sizeof(pt_camera)) == 0;
    // a MOTION FRAME: the one vertex update since the last good frame was announced with its history kept, and the scene still has
    // the positions from before it
    p->frameMotion = p->motion && p->P.temporal && p->haveHist && p->sceneChanged && gen == p->sceneGen + 1 && pt_scene_has_motion(p->scene) == 1;
    const bool rests = p->converge && p->P.temporal && p->scale == 1 && same;
    // centre guides, the camera of the last good frame, and that frame's guide still in place: no feature pass, no guide flip
    const bool reuse = p->guideCentre && same && p->guideFresh;
    const int gn = reuse ? p->curG : (p->P.temporal ? p->curG ^ 1 : 0);
    if (!reuse) p->guideFresh = false;                     // (the feature pass writes A, of which there is one)
    p->framePasses = 0;
    const int r = rests ? preview_stages_converge(p, cam, seed, nxt, gn, reuse)
                        : (p->scale > 1 ? preview_stages_scaled(p, cam, seed, nxt, gn, reuse) : preview_stages(p, cam, seed, nxt, gn, reuse));
    const hipError_t e = hipStreamSynchronize(p->stream);  // also after a failed stage: nothing of this frame is left in flight
    if (r) return r;                                       // (the stage's message stands; cur and the previous camera do too)
    if (e != hipSuccess) return postfx_fail(-2, "pt_preview_frame: the stream failed to synchronise");
    float ms[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, total = 0.0f;
    for (int i = 0; i < 5; i++) POSTFX_HIP_OK(hipEventElapsedTime(&ms[i], p->ev[i], p->ev[i + 1]));
    POSTFX_HIP_OK(hipEventElapsedTime(&total, p->ev[0], p->ev[5]));
    p->cur = nxt;
    p->curG = gn;
    p->guideFresh = true;
    p->guidePasses += p->framePasses;
    p->haveHist = p->P.temporal != 0;
    p->haveFrame = true;
    p->prevCam = *cam;
    p->sceneGen = gen; p->sceneChanged = false;
    p->lastLive = p->frameLive;
    if (p->frameConverged) { p->curT ^= 1; p->haveTiles = true; }
    p->stats.frames++;
    p->stats.render_ms = ms[0]; p->stats.aov_ms = ms[1]; p->stats.accumulate_ms = ms[2]; p->stats.filter_ms = ms[3]; p->stats.resolve_ms = ms[4];
    p->stats.total_ms = total;
    return 0;
}

int pt_preview_read(pt_preview* p, uint8_t* rgba8, float* mean, float* hist, float* hist_len) {
    if (!p) return postfx_fail(-1, "pt_preview_read: null session");
    if (!p->haveFrame) return postfx_fail(-1, "pt_preview_read: no frame since the session was created or reset");
    if ((hist || hist_len) && !p->P.temporal) return postfx_fail(-1, "pt_preview_read: a session with temporal 0 keeps no history");
    const size_t n = (size_t)p->w * p->h;
    if (rgba8) POSTFX_HIP_OK(hipMemcpy(rgba8, p->rgba8, n * 4, hipMemcpyDeviceToHost));
    if (mean) POSTFX_HIP_OK(hipMemcpy(mean, p->mean, n * 16, hipMemcpyDeviceToHost));
    if (hist) POSTFX_HIP_OK(hipMemcpy(hist, p->H[p->cur], n * 16, hipMemcpyDeviceToHost));
    if (hist_len) POSTFX_HIP_OK(hipMemcpy(hist_len, p->L[p->cur], n * 4, hipMemcpyDeviceToHost));
    return 0;
}

const void* pt_preview_device_rgba8(pt_preview* p) { return p ? p->rgba8 : nullptr; }
const void* pt_preview_device_mean(pt_preview* p) { return p ? p->mean : nullptr; }

int pt_preview_last_stats(pt_preview* p, pt_preview_stats* out) {
    if (!p || !out) return postfx_fail(-1, "pt_preview_last_stats: null argument");
    *out = p->stats;
    return 0;
}

}  // extern "C"
