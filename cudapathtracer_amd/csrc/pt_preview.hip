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
//
// pt_preview_frame decides once what kind of frame this is (FramePlan) and preview_stages enqueues it: one sequence, an event after
// each stage. What the options change, stage by stage (SCALED: pt_preview_set_scale > 1; CONVERGING: pt_preview_set_converge, a
// temporal session at scale 1 whose camera rests on a history; MOTION FRAME: pt_preview_set_motion, the frame after one announced
// vertex update that kept its history; a converging frame is neither scaled nor a motion frame):
//   before    scaled: the session's own check of the camera's size, and pt_camera_scaled; nothing is enqueued if either fails.
//             Every other frame gets the camera-size error from its first stage.
//   render    pt_render_moments_device into S and Q. Scaled: the low-res camera and size, into the low-res S and Q. Converging:
//             pt_temporal_select_device on the history, its count read back, pt_render_moments_tiles_device on that list.
//   guides    the display-size feature pass into albedo and the other half of the guide pair: pt_render_aovs_device; with a guide
//             chain pt_render_aovs_chain_device; with centre guides pt_render_aovs_centre_device, and then no pass at all when the
//             camera rests and the last guide is still in place (it has no seed: nothing in it could have changed). A motion frame
//             adds pt_render_motion_device, fused with the guide where that is the centre first-hit pass; with
//             pt_preview_set_motion_chain and a guide chain it is pt_render_motion_chain_device, fused with any centre guide.
//             Scaled: the low-res guide is one more feature pass, before the display pass; with centre guides
//             pt_guide_subsample_device of the display guide, after it, also when that guide is reused.
//   accumulate  temporal 0: nothing. Else one call (preview_accumulate): pt_temporal_accumulate_motion_device on S, Q and albedo;
//             scaled: pt_upsample_device first, then pt_temporal_accumulate_cur_motion_device on its output. Both take the motion
//             buffer on a motion frame and NULL otherwise: the _motion forms with a NULL buffer are the base forms (include/pt_api.h),
//             so the base case has no call of its own. Converging: pt_temporal_accumulate_live_device with the new live map. With
//             respond on (pt_preview_set_respond), a frame with a history that is not converging:
//             pt_temporal_accumulate_respond_device, with the same frame form and motion buffer.
//   filter    pt_denoise_hist_device on the new history, or on the upsampled frame of a scaled frame with temporal 0; filter 0 gives
//             it no iterations. A plain frame with temporal 0: pt_denoise_var_device on S and Q, or with filter 0 nothing.
//   resolve   pt_resolve_device of the filtered frame as a mean, or of S with the frame's spp where nothing filtered. With a selection
//             (pt_preview_set_selection): pt_render_ids_device at display size if the session's ID buffer is stale (ids_stale), then
//             pt_select_overlay_device on the frame's bytes.
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../include/pt_api.h"
#include "pt_postfx_host.h"

namespace pt {

int check_converge_params(const char* fn, const pt_converge_params& P);       // pt_converge.hip
int check_respond_params(const char* fn, const pt_respond_params& R);         // pt_temporal.hip
int check_select_entries(const char* fn, int n, const pt_select_entry* e);    // pt_select.hip

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
    int guidePasses;                      // feature-pass launches of all good frames
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
    int sceneGen;                         // pt_scene_generation at the last good frame (at create before the first)
    bool sceneChanged;                    // pt_preview_scene_changed since the last good frame: the next frame counts as a moved camera
    int motion;                           // 1: MOTION FRAMES reproject moved surfaces (pt_preview_set_motion)
    char* M;                              // w*h float4: pt_render_motion's output (its own allocation, made when motion is first turned on)
    int motionChain;                      // 1: a motion frame of a session with a guide chain runs pt_render_motion_chain_device (MOTION CHAIN)
    bool respond;                         // frames with a history accumulate through pt_temporal_accumulate_respond_device
    pt_respond_params R;
    char* respondWs;                      // its workspace (its own allocation, made when respond is first turned on)
    // selection (pt_preview_set_selection): the entries the overlay draws, and the ID buffer they are drawn from with what it was
    // traced for. The buffer is traced again only when a frame finds it stale: none yet (idsValid false: also after a reset,
    // pt_preview_scene_changed or a frame that failed after tracing it), or another camera, scene generation or max_links.
    int selN;
    pt_select_entry sel[4];
    int selLinks;
    char* ids;                            // w*h int32x4 (its own allocation, made when a selection is first set)
    bool idsValid;
    pt_camera idsCam;
    int idsGen, idsLinks;
    int idPasses;                         // ID-pass launches of all good frames
};

static size_t tile_count(int w, int h) { return (size_t)((w + 7) / 8) * ((h + 7) / 8); }       // 8x8 tiles, as the tile maps count them

// The next frame is a first frame.
static void drop_history(pt_preview* p) { p->haveHist = p->haveFrame = p->haveTiles = false; }

// Whether a frame with camera `cam` at scene generation `gen` has to trace the ID buffer again.
static bool ids_stale(const pt_preview* p, const pt_camera* cam, int gen) {
    return !p->idsValid || gen != p->idsGen || p->selLinks != p->idsLinks || memcmp(cam, &p->idsCam, sizeof(pt_camera)) != 0;
}

// A buffer of its own that the session allocates when an option first needs it, or needs it larger: the one in *slot is freed only
// once the new one exists, so a failure changes nothing (and the caller reports -2). No frame is in flight: pt_preview_frame blocks.
static bool session_alloc(char** slot, size_t bytes) {
    char* fresh = nullptr;
    if (hipMalloc(&fresh, bytes) != hipSuccess) return false;
    if (*slot) (void)hipFree(*slot);
    *slot = fresh;
    return true;
}

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
    if (p->ids) (void)hipFree(p->ids);
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
    else if (tile_count(w, h) * 64 > 0x7fffffffull) bad = postfx_fail(-1, "pt_preview_create: image of %d x %d pixels is too large", w, h);
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
    drop_history(p);
    p->idsValid = false;
    return 0;
}

int pt_preview_scene_changed(pt_preview* p, int keep_history) {
    if (!p) return postfx_fail(-1, "pt_preview_scene_changed: null session");
    if (keep_history != 0 && keep_history != 1) return postfx_fail(-1, "pt_preview_scene_changed: keep_history %d must be 0 or 1", keep_history);
    if (!keep_history) drop_history(p);
    p->sceneChanged = true;
    p->idsValid = false;
    return 0;
}

int pt_preview_set_scale(pt_preview* p, int scale) {
    if (!p) return postfx_fail(-1, "pt_preview_set_scale: null session");
    if (scale < 1 || scale > 8) return postfx_fail(-1, "pt_preview_set_scale: scale %d must be 1..8", scale);
    if (p->w % scale != 0 || p->h % scale != 0)
        return postfx_fail(-1, "pt_preview_set_scale: scale %d must divide the session's size %d x %d", scale, p->w, p->h);
    if (scale > 1) {                      // (curEV stays if lo then fails: it is the size every scale needs)
        const size_t need = (size_t)(p->w / scale) * (p->h / scale);
        if ((!p->curEV && !session_alloc(&p->curEV, (size_t)p->w * p->h * 16)) || (need > p->loCap && !session_alloc(&p->lo, 4 * need * 16)))
            return postfx_fail(-2, "pt_preview_set_scale: could not allocate the buffers of scale %d", scale);
        if (need > p->loCap) p->loCap = need;
    }
    p->scale = scale;
    return 0;
}

int pt_preview_scale(pt_preview* p) { return p ? p->scale : postfx_fail(-1, "pt_preview_scale: null session"); }

int pt_preview_set_guide_chain(pt_preview* p, int max_links) {
    if (!p) return postfx_fail(-1, "pt_preview_set_guide_chain: null session");
    if (max_links < 0 || max_links > 16) return postfx_fail(-1, "pt_preview_set_guide_chain: max_links %d must be 0..16", max_links);
    // guides from before and after a change do not validate against each other: the next frame is a first frame
    if (max_links != p->guideChain) drop_history(p);
    p->guideChain = max_links;
    return 0;
}

int pt_preview_guide_chain(pt_preview* p) { return p ? p->guideChain : postfx_fail(-1, "pt_preview_guide_chain: null session"); }

int pt_preview_set_guide_centre(pt_preview* p, int on) {
    if (on != 0 && on != 1) return postfx_fail(-1, "pt_preview_set_guide_centre: on %d must be 0 or 1", on);
    if (!p) return postfx_fail(-1, "pt_preview_set_guide_centre: null session");
    // jittered and centre guides do not validate against each other: the next frame is a first frame
    if (on != p->guideCentre) drop_history(p);
    p->guideCentre = on;
    return 0;
}

int pt_preview_guide_centre(pt_preview* p) { return p ? p->guideCentre : postfx_fail(-1, "pt_preview_guide_centre: null session"); }

int pt_preview_guide_passes(pt_preview* p) { return p ? p->guidePasses : postfx_fail(-1, "pt_preview_guide_passes: null session"); }

int pt_preview_set_motion(pt_preview* p, int on) {
    if (on != 0 && on != 1) return postfx_fail(-1, "pt_preview_set_motion: on %d must be 0 or 1", on);
    if (!p) return postfx_fail(-1, "pt_preview_set_motion: null session");
    if (on && !p->M && !session_alloc(&p->M, (size_t)p->w * p->h * 16))
        return postfx_fail(-2, "pt_preview_set_motion: could not allocate the motion buffer");
    p->motion = on;                       // (no reset: the guides do not depend on it)
    return 0;
}

int pt_preview_motion(pt_preview* p) { return p ? p->motion : postfx_fail(-1, "pt_preview_motion: null session"); }

int pt_preview_set_motion_chain(pt_preview* p, int on) {
    if (on != 0 && on != 1) return postfx_fail(-1, "pt_preview_set_motion_chain: on %d must be 0 or 1", on);
    if (!p) return postfx_fail(-1, "pt_preview_set_motion_chain: null session");
    p->motionChain = on;                  // (no reset, no buffer: M is pt_preview_set_motion's, without which there is no motion frame)
    return 0;
}

int pt_preview_motion_chain(pt_preview* p) { return p ? p->motionChain : postfx_fail(-1, "pt_preview_motion_chain: null session"); }

int pt_preview_set_respond(pt_preview* p, const pt_respond_params* params) {
    if (!p) return postfx_fail(-1, "pt_preview_set_respond: null session");
    if (!params) { p->respond = false; return 0; }
    if (int r = check_respond_params("pt_preview_set_respond", *params)) return r;
    if (!p->respondWs && !session_alloc(&p->respondWs, pt_temporal_respond_workspace_bytes(p->w, p->h)))
        return postfx_fail(-2, "pt_preview_set_respond: could not allocate the workspace");
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
    if (!p->tiles) {
        const size_t tb = (tile_count(p->w, p->h) * 4 + 15) & ~(size_t)15;
        if (!session_alloc(&p->tiles, 5 * tb + 16)) return postfx_fail(-2, "pt_preview_set_converge: could not allocate the tile buffers");
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
    if (total) *total = (int)tile_count(p->w, p->h);
    return 0;
}

int pt_preview_read_tiles(pt_preview* p, float* tile_err, int32_t* tile_live) {
    if (!p) return postfx_fail(-1, "pt_preview_read_tiles: null session");
    if (!p->haveTiles) return postfx_fail(-1, "pt_preview_read_tiles: no converging frame since the session was created or reset");
    const size_t tb = tile_count(p->w, p->h) * 4;
    if (tile_err) POSTFX_HIP_OK(hipMemcpy(tile_err, p->tErr[p->curT], tb, hipMemcpyDeviceToHost));
    if (tile_live) POSTFX_HIP_OK(hipMemcpy(tile_live, p->tLive[p->curT], tb, hipMemcpyDeviceToHost));
    return 0;
}

// What pt_preview_frame decides about a frame before it enqueues anything, and what the frame's stages find. It travels with the
// frame; the session takes it over only when the frame has succeeded (pt_preview_frame's commit).
struct FramePlan {
    int gen;                              // pt_scene_generation at this frame
    bool same;                            // a history, no change of the scene, and the camera of the last good frame byte for byte
    bool motion;                          // a MOTION FRAME: M is rendered and accumulated through
    bool converging;                      // a resting frame of a converging session: only the tiles its history has not settled
    bool reuse;                           // centre guides, `same`, and the last good frame's guide still in place: no feature pass
    int nxt;                              // the half of the history pair the frame writes
    int gn;                               // the half of the guide pair it writes; when it reuses the guide, the half it reads as this
                                          // frame's guide and the previous frame's at once
    int live;                             // found: the tiles the frame rendered (all of them unless it converges)
    int passes;                           // found: its feature-pass launches
    bool idsTrace;                        // a selection is set and the ID buffer is stale: the frame traces it before the overlay
};

// A feature pass of a frame: the first-hit pass, or the chain pass when the session has a guide chain; with centre guides the
// centre pass of either kind, which has no aov_spp and no seed.
static int preview_aovs(pt_preview* p, FramePlan& f, const pt_camera* cam, int w, int h, uint64_t seed, void* dA, void* dN) {
    f.passes++;
    if (p->guideCentre) return pt_render_aovs_centre_device(p->scene, cam, w, h, p->guideChain, dA, dN, nullptr, p->stream);
    if (p->guideChain > 0) return pt_render_aovs_chain_device(p->scene, cam, w, h, p->P.aov_spp, p->guideChain, seed, dA, dN, nullptr, p->stream);
    return pt_render_aovs_device(p->scene, cam, w, h, p->P.aov_spp, seed, dA, dN, p->stream);
}

// The motion pass of a motion frame, with the display guide outputs (dA, dN) or without (NULL, NULL): pt_render_motion_device, or
// with the motion-chain switch on and a guide chain pt_render_motion_chain_device along that chain.
static int preview_motion(pt_preview* p, FramePlan& f, const pt_camera* cam, void* dA, void* dN) {
    f.passes++;
    if (p->motionChain && p->guideChain > 0)
        return pt_render_motion_chain_device(p->scene, cam, p->w, p->h, p->guideChain, dA, dN, nullptr, p->M, p->stream);
    return pt_render_motion_device(p->scene, cam, p->w, p->h, dA, dN, p->M, p->stream);
}

// The display-size guide of a frame that traces one and, on a motion frame, the motion buffer: one fused pass where a motion pass
// writes the session's guide from its own trace (centre guides: the first-hit guide from pt_render_motion_device, a chain guide from
// pt_render_motion_chain_device), else the guide pass and then the motion pass.
static int preview_display_guide(pt_preview* p, FramePlan& f, const pt_camera* cam, uint64_t seed) {
    if (f.motion && p->guideCentre && (p->guideChain == 0 || p->motionChain)) return preview_motion(p, f, cam, p->A, p->N[f.gn]);
    if (int r = preview_aovs(p, f, cam, p->w, p->h, seed, p->A, p->N[f.gn])) return r;
    return f.motion ? preview_motion(p, f, cam, nullptr, nullptr) : 0;
}

// The one accumulate call of a temporal frame, into H[nxt] and L[nxt]. cur: the upsampled (e, V) frame of a scaled frame, NULL for
// the sums S and Q with albedo A. live: the live map of a converging frame, else NULL. A first frame has no previous camera, guide,
// history or length; a motion frame has all four and hands M on.
static int preview_accumulate(pt_preview* p, const FramePlan& f, const pt_camera* cam, const void* cur, const void* live) {
    const pt_preview_params& P = p->P;
    const int w = p->w, h = p->h;
    const bool hist = p->haveHist;
    const pt_camera* prevCam = hist ? &p->prevCam : nullptr;
    const void *prevN = hist ? p->N[p->curG] : nullptr, *H = hist ? p->H[p->cur] : nullptr, *L = hist ? p->L[p->cur] : nullptr;
    const void *N = p->N[f.gn], *M = f.motion ? p->M : nullptr;
    void *outH = p->H[f.nxt], *outL = p->L[f.nxt];
    if (live)
        return pt_temporal_accumulate_live_device(w, h, cam, prevCam, p->S, p->Q, P.spp, P.batches, p->A, N, prevN, H, L, live, &P.temporal_params,
                                                  outH, outL, p->stream);
    if (p->respond && hist) {             // (either frame form: the sums' arguments are absent beside cur)
        const void *S = cur ? nullptr : p->S, *Q = cur ? nullptr : p->Q, *A = cur ? nullptr : p->A;
        return pt_temporal_accumulate_respond_device(w, h, cam, prevCam, S, Q, cur ? 0 : P.spp, cur ? 0 : P.batches, A, cur, N, prevN, H, L, M,
                                                     &P.temporal_params, &p->R, p->respondWs, outH, outL, nullptr, p->stream);
    }
    // (M NULL: the base forms pt_temporal_accumulate_cur_device and pt_temporal_accumulate_device)
    if (cur) return pt_temporal_accumulate_cur_motion_device(w, h, cam, prevCam, cur, N, prevN, H, L, M, &P.temporal_params, outH, outL, p->stream);
    return pt_temporal_accumulate_motion_device(w, h, cam, prevCam, p->S, p->Q, P.spp, P.batches, p->A, N, prevN, H, L, M, &P.temporal_params, outH,
                                                outL, p->stream);
}

// The five stages of a frame, enqueued on the session's stream with an event after each; the first error ends it. The file's head
// lists what each kind of frame runs in each stage.
static int preview_stages(pt_preview* p, const pt_camera* cam, uint64_t seed, FramePlan& f) {
    const pt_preview_params& P = p->P;
    const int w = p->w, h = p->h, s = p->scale, gn = f.gn;
    const bool scaled = s > 1;
    hipStream_t st = p->stream;
    // what the render writes and at which size: a scaled frame's are the low-res camera and buffers
    const pt_camera* renderCam = cam;
    pt_camera lowCam;
    char *S = p->S, *Q = p->Q, *Al = nullptr, *Nl = nullptr;
    if (scaled) {
        if (cam->w != w || cam->h != h)   // (before the low-res camera is made: the stages would see a size that need not divide)
            return postfx_fail(-1, "pt_preview_frame: camera is %d x %d, the session %d x %d", cam->w, cam->h, w, h);
        if (int r = pt_camera_scaled(cam, s, &lowCam)) return r;
        const size_t lb = p->loCap * 16;
        renderCam = &lowCam;
        S = p->lo; Q = S + lb; Al = Q + lb; Nl = Al + lb;
    }

    POSTFX_HIP_OK(hipEventRecord(p->ev[0], st));
    const int nt = p->curT ^ 1;           // the half of the tile buffers a converging frame writes
    if (f.converging) {
        const int T = (int)tile_count(w, h);
        if (int r = pt_temporal_select_device(w, h, p->H[p->cur], p->L[p->cur], &p->C, p->tErr[nt], p->tLive[nt], p->tList, p->tCount, st)) return r;
        int count = -1;
        POSTFX_HIP_OK(hipMemcpyAsync(&count, p->tCount, sizeof(int), hipMemcpyDeviceToHost, st));
        POSTFX_HIP_OK(hipStreamSynchronize(st));
        if (count < 0 || count > T) return postfx_fail(-2, "pt_preview_frame: the live list holds %d of %d tiles", count, T);
        if (count > 0)
            if (int r = pt_render_moments_tiles_device(p->scene, cam, w, h, P.spp, P.spp / P.batches, P.max_depth, P.integrator, P.use_mis, seed, p->tList,
                                                       count, S, Q, st))
                return r;
        f.live = count;
    } else {
        // (the first stage checks its arguments, the camera's size among them, before it enqueues anything)
        if (int r = pt_render_moments_device(p->scene, renderCam, w / s, h / s, P.spp, P.spp / P.batches, P.max_depth, P.integrator, P.use_mis, seed, S, Q,
                                             st))
            return r;
    }

    POSTFX_HIP_OK(hipEventRecord(p->ev[1], st));
    if (scaled && !p->guideCentre)
        if (int r = preview_aovs(p, f, &lowCam, w / s, h / s, seed, Al, Nl)) return r;
    if (!f.reuse)
        if (int r = preview_display_guide(p, f, cam, seed)) return r;
    if (scaled && p->guideCentre)         // (also when the guide is reused: the scale may have changed since, and the copy is w * h / s^2 pixels)
        if (int r = pt_guide_subsample_device(w, h, s, p->A, p->N[gn], Al, Nl, st)) return r;

    POSTFX_HIP_OK(hipEventRecord(p->ev[2], st));
    if (scaled)
        if (int r = pt_upsample_device(w, h, s, S, Q, P.spp, P.batches, Al, Nl, p->A, p->N[gn], nullptr, p->curEV, st)) return r;
    if (P.temporal)
        if (int r = preview_accumulate(p, f, cam, scaled ? p->curEV : nullptr, f.converging ? p->tLive[nt] : nullptr)) return r;

    POSTFX_HIP_OK(hipEventRecord(p->ev[3], st));
    const void* eV = P.temporal ? p->H[f.nxt] : (scaled ? p->curEV : nullptr);     // the (e, V) buffer the history filter reads, if any
    const void* shown = p->filt;          // what the resolve divides, and by what
    int shownSpp = 1;
    if (eV) {
        pt_denoise_var_params F = P.filter_params;
        if (!P.filter) F.iterations = 0;  // no iteration: the history's mean a e, pass-through pixels as they are
        if (int r = pt_denoise_hist_device(w, h, eV, p->A, p->N[gn], &F, p->ws, p->filt, st)) return r;
    } else {
        shownSpp = P.spp;
        if (!P.filter) shown = S;
        else if (int r = pt_denoise_var_device(w, h, S, Q, P.spp, P.batches, p->A, p->N[gn], &P.filter_params, p->ws, p->filt, st)) return r;
    }

    POSTFX_HIP_OK(hipEventRecord(p->ev[4], st));
    if (int r = pt_resolve_device(w, h, shown, shownSpp, nullptr, &P.resolve_params, p->rgba8, p->mean, st)) return r;
    if (p->selN > 0) {
        if (f.idsTrace)
            if (int r = pt_render_ids_device(p->scene, cam, w, h, p->selLinks, p->ids, st)) return r;
        if (int r = pt_select_overlay_device(w, h, p->ids, p->selN, p->sel, p->rgba8, st)) return r;
    }
    POSTFX_HIP_OK(hipEventRecord(p->ev[5], st));
    return 0;
}

int pt_preview_frame(pt_preview* p, const pt_camera* cam, uint64_t seed) {
    if (!p) return postfx_fail(-1, "pt_preview_frame: null session");
    if (!cam) return postfx_fail(-1, "pt_preview_frame: null camera");
    FramePlan f = {};
    f.nxt = p->P.temporal ? p->cur ^ 1 : 0;
    f.live = (int)tile_count(p->w, p->h);
    // a scene updated behind the session's back: its history and guide are another geometry's, and nobody said to keep them. (What
    // pt_preview_scene_changed(p, 0) would have done: it holds whether or not this frame succeeds, so it is no part of the plan.)
    f.gen = pt_scene_generation(p->scene);
    if (f.gen != p->sceneGen && !p->sceneChanged) { drop_history(p); p->sceneChanged = true; }
    // (a changed scene is a moved camera to the converge and guide-reuse decisions; the accumulation still sees the camera's bytes)
    f.same = p->haveHist && !p->sceneChanged && memcmp(cam, &p->prevCam, sizeof(pt_camera)) == 0;
    // a MOTION FRAME: the one vertex update since the last good frame was announced with its history kept, and the scene still has
    // the positions from before it
    f.motion = p->motion && p->P.temporal && p->haveHist && p->sceneChanged && f.gen == p->sceneGen + 1 && pt_scene_has_motion(p->scene) == 1;
    f.converging = p->converge && p->P.temporal && p->scale == 1 && f.same;
    // centre guides, the camera of the last good frame, and that frame's guide still in place: no feature pass, no guide flip
    f.reuse = p->guideCentre && f.same && p->guideFresh;
    f.gn = f.reuse ? p->curG : (p->P.temporal ? p->curG ^ 1 : 0);
    // the feature pass writes A, of which there is one: the one thing a frame that then fails has done to the session
    if (!f.reuse) p->guideFresh = false;
    f.idsTrace = p->selN > 0 && ids_stale(p, cam, f.gen);
    if (f.idsTrace) p->idsValid = false;   // (as the guide: a frame that fails after tracing it leaves no buffer to trust)
    const int r = preview_stages(p, cam, seed, f);
    const hipError_t e = hipStreamSynchronize(p->stream);  // also after a failed stage: nothing of this frame is left in flight
    if (r) return r;                                       // (the stage's message stands; cur and the previous camera do too)
    if (e != hipSuccess) return postfx_fail(-2, "pt_preview_frame: the stream failed to synchronise");
    float ms[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, total = 0.0f;
    for (int i = 0; i < 5; i++) POSTFX_HIP_OK(hipEventElapsedTime(&ms[i], p->ev[i], p->ev[i + 1]));
    POSTFX_HIP_OK(hipEventElapsedTime(&total, p->ev[0], p->ev[5]));
    // the commit: from here on the frame is the session's last good frame
    p->cur = f.nxt;
    p->curG = f.gn;
    p->guideFresh = true;
    p->guidePasses += f.passes;
    if (f.idsTrace) { p->idsValid = true; p->idsCam = *cam; p->idsGen = f.gen; p->idsLinks = p->selLinks; p->idPasses++; }
    p->haveHist = p->P.temporal != 0;
    p->haveFrame = true;
    p->prevCam = *cam;
    p->sceneGen = f.gen; p->sceneChanged = false;
    p->lastLive = f.live;
    if (f.converging) { p->curT ^= 1; p->haveTiles = true; }
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

int pt_preview_set_selection(pt_preview* p, int n, const pt_select_entry* e, int max_links) {
    const char* fn = "pt_preview_set_selection";
    if (!p) return postfx_fail_fn(-1, fn, "null session");
    if (max_links < 0 || max_links > 16) return postfx_fail_fn(-1, fn, "max_links %d must be 0..16", max_links);
    if (int r = check_select_entries(fn, n, e)) return r;
    if (n > 0 && !p->ids && !session_alloc(&p->ids, (size_t)p->w * p->h * 16)) return postfx_fail_fn(-2, fn, "could not allocate the ID buffer");
    p->selN = n;                          // (no reset: nothing but the frame's bytes depends on it)
    for (int i = 0; i < n; i++) p->sel[i] = e[i];
    if (n > 0) p->selLinks = max_links;
    return 0;
}

int pt_preview_pick(pt_preview* p, int x, int y, int max_links, int32_t out_ids[4], float out_hit[4]) {
    if (!p) return postfx_fail(-1, "pt_preview_pick: null session");
    if (!p->haveFrame) return postfx_fail(-1, "pt_preview_pick: no frame since the session was created or reset");
    const int32_t xy[2] = {x, y};
    return pt_pick(p->scene, &p->prevCam, p->w, p->h, 1, xy, max_links, out_ids, out_hit);     // (the last good frame's camera, at display size)
}

int pt_preview_read_ids(pt_preview* p, int32_t* out) {
    if (!p) return postfx_fail(-1, "pt_preview_read_ids: null session");
    if (!out) return postfx_fail(-1, "pt_preview_read_ids: null output");
    if (!p->ids || !p->idsValid) return postfx_fail(-1, "pt_preview_read_ids: no frame with a selection since the ID buffer was last dropped");
    POSTFX_HIP_OK(hipMemcpy(out, p->ids, (size_t)p->w * p->h * 16, hipMemcpyDeviceToHost));
    return 0;
}

const void* pt_preview_device_ids(pt_preview* p) { return p ? p->ids : nullptr; }

int pt_preview_id_passes(pt_preview* p) { return p ? p->idPasses : postfx_fail(-1, "pt_preview_id_passes: null session"); }

int pt_preview_last_stats(pt_preview* p, pt_preview_stats* out) {
    if (!p || !out) return postfx_fail(-1, "pt_preview_last_stats: null argument");
    *out = p->stats;
    return 0;
}

}  // extern "C"
