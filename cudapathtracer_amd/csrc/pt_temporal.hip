// pt_temporal.hip — temporal accumulation with reprojection (the history stage of SVGF: Schied et al., HPG 2017) on the
// albedo-demodulated mean and its variance, in pt_denoise_var's working format. include/pt_api.h states the arithmetic;
// tests/temporal_ref.py restates it in numpy. Opt-in post-process on buffers: stateless, no workspace, no render path involved.
//
//   temporal_kernel<Source, IDENT, MOTION, LIVE>   the one kernel of all ten entry points: one thread per pixel, 16x16 pixels per
//                 workgroup as four 8x8 tiles (one per wave, the tiling of dn_atrous_kernel: a wave's four gathers fall
//                 into a few lines). The pixel's working value (e, V), then temporal_blend: its world point from its depth along
//                 the unjittered centre ray, projected into the previous camera; up to four bilinear taps of the previous history,
//                 each checked against the previous guide; the blend.
//       Source    FromSums: (e, V) from S and Q (dn_var_pixel, shared with dn_prepare_kernel's VarSource). FromCur: read from a
//                 buffer (pt_upsample's output). Each says which pixels pass through and what they write.
//       IDENT     both cameras are the same bytes: the tap is the pixel itself and no projection is computed.
//       MOTION    a motion buffer (pt_render_motion): a pixel whose motion.w is 1 reprojects the point the buffer names — where its
//                 surface point WAS — and never takes the identity tap; every other pixel runs the base code. One more float4 load.
//       LIVE      a map of live 8x8 tiles (pt_temporal_accumulate_live: a resting viewer whose converged tiles were not rendered).
//                 A wave is one tile, so the map entry is one scalar load and the branch does not diverge: a carried wave copies
//                 its history and length (two loads, two stores), a live wave runs on. FromSums, IDENT and no MOTION only.
//   Nine instantiations exist (temporal_launch's table). Everything travels by value in one TemporalArgs (SGPRs), the two
//   cameras included; plain cached float4 loads, no LDS.
// Host side: every entry point fills a TemporalCall; temporal_run checks it (check_temporal_call), and launches it (temporal_launch)
// on the caller's buffers or, for a host form, on staged copies (postfx_host_form).
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../include/pt_api.h"
#include "pt_denoise_shared.h"
#include "pt_postfx_host.h"

namespace pt {

struct TemporalCam {                      // what the projection reads of a pt_camera
    float ox, oy, oz, fovScale;
    float fx, fy, fz, aspect;             // aspect = (float)w / (float)h, as camera_ray computes it
    float rx, ry, rz, pad0;
    float ux, uy, uz, pad1;
};

static TemporalCam temporal_cam(const pt_camera& c) {
    TemporalCam t;
    t.ox = c.cameraOrigin.x; t.oy = c.cameraOrigin.y; t.oz = c.cameraOrigin.z; t.fovScale = c.fovScale;
    t.fx = c.forward.x; t.fy = c.forward.y; t.fz = c.forward.z; t.aspect = (float)c.w / (float)c.h;
    t.rx = c.right.x; t.ry = c.right.y; t.rz = c.right.z; t.pad0 = 0.0f;
    t.ux = c.up.x; t.uy = c.up.y; t.uz = c.up.z; t.pad1 = 0.0f;
    return t;
}

struct TemporalTap {
    float se_x, se_y, se_z, sv, sn, sw;   // sums over the valid taps of w e, w V, w N and w
};

// One tap of the previous history at (xq, yq) with bilinear weight wt: valid inside the image, not pass-through, at the
// expected depth and with a matching unit normal. An invalid tap is skipped, never multiplied by 0 (its values may be NaN).
__device__ inline void temporal_tap(TemporalTap& t, int w, int h, int xq, int yq, float wt, float4 gp, float zExp, float depthTol, float normalTol,
                                    const float4* __restrict__ prevNd, const float4* __restrict__ hist, const float* __restrict__ histLen) {
    if (xq < 0 || xq >= w || yq < 0 || yq >= h) return;
    const size_t q = (size_t)yq * w + xq;
    const float4 hq = hist[q];
    if (!(hq.w >= 0.0f)) return;
    const float4 gq = dn_unit_guide(prevNd[q]);
    if (!(fabsf(gq.w - zExp) <= depthTol * zExp)) return;
    if (gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f) return;
    if (!(gp.x * gq.x + gp.y * gq.y + gp.z * gq.z >= normalTol)) return;
    t.se_x += wt * hq.x; t.se_y += wt * hq.y; t.se_z += wt * hq.z;
    t.sv += wt * hq.w;
    t.sn += wt * histLen[q];
    t.sw += wt;
}

// Steps 2-5 of the contract for a pixel whose working value `cur` (e, V >= 0) is known: reproject, gather, blend, write.
// MOTION: `motion` is set, and a pixel with motion.w == 1 takes its xyz as the point to reproject (no identity tap for it).
template <bool IDENT, bool MOTION = false>
__device__ inline void temporal_blend(int w, int h, int x, int y, float4 cur, const TemporalCam& cam, const TemporalCam& prev,
                                      const float4* __restrict__ nd, const float4* __restrict__ prevNd, const float4* __restrict__ hist,
                                      const float* __restrict__ histLen, float maxHistory, float depthTol, float normalTol,
                                      float4* __restrict__ outHist, float* __restrict__ outLen, const float4* __restrict__ motion = nullptr) {
    const size_t p = (size_t)y * w + x;
    float4 res = cur;
    float len = 1.0f;
    if (hist != nullptr) {                                    // (uniform: a kernel argument)
        const float4 gp = dn_unit_guide(nd[p]);
        const bool normalP = gp.x != 0.0f || gp.y != 0.0f || gp.z != 0.0f;
        TemporalTap t = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (MOTION) mv = motion[p];                           // (read only with a history)
        const bool moved = MOTION && mv.w == 1.0f;
        if (IDENT && !moved) {
            if (normalP) temporal_tap(t, w, h, x, y, 1.0f, gp, gp.w, depthTol, normalTol, prevNd, hist, histLen);
        } else if (normalP) {
            // the unjittered centre ray of the pixel (camera_ray with both jitters 0 and no lens sample), to the depth z_p
            float px, py, pz;
            if (moved) {                                      // where this surface point was when the previous frame was made
                px = mv.x; py = mv.y; pz = mv.z;
            } else {
                const float u = (2.0f * ((float)x / (float)w) - 1.0f) * cam.aspect * cam.fovScale;
                const float v = (2.0f * ((float)y / (float)h) - 1.0f) * cam.fovScale;
                const float tx = cam.rx * u + cam.ux * v + cam.fx, ty = cam.ry * u + cam.uy * v + cam.fy, tz = cam.rz * u + cam.uz * v + cam.fz;
                const float tl = sqrtf(tx * tx + ty * ty + tz * tz);
                px = cam.ox + tx / tl * gp.w; py = cam.oy + ty / tl * gp.w; pz = cam.oz + tz / tl * gp.w;
            }
            // ... seen from the previous camera
            const float qx = px - prev.ox, qy = py - prev.oy, qz = pz - prev.oz;
            const float zc = qx * prev.fx + qy * prev.fy + qz * prev.fz;
            if (zc > 0.0f) {
                const float fs = prev.aspect * prev.fovScale;
                const float xp = (((qx * prev.rx + qy * prev.ry + qz * prev.rz) / zc) / fs + 1.0f) * (float)w / 2.0f;
                const float yp = (((qx * prev.ux + qy * prev.uy + qz * prev.uz) / zc) / prev.fovScale + 1.0f) * (float)h / 2.0f;
                const float zExp = sqrtf(qx * qx + qy * qy + qz * qz);
                // outside [-1, w) x [-1, h) (or NaN) no tap is inside the image; inside, the conversions to int are safe
                if (xp >= -1.0f && xp < (float)w && yp >= -1.0f && yp < (float)h) {
                    const float x0 = floorf(xp), y0 = floorf(yp);
                    const float ax = xp - x0, ay = yp - y0;
                    const int xi = (int)x0, yi = (int)y0;
                    temporal_tap(t, w, h, xi, yi, (1.0f - ax) * (1.0f - ay), gp, zExp, depthTol, normalTol, prevNd, hist, histLen);
                    temporal_tap(t, w, h, xi + 1, yi, ax * (1.0f - ay), gp, zExp, depthTol, normalTol, prevNd, hist, histLen);
                    temporal_tap(t, w, h, xi, yi + 1, (1.0f - ax) * ay, gp, zExp, depthTol, normalTol, prevNd, hist, histLen);
                    temporal_tap(t, w, h, xi + 1, yi + 1, ax * ay, gp, zExp, depthTol, normalTol, prevNd, hist, histLen);
                }
            }
        }
        if (t.sw >= 0.01f) {
            const float ehx = t.se_x / t.sw, ehy = t.se_y / t.sw, ehz = t.se_z / t.sw, vh = t.sv / t.sw, nh = t.sn / t.sw;
            const float n1 = nh + 1.0f;
            len = n1 < maxHistory ? n1 : maxHistory;
            const float alpha = 1.0f / len, keep = 1.0f - alpha;
            res = make_float4(ehx + alpha * (cur.x - ehx), ehy + alpha * (cur.y - ehy), ehz + alpha * (cur.z - ehz),
                              (keep * keep) * vh + (alpha * alpha) * cur.w);
        }
    }
    outHist[p] = res;
    outLen[p] = len;
}

// Everything a launch hands the kernel. A pointer the instantiation does not use is NULL and never read.
struct TemporalArgs {
    int w, h;
    TemporalCam cam, prev;
    const float4 *sum, *sq, *albedo;          // FromSums
    float spp, batches;
    const float4* cur;                        // FromCur
    const float4 *nd, *prevNd, *hist;
    const float* histLen;
    const float4* motion;                     // MOTION
    const int32_t* tileLive;                  // LIVE
    int tilesX;
    float maxHistory, depthTol, normalTol;
    float4* outHist;
    float* outLen;
};

// The two sources of a pixel's working value: load() returns whether the pixel passes through, and then `raw` is what it writes.
struct FromSums {
    static __device__ inline bool load(const TemporalArgs& a, size_t p, float4& cur, float4& raw) {
        cur = dn_var_pixel(a.sum[p], a.sq[p], a.albedo[p], a.spp, a.batches, raw);
        return cur.w < 0.0f;
    }
};
struct FromCur {                              // (pt_upsample wrote it; a NaN variance passes through as well)
    static __device__ inline bool load(const TemporalArgs& a, size_t p, float4& cur, float4& raw) {
        cur = raw = a.cur[p];
        return !(cur.w >= 0.0f);
    }
};

template <class Source, bool IDENT, bool MOTION, bool LIVE>
__global__ void __launch_bounds__(256) temporal_kernel(TemporalArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = blockIdx.x * 2 + (wave & 1), ty = blockIdx.y * 2 + (wave >> 1);
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    if (x >= a.w || y >= a.h) return;                         // (a tile outside the grid has no lane left: no read past the map)
    const size_t p = (size_t)y * a.w + x;
    // tileLive[tile] == 0: the tile was not rendered this frame and keeps its history and length bit for bit (S, Q and albedo are
    // not read there)
    if (LIVE && a.tileLive[__builtin_amdgcn_readfirstlane(ty * a.tilesX + tx)] == 0) {
        a.outHist[p] = a.hist[p];
        a.outLen[p] = a.histLen[p];
        return;
    }
    float4 cur, raw;
    if (Source::load(a, p, cur, raw)) { a.outHist[p] = make_float4(raw.x, raw.y, raw.z, -1.0f); a.outLen[p] = 0.0f; return; }
    temporal_blend<IDENT, MOTION>(a.w, a.h, x, y, cur, a.cam, a.prev, a.nd, a.prevNd, a.hist, a.histLen, a.maxHistory, a.depthTol, a.normalTol,
                                  a.outHist, a.outLen, a.motion);
}

// One call of any of the ten entry points, on host or on device buffers.
struct TemporalCall {
    const char* fn;                           // the entry point, for the messages of its host form
    int w, h;
    const pt_camera *cam, *prev;
    bool fromCur;                             // the frame is `cur`; otherwise sum, sq, spp, batches and albedo
    const void *sum, *sq, *albedo, *cur;
    int spp, batches;
    const void *nd, *prevNd, *hist, *histLen;
    const void* tileLive;                     // pt_temporal_accumulate_live only
    const void* motion;                       // pt_temporal_accumulate_motion and _cur_motion only
    pt_temporal_params P;
    void *outHist, *outLen;
};

static TemporalCall temporal_call(const char* fn, int w, int h, const pt_camera* cam, const pt_camera* prev, const void* nd, const void* prevNd,
                                  const void* hist, const void* histLen, const pt_temporal_params* params, void* outHist, void* outLen) {
    TemporalCall c = {};
    c.fn = fn; c.w = w; c.h = h; c.cam = cam; c.prev = prev;
    c.nd = nd; c.prevNd = prevNd; c.hist = hist; c.histLen = histLen; c.outHist = outHist; c.outLen = outLen;
    if (params) c.P = *params; else pt_temporal_defaults(&c.P);
    return c;
}
static TemporalCall& from_sums(TemporalCall& c, const void* sum, const void* sq, int spp, int batches, const void* albedo) {
    c.sum = sum; c.sq = sq; c.spp = spp; c.batches = batches; c.albedo = albedo;
    return c;
}
static TemporalCall& from_cur(TemporalCall& c, const void* cur) {
    c.fromCur = true; c.cur = cur;
    return c;
}

static bool temporal_ident(const TemporalCall& c) { return !c.prev || memcmp(c.cam, c.prev, sizeof(pt_camera)) == 0; }

// All of a call's checks, before the first HIP call. The messages carry the name of the entry point that introduced the check.
static int check_temporal_call(const TemporalCall& c) {
    const char* fn = c.fromCur ? "pt_temporal_accumulate_cur" : "pt_temporal_accumulate";
    const int w = c.w, h = c.h;
    if (int r = postfx_check_size(fn, w, h)) return r;
    if (!c.fromCur) {
        if (c.spp <= 0) return postfx_fail_fn(-1, fn, "spp %d must be positive", c.spp);
        if (c.batches < 2) return postfx_fail_fn(-1, fn, "batches %d must be at least 2", c.batches);
        if (c.spp % c.batches != 0) return postfx_fail_fn(-1, fn, "batches %d must divide spp %d", c.batches, c.spp);
    }
    // the cameras, the buffers and the history
    if (!c.cam) return postfx_fail_fn(-1, fn, "null camera");
    if (c.cam->w != w || c.cam->h != h) return postfx_fail_fn(-1, fn, "camera is %d x %d, the frame %d x %d", c.cam->w, c.cam->h, w, h);
    if (c.prev && (c.prev->w != w || c.prev->h != h))
        return postfx_fail_fn(-1, fn, "previous camera is %d x %d, the frame %d x %d", c.prev->w, c.prev->h, w, h);
    if (!(c.fromCur ? c.cur && c.nd : c.sum && c.sq && c.albedo && c.nd)) return postfx_fail_fn(-1, fn, "null buffer");
    if (!c.outHist || !c.outLen) return postfx_fail_fn(-1, fn, "null output");
    const int given = (c.prevNd != nullptr) + (c.hist != nullptr) + (c.histLen != nullptr);
    if (given != 0 && given != 3) return postfx_fail_fn(-1, fn, "prev_normal_depth, hist and hist_len must be all NULL (first frame) or all set");
    const size_t n = (size_t)w * h;
    if (given == 3 && (overlaps(c.outHist, n * 16, c.hist, n * 16) || overlaps(c.outLen, n * 4, c.histLen, n * 4) ||
                       overlaps(c.outHist, n * 16, c.histLen, n * 4) || overlaps(c.outLen, n * 4, c.hist, n * 16)))
        return postfx_fail_fn(-1, fn, "the output history must not alias the input history (ping-pong two pairs)");
    if (c.P.max_history < 1) return postfx_fail_fn(-1, fn, "max_history %d must be at least 1", c.P.max_history);
    if (!(c.P.depth_tol > 0.0f) || !std::isfinite(c.P.depth_tol)) return postfx_fail_fn(-1, fn, "depth_tol must be positive and finite");
    if (!(c.P.normal_tol > 0.0f) || !(c.P.normal_tol <= 1.0f)) return postfx_fail_fn(-1, fn, "normal_tol must be in (0, 1]");
    // what a tile map adds: the identity path and a history, and outputs that leave the map alone
    if (c.tileLive) {
        fn = "pt_temporal_accumulate_live";
        if (!c.hist) return postfx_fail_fn(-1, fn, "a tile map needs a history: a carried pixel keeps what it had");
        if (!temporal_ident(c))
            return postfx_fail_fn(-1, fn, "a tile map needs an unchanged camera (cam_prev NULL or equal to cam): a carried pixel keeps what it had at the same place");
        const size_t tb = (size_t)((w + 7) / 8) * ((h + 7) / 8) * 4;
        if (overlaps(c.outHist, n * 16, c.tileLive, tb) || overlaps(c.outLen, n * 4, c.tileLive, tb))
            return postfx_fail_fn(-1, fn, "the outputs must not alias the tile map");
    }
    // what a motion buffer adds: outputs that leave it alone
    if (c.motion && (overlaps(c.outHist, n * 16, c.motion, n * 16) || overlaps(c.outLen, n * 4, c.motion, n * 16)))
        return postfx_fail_fn(-1, c.fromCur ? "pt_temporal_accumulate_cur_motion" : "pt_temporal_accumulate_motion",
                              "the outputs must not alias the motion buffer");
    return 0;
}

// The nine instantiations, by source, identity and motion; a tile map takes the ninth (check_temporal_call: the identity path, with
// a history). Without a history the motion kernels are not chosen: the buffer is not read.
static int temporal_launch(const TemporalCall& c, hipStream_t stream) {
    using Kernel = void (*)(TemporalArgs);
    static const Kernel table[2][2][2] = {
        {{temporal_kernel<FromSums, false, false, false>, temporal_kernel<FromSums, false, true, false>},
         {temporal_kernel<FromSums, true, false, false>, temporal_kernel<FromSums, true, true, false>}},
        {{temporal_kernel<FromCur, false, false, false>, temporal_kernel<FromCur, false, true, false>},
         {temporal_kernel<FromCur, true, false, false>, temporal_kernel<FromCur, true, true, false>}}};
    const bool motion = c.motion && c.hist;
    const Kernel kernel = c.tileLive ? temporal_kernel<FromSums, true, false, true> : table[c.fromCur][temporal_ident(c)][motion];
    TemporalArgs a = {};
    a.w = c.w; a.h = c.h;
    a.cam = temporal_cam(*c.cam); a.prev = temporal_cam(c.prev ? *c.prev : *c.cam);
    a.sum = (const float4*)c.sum; a.sq = (const float4*)c.sq; a.albedo = (const float4*)c.albedo;
    a.spp = (float)c.spp; a.batches = (float)c.batches;
    a.cur = (const float4*)c.cur;
    a.nd = (const float4*)c.nd; a.prevNd = (const float4*)c.prevNd; a.hist = (const float4*)c.hist; a.histLen = (const float*)c.histLen;
    a.motion = motion ? (const float4*)c.motion : nullptr;
    a.tileLive = (const int32_t*)c.tileLive; a.tilesX = (c.w + 7) / 8;
    a.maxHistory = (float)c.P.max_history; a.depthTol = c.P.depth_tol; a.normalTol = c.P.normal_tol;
    a.outHist = (float4*)c.outHist; a.outLen = (float*)c.outLen;
    hipLaunchKernelGGL(kernel, dim3((c.w + 15) / 16, (c.h + 15) / 16), dim3(256), 0, stream, a);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

// Check and launch: on the caller's device buffers, or (host) on staged copies of the slices the call has. The history slices are
// absent on a first frame, and the motion slice with them (it is not read without a history).
static int temporal_run(const TemporalCall& c, bool host, hipStream_t stream) {
    if (int r = check_temporal_call(c)) return r;
    if (!host) return temporal_launch(c, stream);
    const size_t n = (size_t)c.w * c.h, b16 = n * 16, tb = (size_t)((c.w + 7) / 8) * ((c.h + 7) / 8) * 4;
    const HostIn in[] = {{c.sum, b16}, {c.sq, b16}, {c.albedo, b16}, {c.cur, b16}, {c.nd, b16}, {c.prevNd, b16}, {c.hist, b16},
                         {c.histLen, n * 4}, {c.tileLive, tb}, {c.hist ? c.motion : nullptr, b16}};
    const HostOut out[] = {{c.outHist, b16}, {c.outLen, n * 4}};
    return postfx_host_form(c.fn, 0, in, out, [&](char*, char** dIn, char** dOut) {
        TemporalCall d = c;
        d.sum = dIn[0]; d.sq = dIn[1]; d.albedo = dIn[2]; d.cur = dIn[3]; d.nd = dIn[4]; d.prevNd = dIn[5]; d.hist = dIn[6]; d.histLen = dIn[7];
        d.tileLive = dIn[8]; d.motion = dIn[9];
        d.outHist = dOut[0]; d.outLen = dOut[1];
        return temporal_launch(d, nullptr);
    });
}

}  // namespace pt

using namespace pt;

extern "C" {

void pt_temporal_defaults(pt_temporal_params* out) {
    if (!out) return;
    out->max_history = 32;
    out->depth_tol = 0.10f;
    out->normal_tol = 0.9f;
}

int pt_temporal_accumulate_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_rgba_sum, const void* d_sq_sum, int spp,
                                  int batches, const void* d_albedo, const void* d_normal_depth, const void* d_prev_normal_depth, const void* d_hist,
                                  const void* d_hist_len, const pt_temporal_params* params, void* d_out_hist, void* d_out_hist_len, void* stream) {
    TemporalCall c = temporal_call("pt_temporal_accumulate", w, h, cam, cam_prev, d_normal_depth, d_prev_normal_depth, d_hist, d_hist_len, params,
                                   d_out_hist, d_out_hist_len);
    return temporal_run(from_sums(c, d_rgba_sum, d_sq_sum, spp, batches, d_albedo), false, (hipStream_t)stream);
}

int pt_temporal_accumulate(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* rgba_sum, const float* sq_sum, int spp,
                           int batches, const float* albedo, const float* normal_depth, const float* prev_normal_depth, const float* hist,
                           const float* hist_len, const pt_temporal_params* params, float* out_hist, float* out_hist_len) {
    TemporalCall c = temporal_call("pt_temporal_accumulate", w, h, cam, cam_prev, normal_depth, prev_normal_depth, hist, hist_len, params, out_hist,
                                   out_hist_len);
    return temporal_run(from_sums(c, rgba_sum, sq_sum, spp, batches, albedo), true, nullptr);
}

int pt_temporal_accumulate_live_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_rgba_sum, const void* d_sq_sum,
                                       int spp, int batches, const void* d_albedo, const void* d_normal_depth, const void* d_prev_normal_depth,
                                       const void* d_hist, const void* d_hist_len, const void* d_tile_live, const pt_temporal_params* params,
                                       void* d_out_hist, void* d_out_hist_len, void* stream) {
    TemporalCall c = temporal_call("pt_temporal_accumulate_live", w, h, cam, cam_prev, d_normal_depth, d_prev_normal_depth, d_hist, d_hist_len, params,
                                   d_out_hist, d_out_hist_len);
    c.tileLive = d_tile_live;
    return temporal_run(from_sums(c, d_rgba_sum, d_sq_sum, spp, batches, d_albedo), false, (hipStream_t)stream);
}

int pt_temporal_accumulate_live(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* rgba_sum, const float* sq_sum, int spp,
                                int batches, const float* albedo, const float* normal_depth, const float* prev_normal_depth, const float* hist,
                                const float* hist_len, const int32_t* tile_live, const pt_temporal_params* params, float* out_hist,
                                float* out_hist_len) {
    TemporalCall c = temporal_call("pt_temporal_accumulate_live", w, h, cam, cam_prev, normal_depth, prev_normal_depth, hist, hist_len, params, out_hist,
                                   out_hist_len);
    c.tileLive = tile_live;
    return temporal_run(from_sums(c, rgba_sum, sq_sum, spp, batches, albedo), true, nullptr);
}

int pt_temporal_accumulate_cur_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_cur, const void* d_normal_depth,
                                      const void* d_prev_normal_depth, const void* d_hist, const void* d_hist_len, const pt_temporal_params* params,
                                      void* d_out_hist, void* d_out_hist_len, void* stream) {
    TemporalCall c = temporal_call("pt_temporal_accumulate_cur", w, h, cam, cam_prev, d_normal_depth, d_prev_normal_depth, d_hist, d_hist_len, params,
                                   d_out_hist, d_out_hist_len);
    return temporal_run(from_cur(c, d_cur), false, (hipStream_t)stream);
}

int pt_temporal_accumulate_cur(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* cur, const float* normal_depth,
                               const float* prev_normal_depth, const float* hist, const float* hist_len, const pt_temporal_params* params,
                               float* out_hist, float* out_hist_len) {
    TemporalCall c = temporal_call("pt_temporal_accumulate_cur", w, h, cam, cam_prev, normal_depth, prev_normal_depth, hist, hist_len, params, out_hist,
                                   out_hist_len);
    return temporal_run(from_cur(c, cur), true, nullptr);
}

// ---- with a motion buffer (pt_render_motion): motion NULL is the base function ----------------------------------------------------
int pt_temporal_accumulate_motion_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_rgba_sum, const void* d_sq_sum,
                                         int spp, int batches, const void* d_albedo, const void* d_normal_depth, const void* d_prev_normal_depth,
                                         const void* d_hist, const void* d_hist_len, const void* d_motion, const pt_temporal_params* params,
                                         void* d_out_hist, void* d_out_hist_len, void* stream) {
    TemporalCall c = temporal_call("pt_temporal_accumulate_motion", w, h, cam, cam_prev, d_normal_depth, d_prev_normal_depth, d_hist, d_hist_len, params,
                                   d_out_hist, d_out_hist_len);
    c.motion = d_motion;
    return temporal_run(from_sums(c, d_rgba_sum, d_sq_sum, spp, batches, d_albedo), false, (hipStream_t)stream);
}

int pt_temporal_accumulate_motion(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* rgba_sum, const float* sq_sum, int spp,
                                  int batches, const float* albedo, const float* normal_depth, const float* prev_normal_depth, const float* hist,
                                  const float* hist_len, const float* motion, const pt_temporal_params* params, float* out_hist,
                                  float* out_hist_len) {
    TemporalCall c = temporal_call("pt_temporal_accumulate_motion", w, h, cam, cam_prev, normal_depth, prev_normal_depth, hist, hist_len, params,
                                   out_hist, out_hist_len);
    c.motion = motion;
    return temporal_run(from_sums(c, rgba_sum, sq_sum, spp, batches, albedo), true, nullptr);
}

int pt_temporal_accumulate_cur_motion_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_cur,
                                             const void* d_normal_depth, const void* d_prev_normal_depth, const void* d_hist, const void* d_hist_len,
                                             const void* d_motion, const pt_temporal_params* params, void* d_out_hist, void* d_out_hist_len,
                                             void* stream) {
    TemporalCall c = temporal_call("pt_temporal_accumulate_cur_motion", w, h, cam, cam_prev, d_normal_depth, d_prev_normal_depth, d_hist, d_hist_len,
                                   params, d_out_hist, d_out_hist_len);
    c.motion = d_motion;
    return temporal_run(from_cur(c, d_cur), false, (hipStream_t)stream);
}

int pt_temporal_accumulate_cur_motion(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* cur, const float* normal_depth,
                                      const float* prev_normal_depth, const float* hist, const float* hist_len, const float* motion,
                                      const pt_temporal_params* params, float* out_hist, float* out_hist_len) {
    TemporalCall c = temporal_call("pt_temporal_accumulate_cur_motion", w, h, cam, cam_prev, normal_depth, prev_normal_depth, hist, hist_len, params,
                                   out_hist, out_hist_len);
    c.motion = motion;
    return temporal_run(from_cur(c, cur), true, nullptr);
}

}  // extern "C"
