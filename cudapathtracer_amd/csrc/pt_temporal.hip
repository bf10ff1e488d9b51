// pt_temporal.hip — temporal accumulation with reprojection (the history stage of SVGF: Schied et al., HPG 2017) on the
// albedo-demodulated mean and its variance, in pt_denoise_var's working format. include/pt_api.h states the arithmetic;
// tests/temporal_ref.py restates it in numpy. Opt-in post-process on buffers: stateless, no workspace, no render path involved.
//
//   temporal_accumulate_kernel<IDENT>   one thread per pixel, 16x16 pixels per workgroup as four 8x8 tiles (one per wave, the
//                                       tiling of denoise_var_iter_kernel: a wave's four gathers fall into a few lines).
//                                       This frame's (e, V) from S and Q (dn_var_pixel, shared with denoise_var_prepare_kernel);
//                                       the pixel's world point from its depth along the unjittered centre ray, projected into
//                                       the previous camera; up to four bilinear taps of the previous history, each checked
//                                       against the previous guide; the blend. IDENT: both cameras are the same bytes, the tap
//                                       is the pixel itself and no projection is computed.
//   temporal_accumulate_cur_kernel<IDENT>  the same with this frame's (e, V) read from a buffer (pt_upsample's output): the two
//                                       kernels share temporal_blend, everything after the working pixel.
//   temporal_accumulate_live_kernel    the identity instantiation with a map of live 8x8 tiles (pt_temporal_accumulate_live: a
//                                       resting viewer whose converged tiles were not rendered). A wave is one tile, so the
//                                       map entry is one scalar load and the branch does not diverge: a carried wave copies its
//                                       history and length (two loads, two stores), a live wave runs temporal_accumulate_kernel<true>'s
//                                       code.
//   temporal_accumulate_motion_kernel<IDENT>, temporal_accumulate_cur_motion_kernel<IDENT>  the two kernels above with a motion
//                                       buffer (pt_render_motion): a pixel whose motion.w is 1 reprojects the point the buffer
//                                       names — where its surface point WAS — and never takes the identity tap; every other
//                                       pixel runs the base kernel's code (temporal_blend<IDENT, true>). One more float4 load.
// Both cameras travel by value as kernel arguments (SGPRs); plain cached float4 loads, no LDS.
#include <cmath>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../include/pt_api.h"
#include "pt_denoise_shared.h"

extern "C" int pt_fail_(int code, const char* msg);

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

template <bool IDENT>
__global__ void __launch_bounds__(256) temporal_accumulate_kernel(int w, int h, TemporalCam cam, TemporalCam prev, const float4* __restrict__ sum,
                                                                  const float4* __restrict__ sq, float spp, float batches,
                                                                  const float4* __restrict__ albedo, const float4* __restrict__ nd,
                                                                  const float4* __restrict__ prevNd, const float4* __restrict__ hist,
                                                                  const float* __restrict__ histLen, float maxHistory, float depthTol,
                                                                  float normalTol, float4* __restrict__ outHist, float* __restrict__ outLen) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    float4 m;
    const float4 cur = dn_var_pixel(sum[p], sq[p], albedo[p], spp, batches, m);
    if (cur.w < 0.0f) { outHist[p] = make_float4(m.x, m.y, m.z, -1.0f); outLen[p] = 0.0f; return; }
    temporal_blend<IDENT>(w, h, x, y, cur, cam, prev, nd, prevNd, hist, histLen, maxHistory, depthTol, normalTol, outHist, outLen);
}

// pt_temporal_accumulate_live: the identity path with a tile map. tileLive[tile] == 0: the tile was not rendered this frame and
// keeps its history and length bit for bit (S, Q and albedo are not read there).
__global__ void __launch_bounds__(256) temporal_accumulate_live_kernel(int w, int h, int tilesX, const int32_t* __restrict__ tileLive,
                                                                       const float4* __restrict__ sum, const float4* __restrict__ sq, float spp,
                                                                       float batches, const float4* __restrict__ albedo, const float4* __restrict__ nd,
                                                                       const float4* __restrict__ prevNd, const float4* __restrict__ hist,
                                                                       const float* __restrict__ histLen, float maxHistory, float depthTol,
                                                                       float normalTol, float4* __restrict__ outHist, float* __restrict__ outLen) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = blockIdx.x * 2 + (wave & 1), ty = blockIdx.y * 2 + (wave >> 1);
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    if (x >= w || y >= h) return;                             // (a tile outside the grid has no lane left: no read past the map)
    const size_t p = (size_t)y * w + x;
    if (tileLive[__builtin_amdgcn_readfirstlane(ty * tilesX + tx)] == 0) {
        outHist[p] = hist[p];
        outLen[p] = histLen[p];
        return;
    }
    float4 m;
    const float4 cur = dn_var_pixel(sum[p], sq[p], albedo[p], spp, batches, m);
    if (cur.w < 0.0f) { outHist[p] = make_float4(m.x, m.y, m.z, -1.0f); outLen[p] = 0.0f; return; }
    const TemporalCam none = {};                              // (the identity path reads neither camera)
    temporal_blend<true>(w, h, x, y, cur, none, none, nd, prevNd, hist, histLen, maxHistory, depthTol, normalTol, outHist, outLen);
}

// pt_temporal_accumulate_cur: this frame's working pixel is given (pt_upsample wrote it), not derived from S and Q.
template <bool IDENT>
__global__ void __launch_bounds__(256) temporal_accumulate_cur_kernel(int w, int h, TemporalCam cam, TemporalCam prev, const float4* __restrict__ curIn,
                                                                      const float4* __restrict__ nd, const float4* __restrict__ prevNd,
                                                                      const float4* __restrict__ hist, const float* __restrict__ histLen,
                                                                      float maxHistory, float depthTol, float normalTol,
                                                                      float4* __restrict__ outHist, float* __restrict__ outLen) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const float4 cur = curIn[p];
    if (!(cur.w >= 0.0f)) { outHist[p] = make_float4(cur.x, cur.y, cur.z, -1.0f); outLen[p] = 0.0f; return; }
    temporal_blend<IDENT>(w, h, x, y, cur, cam, prev, nd, prevNd, hist, histLen, maxHistory, depthTol, normalTol, outHist, outLen);
}

// pt_temporal_accumulate_motion / _cur_motion: the two kernels above with the motion buffer (the launch gives them a history).
template <bool IDENT>
__global__ void __launch_bounds__(256) temporal_accumulate_motion_kernel(int w, int h, TemporalCam cam, TemporalCam prev, const float4* __restrict__ sum,
                                                                         const float4* __restrict__ sq, float spp, float batches,
                                                                         const float4* __restrict__ albedo, const float4* __restrict__ nd,
                                                                         const float4* __restrict__ prevNd, const float4* __restrict__ hist,
                                                                         const float* __restrict__ histLen, const float4* __restrict__ motion,
                                                                         float maxHistory, float depthTol, float normalTol,
                                                                         float4* __restrict__ outHist, float* __restrict__ outLen) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    float4 m;
    const float4 cur = dn_var_pixel(sum[p], sq[p], albedo[p], spp, batches, m);
    if (cur.w < 0.0f) { outHist[p] = make_float4(m.x, m.y, m.z, -1.0f); outLen[p] = 0.0f; return; }
    temporal_blend<IDENT, true>(w, h, x, y, cur, cam, prev, nd, prevNd, hist, histLen, maxHistory, depthTol, normalTol, outHist, outLen, motion);
}

template <bool IDENT>
__global__ void __launch_bounds__(256) temporal_accumulate_cur_motion_kernel(int w, int h, TemporalCam cam, TemporalCam prev,
                                                                             const float4* __restrict__ curIn, const float4* __restrict__ nd,
                                                                             const float4* __restrict__ prevNd, const float4* __restrict__ hist,
                                                                             const float* __restrict__ histLen, const float4* __restrict__ motion,
                                                                             float maxHistory, float depthTol, float normalTol,
                                                                             float4* __restrict__ outHist, float* __restrict__ outLen) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const float4 cur = curIn[p];
    if (!(cur.w >= 0.0f)) { outHist[p] = make_float4(cur.x, cur.y, cur.z, -1.0f); outLen[p] = 0.0f; return; }
    temporal_blend<IDENT, true>(w, h, x, y, cur, cam, prev, nd, prevNd, hist, histLen, maxHistory, depthTol, normalTol, outHist, outLen, motion);
}

static int tp_fail(int code, const char* fn, const char* fmt, int a = 0, int b = 0, int c = 0, int d = 0) {
    char buf[256];
    const int n = snprintf(buf, sizeof(buf), "%s: ", fn);
    snprintf(buf + n, sizeof(buf) - n, fmt, a, b, c, d);
    return pt_fail_(code, buf);
}
#define TP_HIP_OK(expr)                                                                                            \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess) {                                                                                    \
            char m_[256]; snprintf(m_, sizeof(m_), "%s failed: %s", #expr, hipGetErrorString(e_));                 \
            return pt_fail_(-2, m_);                                                                               \
        }                                                                                                          \
    } while (0)

static bool overlaps(const void* a, size_t aBytes, const void* b, size_t bBytes) {
    const char* pa = (const char*)a; const char* pb = (const char*)b;
    return pa < pb + bBytes && pb < pa + aBytes;
}

// What both entry points check after their own frame inputs (`inputs`: none of this frame's buffers is NULL).
static int check_history_args(const char* fn, int w, int h, const pt_camera* cam, const pt_camera* prev, bool inputs, const void* prevNd,
                              const void* hist, const void* histLen, const pt_temporal_params& P, const void* outHist, const void* outLen) {
    if (!cam) return tp_fail(-1, fn, "null camera");
    if (cam->w != w || cam->h != h) return tp_fail(-1, fn, "camera is %d x %d, the frame %d x %d", cam->w, cam->h, w, h);
    if (prev && (prev->w != w || prev->h != h)) return tp_fail(-1, fn, "previous camera is %d x %d, the frame %d x %d", prev->w, prev->h, w, h);
    if (!inputs) return tp_fail(-1, fn, "null buffer");
    if (!outHist || !outLen) return tp_fail(-1, fn, "null output");
    const int given = (prevNd != nullptr) + (hist != nullptr) + (histLen != nullptr);
    if (given != 0 && given != 3) return tp_fail(-1, fn, "prev_normal_depth, hist and hist_len must be all NULL (first frame) or all set");
    if (given == 3) {
        const size_t n = (size_t)w * h;
        if (overlaps(outHist, n * 16, hist, n * 16) || overlaps(outLen, n * 4, histLen, n * 4) || overlaps(outHist, n * 16, histLen, n * 4) ||
            overlaps(outLen, n * 4, hist, n * 16))
            return tp_fail(-1, fn, "the output history must not alias the input history (ping-pong two pairs)");
    }
    if (P.max_history < 1) return tp_fail(-1, fn, "max_history %d must be at least 1", P.max_history);
    if (!(P.depth_tol > 0.0f) || !std::isfinite(P.depth_tol)) return tp_fail(-1, fn, "depth_tol must be positive and finite");
    if (!(P.normal_tol > 0.0f) || !(P.normal_tol <= 1.0f)) return tp_fail(-1, fn, "normal_tol must be in (0, 1]");
    return 0;
}

static int check_size(const char* fn, int w, int h) {
    if (w <= 0 || h <= 0) return tp_fail(-1, fn, "image size %d x %d must be positive", w, h);
    if ((long long)w * h > 0x7fffffffll) return tp_fail(-1, fn, "image of %d x %d pixels is too large", w, h);
    return 0;
}

static int check_temporal_args(int w, int h, const pt_camera* cam, const pt_camera* prev, const void* sum, const void* sq, int spp, int batches,
                               const void* albedo, const void* nd, const void* prevNd, const void* hist, const void* histLen,
                               const pt_temporal_params& P, const void* outHist, const void* outLen) {
    const char* fn = "pt_temporal_accumulate";
    if (int r = check_size(fn, w, h)) return r;
    if (spp <= 0) return tp_fail(-1, fn, "spp %d must be positive", spp);
    if (batches < 2) return tp_fail(-1, fn, "batches %d must be at least 2", batches);
    if (spp % batches != 0) return tp_fail(-1, fn, "batches %d must divide spp %d", batches, spp);
    return check_history_args(fn, w, h, cam, prev, sum && sq && albedo && nd, prevNd, hist, histLen, P, outHist, outLen);
}

// What a tile map adds (pt_temporal_accumulate_live): the identity path and a history, and outputs that leave the map alone.
static int check_live_args(int w, int h, const pt_camera* cam, const pt_camera* prev, const void* hist, const void* tileLive, const void* outHist,
                           const void* outLen) {
    const char* fn = "pt_temporal_accumulate_live";
    if (!tileLive) return 0;
    if (!hist) return tp_fail(-1, fn, "a tile map needs a history: a carried pixel keeps what it had");
    if (prev && memcmp(cam, prev, sizeof(pt_camera)) != 0)
        return tp_fail(-1, fn, "a tile map needs an unchanged camera (cam_prev NULL or equal to cam): a carried pixel keeps what it had at the same place");
    const size_t n = (size_t)w * h, tb = (size_t)((w + 7) / 8) * ((h + 7) / 8) * 4;
    if (overlaps(outHist, n * 16, tileLive, tb) || overlaps(outLen, n * 4, tileLive, tb)) return tp_fail(-1, fn, "the outputs must not alias the tile map");
    return 0;
}

static int check_temporal_cur_args(int w, int h, const pt_camera* cam, const pt_camera* prev, const void* cur, const void* nd, const void* prevNd,
                                   const void* hist, const void* histLen, const pt_temporal_params& P, const void* outHist, const void* outLen) {
    const char* fn = "pt_temporal_accumulate_cur";
    if (int r = check_size(fn, w, h)) return r;
    return check_history_args(fn, w, h, cam, prev, cur && nd, prevNd, hist, histLen, P, outHist, outLen);
}

// What a motion buffer adds (pt_temporal_accumulate_motion, _cur_motion): outputs that leave it alone.
static int check_motion_args(const char* fn, int w, int h, const void* motion, const void* outHist, const void* outLen) {
    if (!motion) return 0;
    const size_t n = (size_t)w * h;
    if (overlaps(outHist, n * 16, motion, n * 16) || overlaps(outLen, n * 4, motion, n * 16)) return tp_fail(-1, fn, "the outputs must not alias the motion buffer");
    return 0;
}

static int temporal_launch(int w, int h, const pt_camera* cam, const pt_camera* prev, const float4* sum, const float4* sq, int spp, int batches,
                           const float4* albedo, const float4* nd, const float4* prevNd, const float4* hist, const float* histLen,
                           const pt_temporal_params& P, float4* outHist, float* outLen, hipStream_t stream, const int32_t* tileLive = nullptr,
                           const float4* motion = nullptr) {
    const bool ident = !prev || memcmp(cam, prev, sizeof(pt_camera)) == 0;
    const TemporalCam c = temporal_cam(*cam), q = temporal_cam(prev ? *prev : *cam);
    const dim3 grid((w + 15) / 16, (h + 15) / 16);
    if (tileLive)                                             // (check_live_args: the identity path, with a history)
        hipLaunchKernelGGL(temporal_accumulate_live_kernel, grid, dim3(256), 0, stream, w, h, (w + 7) / 8, tileLive, sum, sq, (float)spp, (float)batches,
                           albedo, nd, prevNd, hist, histLen, (float)P.max_history, P.depth_tol, P.normal_tol, outHist, outLen);
    else if (motion && hist && ident)                         // (without a history the base kernel: the buffer is not read)
        hipLaunchKernelGGL(temporal_accumulate_motion_kernel<true>, grid, dim3(256), 0, stream, w, h, c, q, sum, sq, (float)spp, (float)batches, albedo,
                           nd, prevNd, hist, histLen, motion, (float)P.max_history, P.depth_tol, P.normal_tol, outHist, outLen);
    else if (motion && hist)
        hipLaunchKernelGGL(temporal_accumulate_motion_kernel<false>, grid, dim3(256), 0, stream, w, h, c, q, sum, sq, (float)spp, (float)batches, albedo,
                           nd, prevNd, hist, histLen, motion, (float)P.max_history, P.depth_tol, P.normal_tol, outHist, outLen);
    else if (ident)
        hipLaunchKernelGGL(temporal_accumulate_kernel<true>, grid, dim3(256), 0, stream, w, h, c, q, sum, sq, (float)spp, (float)batches, albedo, nd,
                           prevNd, hist, histLen, (float)P.max_history, P.depth_tol, P.normal_tol, outHist, outLen);
    else
        hipLaunchKernelGGL(temporal_accumulate_kernel<false>, grid, dim3(256), 0, stream, w, h, c, q, sum, sq, (float)spp, (float)batches, albedo, nd,
                           prevNd, hist, histLen, (float)P.max_history, P.depth_tol, P.normal_tol, outHist, outLen);
    TP_HIP_OK(hipGetLastError());
    return 0;
}

static int temporal_cur_launch(int w, int h, const pt_camera* cam, const pt_camera* prev, const float4* cur, const float4* nd, const float4* prevNd,
                               const float4* hist, const float* histLen, const pt_temporal_params& P, float4* outHist, float* outLen,
                               hipStream_t stream, const float4* motion = nullptr) {
    const bool ident = !prev || memcmp(cam, prev, sizeof(pt_camera)) == 0;
    const TemporalCam c = temporal_cam(*cam), q = temporal_cam(prev ? *prev : *cam);
    const dim3 grid((w + 15) / 16, (h + 15) / 16);
    if (motion && hist && ident)
        hipLaunchKernelGGL(temporal_accumulate_cur_motion_kernel<true>, grid, dim3(256), 0, stream, w, h, c, q, cur, nd, prevNd, hist, histLen, motion,
                           (float)P.max_history, P.depth_tol, P.normal_tol, outHist, outLen);
    else if (motion && hist)
        hipLaunchKernelGGL(temporal_accumulate_cur_motion_kernel<false>, grid, dim3(256), 0, stream, w, h, c, q, cur, nd, prevNd, hist, histLen, motion,
                           (float)P.max_history, P.depth_tol, P.normal_tol, outHist, outLen);
    else if (ident)
        hipLaunchKernelGGL(temporal_accumulate_cur_kernel<true>, grid, dim3(256), 0, stream, w, h, c, q, cur, nd, prevNd, hist, histLen,
                           (float)P.max_history, P.depth_tol, P.normal_tol, outHist, outLen);
    else
        hipLaunchKernelGGL(temporal_accumulate_cur_kernel<false>, grid, dim3(256), 0, stream, w, h, c, q, cur, nd, prevNd, hist, histLen,
                           (float)P.max_history, P.depth_tol, P.normal_tol, outHist, outLen);
    TP_HIP_OK(hipGetLastError());
    return 0;
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
    pt_temporal_params P;
    if (params) P = *params; else pt_temporal_defaults(&P);
    if (int r = check_temporal_args(w, h, cam, cam_prev, d_rgba_sum, d_sq_sum, spp, batches, d_albedo, d_normal_depth, d_prev_normal_depth, d_hist,
                                    d_hist_len, P, d_out_hist, d_out_hist_len))
        return r;
    return temporal_launch(w, h, cam, cam_prev, (const float4*)d_rgba_sum, (const float4*)d_sq_sum, spp, batches, (const float4*)d_albedo,
                           (const float4*)d_normal_depth, (const float4*)d_prev_normal_depth, (const float4*)d_hist, (const float*)d_hist_len, P,
                           (float4*)d_out_hist, (float*)d_out_hist_len, (hipStream_t)stream);
}

// The host forms of pt_temporal_accumulate, pt_temporal_accumulate_live (tileLive set) and pt_temporal_accumulate_motion (motion set).
static int temporal_host(const char* fn, int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* rgba_sum, const float* sq_sum,
                         int spp, int batches, const float* albedo, const float* normal_depth, const float* prev_normal_depth, const float* hist,
                         const float* hist_len, const int32_t* tileLive, const pt_temporal_params& P, float* out_hist, float* out_hist_len,
                         const float* motion = nullptr) {
    const size_t n = (size_t)w * h, b16 = n * 16, b4 = (n * 4 + 15) & ~(size_t)15, tb = (size_t)((w + 7) / 8) * ((h + 7) / 8) * 4;
    const bool first = hist == nullptr;
    if (first) motion = nullptr;                              // (not read without a history)
    const size_t tbp = tileLive ? (tb + 15) & ~(size_t)15 : 0;
    char* d = nullptr;
    TP_HIP_OK(hipMalloc(&d, 7 * b16 + 2 * b4 + tbp + (motion ? b16 : 0)));
    char* dS = d; char* dQ = dS + b16; char* dA = dQ + b16; char* dN = dA + b16; char* dPN = dN + b16; char* dH = dPN + b16; char* dO = dH + b16;
    char* dHL = dO + b16; char* dOL = dHL + b4; char* dT = dOL + b4; char* dM = dT + tbp;
    hipError_t e = hipMemcpy(dS, rgba_sum, b16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dQ, sq_sum, b16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dA, albedo, b16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dN, normal_depth, b16, hipMemcpyHostToDevice);
    if (e == hipSuccess && !first) e = hipMemcpy(dPN, prev_normal_depth, b16, hipMemcpyHostToDevice);
    if (e == hipSuccess && !first) e = hipMemcpy(dH, hist, b16, hipMemcpyHostToDevice);
    if (e == hipSuccess && !first) e = hipMemcpy(dHL, hist_len, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && tileLive) e = hipMemcpy(dT, tileLive, tb, hipMemcpyHostToDevice);
    if (e == hipSuccess && motion) e = hipMemcpy(dM, motion, b16, hipMemcpyHostToDevice);
    int r = 0;
    if (e != hipSuccess) {
        r = tp_fail(-2, fn, "upload failed");
    } else if ((r = temporal_launch(w, h, cam, cam_prev, (const float4*)dS, (const float4*)dQ, spp, batches, (const float4*)dA, (const float4*)dN,
                                    first ? nullptr : (const float4*)dPN, first ? nullptr : (const float4*)dH, first ? nullptr : (const float*)dHL, P,
                                    (float4*)dO, (float*)dOL, nullptr, tileLive ? (const int32_t*)dT : nullptr,
                                    motion ? (const float4*)dM : nullptr)) == 0) {
        e = hipMemcpy(out_hist, dO, b16, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(out_hist_len, dOL, n * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) r = tp_fail(-2, fn, "download failed");
    }
    (void)hipFree(d);
    return r;
}

int pt_temporal_accumulate(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* rgba_sum, const float* sq_sum, int spp,
                           int batches, const float* albedo, const float* normal_depth, const float* prev_normal_depth, const float* hist,
                           const float* hist_len, const pt_temporal_params* params, float* out_hist, float* out_hist_len) {
    pt_temporal_params P;
    if (params) P = *params; else pt_temporal_defaults(&P);
    if (int r = check_temporal_args(w, h, cam, cam_prev, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, prev_normal_depth, hist, hist_len, P,
                                    out_hist, out_hist_len))
        return r;
    return temporal_host("pt_temporal_accumulate", w, h, cam, cam_prev, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, prev_normal_depth, hist,
                         hist_len, nullptr, P, out_hist, out_hist_len);
}

int pt_temporal_accumulate_live_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_rgba_sum, const void* d_sq_sum,
                                       int spp, int batches, const void* d_albedo, const void* d_normal_depth, const void* d_prev_normal_depth,
                                       const void* d_hist, const void* d_hist_len, const void* d_tile_live, const pt_temporal_params* params,
                                       void* d_out_hist, void* d_out_hist_len, void* stream) {
    pt_temporal_params P;
    if (params) P = *params; else pt_temporal_defaults(&P);
    if (int r = check_temporal_args(w, h, cam, cam_prev, d_rgba_sum, d_sq_sum, spp, batches, d_albedo, d_normal_depth, d_prev_normal_depth, d_hist,
                                    d_hist_len, P, d_out_hist, d_out_hist_len))
        return r;
    if (int r = check_live_args(w, h, cam, cam_prev, d_hist, d_tile_live, d_out_hist, d_out_hist_len)) return r;
    return temporal_launch(w, h, cam, cam_prev, (const float4*)d_rgba_sum, (const float4*)d_sq_sum, spp, batches, (const float4*)d_albedo,
                           (const float4*)d_normal_depth, (const float4*)d_prev_normal_depth, (const float4*)d_hist, (const float*)d_hist_len, P,
                           (float4*)d_out_hist, (float*)d_out_hist_len, (hipStream_t)stream, (const int32_t*)d_tile_live);
}

int pt_temporal_accumulate_live(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* rgba_sum, const float* sq_sum, int spp,
                                int batches, const float* albedo, const float* normal_depth, const float* prev_normal_depth, const float* hist,
                                const float* hist_len, const int32_t* tile_live, const pt_temporal_params* params, float* out_hist,
                                float* out_hist_len) {
    pt_temporal_params P;
    if (params) P = *params; else pt_temporal_defaults(&P);
    if (int r = check_temporal_args(w, h, cam, cam_prev, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, prev_normal_depth, hist, hist_len, P,
                                    out_hist, out_hist_len))
        return r;
    if (int r = check_live_args(w, h, cam, cam_prev, hist, tile_live, out_hist, out_hist_len)) return r;
    return temporal_host("pt_temporal_accumulate_live", w, h, cam, cam_prev, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, prev_normal_depth,
                         hist, hist_len, tile_live, P, out_hist, out_hist_len);
}

// The host forms of pt_temporal_accumulate_cur and pt_temporal_accumulate_cur_motion (motion set).
static int temporal_cur_host(const char* fn, int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* cur, const float* normal_depth,
                             const float* prev_normal_depth, const float* hist, const float* hist_len, const float* motion,
                             const pt_temporal_params& P, float* out_hist, float* out_hist_len) {
    const size_t n = (size_t)w * h, b16 = n * 16, b4 = (n * 4 + 15) & ~(size_t)15;
    const bool first = hist == nullptr;
    if (first) motion = nullptr;                              // (not read without a history)
    char* d = nullptr;
    TP_HIP_OK(hipMalloc(&d, 5 * b16 + 2 * b4 + (motion ? b16 : 0)));
    char* dC = d; char* dN = dC + b16; char* dPN = dN + b16; char* dH = dPN + b16; char* dO = dH + b16; char* dHL = dO + b16; char* dOL = dHL + b4;
    char* dM = dOL + b4;
    hipError_t e = hipMemcpy(dC, cur, b16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dN, normal_depth, b16, hipMemcpyHostToDevice);
    if (e == hipSuccess && !first) e = hipMemcpy(dPN, prev_normal_depth, b16, hipMemcpyHostToDevice);
    if (e == hipSuccess && !first) e = hipMemcpy(dH, hist, b16, hipMemcpyHostToDevice);
    if (e == hipSuccess && !first) e = hipMemcpy(dHL, hist_len, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && motion) e = hipMemcpy(dM, motion, b16, hipMemcpyHostToDevice);
    int r = 0;
    if (e != hipSuccess) {
        r = tp_fail(-2, fn, "upload failed");
    } else if ((r = temporal_cur_launch(w, h, cam, cam_prev, (const float4*)dC, (const float4*)dN, first ? nullptr : (const float4*)dPN,
                                        first ? nullptr : (const float4*)dH, first ? nullptr : (const float*)dHL, P, (float4*)dO, (float*)dOL,
                                        nullptr, motion ? (const float4*)dM : nullptr)) == 0) {
        e = hipMemcpy(out_hist, dO, b16, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(out_hist_len, dOL, n * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) r = tp_fail(-2, fn, "download failed");
    }
    (void)hipFree(d);
    return r;
}

int pt_temporal_accumulate_cur_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_cur, const void* d_normal_depth,
                                      const void* d_prev_normal_depth, const void* d_hist, const void* d_hist_len, const pt_temporal_params* params,
                                      void* d_out_hist, void* d_out_hist_len, void* stream) {
    pt_temporal_params P;
    if (params) P = *params; else pt_temporal_defaults(&P);
    if (int r = check_temporal_cur_args(w, h, cam, cam_prev, d_cur, d_normal_depth, d_prev_normal_depth, d_hist, d_hist_len, P, d_out_hist,
                                        d_out_hist_len))
        return r;
    return temporal_cur_launch(w, h, cam, cam_prev, (const float4*)d_cur, (const float4*)d_normal_depth, (const float4*)d_prev_normal_depth,
                               (const float4*)d_hist, (const float*)d_hist_len, P, (float4*)d_out_hist, (float*)d_out_hist_len, (hipStream_t)stream);
}

int pt_temporal_accumulate_cur(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* cur, const float* normal_depth,
                               const float* prev_normal_depth, const float* hist, const float* hist_len, const pt_temporal_params* params,
                               float* out_hist, float* out_hist_len) {
    pt_temporal_params P;
    if (params) P = *params; else pt_temporal_defaults(&P);
    if (int r = check_temporal_cur_args(w, h, cam, cam_prev, cur, normal_depth, prev_normal_depth, hist, hist_len, P, out_hist, out_hist_len)) return r;
    return temporal_cur_host("pt_temporal_accumulate_cur", w, h, cam, cam_prev, cur, normal_depth, prev_normal_depth, hist, hist_len, nullptr, P, out_hist,
                             out_hist_len);
}

// ---- with a motion buffer (pt_render_motion): motion NULL is the base function ----------------------------------------------------
int pt_temporal_accumulate_motion_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_rgba_sum, const void* d_sq_sum,
                                         int spp, int batches, const void* d_albedo, const void* d_normal_depth, const void* d_prev_normal_depth,
                                         const void* d_hist, const void* d_hist_len, const void* d_motion, const pt_temporal_params* params,
                                         void* d_out_hist, void* d_out_hist_len, void* stream) {
    pt_temporal_params P;
    if (params) P = *params; else pt_temporal_defaults(&P);
    if (int r = check_temporal_args(w, h, cam, cam_prev, d_rgba_sum, d_sq_sum, spp, batches, d_albedo, d_normal_depth, d_prev_normal_depth, d_hist,
                                    d_hist_len, P, d_out_hist, d_out_hist_len))
        return r;
    if (int r = check_motion_args("pt_temporal_accumulate_motion", w, h, d_motion, d_out_hist, d_out_hist_len)) return r;
    return temporal_launch(w, h, cam, cam_prev, (const float4*)d_rgba_sum, (const float4*)d_sq_sum, spp, batches, (const float4*)d_albedo,
                           (const float4*)d_normal_depth, (const float4*)d_prev_normal_depth, (const float4*)d_hist, (const float*)d_hist_len, P,
                           (float4*)d_out_hist, (float*)d_out_hist_len, (hipStream_t)stream, nullptr, (const float4*)d_motion);
}

int pt_temporal_accumulate_motion(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* rgba_sum, const float* sq_sum, int spp,
                                  int batches, const float* albedo, const float* normal_depth, const float* prev_normal_depth, const float* hist,
                                  const float* hist_len, const float* motion, const pt_temporal_params* params, float* out_hist,
                                  float* out_hist_len) {
    pt_temporal_params P;
    if (params) P = *params; else pt_temporal_defaults(&P);
    if (int r = check_temporal_args(w, h, cam, cam_prev, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, prev_normal_depth, hist, hist_len, P,
                                    out_hist, out_hist_len))
        return r;
    if (int r = check_motion_args("pt_temporal_accumulate_motion", w, h, motion, out_hist, out_hist_len)) return r;
    return temporal_host("pt_temporal_accumulate_motion", w, h, cam, cam_prev, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, prev_normal_depth,
                         hist, hist_len, nullptr, P, out_hist, out_hist_len, motion);
}

int pt_temporal_accumulate_cur_motion_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_cur,
                                             const void* d_normal_depth, const void* d_prev_normal_depth, const void* d_hist, const void* d_hist_len,
                                             const void* d_motion, const pt_temporal_params* params, void* d_out_hist, void* d_out_hist_len,
                                             void* stream) {
    pt_temporal_params P;
    if (params) P = *params; else pt_temporal_defaults(&P);
    if (int r = check_temporal_cur_args(w, h, cam, cam_prev, d_cur, d_normal_depth, d_prev_normal_depth, d_hist, d_hist_len, P, d_out_hist,
                                        d_out_hist_len))
        return r;
    if (int r = check_motion_args("pt_temporal_accumulate_cur_motion", w, h, d_motion, d_out_hist, d_out_hist_len)) return r;
    return temporal_cur_launch(w, h, cam, cam_prev, (const float4*)d_cur, (const float4*)d_normal_depth, (const float4*)d_prev_normal_depth,
                               (const float4*)d_hist, (const float*)d_hist_len, P, (float4*)d_out_hist, (float*)d_out_hist_len, (hipStream_t)stream,
                               (const float4*)d_motion);
}

int pt_temporal_accumulate_cur_motion(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* cur, const float* normal_depth,
                                      const float* prev_normal_depth, const float* hist, const float* hist_len, const float* motion,
                                      const pt_temporal_params* params, float* out_hist, float* out_hist_len) {
    pt_temporal_params P;
    if (params) P = *params; else pt_temporal_defaults(&P);
    if (int r = check_temporal_cur_args(w, h, cam, cam_prev, cur, normal_depth, prev_normal_depth, hist, hist_len, P, out_hist, out_hist_len)) return r;
    if (int r = check_motion_args("pt_temporal_accumulate_cur_motion", w, h, motion, out_hist, out_hist_len)) return r;
    return temporal_cur_host("pt_temporal_accumulate_cur_motion", w, h, cam, cam_prev, cur, normal_depth, prev_normal_depth, hist, hist_len, motion, P,
                             out_hist, out_hist_len);
}

}  // extern "C"
