// pt_temporal.hip — temporal accumulation with reprojection (the history stage of SVGF: Schied et al., HPG 2017) on the
// albedo-demodulated mean and its variance, in pt_denoise_var's working format. include/pt_api.h states the arithmetic;
// tests/temporal_ref.py restates it in numpy (tests/respond_ref.py: the responsive form). Opt-in post-process on buffers: stateless,
// no render path involved; only the responsive form needs a workspace.
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
//   temporal_gather_kernel<Source, IDENT, MOTION> and temporal_respond_kernel<Source>: pt_temporal_accumulate_respond's two launches
//                 (RESPOND below): the same statements through the taps (temporal_gather), a window walk over LDS, the same blend.
//   Nine instantiations of temporal_kernel exist (temporal_launch's table). Everything travels by value in one TemporalArgs (SGPRs), the two
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

// Steps 2-4 of the contract for pixel p = (x, y): reproject, gather. Returns whether the valid tap weight W reached 0.01, and then the
// gathered history: eh = (e_h, V_h), nh = N_h. `hist` is set (the callers test it: a kernel argument).
// MOTION: `motion` is set, and a pixel with motion.w == 1 takes its xyz as the point to reproject (no identity tap for it).
template <bool IDENT, bool MOTION = false>
__device__ inline bool temporal_gather(int w, int h, int x, int y, size_t p, const TemporalCam& cam, const TemporalCam& prev, const float4* __restrict__ nd,
                                       const float4* __restrict__ prevNd, const float4* __restrict__ hist, const float* __restrict__ histLen,
                                       float depthTol, float normalTol, const float4* __restrict__ motion, float4& eh, float& nh) {
    const float4 gp = dn_unit_guide(nd[p]);
    const bool normalP = gp.x != 0.0f || gp.y != 0.0f || gp.z != 0.0f;
    TemporalTap t = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (MOTION) mv = motion[p];                               // (read only with a history)
    const bool moved = MOTION && mv.w == 1.0f;
    if (IDENT && !moved) {
        if (normalP) temporal_tap(t, w, h, x, y, 1.0f, gp, gp.w, depthTol, normalTol, prevNd, hist, histLen);
    } else if (normalP) {
        // the unjittered centre ray of the pixel (camera_ray with both jitters 0 and no lens sample), to the depth z_p
        float px, py, pz;
        if (moved) {                                          // where this surface point was when the previous frame was made
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
    if (!(t.sw >= 0.01f)) return false;
    eh = make_float4(t.se_x / t.sw, t.se_y / t.sw, t.se_z / t.sw, t.sv / t.sw);
    nh = t.sn / t.sw;
    return true;
}

// Step 5: the working value `cur` (e, V >= 0) blended into the gathered history (e_h, V_h) of length nh; `len` is the new length.
__device__ inline float4 temporal_blend(float4 cur, float4 eh, float nh, float maxHistory, float& len) {
    const float n1 = nh + 1.0f;
    len = n1 < maxHistory ? n1 : maxHistory;
    const float alpha = 1.0f / len, keep = 1.0f - alpha;
    return make_float4(eh.x + alpha * (cur.x - eh.x), eh.y + alpha * (cur.y - eh.y), eh.z + alpha * (cur.z - eh.z),
                       (keep * keep) * eh.w + (alpha * alpha) * cur.w);
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
    float4 res = cur, eh;
    float len = 1.0f, nh;
    if (a.hist != nullptr &&                                  // (uniform: a kernel argument)
        temporal_gather<IDENT, MOTION>(a.w, a.h, x, y, p, a.cam, a.prev, a.nd, a.prevNd, a.hist, a.histLen, a.depthTol, a.normalTol, a.motion, eh, nh))
        res = temporal_blend(cur, eh, nh, a.maxHistory, len);
    a.outHist[p] = res;
    a.outLen[p] = len;
}

// ---- RESPOND: a variance-based change test that shortens the history per pixel (include/pt_api.h, "RESPOND") -----------------------
// Two launches with a private workspace of 36 bytes per pixel between them, three planes:
//   G  float4  the gathered history (e_h, V_h); V_h = -1 marks a pixel without one (a gathered V_h is never negative: the taps'
//              variances and weights are not)
//   W  float4  the witness record (d = e - e_h, v = V + V_h); v = NaN for a pixel that is no witness
//   N  float   N_h
struct RespondArgs {
    TemporalArgs t;
    float4 *wsG, *wsW;
    float* wsN;
    int radius, power;
    float k2;                                 // threshold * threshold, rounded once on the host
    float* outScale;
};

// temporal_kernel's tiling and its statements through the taps; what it would have blended goes to the workspace instead.
template <class Source, bool IDENT, bool MOTION>
__global__ void __launch_bounds__(256) temporal_gather_kernel(RespondArgs r) {
    const TemporalArgs& a = r.t;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = blockIdx.x * 2 + (wave & 1), ty = blockIdx.y * 2 + (wave >> 1);
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    if (x >= a.w || y >= a.h) return;
    const size_t p = (size_t)y * a.w + x;
    float4 cur, raw, eh = make_float4(0.0f, 0.0f, 0.0f, -1.0f), wit = make_float4(0.0f, 0.0f, 0.0f, __builtin_nanf(""));
    float nh = 0.0f;
    if (!Source::load(a, p, cur, raw) && a.hist != nullptr &&
        temporal_gather<IDENT, MOTION>(a.w, a.h, x, y, p, a.cam, a.prev, a.nd, a.prevNd, a.hist, a.histLen, a.depthTol, a.normalTol, a.motion, eh, nh))
        wit = make_float4(cur.x - eh.x, cur.y - eh.y, cur.z - eh.z, cur.w + eh.w);
    r.wsG[p] = eh;
    r.wsW[p] = wit;
    r.wsN[p] = nh;
}

// The window walk and the blend. A workgroup stages the witness records and the unit guides of its (16 + 2 radius)^2 region in LDS:
// two float4 arrays with rows of 24 entries. A row stride of 8 mod 16 slots of 16 bytes puts the four rows that one lane group of a
// 16-byte LDS read touches (8x8 wave tiles: half rows of four lanes) on different quarters of the 256-byte bank row, at every radius.
// A record that cannot count (outside the image, no witness, a non-finite d or v, a zero normal) is staged with v = NaN.
constexpr int RESPOND_MAX_RADIUS = 3, RESPOND_ROW = 24, RESPOND_SIDE = 16 + 2 * RESPOND_MAX_RADIUS;

template <class Source>
__global__ void __launch_bounds__(256) temporal_respond_kernel(RespondArgs r) {
    __shared__ float4 sRec[RESPOND_SIDE * RESPOND_ROW], sGuide[RESPOND_SIDE * RESPOND_ROW];
    const TemporalArgs& a = r.t;
    const int rad = r.radius, side = 16 + 2 * rad;
    const int bx = blockIdx.x * 16 - rad, by = blockIdx.y * 16 - rad;
    for (int i = threadIdx.x; i < side * side; i += 256) {
        const int iy = i / side, ix = i - iy * side;
        const int gx = bx + ix, gy = by + iy;
        float4 rec = make_float4(0.0f, 0.0f, 0.0f, __builtin_nanf("")), g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gx >= 0 && gx < a.w && gy >= 0 && gy < a.h) {
            const size_t q = (size_t)gy * a.w + gx;
            const float4 wq = r.wsW[q];
            g = dn_unit_guide(a.nd[q]);
            const bool counts = finite3(wq) && __builtin_isfinite(wq.w) && (g.x != 0.0f || g.y != 0.0f || g.z != 0.0f);
            if (counts) rec = wq;
        }
        sRec[iy * RESPOND_ROW + ix] = rec;
        sGuide[iy * RESPOND_ROW + ix] = g;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lx = (wave & 1) * 8 + (lane & 7), ly = (wave >> 1) * 8 + (lane >> 3);
    const int x = blockIdx.x * 16 + lx, y = blockIdx.y * 16 + ly;
    if (x >= a.w || y >= a.h) return;
    const size_t p = (size_t)y * a.w + x;
    float4 cur, raw;
    if (Source::load(a, p, cur, raw)) {
        a.outHist[p] = make_float4(raw.x, raw.y, raw.z, -1.0f);
        a.outLen[p] = 0.0f;
        if (r.outScale) r.outScale[p] = 1.0f;
        return;
    }
    const float4 eh = r.wsG[p];
    float4 res = cur;
    float len = 1.0f, lambda = 1.0f;
    if (eh.w != -1.0f) {                                      // a history was gathered (a NaN V_h is one too)
        const int c = (ly + rad) * RESPOND_ROW + lx + rad;
        const float4 own = sRec[c];
        if (own.w == own.w) {                                 // the pixel counts itself: it runs the test
            const float4 gp = sGuide[c];
            const float zLim = a.depthTol * gp.w;
            float dx_ = 0.0f, dy_ = 0.0f, dz_ = 0.0f, vs = 0.0f;
            for (int dy = -rad; dy <= rad; dy++)
                for (int dx = -rad; dx <= rad; dx++) {
                    const int k = c + dy * RESPOND_ROW + dx;
                    // (both 16-byte reads at once and selects, not branches: the sums start at +0 and never reach -0, so adding +0
                    // for a skipped pixel leaves them bit for bit what skipping it leaves; its values are never touched)
                    const float4 q = sRec[k], gq = sGuide[k];
                    const bool in = (q.w == q.w) & (fabsf(gq.w - gp.w) <= zLim) & (gp.x * gq.x + gp.y * gq.y + gp.z * gq.z >= a.normalTol);
                    dx_ += in ? q.x : 0.0f; dy_ += in ? q.y : 0.0f; dz_ += in ? q.z : 0.0f; vs += in ? q.w : 0.0f;
                }
            const float T = dx_ * dx_ + dy_ * dy_ + dz_ * dz_;
            const float lim = r.k2 * vs;
            if (T > lim) {
                const float rho = lim / T;
                lambda = r.power == 1 ? rho : (r.power == 2 ? rho * rho : (rho * rho) * (rho * rho));
            }
        }
        res = temporal_blend(cur, eh, lambda * r.wsN[p], a.maxHistory, len);
    }
    a.outHist[p] = res;
    a.outLen[p] = len;
    if (r.outScale) r.outScale[p] = lambda;
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
static TemporalArgs temporal_args(const TemporalCall& c) {
    const bool motion = c.motion && c.hist;
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
    return a;
}

static int temporal_launch(const TemporalCall& c, hipStream_t stream) {
    using Kernel = void (*)(TemporalArgs);
    static const Kernel table[2][2][2] = {
        {{temporal_kernel<FromSums, false, false, false>, temporal_kernel<FromSums, false, true, false>},
         {temporal_kernel<FromSums, true, false, false>, temporal_kernel<FromSums, true, true, false>}},
        {{temporal_kernel<FromCur, false, false, false>, temporal_kernel<FromCur, false, true, false>},
         {temporal_kernel<FromCur, true, false, false>, temporal_kernel<FromCur, true, true, false>}}};
    const bool motion = c.motion && c.hist;
    const Kernel kernel = c.tileLive ? temporal_kernel<FromSums, true, false, true> : table[c.fromCur][temporal_ident(c)][motion];
    hipLaunchKernelGGL(kernel, dim3((c.w + 15) / 16, (c.h + 15) / 16), dim3(256), 0, stream, temporal_args(c));
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

// ---- RESPOND, host side ------------------------------------------------------------------------------------------------------------
static size_t respond_workspace_bytes(int w, int h) { return (size_t)w * h * 36; }

int check_respond_params(const char* fn, const pt_respond_params& R) {       // (pt_preview.hip checks its option with it)
    if (R.radius < 1 || R.radius > RESPOND_MAX_RADIUS) return postfx_fail_fn(-1, fn, "radius %d must be 1..%d", R.radius, RESPOND_MAX_RADIUS);
    if (R.power != 1 && R.power != 2 && R.power != 4) return postfx_fail_fn(-1, fn, "power %d must be 1, 2 or 4", R.power);
    if (!(R.threshold > 0.0f)) return postfx_fail_fn(-1, fn, "threshold must be positive (+inf is allowed)");
    return 0;
}

// The call's own checks on top of check_temporal_call's; ws is NULL for a host form (it stages its own).
static int check_respond_call(const TemporalCall& c, const pt_respond_params& R, bool host, const void* ws, const void* outScale) {
    const char* fn = "pt_temporal_accumulate_respond";
    const bool sums = c.sum || c.sq || c.albedo;
    if (sums == (c.cur != nullptr))
        return postfx_fail_fn(-1, fn, "give exactly one frame form: rgba_sum, sq_sum and albedo, or cur");
    if (int r = check_temporal_call(c)) return r;
    if (int r = check_respond_params(fn, R)) return r;
    if (!host && !ws) return postfx_fail_fn(-1, fn, "null workspace");
    const size_t n = (size_t)c.w * c.h, b16 = n * 16, wsBytes = respond_workspace_bytes(c.w, c.h);
    const struct { const void* p; size_t bytes; } others[] = {{c.sum, b16}, {c.sq, b16}, {c.albedo, b16}, {c.cur, b16}, {c.nd, b16}, {c.prevNd, b16},
                                                              {c.hist, b16}, {c.histLen, n * 4}, {c.motion, b16}, {c.outHist, b16}, {c.outLen, n * 4}};
    for (const auto& o : others) {
        if (!o.p) continue;
        if (ws && overlaps(ws, wsBytes, o.p, o.bytes)) return postfx_fail_fn(-1, fn, "the workspace must not alias any other buffer");
        if (outScale && overlaps(outScale, n * 4, o.p, o.bytes)) return postfx_fail_fn(-1, fn, "out_scale must not alias any other buffer");
    }
    if (ws && outScale && overlaps(ws, wsBytes, outScale, n * 4)) return postfx_fail_fn(-1, fn, "the workspace must not alias out_scale");
    return 0;
}

// The two launches: the gather by source, identity and motion; the walk and the blend by source.
static int respond_launch(const TemporalCall& c, const pt_respond_params& R, void* ws, void* outScale, hipStream_t stream) {
    using Kernel = void (*)(RespondArgs);
    static const Kernel gather[2][2][2] = {
        {{temporal_gather_kernel<FromSums, false, false>, temporal_gather_kernel<FromSums, false, true>},
         {temporal_gather_kernel<FromSums, true, false>, temporal_gather_kernel<FromSums, true, true>}},
        {{temporal_gather_kernel<FromCur, false, false>, temporal_gather_kernel<FromCur, false, true>},
         {temporal_gather_kernel<FromCur, true, false>, temporal_gather_kernel<FromCur, true, true>}}};
    static const Kernel respond[2] = {temporal_respond_kernel<FromSums>, temporal_respond_kernel<FromCur>};
    const size_t n = (size_t)c.w * c.h;
    RespondArgs r = {};
    r.t = temporal_args(c);
    r.wsG = (float4*)ws; r.wsW = r.wsG + n; r.wsN = (float*)(r.wsW + n);
    r.radius = R.radius; r.power = R.power; r.k2 = R.threshold * R.threshold;
    r.outScale = (float*)outScale;
    const dim3 grid((c.w + 15) / 16, (c.h + 15) / 16);
    hipLaunchKernelGGL(gather[c.fromCur][temporal_ident(c)][r.t.motion != nullptr], grid, dim3(256), 0, stream, r);
    POSTFX_HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(respond[c.fromCur], grid, dim3(256), 0, stream, r);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

static int respond_run(TemporalCall c, const pt_respond_params* params, bool host, void* ws, void* outScale, hipStream_t stream) {
    pt_respond_params R;
    if (params) R = *params; else pt_respond_defaults(&R);
    c.fromCur = c.cur != nullptr;
    if (int r = check_respond_call(c, R, host, ws, outScale)) return r;
    if (!host) return respond_launch(c, R, ws, outScale, stream);
    const size_t n = (size_t)c.w * c.h, b16 = n * 16;
    const HostIn in[] = {{c.sum, b16}, {c.sq, b16}, {c.albedo, b16}, {c.cur, b16}, {c.nd, b16}, {c.prevNd, b16}, {c.hist, b16},
                         {c.histLen, n * 4}, {c.hist ? c.motion : nullptr, b16}};
    const HostOut out[] = {{c.outHist, b16}, {c.outLen, n * 4}, {outScale, n * 4}};
    return postfx_host_form(c.fn, respond_workspace_bytes(c.w, c.h), in, out, [&](char* dWs, char** dIn, char** dOut) {
        TemporalCall d = c;
        d.sum = dIn[0]; d.sq = dIn[1]; d.albedo = dIn[2]; d.cur = dIn[3]; d.nd = dIn[4]; d.prevNd = dIn[5]; d.hist = dIn[6]; d.histLen = dIn[7];
        d.motion = dIn[8];
        d.outHist = dOut[0]; d.outLen = dOut[1];
        return respond_launch(d, R, dWs, dOut[2], nullptr);
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

// ---- RESPOND: the base, _cur, _motion and _cur_motion forms with a per-pixel change test (see the header) ---------------------------
void pt_respond_defaults(pt_respond_params* out) {
    if (!out) return;
    out->radius = 3;                      // the pick of tests/respond_seq.py --sweep
    out->power = 4;
    out->threshold = 2.0f;
}

size_t pt_temporal_respond_workspace_bytes(int w, int h) { return w > 0 && h > 0 ? respond_workspace_bytes(w, h) : 0; }

int pt_temporal_accumulate_respond_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_rgba_sum, const void* d_sq_sum,
                                          int spp, int batches, const void* d_albedo, const void* d_cur, const void* d_normal_depth,
                                          const void* d_prev_normal_depth, const void* d_hist, const void* d_hist_len, const void* d_motion,
                                          const pt_temporal_params* params, const pt_respond_params* respond, void* d_workspace, void* d_out_hist,
                                          void* d_out_hist_len, void* d_out_scale, void* stream) {
    TemporalCall c = temporal_call("pt_temporal_accumulate_respond", w, h, cam, cam_prev, d_normal_depth, d_prev_normal_depth, d_hist, d_hist_len,
                                   params, d_out_hist, d_out_hist_len);
    c.cur = d_cur; c.motion = d_motion;
    return respond_run(from_sums(c, d_rgba_sum, d_sq_sum, spp, batches, d_albedo), respond, false, d_workspace, d_out_scale, (hipStream_t)stream);
}

int pt_temporal_accumulate_respond(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* rgba_sum, const float* sq_sum, int spp,
                                   int batches, const float* albedo, const float* cur, const float* normal_depth, const float* prev_normal_depth,
                                   const float* hist, const float* hist_len, const float* motion, const pt_temporal_params* params,
                                   const pt_respond_params* respond, float* out_hist, float* out_hist_len, float* out_scale) {
    TemporalCall c = temporal_call("pt_temporal_accumulate_respond", w, h, cam, cam_prev, normal_depth, prev_normal_depth, hist, hist_len, params,
                                   out_hist, out_hist_len);
    c.cur = cur; c.motion = motion;
    return respond_run(from_sums(c, rgba_sum, sq_sum, spp, batches, albedo), respond, true, nullptr, out_scale, nullptr);
}

}  // extern "C"
