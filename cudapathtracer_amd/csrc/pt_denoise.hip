// pt_denoise.hip — edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) on albedo-demodulated colour, guided by
// the first-hit feature buffers of pt_render_aovs (include/pt_api.h states the arithmetic; tests/denoise_ref.py restates it
// in numpy). Opt-in post-process: it is not part of the reference's image.
//
//   denoise_prepare_kernel   m = S / spp; pass-through flag; e = m / a (a = albedo where >= 0.01, else 1); the normalised mean
//                            normal and depth; per-workgroup luminance partial sums (fixed order: reproducible)
//   denoise_reduce_kernel    one workgroup: the mean luminance L of e over the filtered pixels
//   denoise_iter_kernel      one launch per step s = 2^i: the 5x5 B3-spline taps at stride s, weighted by colour, normal, depth
//   denoise_finish_kernel    out = spp * a * e, or S itself for pass-through pixels
//
// pt_denoise_var's kernels (the variance-guided colour weight) follow pt_denoise's below and share its reduction and workspace layout;
// pt_denoise_var_tiles' prepare and finish kernels (the sample count per 8x8 tile, an adaptive frame's map) follow those.
//
// Workspace (pt_denoise_workspace_bytes): e ping-pong (2 x w*h float4: rgb, w = 1 filtered / 0 pass-through), the normal-depth
// guide (w*h float4: unit normal or 0, depth), the partial sums (one float2 per 256 pixels) and the result of the reduction.
#include <algorithm>
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/pt_api.h"
#include "pt_denoise_shared.h"
#include "pt_postfx_host.h"

namespace pt {

constexpr int kDnBlock = 256;              // prepare / reduce / finish: one pixel per thread
constexpr int kDnMaxIterations = 16;

struct DnLayout {
    size_t n, e0, e1, guide, partials, lum, total;
    int nParts;
};
static DnLayout dn_layout(int w, int h) {
    DnLayout L;
    L.n = (size_t)w * h;
    L.nParts = (int)((L.n + kDnBlock - 1) / kDnBlock);
    L.e0 = 0;
    L.e1 = L.e0 + L.n * 16;
    L.guide = L.e1 + L.n * 16;
    L.partials = L.guide + L.n * 16;
    L.lum = L.partials + (((size_t)L.nParts * 8 + 15) & ~(size_t)15);
    L.total = L.lum + 16;
    return L;
}

__global__ void __launch_bounds__(kDnBlock) denoise_prepare_kernel(int n, const float4* __restrict__ sum, float spp, const float4* __restrict__ albedo,
                                                                   const float4* __restrict__ nd, float4* __restrict__ e, float4* __restrict__ guide,
                                                                   float2* __restrict__ partials) {
    __shared__ float sLum[kDnBlock], sCnt[kDnBlock];
    const int i = blockIdx.x * kDnBlock + threadIdx.x;
    float lum = 0.0f, cnt = 0.0f;
    if (i < n) {
        const float4 s = sum[i], a = albedo[i], g = nd[i];
        const float4 m = make_float4(s.x / spp, s.y / spp, s.z / spp, s.w / spp);
        const bool filtered = a.w > 0.0f && finite3(m);
        float4 ev = make_float4(m.x / demod_albedo(a.x), m.y / demod_albedo(a.y), m.z / demod_albedo(a.z), filtered ? 1.0f : 0.0f);
        e[i] = ev;
        const float len = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
        guide[i] = len > 0.0f ? make_float4(g.x / len, g.y / len, g.z / len, g.w) : make_float4(0.0f, 0.0f, 0.0f, g.w);
        if (filtered) { lum = 0.2126f * ev.x + 0.7152f * ev.y + 0.0722f * ev.z; cnt = 1.0f; }
    }
    sLum[threadIdx.x] = lum; sCnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int k = kDnBlock / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) { sLum[threadIdx.x] += sLum[threadIdx.x + k]; sCnt[threadIdx.x] += sCnt[threadIdx.x + k]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = make_float2(sLum[0], sCnt[0]);
}

// One workgroup; every thread sums a fixed stride of the partials, then a fixed tree: the same L on every run.
__global__ void __launch_bounds__(kDnBlock) denoise_reduce_kernel(int nParts, const float2* __restrict__ partials, float4* __restrict__ lum) {
    __shared__ double sLum[kDnBlock], sCnt[kDnBlock];
    double l = 0.0, c = 0.0;
    for (int k = threadIdx.x; k < nParts; k += kDnBlock) { l += partials[k].x; c += partials[k].y; }
    sLum[threadIdx.x] = l; sCnt[threadIdx.x] = c;
    __syncthreads();
    for (int k = kDnBlock / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) { sLum[threadIdx.x] += sLum[threadIdx.x + k]; sCnt[threadIdx.x] += sCnt[threadIdx.x + k]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) lum[0] = make_float4(sCnt[0] > 0.0 ? (float)(sLum[0] / sCnt[0]) : 0.0f, (float)sCnt[0], 0.0f, 0.0f);
}

// 16x16 pixels per workgroup as four 8x8 tiles, one per wave. Taps are plain cached float4 loads: at step s the 5x5 footprints
// of neighbouring pixels share most of their lines.
__global__ void __launch_bounds__(256) denoise_iter_kernel(int w, int h, int step, float colorScale, float sigmaNormal, float sigmaDepth,
                                                           const float4* __restrict__ lum, const float4* __restrict__ eIn,
                                                           const float4* __restrict__ guide, float4* __restrict__ eOut) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const float4 ep = eIn[p];
    if (ep.w == 0.0f) { eOut[p] = ep; return; }
    const float4 gp = guide[p];
    const bool normalP = gp.x != 0.0f || gp.y != 0.0f || gp.z != 0.0f;
    const float L = lum[0].x;
    // w_c = exp(-|de|^2 / (sigma_c^2 L^2 2^-i + 1e-20)), w_z = exp(-|dz| / (sigma_z z_p)), w_n = max(0, n.n')^sigma_n: one exp2 per tap
    const float log2e = 1.4426950408889634f;
    const float kc = log2e / (colorScale * L * L + 1e-20f), kz = log2e / (sigmaDepth * gp.w);
    const float hk[3] = {0.375f, 0.25f, 0.0625f};
    float sx = 0.140625f * ep.x, sy = 0.140625f * ep.y, sz = 0.140625f * ep.z, sw = 0.140625f;     // centre tap: h(0)^2
    if (normalP) {
        for (int dy = -2; dy <= 2; dy++) {
            const int yq = y + dy * step;
            if (yq < 0 || yq >= h) continue;
            for (int dx = -2; dx <= 2; dx++) {
                const int xq = x + dx * step;
                if (xq < 0 || xq >= w || (dx == 0 && dy == 0)) continue;
                const size_t q = (size_t)yq * w + xq;
                const float4 eq = eIn[q];
                if (eq.w == 0.0f) continue;
                const float4 gq = guide[q];
                if (gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f) continue;
                const float cs = gp.x * gq.x + gp.y * gq.y + gp.z * gq.z;
                float ln;
                if (sigmaNormal == 0.0f) ln = 0.0f;
                else if (cs > 0.0f) ln = sigmaNormal * __builtin_log2f(cs);
                else continue;
                const float dr = ep.x - eq.x, dg = ep.y - eq.y, db = ep.z - eq.z;
                const float dc = dr * dr + dg * dg + db * db, dz = fabsf(gp.w - gq.w);
                const float wt = (hk[dx < 0 ? -dx : dx] * hk[dy < 0 ? -dy : dy]) * __builtin_exp2f(ln - dc * kc - dz * kz);
                sx += wt * eq.x; sy += wt * eq.y; sz += wt * eq.z; sw += wt;
            }
        }
    }
    eOut[p] = make_float4(sx / sw, sy / sw, sz / sw, 1.0f);
}

__global__ void __launch_bounds__(kDnBlock) denoise_finish_kernel(int n, const float4* sum, float spp, const float4* __restrict__ albedo,
                                                                  const float4* __restrict__ e, float4* out) {
    const int i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= n) return;
    const float4 s = sum[i], ev = e[i];          // (out may alias sum: each thread reads its own pixel before it writes it)
    if (ev.w == 0.0f) { out[i] = s; return; }
    const float4 a = albedo[i];
    out[i] = make_float4(spp * (demod_albedo(a.x) * ev.x), spp * (demod_albedo(a.y) * ev.y), spp * (demod_albedo(a.z) * ev.z), s.w);
}

// ---- pt_denoise_var: the same filter with a variance-guided colour weight (include/pt_api.h) --------------------------------
// e.w carries the pixel's variance V of the demodulated mean (>= 0) or -1 for a pass-through pixel, so a tap is still one
// float4 of e and one of the guide.
//
//   denoise_var_prepare_kernel   as denoise_prepare_kernel, plus V from S and Q in f32 in the header's order
//   denoise_var_iter_kernel      the 3x3 binomial of V around p (plain cached loads of e.w: the step-1 taps of the same wave
//                                read those lines anyway), then the 5x5 taps; e' = sum w e / sum w, V' = sum w^2 V / (sum w)^2
//   denoise_var_finish_kernel    denoise_finish_kernel with the pass-through mark of this layout
__global__ void __launch_bounds__(kDnBlock) denoise_var_prepare_kernel(int n, const float4* __restrict__ sum, const float4* __restrict__ sq, float spp,
                                                                       float batches, const float4* __restrict__ albedo,
                                                                       const float4* __restrict__ nd, float4* __restrict__ e,
                                                                       float4* __restrict__ guide, float2* __restrict__ partials) {
    __shared__ float sLum[kDnBlock], sCnt[kDnBlock];
    const int i = blockIdx.x * kDnBlock + threadIdx.x;
    float lum = 0.0f, cnt = 0.0f;
    if (i < n) {
        float4 m;
        const float4 ev = dn_var_pixel(sum[i], sq[i], albedo[i], spp, batches, m);
        e[i] = ev;
        guide[i] = dn_unit_guide(nd[i]);
        if (ev.w >= 0.0f) { lum = 0.2126f * ev.x + 0.7152f * ev.y + 0.0722f * ev.z; cnt = 1.0f; }
    }
    sLum[threadIdx.x] = lum; sCnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int k = kDnBlock / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) { sLum[threadIdx.x] += sLum[threadIdx.x + k]; sCnt[threadIdx.x] += sCnt[threadIdx.x + k]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = make_float2(sLum[0], sCnt[0]);
}

// The launch shape of denoise_iter_kernel: 16x16 pixels per workgroup as four 8x8 tiles, one per wave.
__global__ void __launch_bounds__(256) denoise_var_iter_kernel(int w, int h, int step, float sigmaVar, float sigmaNormal, float sigmaDepth,
                                                               const float4* __restrict__ lum, const float4* __restrict__ eIn,
                                                               const float4* __restrict__ guide, float4* __restrict__ eOut) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const float4 ep = eIn[p];
    if (ep.w < 0.0f) { eOut[p] = ep; return; }
    const float4 gp = guide[p];
    const bool normalP = gp.x != 0.0f || gp.y != 0.0f || gp.z != 0.0f;
    const float hk[3] = {0.375f, 0.25f, 0.0625f};
    float sx = 0.140625f * ep.x, sy = 0.140625f * ep.y, sz = 0.140625f * ep.z, sw = 0.140625f;     // centre tap: h(0)^2
    float sv = (0.140625f * 0.140625f) * ep.w;
    if (normalP) {
        // the 3x3 binomial of V, (1, 2, 1) x (1, 2, 1) / 16 at stride 1: a neighbour outside the image or pass-through gives V_p
        float vt = 0.0f;
        for (int dy = -1; dy <= 1; dy++) {
            const int yq = y + dy;
            for (int dx = -1; dx <= 1; dx++) {
                const int xq = x + dx;
                float v = ep.w;
                if (yq >= 0 && yq < h && xq >= 0 && xq < w) {
                    const float vq = eIn[(size_t)yq * w + xq].w;
                    if (vq >= 0.0f) v = vq;
                }
                vt += ((dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f)) * v;
            }
        }
        // w_c = exp(-|de| / (sigma_var sqrt(Vt) + 1e-3 L + 1e-20)), w_z = exp(-|dz| / (sigma_z z_p)), w_n = max(0, n.n')^sigma_n: one exp2 per tap
        const float log2e = 1.4426950408889634f;
        const float kc = log2e / (sigmaVar * __builtin_sqrtf(vt) + 1e-3f * lum[0].x + 1e-20f), kz = log2e / (sigmaDepth * gp.w);
        for (int dy = -2; dy <= 2; dy++) {
            const int yq = y + dy * step;
            if (yq < 0 || yq >= h) continue;
            for (int dx = -2; dx <= 2; dx++) {
                const int xq = x + dx * step;
                if (xq < 0 || xq >= w || (dx == 0 && dy == 0)) continue;
                const size_t q = (size_t)yq * w + xq;
                const float4 eq = eIn[q];
                if (eq.w < 0.0f) continue;
                const float4 gq = guide[q];
                if (gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f) continue;
                const float cs = gp.x * gq.x + gp.y * gq.y + gp.z * gq.z;
                float ln;
                if (sigmaNormal == 0.0f) ln = 0.0f;
                else if (cs > 0.0f) ln = sigmaNormal * __builtin_log2f(cs);
                else continue;
                const float dr = ep.x - eq.x, dg = ep.y - eq.y, db = ep.z - eq.z;
                const float dc = __builtin_sqrtf(dr * dr + dg * dg + db * db), dz = fabsf(gp.w - gq.w);
                const float wt = (hk[dx < 0 ? -dx : dx] * hk[dy < 0 ? -dy : dy]) * __builtin_exp2f(ln - dc * kc - dz * kz);
                sx += wt * eq.x; sy += wt * eq.y; sz += wt * eq.z; sw += wt;
                sv += (wt * wt) * eq.w;
            }
        }
    }
    eOut[p] = make_float4(sx / sw, sy / sw, sz / sw, sv / (sw * sw));
}

__global__ void __launch_bounds__(kDnBlock) denoise_var_finish_kernel(int n, const float4* sum, float spp, const float4* __restrict__ albedo,
                                                                      const float4* __restrict__ e, float4* out) {
    const int i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= n) return;
    const float4 s = sum[i], ev = e[i];          // (out may alias sum: each thread reads its own pixel before it writes it)
    if (ev.w < 0.0f) { out[i] = s; return; }
    const float4 a = albedo[i];
    out[i] = make_float4(spp * (demod_albedo(a.x) * ev.x), spp * (demod_albedo(a.y) * ev.y), spp * (demod_albedo(a.z) * ev.z), s.w);
}

// ---- pt_denoise_var_tiles: pt_denoise_var on an adaptive frame (include/pt_api.h) --------------------------------------------
// spp and the batch count come per pixel from the frame's tile map, tile = (y / 8) * ceil(w / 8) + x / 8, as pt_resolve reads it;
// denoise_reduce_kernel and denoise_var_iter_kernel run unchanged on the same workspace.
//
//   denoise_var_tiles_prepare_kernel   denoise_var_prepare_kernel with spp_p = map[tile], B_p = spp_p / batch_spp
//   denoise_var_tiles_finish_kernel    denoise_var_finish_kernel with spp_p
// A thread is a pixel of the scan-line frame, so the 64 lanes of a wave read at most 9 entries of the map (8 where w is a
// multiple of 8): cached loads, 4 B against the pixel's 64 B. The map is trusted here: the host form checks it.
__device__ inline int dn_tile_spp(const int32_t* __restrict__ tileSpp, int i, int w, int tilesX) {
    const int y = i / w, x = i - y * w;
    return tileSpp[(y >> 3) * tilesX + (x >> 3)];
}

__global__ void __launch_bounds__(kDnBlock) denoise_var_tiles_prepare_kernel(int n, int w, int tilesX, const float4* __restrict__ sum,
                                                                             const float4* __restrict__ sq, const int32_t* __restrict__ tileSpp,
                                                                             int batchSpp, const float4* __restrict__ albedo,
                                                                             const float4* __restrict__ nd, float4* __restrict__ e,
                                                                             float4* __restrict__ guide, float2* __restrict__ partials) {
    __shared__ float sLum[kDnBlock], sCnt[kDnBlock];
    const int i = blockIdx.x * kDnBlock + threadIdx.x;
    float lum = 0.0f, cnt = 0.0f;
    if (i < n) {
        const int spp = dn_tile_spp(tileSpp, i, w, tilesX);
        float4 m;
        const float4 ev = dn_var_pixel(sum[i], sq[i], albedo[i], (float)spp, (float)(spp / batchSpp), m);
        e[i] = ev;
        guide[i] = dn_unit_guide(nd[i]);
        if (ev.w >= 0.0f) { lum = 0.2126f * ev.x + 0.7152f * ev.y + 0.0722f * ev.z; cnt = 1.0f; }
    }
    sLum[threadIdx.x] = lum; sCnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int k = kDnBlock / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) { sLum[threadIdx.x] += sLum[threadIdx.x + k]; sCnt[threadIdx.x] += sCnt[threadIdx.x + k]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = make_float2(sLum[0], sCnt[0]);
}

__global__ void __launch_bounds__(kDnBlock) denoise_var_tiles_finish_kernel(int n, int w, int tilesX, const float4* sum,
                                                                            const int32_t* __restrict__ tileSpp,
                                                                            const float4* __restrict__ albedo, const float4* __restrict__ e,
                                                                            float4* out) {
    const int i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= n) return;
    const float4 s = sum[i], ev = e[i];          // (out may alias sum: each thread reads its own pixel before it writes it)
    if (ev.w < 0.0f) { out[i] = s; return; }
    const float4 a = albedo[i];
    const float spp = (float)dn_tile_spp(tileSpp, i, w, tilesX);
    out[i] = make_float4(spp * (demod_albedo(a.x) * ev.x), spp * (demod_albedo(a.y) * ev.y), spp * (demod_albedo(a.z) * ev.z), s.w);
}

// ---- pt_denoise_hist: pt_denoise_var's filter on a history buffer of pt_temporal_accumulate (include/pt_api.h) -------------------
// (e, V) come from `hist` instead of S and Q; denoise_reduce_kernel and denoise_var_iter_kernel run unchanged on the same workspace.
//
//   denoise_hist_prepare_kernel   copy hist into the working buffer (a pixel whose e or V is not finite is marked pass-through
//                                 there), the normalised guide, the luminance partials
//   denoise_hist_finish_kernel    out = (a e, 0): the radiance MEAN; a pass-through pixel returns its hist.rgb
__global__ void __launch_bounds__(kDnBlock) denoise_hist_prepare_kernel(int n, const float4* __restrict__ hist, const float4* __restrict__ nd,
                                                                        float4* __restrict__ e, float4* __restrict__ guide,
                                                                        float2* __restrict__ partials) {
    __shared__ float sLum[kDnBlock], sCnt[kDnBlock];
    const int i = blockIdx.x * kDnBlock + threadIdx.x;
    float lum = 0.0f, cnt = 0.0f;
    if (i < n) {
        float4 ev = hist[i];
        const bool filtered = ev.w >= 0.0f && __builtin_isfinite(ev.w) && finite3(ev);
        if (!filtered) ev.w = -1.0f;
        e[i] = ev;
        guide[i] = dn_unit_guide(nd[i]);
        if (filtered) { lum = 0.2126f * ev.x + 0.7152f * ev.y + 0.0722f * ev.z; cnt = 1.0f; }
    }
    sLum[threadIdx.x] = lum; sCnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int k = kDnBlock / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) { sLum[threadIdx.x] += sLum[threadIdx.x + k]; sCnt[threadIdx.x] += sCnt[threadIdx.x + k]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = make_float2(sLum[0], sCnt[0]);
}

__global__ void __launch_bounds__(kDnBlock) denoise_hist_finish_kernel(int n, const float4* __restrict__ albedo, const float4* __restrict__ e,
                                                                       float4* __restrict__ out) {
    const int i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= n) return;
    const float4 ev = e[i];
    if (ev.w < 0.0f) { out[i] = make_float4(ev.x, ev.y, ev.z, 0.0f); return; }
    const float4 a = albedo[i];
    out[i] = make_float4(demod_albedo(a.x) * ev.x, demod_albedo(a.y) * ev.y, demod_albedo(a.z) * ev.z, 0.0f);
}

static int check_denoise_args(int w, int h, const void* in, int spp, const void* albedo, const void* nd, const pt_denoise_params& P,
                              const void* out) {
    if (int r = postfx_check_size("pt_denoise", w, h)) return r;
    if (spp <= 0) return postfx_fail(-1, "pt_denoise: spp %d must be positive", spp);
    if (!in || !albedo || !nd || !out) return postfx_fail(-1, "pt_denoise: null buffer");
    if (P.iterations < 0 || P.iterations > kDnMaxIterations) return postfx_fail(-1, "pt_denoise: iterations %d out of range 0..%d", P.iterations, kDnMaxIterations);
    if (!(P.sigma_color > 0.0f) || !std::isfinite(P.sigma_color)) return postfx_fail(-1, "pt_denoise: sigma_color must be positive and finite");
    if (!(P.sigma_normal >= 0.0f) || !std::isfinite(P.sigma_normal)) return postfx_fail(-1, "pt_denoise: sigma_normal must be >= 0 and finite");
    if (!(P.sigma_depth > 0.0f) || !std::isfinite(P.sigma_depth)) return postfx_fail(-1, "pt_denoise: sigma_depth must be positive and finite");
    return 0;
}

static int denoise_launch(int w, int h, const float4* in, int spp, const float4* albedo, const float4* nd, const pt_denoise_params& P,
                          char* ws, float4* out, hipStream_t stream) {
    const DnLayout L = dn_layout(w, h);
    float4* e[2] = {(float4*)(ws + L.e0), (float4*)(ws + L.e1)};
    float4* guide = (float4*)(ws + L.guide);
    float2* partials = (float2*)(ws + L.partials);
    float4* lum = (float4*)(ws + L.lum);
    const int n = (int)L.n;
    const float fspp = (float)spp;
    hipLaunchKernelGGL(denoise_prepare_kernel, dim3(L.nParts), dim3(kDnBlock), 0, stream, n, in, fspp, albedo, nd, e[0], guide, partials);
    POSTFX_HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(denoise_reduce_kernel, dim3(1), dim3(kDnBlock), 0, stream, L.nParts, partials, lum);
    POSTFX_HIP_OK(hipGetLastError());
    const dim3 grid((w + 15) / 16, (h + 15) / 16);
    for (int i = 0; i < P.iterations; i++) {
        const float colorScale = P.sigma_color * P.sigma_color * std::ldexp(1.0f, -i);
        hipLaunchKernelGGL(denoise_iter_kernel, grid, dim3(256), 0, stream, w, h, 1 << i, colorScale, P.sigma_normal, P.sigma_depth, lum,
                           e[i & 1], guide, e[(i + 1) & 1]);
        POSTFX_HIP_OK(hipGetLastError());
    }
    hipLaunchKernelGGL(denoise_finish_kernel, dim3(L.nParts), dim3(kDnBlock), 0, stream, n, in, fspp, albedo, e[P.iterations & 1], out);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

static int check_denoise_var_args(int w, int h, const void* in, const void* sq, int spp, int batches, const void* albedo, const void* nd,
                                  const pt_denoise_var_params& P, const void* out) {
    if (int r = postfx_check_size("pt_denoise_var", w, h)) return r;
    if (spp <= 0) return postfx_fail(-1, "pt_denoise_var: spp %d must be positive", spp);
    if (batches < 2) return postfx_fail(-1, "pt_denoise_var: batches %d must be at least 2", batches);
    if (spp % batches != 0) return postfx_fail(-1, "pt_denoise_var: batches %d must divide spp %d", batches, spp);
    if (!in || !sq || !albedo || !nd || !out) return postfx_fail(-1, "pt_denoise_var: null buffer");
    if (P.iterations < 0 || P.iterations > kDnMaxIterations) return postfx_fail(-1, "pt_denoise_var: iterations %d out of range 0..%d", P.iterations, kDnMaxIterations);
    if (!(P.sigma_var > 0.0f) || !std::isfinite(P.sigma_var)) return postfx_fail(-1, "pt_denoise_var: sigma_var must be positive and finite");
    if (!(P.sigma_normal >= 0.0f) || !std::isfinite(P.sigma_normal)) return postfx_fail(-1, "pt_denoise_var: sigma_normal must be >= 0 and finite");
    if (!(P.sigma_depth > 0.0f) || !std::isfinite(P.sigma_depth)) return postfx_fail(-1, "pt_denoise_var: sigma_depth must be positive and finite");
    return 0;
}

static int denoise_var_launch(int w, int h, const float4* in, const float4* sq, int spp, int batches, const float4* albedo, const float4* nd,
                              const pt_denoise_var_params& P, char* ws, float4* out, hipStream_t stream) {
    const DnLayout L = dn_layout(w, h);
    float4* e[2] = {(float4*)(ws + L.e0), (float4*)(ws + L.e1)};
    float4* guide = (float4*)(ws + L.guide);
    float2* partials = (float2*)(ws + L.partials);
    float4* lum = (float4*)(ws + L.lum);
    const int n = (int)L.n;
    const float fspp = (float)spp;
    hipLaunchKernelGGL(denoise_var_prepare_kernel, dim3(L.nParts), dim3(kDnBlock), 0, stream, n, in, sq, fspp, (float)batches, albedo, nd, e[0], guide,
                       partials);
    POSTFX_HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(denoise_reduce_kernel, dim3(1), dim3(kDnBlock), 0, stream, L.nParts, partials, lum);
    POSTFX_HIP_OK(hipGetLastError());
    const dim3 grid((w + 15) / 16, (h + 15) / 16);
    for (int i = 0; i < P.iterations; i++) {
        hipLaunchKernelGGL(denoise_var_iter_kernel, grid, dim3(256), 0, stream, w, h, 1 << i, P.sigma_var, P.sigma_normal, P.sigma_depth, lum,
                           e[i & 1], guide, e[(i + 1) & 1]);
        POSTFX_HIP_OK(hipGetLastError());
    }
    hipLaunchKernelGGL(denoise_var_finish_kernel, dim3(L.nParts), dim3(kDnBlock), 0, stream, n, in, fspp, albedo, e[P.iterations & 1], out);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

// pt_denoise_var's checks that do not concern spp / batches, then batch_spp and the map's pointer.
static int check_denoise_var_tiles_args(int w, int h, const void* in, const void* sq, const void* tileSpp, int batchSpp, const void* albedo,
                                        const void* nd, const pt_denoise_var_params& P, const void* out) {
    if (int r = check_denoise_var_args(w, h, in, sq, 2, 2, albedo, nd, P, out)) return r;
    if (batchSpp < 1) return postfx_fail(-1, "pt_denoise_var_tiles: batch_spp %d must be positive", batchSpp);
    if (!tileSpp) return postfx_fail(-1, "pt_denoise_var_tiles: null tile map");
    return 0;
}

static int denoise_var_tiles_launch(int w, int h, const float4* in, const float4* sq, const int32_t* tileSpp, int batchSpp, const float4* albedo,
                                    const float4* nd, const pt_denoise_var_params& P, char* ws, float4* out, hipStream_t stream) {
    const DnLayout L = dn_layout(w, h);
    float4* e[2] = {(float4*)(ws + L.e0), (float4*)(ws + L.e1)};
    float4* guide = (float4*)(ws + L.guide);
    float2* partials = (float2*)(ws + L.partials);
    float4* lum = (float4*)(ws + L.lum);
    const int n = (int)L.n, tilesX = (w + 7) / 8;
    hipLaunchKernelGGL(denoise_var_tiles_prepare_kernel, dim3(L.nParts), dim3(kDnBlock), 0, stream, n, w, tilesX, in, sq, tileSpp, batchSpp, albedo,
                       nd, e[0], guide, partials);
    POSTFX_HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(denoise_reduce_kernel, dim3(1), dim3(kDnBlock), 0, stream, L.nParts, partials, lum);
    POSTFX_HIP_OK(hipGetLastError());
    const dim3 grid((w + 15) / 16, (h + 15) / 16);
    for (int i = 0; i < P.iterations; i++) {
        hipLaunchKernelGGL(denoise_var_iter_kernel, grid, dim3(256), 0, stream, w, h, 1 << i, P.sigma_var, P.sigma_normal, P.sigma_depth, lum,
                           e[i & 1], guide, e[(i + 1) & 1]);
        POSTFX_HIP_OK(hipGetLastError());
    }
    hipLaunchKernelGGL(denoise_var_tiles_finish_kernel, dim3(L.nParts), dim3(kDnBlock), 0, stream, n, w, tilesX, in, tileSpp, albedo,
                       e[P.iterations & 1], out);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

static int check_denoise_hist_args(int w, int h, const void* hist, const void* albedo, const void* nd, const pt_denoise_var_params& P, const void* out) {
    if (int r = postfx_check_size("pt_denoise_hist", w, h)) return r;
    if (!hist || !albedo || !nd || !out) return postfx_fail(-1, "pt_denoise_hist: null buffer");
    if (P.iterations < 0 || P.iterations > kDnMaxIterations) return postfx_fail(-1, "pt_denoise_hist: iterations %d out of range 0..%d", P.iterations, kDnMaxIterations);
    if (!(P.sigma_var > 0.0f) || !std::isfinite(P.sigma_var)) return postfx_fail(-1, "pt_denoise_hist: sigma_var must be positive and finite");
    if (!(P.sigma_normal >= 0.0f) || !std::isfinite(P.sigma_normal)) return postfx_fail(-1, "pt_denoise_hist: sigma_normal must be >= 0 and finite");
    if (!(P.sigma_depth > 0.0f) || !std::isfinite(P.sigma_depth)) return postfx_fail(-1, "pt_denoise_hist: sigma_depth must be positive and finite");
    return 0;
}

static int denoise_hist_launch(int w, int h, const float4* hist, const float4* albedo, const float4* nd, const pt_denoise_var_params& P, char* ws,
                               float4* out, hipStream_t stream) {
    const DnLayout L = dn_layout(w, h);
    float4* e[2] = {(float4*)(ws + L.e0), (float4*)(ws + L.e1)};
    float4* guide = (float4*)(ws + L.guide);
    float2* partials = (float2*)(ws + L.partials);
    float4* lum = (float4*)(ws + L.lum);
    const int n = (int)L.n;
    hipLaunchKernelGGL(denoise_hist_prepare_kernel, dim3(L.nParts), dim3(kDnBlock), 0, stream, n, hist, nd, e[0], guide, partials);
    POSTFX_HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(denoise_reduce_kernel, dim3(1), dim3(kDnBlock), 0, stream, L.nParts, partials, lum);
    POSTFX_HIP_OK(hipGetLastError());
    const dim3 grid((w + 15) / 16, (h + 15) / 16);
    for (int i = 0; i < P.iterations; i++) {
        hipLaunchKernelGGL(denoise_var_iter_kernel, grid, dim3(256), 0, stream, w, h, 1 << i, P.sigma_var, P.sigma_normal, P.sigma_depth, lum,
                           e[i & 1], guide, e[(i + 1) & 1]);
        POSTFX_HIP_OK(hipGetLastError());
    }
    hipLaunchKernelGGL(denoise_hist_finish_kernel, dim3(L.nParts), dim3(kDnBlock), 0, stream, n, albedo, e[P.iterations & 1], out);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace pt

using namespace pt;

extern "C" {

void pt_denoise_defaults(pt_denoise_params* out) {
    if (!out) return;
    out->iterations = 5;
    out->sigma_color = 1.0f;
    out->sigma_normal = 64.0f;
    out->sigma_depth = 0.02f;
}

size_t pt_denoise_workspace_bytes(int w, int h) {
    if (w <= 0 || h <= 0) return 0;
    return dn_layout(w, h).total;
}

int pt_denoise_device(int w, int h, const void* d_rgba_sum, int spp, const void* d_albedo, const void* d_normal_depth,
                      const pt_denoise_params* params, void* d_workspace, void* d_out, void* stream) {
    pt_denoise_params P;
    if (params) P = *params; else pt_denoise_defaults(&P);
    if (int r = check_denoise_args(w, h, d_rgba_sum, spp, d_albedo, d_normal_depth, P, d_out)) return r;
    if (!d_workspace) return pt_fail_(-1, "pt_denoise_device: null workspace");
    return denoise_launch(w, h, (const float4*)d_rgba_sum, spp, (const float4*)d_albedo, (const float4*)d_normal_depth, P, (char*)d_workspace,
                          (float4*)d_out, (hipStream_t)stream);
}

int pt_denoise(int w, int h, const float* rgba_sum, int spp, const float* albedo, const float* normal_depth, const pt_denoise_params* params,
               float* out_rgba_sum) {
    pt_denoise_params P;
    if (params) P = *params; else pt_denoise_defaults(&P);
    if (int r = check_denoise_args(w, h, rgba_sum, spp, albedo, normal_depth, P, out_rgba_sum)) return r;
    const size_t bytes = (size_t)w * h * 16;
    const HostIn in[] = {{rgba_sum, bytes}, {albedo, bytes}, {normal_depth, bytes}};
    const HostOut out[] = {{out_rgba_sum, bytes, 0}};          // in and out share one buffer (out may alias in)
    return postfx_host_form("pt_denoise", dn_layout(w, h).total, in, out, [&](char* ws, char** d, char**) {
        return denoise_launch(w, h, (const float4*)d[0], spp, (const float4*)d[1], (const float4*)d[2], P, ws, (float4*)d[0], nullptr);
    });
}

void pt_denoise_var_defaults(pt_denoise_var_params* out) {
    if (!out) return;
    out->iterations = 3;
    out->sigma_var = 6.0f;
    out->sigma_normal = 64.0f;
    out->sigma_depth = 0.02f;
}

size_t pt_denoise_var_workspace_bytes(int w, int h) {
    if (w <= 0 || h <= 0) return 0;
    return dn_layout(w, h).total;
}

int pt_denoise_var_device(int w, int h, const void* d_rgba_sum, const void* d_sq_sum, int spp, int batches, const void* d_albedo,
                          const void* d_normal_depth, const pt_denoise_var_params* params, void* d_workspace, void* d_out, void* stream) {
    pt_denoise_var_params P;
    if (params) P = *params; else pt_denoise_var_defaults(&P);
    if (int r = check_denoise_var_args(w, h, d_rgba_sum, d_sq_sum, spp, batches, d_albedo, d_normal_depth, P, d_out)) return r;
    if (!d_workspace) return pt_fail_(-1, "pt_denoise_var_device: null workspace");
    return denoise_var_launch(w, h, (const float4*)d_rgba_sum, (const float4*)d_sq_sum, spp, batches, (const float4*)d_albedo,
                              (const float4*)d_normal_depth, P, (char*)d_workspace, (float4*)d_out, (hipStream_t)stream);
}

int pt_denoise_var(int w, int h, const float* rgba_sum, const float* sq_sum, int spp, int batches, const float* albedo, const float* normal_depth,
                   const pt_denoise_var_params* params, float* out_rgba_sum) {
    pt_denoise_var_params P;
    if (params) P = *params; else pt_denoise_var_defaults(&P);
    if (int r = check_denoise_var_args(w, h, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, P, out_rgba_sum)) return r;
    const size_t bytes = (size_t)w * h * 16;
    const HostIn in[] = {{rgba_sum, bytes}, {sq_sum, bytes}, {albedo, bytes}, {normal_depth, bytes}};
    const HostOut out[] = {{out_rgba_sum, bytes, 0}};          // in and out share one buffer (out may alias in)
    return postfx_host_form("pt_denoise_var", dn_layout(w, h).total, in, out, [&](char* ws, char** d, char**) {
        return denoise_var_launch(w, h, (const float4*)d[0], (const float4*)d[1], spp, batches, (const float4*)d[2], (const float4*)d[3], P, ws,
                                  (float4*)d[0], nullptr);
    });
}

size_t pt_denoise_var_tiles_workspace_bytes(int w, int h) {
    if (w <= 0 || h <= 0) return 0;
    return dn_layout(w, h).total;
}

int pt_denoise_var_tiles_device(int w, int h, const void* d_rgba_sum, const void* d_sq_sum, const void* d_tile_spp, int batch_spp,
                                const void* d_albedo, const void* d_normal_depth, const pt_denoise_var_params* params, void* d_workspace,
                                void* d_out, void* stream) {
    pt_denoise_var_params P;
    if (params) P = *params; else pt_denoise_var_defaults(&P);
    if (int r = check_denoise_var_tiles_args(w, h, d_rgba_sum, d_sq_sum, d_tile_spp, batch_spp, d_albedo, d_normal_depth, P, d_out)) return r;
    if (!d_workspace) return pt_fail_(-1, "pt_denoise_var_tiles_device: null workspace");
    return denoise_var_tiles_launch(w, h, (const float4*)d_rgba_sum, (const float4*)d_sq_sum, (const int32_t*)d_tile_spp, batch_spp,
                                    (const float4*)d_albedo, (const float4*)d_normal_depth, P, (char*)d_workspace, (float4*)d_out,
                                    (hipStream_t)stream);
}

int pt_denoise_var_tiles(int w, int h, const float* rgba_sum, const float* sq_sum, const int32_t* tile_spp, int batch_spp, const float* albedo,
                         const float* normal_depth, const pt_denoise_var_params* params, float* out_rgba_sum) {
    pt_denoise_var_params P;
    if (params) P = *params; else pt_denoise_var_defaults(&P);
    if (int r = check_denoise_var_tiles_args(w, h, rgba_sum, sq_sum, tile_spp, batch_spp, albedo, normal_depth, P, out_rgba_sum)) return r;
    const int T = ((w + 7) / 8) * ((h + 7) / 8);
    for (int t = 0; t < T; t++)
        if (tile_spp[t] <= 0 || tile_spp[t] % batch_spp != 0 || tile_spp[t] < 2 * batch_spp)
            return postfx_fail(-1, "pt_denoise_var_tiles: tile_spp[%d] = %d must be a positive multiple of batch_spp that gives at least 2 batches", t,
                           tile_spp[t]);
    const size_t bytes = (size_t)w * h * 16;
    const HostIn in[] = {{rgba_sum, bytes}, {sq_sum, bytes}, {albedo, bytes}, {normal_depth, bytes}, {tile_spp, (size_t)T * sizeof(int32_t)}};
    const HostOut out[] = {{out_rgba_sum, bytes, 0}};          // in and out share one buffer (out may alias in)
    return postfx_host_form("pt_denoise_var_tiles", dn_layout(w, h).total, in, out, [&](char* ws, char** d, char**) {
        return denoise_var_tiles_launch(w, h, (const float4*)d[0], (const float4*)d[1], (const int32_t*)d[4], batch_spp, (const float4*)d[2],
                                        (const float4*)d[3], P, ws, (float4*)d[0], nullptr);
    });
}

size_t pt_denoise_hist_workspace_bytes(int w, int h) {
    if (w <= 0 || h <= 0) return 0;
    return dn_layout(w, h).total;
}

int pt_denoise_hist_device(int w, int h, const void* d_hist, const void* d_albedo, const void* d_normal_depth, const pt_denoise_var_params* params,
                           void* d_workspace, void* d_out, void* stream) {
    pt_denoise_var_params P;
    if (params) P = *params; else pt_denoise_var_defaults(&P);
    if (int r = check_denoise_hist_args(w, h, d_hist, d_albedo, d_normal_depth, P, d_out)) return r;
    if (!d_workspace) return pt_fail_(-1, "pt_denoise_hist_device: null workspace");
    return denoise_hist_launch(w, h, (const float4*)d_hist, (const float4*)d_albedo, (const float4*)d_normal_depth, P, (char*)d_workspace,
                               (float4*)d_out, (hipStream_t)stream);
}

int pt_denoise_hist(int w, int h, const float* hist, const float* albedo, const float* normal_depth, const pt_denoise_var_params* params,
                    float* out_rgba_mean) {
    pt_denoise_var_params P;
    if (params) P = *params; else pt_denoise_var_defaults(&P);
    if (int r = check_denoise_hist_args(w, h, hist, albedo, normal_depth, P, out_rgba_mean)) return r;
    const size_t bytes = (size_t)w * h * 16;
    const HostIn in[] = {{hist, bytes}, {albedo, bytes}, {normal_depth, bytes}};
    const HostOut out[] = {{out_rgba_mean, bytes, 0}};         // hist and out share one buffer (out may alias hist)
    return postfx_host_form("pt_denoise_hist", dn_layout(w, h).total, in, out, [&](char* ws, char** d, char**) {
        return denoise_hist_launch(w, h, (const float4*)d[0], (const float4*)d[1], (const float4*)d[2], P, ws, (float4*)d[0], nullptr);
    });
}

}  // extern "C"
