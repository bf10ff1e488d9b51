// pt_denoise.hip — edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) on albedo-demodulated colour, guided by
// the first-hit feature buffers of pt_render_aovs (include/pt_api.h states the arithmetic; tests/denoise_ref.py and
// tests/denoise_var_ref.py restate it in numpy). Opt-in post-process: it is not part of the reference's image.
//
// Four filters share one chain of kernels. A Source is what tells them apart outside the taps, a Weight inside them:
//   dn_prepare_kernel<Source>   the pixel's working value e (Source::load), the normalised mean normal and depth (dn_unit_guide),
//                               per-workgroup luminance partial sums of the filtered pixels (fixed order: reproducible)
//   denoise_reduce_kernel       one workgroup: the mean luminance L of e over the filtered pixels
//   dn_atrous_kernel<Weight>    one launch per step s = 2^i: the 5x5 B3-spline taps at stride s, weighted by colour, normal, depth
//   dn_finish_kernel<Source>    out = scale * (a * e) (a = albedo where >= 0.01, else 1), or Source::raw for a pass-through pixel
//       Source    SumSource       pt_denoise: e = (S / spp) / a; e.w = 1 filtered / 0 pass-through; out = spp a e, or S itself
//                 VarSource       pt_denoise_var: e.w carries the variance V of e from S and Q (dn_var_pixel), -1 for pass-through
//                 VarTilesSource  pt_denoise_var_tiles: VarSource with spp and the batch count per pixel from an adaptive frame's map
//                 HistSource      pt_denoise_hist: (e, V) are a history buffer of pt_temporal_accumulate; out = (a e, 0), the MEAN
//       Weight    ColorWeight     w_c = exp(-|de|^2 / (sigma_color^2 L^2 2^-i + 1e-20)); e.w stays a flag
//                 VarianceWeight  w_c = exp(-|de| / (sigma_var sqrt(Vt) + 1e-3 L + 1e-20)), Vt the 3x3 binomial of V; V is filtered
//                                 along with e: e' = sum w e / sum w, V' = sum w^2 V / (sum w)^2
// Host side: every entry point fills a DnCall; dn_run checks it (check_dn_call) and launches it (dn_launch) on the caller's buffers
// or, for a host form, on staged copies (postfx_host_form).
//
// Workspace (pt_denoise_workspace_bytes): e ping-pong (2 x w*h float4), the normal-depth guide (w*h float4: unit normal or 0,
// depth), the partial sums (one float2 per 256 pixels) and the result of the reduction.
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

// Everything a launch hands the prepare and the finish kernel. A pointer the instantiation does not use is NULL and never read.
struct DnArgs {
    int n, w, tilesX;
    const float4 *in, *sq;                    // S (HistSource: the history) and Q
    const int32_t* tileSpp;                   // VarTilesSource
    float spp, batches;
    int batchSpp;
    const float4 *albedo, *nd;
    float4 *e, *guide;                        // prepare writes e, finish reads it
    float2* partials;
    float4* out;
};

// A thread is a pixel of the scan-line frame, tile = (y / 8) * ceil(w / 8) + x / 8 as pt_resolve reads the map, so the 64 lanes of
// a wave read at most 9 entries of it (8 where w is a multiple of 8): cached loads, 4 B against the pixel's 64 B. The map is
// trusted here: the host form checks it.
__device__ inline int dn_tile_spp(const int32_t* __restrict__ tileSpp, int i, int w, int tilesX) {
    const int y = i / w, x = i - y * w;
    return tileSpp[(y >> 3) * tilesX + (x >> 3)];
}

// The two colour weights of the taps: which e.w marks a pass-through pixel, whether e.w is a variance that is filtered with e,
// kc = log2(e) / (the weight's denominator) and the colour distance from |de|^2.
struct ColorWeight {
    static constexpr bool kVariance = false;
    static __device__ inline bool skip(float w) { return w == 0.0f; }
    static __device__ inline float kc(float colorScale, float L, float) { return 1.4426950408889634f / (colorScale * L * L + 1e-20f); }
    static __device__ inline float distance(float d2) { return d2; }
};
struct VarianceWeight {
    static constexpr bool kVariance = true;
    static __device__ inline bool skip(float w) { return w < 0.0f; }
    static __device__ inline float kc(float sigmaVar, float L, float vt) {
        return 1.4426950408889634f / (sigmaVar * __builtin_sqrtf(vt) + 1e-3f * L + 1e-20f);
    }
    static __device__ inline float distance(float d2) { return __builtin_sqrtf(d2); }
};

// The four sources. load: the working pixel for dn_prepare_kernel and whether it is filtered. raw: what dn_finish_kernel writes for
// a pass-through pixel; its w is the w of every result. scale: what a filtered pixel's a * e is multiplied by.
struct SumSource {
    using Weight = ColorWeight;
    static __device__ inline float4 load(const DnArgs& a, int i, bool& filtered) {
        const float4 s = a.in[i], al = a.albedo[i];
        const float4 m = make_float4(s.x / a.spp, s.y / a.spp, s.z / a.spp, s.w / a.spp);
        filtered = al.w > 0.0f && finite3(m);
        return make_float4(m.x / demod_albedo(al.x), m.y / demod_albedo(al.y), m.z / demod_albedo(al.z), filtered ? 1.0f : 0.0f);
    }
    static __device__ inline float4 raw(const DnArgs& a, int i, float4) { return a.in[i]; }
    static __device__ inline float scale(const DnArgs& a, int) { return a.spp; }
};
struct VarSource : SumSource {
    using Weight = VarianceWeight;
    static __device__ inline float4 load(const DnArgs& a, int i, bool& filtered) {
        float4 m;
        const float4 ev = dn_var_pixel(a.in[i], a.sq[i], a.albedo[i], a.spp, a.batches, m);
        filtered = ev.w >= 0.0f;
        return ev;
    }
};
struct VarTilesSource : VarSource {               // spp_p = map[tile], B_p = spp_p / batch_spp
    static __device__ inline float4 load(const DnArgs& a, int i, bool& filtered) {
        const int spp = dn_tile_spp(a.tileSpp, i, a.w, a.tilesX);
        float4 m;
        const float4 ev = dn_var_pixel(a.in[i], a.sq[i], a.albedo[i], (float)spp, (float)(spp / a.batchSpp), m);
        filtered = ev.w >= 0.0f;
        return ev;
    }
    static __device__ inline float scale(const DnArgs& a, int i) { return (float)dn_tile_spp(a.tileSpp, i, a.w, a.tilesX); }
};
struct HistSource {                               // a pixel whose e or V is not finite is marked pass-through in the working buffer
    using Weight = VarianceWeight;
    static __device__ inline float4 load(const DnArgs& a, int i, bool& filtered) {
        float4 ev = a.in[i];
        filtered = ev.w >= 0.0f && __builtin_isfinite(ev.w) && finite3(ev);
        if (!filtered) ev.w = -1.0f;
        return ev;
    }
    static __device__ inline float4 raw(const DnArgs&, int, float4 ev) { return make_float4(ev.x, ev.y, ev.z, 0.0f); }
    static __device__ inline float scale(const DnArgs&, int) { return 1.0f; }      // (1 * x is x: the mean a e itself, exactly)
};

template <class Source>
__global__ void __launch_bounds__(kDnBlock) dn_prepare_kernel(DnArgs a) {
    __shared__ float sLum[kDnBlock], sCnt[kDnBlock];
    const int i = blockIdx.x * kDnBlock + threadIdx.x;
    float lum = 0.0f, cnt = 0.0f;
    if (i < a.n) {
        bool filtered;
        const float4 ev = Source::load(a, i, filtered);
        a.e[i] = ev;
        a.guide[i] = dn_unit_guide(a.nd[i]);
        if (filtered) { lum = 0.2126f * ev.x + 0.7152f * ev.y + 0.0722f * ev.z; cnt = 1.0f; }
    }
    sLum[threadIdx.x] = lum; sCnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int k = kDnBlock / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) { sLum[threadIdx.x] += sLum[threadIdx.x + k]; sCnt[threadIdx.x] += sCnt[threadIdx.x + k]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) a.partials[blockIdx.x] = make_float2(sLum[0], sCnt[0]);
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
// of neighbouring pixels share most of their lines (and the 3x3 of V reads e.w from lines the step-1 taps of the same wave read
// anyway). `sigma` is the Weight's: sigma_color^2 2^-i or sigma_var.
template <class Weight>
__global__ void __launch_bounds__(256) dn_atrous_kernel(int w, int h, int step, float sigma, float sigmaNormal, float sigmaDepth,
                                                        const float4* __restrict__ lum, const float4* __restrict__ eIn,
                                                        const float4* __restrict__ guide, float4* __restrict__ eOut) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const float4 ep = eIn[p];
    if (Weight::skip(ep.w)) { eOut[p] = ep; return; }
    const float4 gp = guide[p];
    const bool normalP = gp.x != 0.0f || gp.y != 0.0f || gp.z != 0.0f;
    const float hk[3] = {0.375f, 0.25f, 0.0625f};
    float sx = 0.140625f * ep.x, sy = 0.140625f * ep.y, sz = 0.140625f * ep.z, sw = 0.140625f;     // centre tap: h(0)^2
    float sv = (0.140625f * 0.140625f) * ep.w;
    if (normalP) {
        // the 3x3 binomial of V, (1, 2, 1) x (1, 2, 1) / 16 at stride 1: a neighbour outside the image or pass-through gives V_p
        float vt = 0.0f;
        if (Weight::kVariance) {
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
        }
        // w_c = exp(-distance kc), w_z = exp(-|dz| / (sigma_z z_p)), w_n = max(0, n.n')^sigma_n: one exp2 per tap
        const float kc = Weight::kc(sigma, lum[0].x, vt), kz = 1.4426950408889634f / (sigmaDepth * gp.w);
        for (int dy = -2; dy <= 2; dy++) {
            const int yq = y + dy * step;
            if (yq < 0 || yq >= h) continue;
            for (int dx = -2; dx <= 2; dx++) {
                const int xq = x + dx * step;
                if (xq < 0 || xq >= w || (dx == 0 && dy == 0)) continue;
                const size_t q = (size_t)yq * w + xq;
                const float4 eq = eIn[q];
                if (Weight::skip(eq.w)) continue;
                const float4 gq = guide[q];
                if (gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f) continue;
                const float cs = gp.x * gq.x + gp.y * gq.y + gp.z * gq.z;
                float ln;
                if (sigmaNormal == 0.0f) ln = 0.0f;
                else if (cs > 0.0f) ln = sigmaNormal * __builtin_log2f(cs);
                else continue;
                const float dr = ep.x - eq.x, dg = ep.y - eq.y, db = ep.z - eq.z;
                const float dc = Weight::distance(dr * dr + dg * dg + db * db), dz = fabsf(gp.w - gq.w);
                const float wt = (hk[dx < 0 ? -dx : dx] * hk[dy < 0 ? -dy : dy]) * __builtin_exp2f(ln - dc * kc - dz * kz);
                sx += wt * eq.x; sy += wt * eq.y; sz += wt * eq.z; sw += wt;
                if (Weight::kVariance) sv += (wt * wt) * eq.w;
            }
        }
    }
    eOut[p] = make_float4(sx / sw, sy / sw, sz / sw, Weight::kVariance ? sv / (sw * sw) : 1.0f);
}

template <class Source>
__global__ void __launch_bounds__(kDnBlock) dn_finish_kernel(DnArgs a) {
    const int i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= a.n) return;
    const float4 ev = a.e[i];
    const float4 s = Source::raw(a, i, ev);      // (out may alias in: each thread reads its own pixel before it writes it)
    if (Source::Weight::skip(ev.w)) { a.out[i] = s; return; }
    const float4 al = a.albedo[i];
    const float k = Source::scale(a, i);
    a.out[i] = make_float4(k * (demod_albedo(al.x) * ev.x), k * (demod_albedo(al.y) * ev.y), k * (demod_albedo(al.z) * ev.z), s.w);
}

// One call of any of the eight filter entry points, on host or on device buffers.
enum DnKind { kDnSum, kDnVar, kDnVarTiles, kDnHist };
struct DnCall {
    const char* fn;                           // the entry point's host form, for its messages
    DnKind kind;
    int w, h;
    const void *in, *sq;                      // S (kDnHist: the history); Q for the two kDnVar* kinds
    int spp, batches;                         // kDnSum: spp; kDnVar: both
    const void* tileSpp;                      // kDnVarTiles
    int batchSpp;
    const void *albedo, *nd;
    int iterations;
    float sigma, sigmaNormal, sigmaDepth;     // sigma: sigma_color (kDnSum) or sigma_var
    void *ws, *out;
};

static DnCall dn_call(const char* fn, DnKind kind, int w, int h, const void* in, const void* albedo, const void* nd,
                      const pt_denoise_var_params* params, void* ws, void* out) {
    pt_denoise_var_params P;
    if (params) P = *params; else pt_denoise_var_defaults(&P);
    DnCall c = {};
    c.fn = fn; c.kind = kind; c.w = w; c.h = h; c.in = in; c.albedo = albedo; c.nd = nd; c.ws = ws; c.out = out;
    c.iterations = P.iterations; c.sigma = P.sigma_var; c.sigmaNormal = P.sigma_normal; c.sigmaDepth = P.sigma_depth;
    return c;
}

// All of a call's checks, before the first HIP call. The shared checks of pt_denoise_var_tiles speak as pt_denoise_var's.
static int check_dn_call(const DnCall& c, bool host) {
    const char* fn = c.kind == kDnSum ? "pt_denoise" : c.kind == kDnHist ? "pt_denoise_hist" : "pt_denoise_var";
    const bool needSq = c.kind == kDnVar || c.kind == kDnVarTiles;
    if (int r = postfx_check_size(fn, c.w, c.h)) return r;
    if ((c.kind == kDnSum || c.kind == kDnVar) && c.spp <= 0) return postfx_fail_fn(-1, fn, "spp %d must be positive", c.spp);
    if (c.kind == kDnVar) {
        if (c.batches < 2) return postfx_fail_fn(-1, fn, "batches %d must be at least 2", c.batches);
        if (c.spp % c.batches != 0) return postfx_fail_fn(-1, fn, "batches %d must divide spp %d", c.batches, c.spp);
    }
    if (!c.in || (needSq && !c.sq) || !c.albedo || !c.nd || !c.out) return postfx_fail_fn(-1, fn, "null buffer");
    if (c.iterations < 0 || c.iterations > kDnMaxIterations)
        return postfx_fail_fn(-1, fn, "iterations %d out of range 0..%d", c.iterations, kDnMaxIterations);
    if (!(c.sigma > 0.0f) || !std::isfinite(c.sigma))
        return postfx_fail_fn(-1, fn, "%s must be positive and finite", c.kind == kDnSum ? "sigma_color" : "sigma_var");
    if (!(c.sigmaNormal >= 0.0f) || !std::isfinite(c.sigmaNormal)) return postfx_fail_fn(-1, fn, "sigma_normal must be >= 0 and finite");
    if (!(c.sigmaDepth > 0.0f) || !std::isfinite(c.sigmaDepth)) return postfx_fail_fn(-1, fn, "sigma_depth must be positive and finite");
    if (c.kind == kDnVarTiles) {
        if (c.batchSpp < 1) return postfx_fail_fn(-1, c.fn, "batch_spp %d must be positive", c.batchSpp);
        if (!c.tileSpp) return postfx_fail_fn(-1, c.fn, "null tile map");
        const int32_t* map = (const int32_t*)c.tileSpp;           // read on the host only: the device form trusts the map
        const int T = host ? ((c.w + 7) / 8) * ((c.h + 7) / 8) : 0;
        for (int t = 0; t < T; t++)
            if (map[t] <= 0 || map[t] % c.batchSpp != 0 || map[t] < 2 * c.batchSpp)
                return postfx_fail_fn(-1, c.fn, "tile_spp[%d] = %d must be a positive multiple of batch_spp that gives at least 2 batches", t, map[t]);
    }
    if (!host && !c.ws) return postfx_fail(-1, "%s_device: null workspace", c.fn);
    return 0;
}

// The chain of a kind: prepare, reduce, one a-trous launch per iteration between the two halves of e, finish.
static int dn_launch(const DnCall& c, hipStream_t stream) {
    struct Kernels {
        void (*prepare)(DnArgs);
        void (*atrous)(int, int, int, float, float, float, const float4*, const float4*, const float4*, float4*);
        void (*finish)(DnArgs);
    };
    static const Kernels table[] = {{dn_prepare_kernel<SumSource>, dn_atrous_kernel<ColorWeight>, dn_finish_kernel<SumSource>},
                                    {dn_prepare_kernel<VarSource>, dn_atrous_kernel<VarianceWeight>, dn_finish_kernel<VarSource>},
                                    {dn_prepare_kernel<VarTilesSource>, dn_atrous_kernel<VarianceWeight>, dn_finish_kernel<VarTilesSource>},
                                    {dn_prepare_kernel<HistSource>, dn_atrous_kernel<VarianceWeight>, dn_finish_kernel<HistSource>}};
    const Kernels& k = table[c.kind];
    const DnLayout L = dn_layout(c.w, c.h);
    char* ws = (char*)c.ws;
    float4* e[2] = {(float4*)(ws + L.e0), (float4*)(ws + L.e1)};
    float4* lum = (float4*)(ws + L.lum);
    DnArgs a = {};
    a.n = (int)L.n; a.w = c.w; a.tilesX = (c.w + 7) / 8;
    a.in = (const float4*)c.in; a.sq = (const float4*)c.sq; a.tileSpp = (const int32_t*)c.tileSpp;
    a.spp = (float)c.spp; a.batches = (float)c.batches; a.batchSpp = c.batchSpp;
    a.albedo = (const float4*)c.albedo; a.nd = (const float4*)c.nd;
    a.e = e[0]; a.guide = (float4*)(ws + L.guide); a.partials = (float2*)(ws + L.partials); a.out = (float4*)c.out;
    hipLaunchKernelGGL(k.prepare, dim3(L.nParts), dim3(kDnBlock), 0, stream, a);
    POSTFX_HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(denoise_reduce_kernel, dim3(1), dim3(kDnBlock), 0, stream, L.nParts, a.partials, lum);
    POSTFX_HIP_OK(hipGetLastError());
    const dim3 grid((c.w + 15) / 16, (c.h + 15) / 16);
    for (int i = 0; i < c.iterations; i++) {
        const float sigma = c.kind == kDnSum ? c.sigma * c.sigma * std::ldexp(1.0f, -i) : c.sigma;
        hipLaunchKernelGGL(k.atrous, grid, dim3(256), 0, stream, c.w, c.h, 1 << i, sigma, c.sigmaNormal, c.sigmaDepth, lum, e[i & 1], a.guide,
                           e[(i + 1) & 1]);
        POSTFX_HIP_OK(hipGetLastError());
    }
    a.e = e[c.iterations & 1];
    hipLaunchKernelGGL(k.finish, dim3(L.nParts), dim3(kDnBlock), 0, stream, a);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

// Check and launch: on the caller's device buffers and workspace, or (host) on staged copies of the slices the call has. The
// input and the output share one slice (out may alias in).
static int dn_run(const DnCall& c, bool host, hipStream_t stream) {
    if (int r = check_dn_call(c, host)) return r;
    if (!host) return dn_launch(c, stream);
    const size_t bytes = (size_t)c.w * c.h * 16, mapBytes = (size_t)((c.w + 7) / 8) * ((c.h + 7) / 8) * sizeof(int32_t);
    const HostIn in[] = {{c.in, bytes}, {c.sq, bytes}, {c.albedo, bytes}, {c.nd, bytes}, {c.tileSpp, mapBytes}};
    const HostOut out[] = {{c.out, bytes, 0}};
    return postfx_host_form(c.fn, dn_layout(c.w, c.h).total, in, out, [&](char* ws, char** dIn, char** dOut) {
        DnCall d = c;
        d.in = dIn[0]; d.sq = dIn[1]; d.albedo = dIn[2]; d.nd = dIn[3]; d.tileSpp = dIn[4];
        d.ws = ws; d.out = dOut[0];
        return dn_launch(d, nullptr);
    });
}

static size_t dn_workspace_bytes(int w, int h) { return w <= 0 || h <= 0 ? 0 : dn_layout(w, h).total; }

// pt_denoise's parameters in the form the others have: sigma_color takes sigma_var's place.
static DnCall dn_sum_call(int w, int h, const void* in, int spp, const void* albedo, const void* nd, const pt_denoise_params* params, void* ws,
                          void* out) {
    pt_denoise_params P;
    if (params) P = *params; else pt_denoise_defaults(&P);
    const pt_denoise_var_params V = {P.iterations, P.sigma_color, P.sigma_normal, P.sigma_depth};
    DnCall c = dn_call("pt_denoise", kDnSum, w, h, in, albedo, nd, &V, ws, out);
    c.spp = spp;
    return c;
}
static DnCall dn_var_call(int w, int h, const void* in, const void* sq, int spp, int batches, const void* albedo, const void* nd,
                          const pt_denoise_var_params* params, void* ws, void* out) {
    DnCall c = dn_call("pt_denoise_var", kDnVar, w, h, in, albedo, nd, params, ws, out);
    c.sq = sq; c.spp = spp; c.batches = batches;
    return c;
}
static DnCall dn_var_tiles_call(int w, int h, const void* in, const void* sq, const void* tileSpp, int batchSpp, const void* albedo, const void* nd,
                                const pt_denoise_var_params* params, void* ws, void* out) {
    DnCall c = dn_call("pt_denoise_var_tiles", kDnVarTiles, w, h, in, albedo, nd, params, ws, out);
    c.sq = sq; c.tileSpp = tileSpp; c.batchSpp = batchSpp;
    return c;
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

void pt_denoise_var_defaults(pt_denoise_var_params* out) {
    if (!out) return;
    out->iterations = 3;
    out->sigma_var = 6.0f;
    out->sigma_normal = 64.0f;
    out->sigma_depth = 0.02f;
}

size_t pt_denoise_workspace_bytes(int w, int h) { return dn_workspace_bytes(w, h); }
size_t pt_denoise_var_workspace_bytes(int w, int h) { return dn_workspace_bytes(w, h); }
size_t pt_denoise_var_tiles_workspace_bytes(int w, int h) { return dn_workspace_bytes(w, h); }
size_t pt_denoise_hist_workspace_bytes(int w, int h) { return dn_workspace_bytes(w, h); }

int pt_denoise_device(int w, int h, const void* d_rgba_sum, int spp, const void* d_albedo, const void* d_normal_depth,
                      const pt_denoise_params* params, void* d_workspace, void* d_out, void* stream) {
    return dn_run(dn_sum_call(w, h, d_rgba_sum, spp, d_albedo, d_normal_depth, params, d_workspace, d_out), false, (hipStream_t)stream);
}

int pt_denoise(int w, int h, const float* rgba_sum, int spp, const float* albedo, const float* normal_depth, const pt_denoise_params* params,
               float* out_rgba_sum) {
    return dn_run(dn_sum_call(w, h, rgba_sum, spp, albedo, normal_depth, params, nullptr, out_rgba_sum), true, nullptr);
}

int pt_denoise_var_device(int w, int h, const void* d_rgba_sum, const void* d_sq_sum, int spp, int batches, const void* d_albedo,
                          const void* d_normal_depth, const pt_denoise_var_params* params, void* d_workspace, void* d_out, void* stream) {
    return dn_run(dn_var_call(w, h, d_rgba_sum, d_sq_sum, spp, batches, d_albedo, d_normal_depth, params, d_workspace, d_out), false,
                  (hipStream_t)stream);
}

int pt_denoise_var(int w, int h, const float* rgba_sum, const float* sq_sum, int spp, int batches, const float* albedo, const float* normal_depth,
                   const pt_denoise_var_params* params, float* out_rgba_sum) {
    return dn_run(dn_var_call(w, h, rgba_sum, sq_sum, spp, batches, albedo, normal_depth, params, nullptr, out_rgba_sum), true, nullptr);
}

int pt_denoise_var_tiles_device(int w, int h, const void* d_rgba_sum, const void* d_sq_sum, const void* d_tile_spp, int batch_spp,
                                const void* d_albedo, const void* d_normal_depth, const pt_denoise_var_params* params, void* d_workspace,
                                void* d_out, void* stream) {
    return dn_run(dn_var_tiles_call(w, h, d_rgba_sum, d_sq_sum, d_tile_spp, batch_spp, d_albedo, d_normal_depth, params, d_workspace, d_out), false,
                  (hipStream_t)stream);
}

int pt_denoise_var_tiles(int w, int h, const float* rgba_sum, const float* sq_sum, const int32_t* tile_spp, int batch_spp, const float* albedo,
                         const float* normal_depth, const pt_denoise_var_params* params, float* out_rgba_sum) {
    return dn_run(dn_var_tiles_call(w, h, rgba_sum, sq_sum, tile_spp, batch_spp, albedo, normal_depth, params, nullptr, out_rgba_sum), true, nullptr);
}

int pt_denoise_hist_device(int w, int h, const void* d_hist, const void* d_albedo, const void* d_normal_depth, const pt_denoise_var_params* params,
                           void* d_workspace, void* d_out, void* stream) {
    return dn_run(dn_call("pt_denoise_hist", kDnHist, w, h, d_hist, d_albedo, d_normal_depth, params, d_workspace, d_out), false,
                  (hipStream_t)stream);
}

int pt_denoise_hist(int w, int h, const float* hist, const float* albedo, const float* normal_depth, const pt_denoise_var_params* params,
                    float* out_rgba_mean) {
    return dn_run(dn_call("pt_denoise_hist", kDnHist, w, h, hist, albedo, normal_depth, params, nullptr, out_rgba_mean), true, nullptr);
}

}  // extern "C"
