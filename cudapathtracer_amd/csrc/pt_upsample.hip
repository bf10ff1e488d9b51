// pt_upsample.hip — the render scale's spatial stage: a frame rendered at 1/s of the display resolution in each axis, brought to
// display size in pt_denoise_var's working format (e, V), guided by the display camera's feature buffers (joint bilateral
// upsampling: Kopf et al., SIGGRAPH 2007, with the a-trous filters' normal and depth weights). include/pt_api.h states the
// arithmetic; tests/upsample_ref.py restates it in numpy. Stateless, no workspace, no render path involved.
//
//   upsample_kernel   one thread per display pixel, 16x16 pixels per workgroup as four 8x8 tiles (one per wave, the tiling of
//                     temporal_kernel and resolve_kernel): a wave's tile reads at most (8 / s + 1)^2 low-res pixels of
//                     each of the four low-res buffers, a few lines. Each tap's working pixel comes from S and Q again
//                     (dn_var_pixel, shared with dn_prepare_kernel's VarSource): no prepare pass, no workspace. Plain cached float4
//                     loads, no LDS.
//   guide_subsample_kernel   the low-res guide of CENTRE feature buffers (pt_guide_subsample): out[Y][X] = in[sY][sX] for both buffers,
//                     one thread per low-res pixel. A strided copy, because the centre ray of low-res pixel (X, Y) is the centre ray
//                     of display pixel (sX, sY) bit for bit.
// pt_camera_scaled lives here as well: the low-res camera of a scaled frame.
#include <cmath>

#include <hip/hip_runtime.h>

#include "../../include/pt_api.h"
#include "pt_denoise_shared.h"
#include "pt_postfx_host.h"

namespace pt {

__global__ void __launch_bounds__(256) upsample_kernel(int w, int h, int s, const float4* __restrict__ sumLo, const float4* __restrict__ sqLo,
                                                       float spp, float batches, const float4* __restrict__ albedoLo,
                                                       const float4* __restrict__ ndLo, const float4* __restrict__ albedo,
                                                       const float4* __restrict__ nd, float sigmaNormal, float sigmaDepth,
                                                       float4* __restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const int wl = w / s, hl = h / s;
    const int X0 = x / s, Y0 = y / s;
    const float fx = (float)(x - s * X0) / (float)s, fy = (float)(y - s * Y0) / (float)s;
    const float b[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
    const bool hitP = albedo[p].w > 0.0f;
    const float4 gp = dn_unit_guide(nd[p]);
    const bool normalP = gp.x != 0.0f || gp.y != 0.0f || gp.z != 0.0f;
    const float kz = 1.4426950408889634f / (sigmaDepth * gp.w);             // w_z = exp2(-|dz| kz), as dn_atrous_kernel forms it
    float4 candM = make_float4(0.0f, 0.0f, 0.0f, 0.0f), useE = candM;       // the nearest candidate's raw mean, the nearest usable tap's (e, V)
    float candB = 0.0f, useB = 0.0f;                                        // (b > 0 for both kinds of tap: 0 = none yet)
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f, sw = 0.0f;
    for (int k = 0; k < 4; k++) {
        const int xk = X0 + (k & 1), yk = Y0 + (k >> 1);
        if (!(b[k] > 0.0f) || xk >= wl || yk >= hl) continue;
        const size_t q = (size_t)yk * wl + xk;
        float4 m;
        const float4 ek = dn_var_pixel(sumLo[q], sqLo[q], albedoLo[q], spp, batches, m);
        if (b[k] > candB) { candB = b[k]; candM = m; }
        if (!hitP || ek.w < 0.0f) continue;
        if (b[k] > useB) { useB = b[k]; useE = ek; }
        if (!normalP) continue;
        const float4 gk = dn_unit_guide(ndLo[q]);
        if (gk.x == 0.0f && gk.y == 0.0f && gk.z == 0.0f) continue;
        const float cs = gp.x * gk.x + gp.y * gk.y + gp.z * gk.z;
        float ln;
        if (sigmaNormal == 0.0f) ln = 0.0f;
        else if (cs > 0.0f) ln = sigmaNormal * __builtin_log2f(cs);
        else continue;
        const float wk = b[k] * __builtin_exp2f(ln - fabsf(gp.w - gk.w) * kz);
        if (!(wk > 0.0f)) continue;                                         // 0 or NaN: skipped, never multiplied in
        sx += wk * ek.x; sy += wk * ek.y; sz += wk * ek.z; sw += wk;
        sv += (wk * wk) * ek.w;
    }
    if (!(useB > 0.0f)) out[p] = make_float4(candM.x, candM.y, candM.z, -1.0f);   // nothing hit here, or no usable tap
    else if (sw >= 1e-4f) out[p] = make_float4(sx / sw, sy / sw, sz / sw, sv / (sw * sw));
    else out[p] = useE;
}

__global__ void __launch_bounds__(256) guide_subsample_kernel(int w, int wl, int hl, int s, const float4* __restrict__ albedo,
                                                              const float4* __restrict__ nd, float4* __restrict__ albedoLo,
                                                              float4* __restrict__ ndLo) {
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);      // a wave: 64 pixels of one row
    if (X >= wl || Y >= hl) return;
    const size_t q = (size_t)Y * wl + X, p = (size_t)(Y * s) * w + (size_t)X * s;
    albedoLo[q] = albedo[p];
    ndLo[q] = nd[p];
}

static int check_upsample_args(int w, int h, int s, const void* sumLo, const void* sqLo, int spp, int batches, const void* albedoLo,
                               const void* ndLo, const void* albedo, const void* nd, const pt_upsample_params& P, const void* out) {
    if (int r = postfx_check_size("pt_upsample", w, h)) return r;
    if (s < 2 || s > 8) return postfx_fail(-1, "pt_upsample: scale %d must be 2..8", s);
    if (w % s != 0 || h % s != 0) return postfx_fail(-1, "pt_upsample: scale %d must divide the image size %d x %d", s, w, h);
    if (spp <= 0) return postfx_fail(-1, "pt_upsample: spp %d must be positive", spp);
    if (batches < 2) return postfx_fail(-1, "pt_upsample: batches %d must be at least 2", batches);
    if (spp % batches != 0) return postfx_fail(-1, "pt_upsample: batches %d must divide spp %d", batches, spp);
    if (!sumLo || !sqLo || !albedoLo || !ndLo || !albedo || !nd) return postfx_fail(-1, "pt_upsample: null buffer");
    if (!out) return postfx_fail(-1, "pt_upsample: null output");
    const size_t full = (size_t)w * h * 16, lo = (size_t)(w / s) * (h / s) * 16;
    if (overlaps(out, full, sumLo, lo) || overlaps(out, full, sqLo, lo) || overlaps(out, full, albedoLo, lo) || overlaps(out, full, ndLo, lo) ||
        overlaps(out, full, albedo, full) || overlaps(out, full, nd, full))
        return postfx_fail(-1, "pt_upsample: the output must not alias an input (the gather reads neighbours)");
    if (!(P.sigma_normal >= 0.0f) || !std::isfinite(P.sigma_normal)) return postfx_fail(-1, "pt_upsample: sigma_normal must be finite and >= 0");
    if (!(P.sigma_depth > 0.0f) || !std::isfinite(P.sigma_depth)) return postfx_fail(-1, "pt_upsample: sigma_depth must be finite and > 0");
    return 0;
}

static int upsample_launch(int w, int h, int s, const float4* sumLo, const float4* sqLo, int spp, int batches, const float4* albedoLo,
                           const float4* ndLo, const float4* albedo, const float4* nd, const pt_upsample_params& P, float4* out, hipStream_t stream) {
    hipLaunchKernelGGL(upsample_kernel, dim3((w + 15) / 16, (h + 15) / 16), dim3(256), 0, stream, w, h, s, sumLo, sqLo, (float)spp, (float)batches,
                       albedoLo, ndLo, albedo, nd, P.sigma_normal, P.sigma_depth, out);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

static int check_subsample_args(int w, int h, int s, const void* albedo, const void* nd, const void* outA, const void* outN) {
    if (int r = postfx_check_size("pt_guide_subsample", w, h)) return r;
    if (s < 2 || s > 8) return postfx_fail(-1, "pt_guide_subsample: scale %d must be 2..8", s);
    if (w % s != 0 || h % s != 0) return postfx_fail(-1, "pt_guide_subsample: scale %d must divide the image size %d x %d", s, w, h);
    if (!albedo || !nd) return postfx_fail(-1, "pt_guide_subsample: null buffer");
    if (!outA || !outN) return postfx_fail(-1, "pt_guide_subsample: null output");
    const size_t full = (size_t)w * h * 16, lo = (size_t)(w / s) * (h / s) * 16;
    if (overlaps(outA, lo, albedo, full) || overlaps(outA, lo, nd, full) || overlaps(outN, lo, albedo, full) || overlaps(outN, lo, nd, full) ||
        overlaps(outA, lo, outN, lo))
        return postfx_fail(-1, "pt_guide_subsample: the outputs must not alias the inputs or each other");
    return 0;
}

static int subsample_launch(int w, int h, int s, const float4* albedo, const float4* nd, float4* outA, float4* outN, hipStream_t stream) {
    const int wl = w / s, hl = h / s;
    hipLaunchKernelGGL(guide_subsample_kernel, dim3((wl + 63) / 64, (hl + 3) / 4), dim3(256), 0, stream, w, wl, hl, s, albedo, nd, outA, outN);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace pt

using namespace pt;

extern "C" {

void pt_upsample_defaults(pt_upsample_params* out) {
    if (!out) return;
    out->sigma_normal = 64.0f;
    out->sigma_depth = 0.10f;
}

int pt_camera_scaled(const pt_camera* cam, int scale, pt_camera* out) {
    if (!cam || !out) return postfx_fail(-1, "pt_camera_scaled: null camera");
    if (scale < 1 || scale > 8) return postfx_fail(-1, "pt_camera_scaled: scale %d must be 1..8", scale);
    if (cam->w <= 0 || cam->h <= 0 || cam->w % scale != 0 || cam->h % scale != 0)
        return postfx_fail(-1, "pt_camera_scaled: scale %d must divide the camera's size %d x %d", scale, cam->w, cam->h);
    *out = *cam;
    out->w = cam->w / scale; out->h = cam->h / scale;
    return 0;
}

int pt_upsample_device(int w, int h, int scale, const void* d_rgba_sum_lo, const void* d_sq_sum_lo, int spp, int batches, const void* d_albedo_lo,
                       const void* d_normal_depth_lo, const void* d_albedo, const void* d_normal_depth, const pt_upsample_params* params,
                       void* d_out_cur, void* stream) {
    pt_upsample_params P;
    if (params) P = *params; else pt_upsample_defaults(&P);
    if (int r = check_upsample_args(w, h, scale, d_rgba_sum_lo, d_sq_sum_lo, spp, batches, d_albedo_lo, d_normal_depth_lo, d_albedo, d_normal_depth, P,
                                    d_out_cur))
        return r;
    return upsample_launch(w, h, scale, (const float4*)d_rgba_sum_lo, (const float4*)d_sq_sum_lo, spp, batches, (const float4*)d_albedo_lo,
                           (const float4*)d_normal_depth_lo, (const float4*)d_albedo, (const float4*)d_normal_depth, P, (float4*)d_out_cur,
                           (hipStream_t)stream);
}

int pt_upsample(int w, int h, int scale, const float* rgba_sum_lo, const float* sq_sum_lo, int spp, int batches, const float* albedo_lo,
                const float* normal_depth_lo, const float* albedo, const float* normal_depth, const pt_upsample_params* params, float* out_cur) {
    pt_upsample_params P;
    if (params) P = *params; else pt_upsample_defaults(&P);
    if (int r = check_upsample_args(w, h, scale, rgba_sum_lo, sq_sum_lo, spp, batches, albedo_lo, normal_depth_lo, albedo, normal_depth, P, out_cur))
        return r;
    const size_t full = (size_t)w * h * 16, lo = (size_t)(w / scale) * (h / scale) * 16;
    const HostIn in[] = {{rgba_sum_lo, lo}, {sq_sum_lo, lo}, {albedo_lo, lo}, {normal_depth_lo, lo}, {albedo, full}, {normal_depth, full}};
    const HostOut out[] = {{out_cur, full}};
    return postfx_host_form("pt_upsample", 0, in, out, [&](char*, char** d, char** o) {
        return upsample_launch(w, h, scale, (const float4*)d[0], (const float4*)d[1], spp, batches, (const float4*)d[2], (const float4*)d[3],
                               (const float4*)d[4], (const float4*)d[5], P, (float4*)o[0], nullptr);
    });
}

int pt_guide_subsample_device(int w, int h, int scale, const void* d_albedo, const void* d_normal_depth, void* d_out_albedo_lo,
                              void* d_out_normal_depth_lo, void* stream) {
    if (int r = check_subsample_args(w, h, scale, d_albedo, d_normal_depth, d_out_albedo_lo, d_out_normal_depth_lo)) return r;
    return subsample_launch(w, h, scale, (const float4*)d_albedo, (const float4*)d_normal_depth, (float4*)d_out_albedo_lo,
                            (float4*)d_out_normal_depth_lo, (hipStream_t)stream);
}

int pt_guide_subsample(int w, int h, int scale, const float* albedo, const float* normal_depth, float* out_albedo_lo, float* out_normal_depth_lo) {
    if (int r = check_subsample_args(w, h, scale, albedo, normal_depth, out_albedo_lo, out_normal_depth_lo)) return r;
    const size_t full = (size_t)w * h * 16, lo = (size_t)(w / scale) * (h / scale) * 16;
    const HostIn in[] = {{albedo, full}, {normal_depth, full}};
    const HostOut out[] = {{out_albedo_lo, lo}, {out_normal_depth_lo, lo}};
    return postfx_host_form("pt_guide_subsample", 0, in, out, [&](char*, char** d, char** o) {
        return subsample_launch(w, h, scale, (const float4*)d[0], (const float4*)d[1], (float4*)o[0], (float4*)o[1], nullptr);
    });
}

}  // extern "C"
