// pt_grid_relocate.hip — probes that move out of the way (pt_grid_relocate[_device]; include/pt_api.h): an offset
// per probe from its distance map's means and hit counts. The lookup that reads a probe's position as grid position + offset is
// pt_grid.hip's (pt_grid_irradiance_offsets). Scene-free and stateless as pt_grid.hip and pt_grid_live.hip, whose desc and list
// checks it shares (pt_grid.h). tests/grid_relocate_ref.py restates it.
//   reloc_kernel                 one wave per listed probe, as live_classify_kernel: the lanes stride its R^2 texels, summing the hits
//                                H and the hits seen from behind K and keeping the nearest majority-back and the nearest front texel
//                                by the key (mean, l); a butterfly over the wave (the key is total: every order gives the same
//                                texel); lane 0 makes the texel-centre direction, moves the offset, clamps it and writes it
#include "pt_grid.h"

namespace pt {

// (m1, l1) before (m2, l2): the smaller mean by f32 comparison (+0 and -0 equal), ties to the smaller texel. Never called with a NaN.
PT_DEV bool reloc_before(float m1, int l1, float m2, int l2) { return m1 < m2 || (m1 == m2 && l1 < l2); }

__global__ void __launch_bounds__(256) reloc_kernel(int n, int R, int k, const int* __restrict__ indices, const float4* __restrict__ maps,
                                                    float mapSamples, float backFraction, float minDist, float maxX, float maxY, float maxZ,
                                                    float4* offsets) {
    const int row = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (row >= k) return;
    const int j = indices ? indices[row] : row;
    if (j < 0 || j >= n) return;
    const float4* map = maps + (size_t)row * R * R;
    const float inf = __uint_as_float(0x7f800000u);
    const int none = 0x7fffffff;
    float H = 0.0f, K = 0.0f, mB = inf, mF = inf;
    int lB = none, lF = none;
    for (int l = lane; l < R * R; l += 64) {
        const float4 a = map[l];
        H = H + a.z; K = K + a.w;
        const float m = a.x / mapSamples;
        const bool back = a.w + a.w > a.z;
        if (m >= 0.0f) {
            if (back) { if (reloc_before(m, l, mB, lB)) { mB = m; lB = l; } }
            else if (a.z > 0.0f) { if (reloc_before(m, l, mF, lF)) { mF = m; lF = l; } }
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        H = H + __shfl_xor(H, s, 64); K = K + __shfl_xor(K, s, 64);
        const float oB = __shfl_xor(mB, s, 64), oF = __shfl_xor(mF, s, 64);
        const int pB = __shfl_xor(lB, s, 64), pF = __shfl_xor(lF, s, 64);
        if (reloc_before(oB, pB, mB, lB)) { mB = oB; lB = pB; }
        if (reloc_before(oF, pF, mF, lF)) { mF = oF; lF = pF; }
    }
    if (lane != 0) return;
    const bool inside = K > backFraction * H;
    const float m = inside ? mB : mF;
    const int l = inside ? lB : lF;
    const float4 old = offsets[j];
    float nx = old.x, ny = old.y, nz = old.z, code = 0.0f;
    if (l != none && (inside || m < minDist)) {
        // pt_query_distance's direction arithmetic at u1 = u2 = 0.5 (pt_distance.hip's oct_ray)
        const float invR = 1.0f / (float)R;
        const int tx = l & (R - 1), ty = l / R;
        const float px = ((float)tx + 0.5f) * invR, py = ((float)ty + 0.5f) * invR;
        const float fx = 2.0f * px - 1.0f, fy = 2.0f * py - 1.0f;
        const float ax = __builtin_fabsf(fx), ay = __builtin_fabsf(fy);
        const float z = (1.0f - ax) - ay;
        float x = fx, y = fy;
        if (z < 0.0f) { x = __builtin_copysignf(1.0f - ay, fx); y = __builtin_copysignf(1.0f - ax, fy); }
        const V3 c = normalize(v3(x, y, z));
        if (inside) {
            const float t = m + 0.5f * minDist;
            nx = __builtin_fmaf(c.x, t, old.x); ny = __builtin_fmaf(c.y, t, old.y); nz = __builtin_fmaf(c.z, t, old.z);
            code = 1.0f;
        } else {
            const float t = minDist - m;
            nx = __builtin_fmaf(-c.x, t, old.x); ny = __builtin_fmaf(-c.y, t, old.y); nz = __builtin_fmaf(-c.z, t, old.z);
            code = 2.0f;
        }
    }
    offsets[j] = make_float4(fminf_(fmaxf_(nx, -maxX), maxX), fminf_(fmaxf_(ny, -maxY), maxY), fminf_(fmaxf_(nz, -maxZ), maxZ), code);
}

static int reloc_launch(const GridParams& G, int k, const void* indices, const void* maps, float backFraction, float minDist, const float* maxOffset,
                        void* offsets, hipStream_t stream) {
    hipLaunchKernelGGL(reloc_kernel, dim3((unsigned)(((size_t)k + 3) / 4)), dim3(256), 0, stream, G.n, G.R, k, (const int*)indices, (const float4*)maps,
                       G.mapSamples, backFraction, minDist, maxOffset[0], maxOffset[1], maxOffset[2], (float4*)offsets);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

static int reloc_run(const char* fn, const pt_grid_desc* desc, int k, const void* indices, const void* maps, float backFraction, float minDist,
                     const float* maxOffset, void* offsets, bool host, hipStream_t stream) {
    GridParams G;
    if (int r = grid_params(fn, desc, G)) return r;
    if (G.R == 0) return postfx_fail_fn(-1, fn, "map_res is 0: a grid without maps has no positions to read");
    if (k < 0) return postfx_fail_fn(-1, fn, "k %d must not be negative", k);
    if (k == 0) return 0;
    if (int r = live_list_checks(fn, G, k, indices)) return r;
    if (!(backFraction >= 0.0f && backFraction <= 1.0f)) return postfx_fail_fn(-1, fn, "back_fraction %g must be in [0, 1]", backFraction);
    if (!(std::isfinite(minDist) && minDist >= 0.0f)) return postfx_fail_fn(-1, fn, "min_dist %g must be finite and not negative", minDist);
    for (int a = 0; maxOffset && a < 3; a++)
        if (!(std::isfinite(maxOffset[a]) && maxOffset[a] >= 0.0f))
            return postfx_fail_fn(-1, fn, "max_offset[%d] = %g must be finite and not negative", a, maxOffset[a]);
    if (!maps) return postfx_fail_fn(-1, fn, "null maps");
    if (!maxOffset) return postfx_fail_fn(-1, fn, "null max_offset");
    if (!offsets) return postfx_fail_fn(-1, fn, "null offsets");
    const size_t mapBytes = (size_t)k * G.R * G.R * sizeof(float4), offBytes = (size_t)G.n * sizeof(float4), listBytes = (size_t)k * 4;
    if (!host) {
        if (overlaps(offsets, offBytes, maps, mapBytes) || (indices && overlaps(offsets, offBytes, indices, listBytes)))
            return postfx_fail_fn(-1, fn, "the offsets overlap an input");
        return reloc_launch(G, k, indices, maps, backFraction, minDist, maxOffset, offsets, stream);
    }
    const HostIn in[] = {{indices, listBytes}, {maps, mapBytes}, {offsets, offBytes}};
    const HostOut out[] = {{offsets, offBytes, 2}};
    return postfx_host_form(fn, 0, in, out,
                            [&](char*, char** dIn, char** dOut) { return reloc_launch(G, k, dIn[0], dIn[1], backFraction, minDist, maxOffset, dOut[0], nullptr); });
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_grid_relocate_device(const pt_grid_desc* desc, int k, const void* d_indices, const void* d_maps, float back_fraction, float min_dist,
                            const float* max_offset, void* d_offsets, void* stream) {
    return reloc_run("pt_grid_relocate", desc, k, d_indices, d_maps, back_fraction, min_dist, max_offset, d_offsets, false, (hipStream_t)stream);
}

int pt_grid_relocate(const pt_grid_desc* desc, int k, const int32_t* indices, const float* maps4, float back_fraction, float min_dist,
                     const float* max_offset, float* offsets4) {
    return reloc_run("pt_grid_relocate", desc, k, indices, maps4, back_fraction, min_dist, max_offset, offsets4, true, nullptr);
}

}  // extern "C"
