// pt_grid_relocate.hip — probes that move out of the way (pt_grid_relocate[_device], pt_grid_irradiance_offsets[_device];
// include/pt_api.h): an offset per probe from its distance map's means and hit counts, and the lookup that reads a
// probe's position as grid position + offset. Scene-free and stateless as pt_grid.hip and pt_grid_live.hip, whose desc checks, layout
// and visibility it shares (pt_grid.h); their kernels are untouched. tests/grid_relocate_ref.py restates it.
//   reloc_kernel                 one wave per listed probe, as live_classify_kernel: the lanes stride its R^2 texels, summing the hits
//                                H and the hits seen from behind K and keeping the nearest majority-back and the nearest front texel
//                                by the key (mean, l); a butterfly over the wave (the key is total: every order gives the same
//                                texel); lane 0 makes the texel-centre direction, moves the offset, clamps it and writes it
//   reloc_lookup_kernel<STATES>  live_lookup_kernel<true> with the probe at fma(i, step, lo) + offset; without STATES no state word
//                                is read and the end is grid_irradiance_kernel<true>'s. On the wave-uniform path a corner's offset and
//                                state word arrive by scalar loads and a dead corner is a scalar branch.
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

// live_corners<true> (pt_grid_live.hip) with an offset per probe: the probe stands at fma(i, step, lo) + offset, one rounded add per
// axis; the cell, the trilinear weights and the corner order stay the regular grid's. Without STATES no corner is dead and the end is
// grid_corners<true>'s (pt_grid.hip). This unit's own copy: the two older units' code stays as it was, byte for byte.
template <bool STATES>
PT_DEV float4 reloc_corners(const GridParams& G, const float4* __restrict__ coeff, const float2* __restrict__ texels,
                            const unsigned* __restrict__ states, const float4* __restrict__ offsets, const float (&p)[3], const float (&y)[9],
                            const int (&low)[3], const float (&f)[3]) {
    float plain[3] = {0.0f, 0.0f, 0.0f}, num[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f, T = 0.0f;
    bool skipped = false;
    const int B2 = (G.R + 2) * (G.R + 2);
#pragma nounroll
    for (int c = 0; c < 8; c++) {
        const int cx = c & 1, cy = (c >> 1) & 1, cz = c >> 2;
        const int ix = low[0] + (G.counts[0] > 1 ? cx : 0), iy = low[1] + (G.counts[1] > 1 ? cy : 0), iz = low[2] + (G.counts[2] > 1 ? cz : 0);
        const int j = (iz * G.counts[1] + iy) * G.counts[0] + ix;
        if constexpr (STATES) {
            if (states[j] & 1u) { skipped = true; continue; }
        }
        const float tri = ((cx ? f[0] : 1.0f - f[0]) * (cy ? f[1] : 1.0f - f[1])) * (cz ? f[2] : 1.0f - f[2]);
        const float4* E = coeff + (size_t)j * 9;
        const float4 e0 = E[0];
        float e[3] = {e0.x * y[0], e0.y * y[0], e0.z * y[0]};
#pragma unroll
        for (int k = 1; k < 9; k++) {
            const float4 ek = E[k];
            e[0] = __builtin_fmaf(ek.x, y[k], e[0]); e[1] = __builtin_fmaf(ek.y, y[k], e[1]); e[2] = __builtin_fmaf(ek.z, y[k], e[2]);
        }
        for (int ch = 0; ch < 3; ch++) plain[ch] = __builtin_fmaf(tri, e[ch], plain[ch]);
        if constexpr (STATES) T = T + tri;
        const float4 off = offsets[j];
        const V3 at = v3(__builtin_fmaf((float)ix, G.step[0], G.lo[0]) + off.x, __builtin_fmaf((float)iy, G.step[1], G.lo[1]) + off.y,
                         __builtin_fmaf((float)iz, G.step[2], G.lo[2]) + off.z);
        const float w = tri * grid_visibility(G, texels + (size_t)j * B2, v3(p[0], p[1], p[2]) - at);
        for (int ch = 0; ch < 3; ch++) num[ch] = __builtin_fmaf(w, e[ch], num[ch]);
        W = W + w;
    }
    if (W >= 1e-6f) return make_float4(num[0] / W, num[1] / W, num[2] / W, W);
    if (!STATES || !skipped) return make_float4(plain[0], plain[1], plain[2], W);
    if (T > 0.0f) return make_float4(plain[0] / T, plain[1] / T, plain[2] / T, W);
    return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

template <bool STATES>
__global__ void __launch_bounds__(256) reloc_lookup_kernel(GridParams G, const float4* __restrict__ coeff, const float2* __restrict__ texels,
                                                           const unsigned* __restrict__ states, const float4* __restrict__ offsets, int m,
                                                           const float4* __restrict__ recs, float4* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)m) return;
    const float4 a = recs[2 * i], b = recs[2 * i + 1];
    if (!(finite_(a.x) && finite_(a.y) && finite_(a.z) && finite_(b.x) && finite_(b.y) && finite_(b.z))) {
        out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float p[3] = {a.x, a.y, a.z};
    int low[3];
    float f[3];
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        low[ax] = 0; f[ax] = 0.0f;
        if (G.counts[ax] > 1) {
            const float g = (p[ax] - G.lo[ax]) * G.inv[ax];
            const float l = fminf_(fmaxf_(__builtin_floorf(g), 0.0f), G.top[ax]);
            low[ax] = (int)l;
            f[ax] = fminf_(fmaxf_(g - l, 0.0f), 1.0f);
        }
    }
    const float nx = b.x, ny = b.y, nz = b.z;
    const float y[9] = {kShC0, kShC1 * ny, kShC1 * nz, kShC1 * nx, kShC2 * (nx * ny), kShC2 * (ny * nz), kShC3 * (3.0f * (nz * nz) - 1.0f),
                        kShC2 * (nx * nz), kShC4 * (nx * nx - ny * ny)};
    const int cell = (low[2] * G.counts[1] + low[1]) * G.counts[0] + low[0];
    if (__builtin_amdgcn_ballot_w64(cell != __builtin_amdgcn_readfirstlane(cell)) == 0) {
        const int u[3] = {__builtin_amdgcn_readfirstlane(low[0]), __builtin_amdgcn_readfirstlane(low[1]), __builtin_amdgcn_readfirstlane(low[2])};
        out[i] = reloc_corners<STATES>(G, coeff, texels, states, offsets, p, y, u, f);
        return;
    }
    out[i] = reloc_corners<STATES>(G, coeff, texels, states, offsets, p, y, low, f);
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

static int reloc_lookup_launch(const GridParams& G, const void* packed, const void* states, const void* offsets, int m, const void* recs, void* out,
                               hipStream_t stream) {
    const float4* coeff = (const float4*)packed;
    const float2* texels = (const float2*)((const char*)packed + grid_coeff_bytes(G));
    const dim3 grid((unsigned)(((size_t)m + 255) / 256)), block(256);
    if (states)
        hipLaunchKernelGGL(reloc_lookup_kernel<true>, grid, block, 0, stream, G, coeff, texels, (const unsigned*)states, (const float4*)offsets, m,
                           (const float4*)recs, (float4*)out);
    else
        hipLaunchKernelGGL(reloc_lookup_kernel<false>, grid, block, 0, stream, G, coeff, texels, (const unsigned*)nullptr, (const float4*)offsets, m,
                           (const float4*)recs, (float4*)out);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

static int reloc_lookup_run(const char* fn, const pt_grid_desc* desc, const void* packed, const void* states, const void* offsets, int m, const void* recs,
                            void* out, bool host, hipStream_t stream) {
    GridParams G;
    if (int r = grid_params(fn, desc, G)) return r;
    if (G.R == 0) return postfx_fail_fn(-1, fn, "map_res is 0: a grid without maps has no positions to read");
    if (m < 0) return postfx_fail_fn(-1, fn, "m %d must not be negative", m);
    if (m == 0) return 0;
    if (!packed) return postfx_fail_fn(-1, fn, "null packed buffer");
    if (!offsets) return postfx_fail_fn(-1, fn, "null offsets");
    if (!recs) return postfx_fail_fn(-1, fn, "null records");
    if (!out) return postfx_fail_fn(-1, fn, "null output buffer");
    const size_t recBytes = (size_t)m * 32, outBytes = (size_t)m * 16, stateBytes = (size_t)G.n * 4, offBytes = (size_t)G.n * sizeof(float4);
    if (!host) {
        if (overlaps(out, outBytes, recs, recBytes) || overlaps(out, outBytes, packed, grid_bytes(G)) ||
            (states && overlaps(out, outBytes, states, stateBytes)) || overlaps(out, outBytes, offsets, offBytes))
            return postfx_fail_fn(-1, fn, "the output buffer overlaps an input");
        return reloc_lookup_launch(G, packed, states, offsets, m, recs, out, stream);
    }
    const HostIn in[] = {{packed, grid_bytes(G)}, {states, stateBytes}, {offsets, offBytes}, {recs, recBytes}};
    const HostOut o[] = {{out, outBytes}};
    return postfx_host_form(fn, 0, in, o, [&](char*, char** dIn, char** dOut) { return reloc_lookup_launch(G, dIn[0], dIn[1], dIn[2], m, dIn[3], dOut[0], nullptr); });
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

int pt_grid_irradiance_offsets_device(const pt_grid_desc* desc, const void* d_packed, const void* d_states, const void* d_offsets, int m,
                                      const void* d_records, void* d_out, void* stream) {
    return reloc_lookup_run("pt_grid_irradiance_offsets", desc, d_packed, d_states, d_offsets, m, d_records, d_out, false, (hipStream_t)stream);
}

int pt_grid_irradiance_offsets(const pt_grid_desc* desc, const void* packed, const uint32_t* states, const float* offsets4, int m, const pt_ray* records,
                               float* out4) {
    return reloc_lookup_run("pt_grid_irradiance_offsets", desc, packed, states, offsets4, m, records, out4, true, nullptr);
}

}  // extern "C"
