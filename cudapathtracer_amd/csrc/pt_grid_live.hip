// pt_grid_live.hip — a probe volume that stays current (pt_grid_classify[_device], pt_grid_update[_device],
// pt_grid_irradiance_states[_device]; include/pt_api.h): a state word per probe from its distance map's hit counts,
// lookups that leave out the probes found inside an object, and fresh query sums blended into a packed buffer in place. Scene-free
// and stateless as pt_grid.hip, whose desc checks, layout and visibility it shares (pt_grid.h). tests/grid_live_ref.py restates it.
//   live_classify_kernel      one wave per listed probe: the lanes stride its R^2 texels, summing the hits H and the hits seen from
//                             behind K (whole numbers, at most 2^22 in all: every order is exact), a butterfly over the wave, lane 0
//                             writes the probe's word
//   live_update_kernel        one thread per (listed probe, coefficient row) and per (listed probe, bordered texel): the word
//                             grid_pack_kernel computes from the fresh row, blended with the word that is there
//   live_lookup_kernel<MAPS>  grid_irradiance_kernel with a state word per corner: a corner whose bit 0 is set loads nothing more.
//                             On the wave-uniform path the word arrives by a scalar load and the skip is a scalar branch.
#include "pt_grid.h"

namespace pt {

__global__ void __launch_bounds__(256) live_classify_kernel(int n, int R, int k, const int* __restrict__ indices, const float4* __restrict__ maps,
                                                            float backFraction, unsigned* __restrict__ states) {
    const int row = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (row >= k) return;
    const int j = indices ? indices[row] : row;
    if (j < 0 || j >= n) return;
    const float4* map = maps + (size_t)row * R * R;
    float H = 0.0f, K = 0.0f;
    for (int l = lane; l < R * R; l += 64) {
        const float4 a = map[l];
        H = H + a.z; K = K + a.w;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        H = H + __shfl_xor(H, s, 64); K = K + __shfl_xor(K, s, 64);
    }
    if (lane == 0) states[j] = (K > backFraction * H ? PT_PROBE_INSIDE : 0u) | (H == 0.0f ? PT_PROBE_IDLE : 0u);
}

// The interior texel (sx, sy) that texel l of a probe's bordered (R + 2)^2 map copies: itself off the gutter, rays.oct_border's rule on it,
// as grid_pack_kernel (pt_grid.hip) finds it.
PT_DEV void live_border_source(int R, int l, int& sx, int& sy) {
    const int B = R + 2;
    sx = l % B - 1; sy = l / B - 1;
    if (sx < 0) { sx = -1 - sx; sy = R - 1 - sy; } else if (sx > R - 1) { sx = 2 * R - 1 - sx; sy = R - 1 - sy; }
    if (sy < 0) { sy = -1 - sy; sx = R - 1 - sx; } else if (sy > R - 1) { sy = 2 * R - 1 - sy; sx = R - 1 - sx; }
}

PT_DEV float live_blend(float h, float old, float fresh) { return h == 0.0f ? fresh : __builtin_fmaf(h, old - fresh, fresh); }

__global__ void __launch_bounds__(256) live_update_kernel(GridParams G, int k, const int* __restrict__ indices, const float4* __restrict__ sums,
                                                          const float4* __restrict__ maps, float h, float4* coeff, float2* texels) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t rows = (size_t)k * 9;
    if (g < rows) {
        const int row = (int)(g / 9), t = (int)(g % 9);
        const int j = indices ? indices[row] : row;
        if (j < 0 || j >= G.n) return;
        const float lobe = t == 0 ? 3.14159265358979323846f : (t < 4 ? 2.09439510239319549231f : 0.78539816339744830962f);
        const float4 c = sums[g];
        float4* at = coeff + (size_t)j * 9 + t;
        const float4 old = *at;
        *at = make_float4(live_blend(h, old.x, (c.x * G.scale) * lobe), live_blend(h, old.y, (c.y * G.scale) * lobe),
                          live_blend(h, old.z, (c.z * G.scale) * lobe), 0.0f);
        return;
    }
    const int R = G.R, B = R + 2;
    const size_t t = g - rows;
    if (R == 0 || t >= (size_t)k * B * B) return;
    const int row = (int)(t / ((size_t)B * B));
    const int l = (int)(t - (size_t)row * B * B);
    const int j = indices ? indices[row] : row;
    if (j < 0 || j >= G.n) return;
    int sx, sy;
    live_border_source(R, l, sx, sy);
    const float4 a = maps[(size_t)row * R * R + (size_t)sy * R + sx];
    float2* at = texels + (size_t)j * B * B + l;
    const float2 old = *at;
    *at = make_float2(live_blend(h, old.x, a.x / G.mapSamples), live_blend(h, old.y, a.y / G.mapSamples));
}

// grid_corners (pt_grid.hip) with the probes' state words: a corner whose bit 0 is set adds nothing, the live ones also sum their
// trilinear weights in T, and the end divides the plain mix by T where a corner was left out (include/pt_api.h).
template <bool MAPS>
PT_DEV float4 live_corners(const GridParams& G, const float4* __restrict__ coeff, const float2* __restrict__ texels,
                           const unsigned* __restrict__ states, const float (&p)[3], const float (&y)[9], const int (&low)[3], const float (&f)[3]) {
    float plain[3] = {0.0f, 0.0f, 0.0f}, num[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f, T = 0.0f;
    bool skipped = false;
    const int B2 = (G.R + 2) * (G.R + 2);
#pragma nounroll
    for (int c = 0; c < 8; c++) {
        const int cx = c & 1, cy = (c >> 1) & 1, cz = c >> 2;
        const int ix = low[0] + (G.counts[0] > 1 ? cx : 0), iy = low[1] + (G.counts[1] > 1 ? cy : 0), iz = low[2] + (G.counts[2] > 1 ? cz : 0);
        const int j = (iz * G.counts[1] + iy) * G.counts[0] + ix;
        if (states[j] & 1u) { skipped = true; continue; }
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
        T = T + tri;
        if constexpr (MAPS) {
            const V3 at = v3(__builtin_fmaf((float)ix, G.step[0], G.lo[0]), __builtin_fmaf((float)iy, G.step[1], G.lo[1]),
                             __builtin_fmaf((float)iz, G.step[2], G.lo[2]));
            const float w = tri * grid_visibility(G, texels + (size_t)j * B2, v3(p[0], p[1], p[2]) - at);
            for (int ch = 0; ch < 3; ch++) num[ch] = __builtin_fmaf(w, e[ch], num[ch]);
            W = W + w;
        }
    }
    if (!MAPS) W = T;
    if (MAPS && W >= 1e-6f) return make_float4(num[0] / W, num[1] / W, num[2] / W, W);
    if (!skipped) return make_float4(plain[0], plain[1], plain[2], W);
    if (T > 0.0f) return make_float4(plain[0] / T, plain[1] / T, plain[2] / T, W);
    return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

template <bool MAPS>
__global__ void __launch_bounds__(256) live_lookup_kernel(GridParams G, const float4* __restrict__ coeff, const float2* __restrict__ texels,
                                                          const unsigned* __restrict__ states, int m, const float4* __restrict__ recs,
                                                          float4* __restrict__ out) {
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
        out[i] = live_corners<MAPS>(G, coeff, texels, states, p, y, u, f);
        return;
    }
    out[i] = live_corners<MAPS>(G, coeff, texels, states, p, y, low, f);
}

static int live_classify_launch(const GridParams& G, int k, const void* indices, const void* maps, float backFraction, void* states, hipStream_t stream) {
    hipLaunchKernelGGL(live_classify_kernel, dim3((unsigned)(((size_t)k + 3) / 4)), dim3(256), 0, stream, G.n, G.R, k, (const int*)indices,
                       (const float4*)maps, backFraction, (unsigned*)states);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

static int live_classify_run(const char* fn, const pt_grid_desc* desc, int k, const void* indices, const void* maps, float backFraction, void* states,
                             bool host, hipStream_t stream) {
    GridParams G;
    if (int r = grid_params(fn, desc, G)) return r;
    if (G.R == 0) return postfx_fail_fn(-1, fn, "map_res is 0: a grid without maps has nothing to classify");
    if (k < 0) return postfx_fail_fn(-1, fn, "k %d must not be negative", k);
    if (k == 0) return 0;
    if (int r = live_list_checks(fn, G, k, indices)) return r;
    if (!(backFraction >= 0.0f && backFraction <= 1.0f)) return postfx_fail_fn(-1, fn, "back_fraction %g must be in [0, 1]", backFraction);
    if (!maps) return postfx_fail_fn(-1, fn, "null maps");
    if (!states) return postfx_fail_fn(-1, fn, "null states");
    const size_t mapBytes = (size_t)k * G.R * G.R * sizeof(float4), stateBytes = (size_t)G.n * 4, listBytes = (size_t)k * 4;
    if (!host) {
        if (overlaps(states, stateBytes, maps, mapBytes) || (indices && overlaps(states, stateBytes, indices, listBytes)))
            return postfx_fail_fn(-1, fn, "the states overlap an input");
        return live_classify_launch(G, k, indices, maps, backFraction, states, stream);
    }
    const HostIn in[] = {{indices, listBytes}, {maps, mapBytes}, {states, stateBytes}};
    const HostOut out[] = {{states, stateBytes, 2}};
    return postfx_host_form(fn, 0, in, out, [&](char*, char** dIn, char** dOut) { return live_classify_launch(G, k, dIn[0], dIn[1], backFraction, dOut[0], nullptr); });
}

static int live_update_launch(const GridParams& G, int k, const void* indices, const void* sums, const void* maps, float h, void* packed, hipStream_t stream) {
    const size_t threads = (size_t)k * 9 + (G.R ? (size_t)k * (G.R + 2) * (G.R + 2) : 0);
    hipLaunchKernelGGL(live_update_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, G, k, (const int*)indices, (const float4*)sums,
                       (const float4*)maps, h, (float4*)packed, (float2*)((char*)packed + grid_coeff_bytes(G)));
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

static int live_update_run(const char* fn, const pt_grid_desc* desc, int k, const void* indices, const void* sums, const void* maps, float h, void* packed,
                           bool host, hipStream_t stream) {
    GridParams G;
    if (int r = grid_params(fn, desc, G)) return r;
    if (k < 0) return postfx_fail_fn(-1, fn, "k %d must not be negative", k);
    if (k == 0) return 0;
    if (int r = live_list_checks(fn, G, k, indices)) return r;
    if (!(h >= 0.0f && h < 1.0f)) return postfx_fail_fn(-1, fn, "hysteresis %g must be in [0, 1)", h);
    if (!sums) return postfx_fail_fn(-1, fn, "null coeff_sums");
    if (!packed) return postfx_fail_fn(-1, fn, "null packed buffer");
    if (G.R == 0 && maps) return postfx_fail_fn(-1, fn, "maps given although map_res is 0");
    if (G.R != 0 && !maps) return postfx_fail_fn(-1, fn, "null maps although map_res is %d", G.R);
    const size_t sumBytes = (size_t)k * 9 * sizeof(float4), mapBytes = (size_t)k * G.R * G.R * sizeof(float4), listBytes = (size_t)k * 4;
    if (!host) {
        if (overlaps(packed, grid_bytes(G), sums, sumBytes) || (maps && overlaps(packed, grid_bytes(G), maps, mapBytes)) ||
            (indices && overlaps(packed, grid_bytes(G), indices, listBytes)))
            return postfx_fail_fn(-1, fn, "the packed buffer overlaps an input");
        return live_update_launch(G, k, indices, sums, maps, h, packed, stream);
    }
    const HostIn in[] = {{indices, listBytes}, {sums, sumBytes}, {maps, mapBytes}, {packed, grid_bytes(G)}};
    const HostOut out[] = {{packed, grid_bytes(G), 3}};
    return postfx_host_form(fn, 0, in, out, [&](char*, char** dIn, char** dOut) { return live_update_launch(G, k, dIn[0], dIn[1], dIn[2], h, dOut[0], nullptr); });
}

static int live_lookup_launch(const GridParams& G, const void* packed, const void* states, int m, const void* recs, void* out, hipStream_t stream) {
    const float4* coeff = (const float4*)packed;
    const float2* texels = (const float2*)((const char*)packed + grid_coeff_bytes(G));
    const dim3 grid((unsigned)(((size_t)m + 255) / 256)), block(256);
    if (G.R) hipLaunchKernelGGL(live_lookup_kernel<true>, grid, block, 0, stream, G, coeff, texels, (const unsigned*)states, m, (const float4*)recs, (float4*)out);
    else hipLaunchKernelGGL(live_lookup_kernel<false>, grid, block, 0, stream, G, coeff, texels, (const unsigned*)states, m, (const float4*)recs, (float4*)out);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

static int live_lookup_run(const char* fn, const pt_grid_desc* desc, const void* packed, const void* states, int m, const void* recs, void* out, bool host,
                           hipStream_t stream) {
    GridParams G;
    if (int r = grid_params(fn, desc, G)) return r;
    if (m < 0) return postfx_fail_fn(-1, fn, "m %d must not be negative", m);
    if (m == 0) return 0;
    if (!packed) return postfx_fail_fn(-1, fn, "null packed buffer");
    if (!states) return postfx_fail_fn(-1, fn, "null states");
    if (!recs) return postfx_fail_fn(-1, fn, "null records");
    if (!out) return postfx_fail_fn(-1, fn, "null output buffer");
    const size_t recBytes = (size_t)m * 32, outBytes = (size_t)m * 16, stateBytes = (size_t)G.n * 4;
    if (!host) {
        if (overlaps(out, outBytes, recs, recBytes) || overlaps(out, outBytes, packed, grid_bytes(G)) || overlaps(out, outBytes, states, stateBytes))
            return postfx_fail_fn(-1, fn, "the output buffer overlaps an input");
        return live_lookup_launch(G, packed, states, m, recs, out, stream);
    }
    const HostIn in[] = {{packed, grid_bytes(G)}, {states, stateBytes}, {recs, recBytes}};
    const HostOut o[] = {{out, outBytes}};
    return postfx_host_form(fn, 0, in, o, [&](char*, char** dIn, char** dOut) { return live_lookup_launch(G, dIn[0], dIn[1], m, dIn[2], dOut[0], nullptr); });
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_grid_classify_device(const pt_grid_desc* desc, int k, const void* d_indices, const void* d_maps, float back_fraction, void* d_states, void* stream) {
    return live_classify_run("pt_grid_classify", desc, k, d_indices, d_maps, back_fraction, d_states, false, (hipStream_t)stream);
}

int pt_grid_classify(const pt_grid_desc* desc, int k, const int32_t* indices, const float* maps4, float back_fraction, uint32_t* states) {
    return live_classify_run("pt_grid_classify", desc, k, indices, maps4, back_fraction, states, true, nullptr);
}

int pt_grid_update_device(const pt_grid_desc* desc, int k, const void* d_indices, const void* d_coeff_sums, const void* d_maps, float hysteresis,
                          void* d_packed, void* stream) {
    return live_update_run("pt_grid_update", desc, k, d_indices, d_coeff_sums, d_maps, hysteresis, d_packed, false, (hipStream_t)stream);
}

int pt_grid_update(const pt_grid_desc* desc, int k, const int32_t* indices, const float* coeff_sums, const float* maps4, float hysteresis, void* packed) {
    return live_update_run("pt_grid_update", desc, k, indices, coeff_sums, maps4, hysteresis, packed, true, nullptr);
}

int pt_grid_irradiance_states_device(const pt_grid_desc* desc, const void* d_packed, const void* d_states, int m, const void* d_records, void* d_out,
                                     void* stream) {
    return live_lookup_run("pt_grid_irradiance_states", desc, d_packed, d_states, m, d_records, d_out, false, (hipStream_t)stream);
}

int pt_grid_irradiance_states(const pt_grid_desc* desc, const void* packed, const uint32_t* states, int m, const pt_ray* records, float* out4) {
    return live_lookup_run("pt_grid_irradiance_states", desc, packed, states, m, records, out4, true, nullptr);
}

}  // extern "C"
