// pt_grid_live.hip — a probe volume that stays current (pt_grid_classify[_device], pt_grid_update[_device]; include/pt_api.h;
// DESIGN.md §30): a state word per probe from its distance map's hit counts, and fresh query sums blended into a packed buffer in
// place. The lookup that reads the state words is pt_grid.hip's (pt_grid_irradiance_states). Scene-free and stateless as pt_grid.hip,
// whose desc checks, layout and packed words it shares (pt_grid.h). tests/grid_live_ref.py restates it.
//   live_classify_kernel      one wave per listed probe: the lanes stride its R^2 texels, summing the hits H and the hits seen from
//                             behind K (whole numbers, at most 2^22 in all: every order is exact), a butterfly over the wave, lane 0
//                             writes the probe's word
//   live_update_kernel        one thread per (listed probe, coefficient row) and per (listed probe, bordered texel): the word
//                             grid_pack_kernel computes from the fresh row, blended with the word that is there
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

PT_DEV float live_blend(float h, float old, float fresh) { return h == 0.0f ? fresh : __builtin_fmaf(h, old - fresh, fresh); }

__global__ void __launch_bounds__(256) live_update_kernel(GridParams G, int k, const int* __restrict__ indices, const float4* __restrict__ sums,
                                                          const float4* __restrict__ maps, float h, float4* coeff, float2* texels) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t rows = (size_t)k * 9;
    if (g < rows) {
        const int row = (int)(g / 9), t = (int)(g % 9);
        const int j = indices ? indices[row] : row;
        if (j < 0 || j >= G.n) return;
        const float4 fresh = grid_fresh_row(G, t, sums[g]);
        float4* at = coeff + (size_t)j * 9 + t;
        const float4 old = *at;
        *at = make_float4(live_blend(h, old.x, fresh.x), live_blend(h, old.y, fresh.y), live_blend(h, old.z, fresh.z), 0.0f);
        return;
    }
    const int R = G.R, B = R + 2;
    const size_t t = g - rows;
    if (R == 0 || t >= (size_t)k * B * B) return;
    const int row = (int)(t / ((size_t)B * B));
    const int l = (int)(t - (size_t)row * B * B);
    const int j = indices ? indices[row] : row;
    if (j < 0 || j >= G.n) return;
    const int2 s = grid_border_source(R, l);
    const float4 a = maps[(size_t)row * R * R + (size_t)s.y * R + s.x];
    float2* at = texels + (size_t)j * B * B + l;
    const float2 old = *at;
    *at = make_float2(live_blend(h, old.x, a.x / G.mapSamples), live_blend(h, old.y, a.y / G.mapSamples));
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

}  // extern "C"
