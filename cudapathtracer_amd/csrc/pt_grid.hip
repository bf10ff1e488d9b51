// pt_grid.hip — the lookup side of a probe volume (pt_grid_packed_bytes, pt_grid_pack[_device], pt_grid_irradiance[_device],
// pt_grid_irradiance_states[_device], pt_grid_irradiance_offsets[_device]; include/pt_api.h): irradiance at
// surface points from a regular grid of pt_query_sh's SH probes, each weighted trilinearly times the Chebyshev visibility its
// pt_query_distance map gives the point; with a state word per probe the probes found inside an object are left out (§30), with an
// offset per probe it stands at grid position + offset (§31). Scene-free, stateless, no workspace: arrays in, arrays out, as the
// post-process calls. include/pt_api.h states the arithmetic; tests/grid_ref.py, grid_live_ref.py and grid_relocate_ref.py restate it.
//   grid_pack_kernel          one thread per coefficient row (n * 9: the sums scaled and convolved with the cosine lobe) and per texel of
//                             the bordered maps (n * (R + 2)^2: the means, the gutter copied by rays.oct_border's rule)
//   grid_lookup_kernel<MAPS, STATES, OFFSETS>
//                             one lane per record: the cell and its three fractions, the nine basis values at the normal, then the
//                             eight corners in turn: nine float4 of coefficients and, with MAPS, four float2 taps of the probe's
//                             bordered map, a plain bilinear fetch with no wrap logic. No LDS. Six forms, one loop (§32): without MAPS
//                             no map code, with STATES a corner whose word has bit 0 set loads nothing more, with OFFSETS (MAPS only)
//                             the probe stands at fma(i, step, lo) + offset. A form carries no code of a part it lacks.
//                             Neighbouring records mostly share their cell: when a ballot says that every lane of the wave has the
//                             same one, the cell's index goes to SGPRs and the coefficients, a corner's state word and its offset
//                             arrive by scalar loads, a dead corner is a scalar branch (measured: §29).
// Every min and max is v_min_f32 / v_max_f32, which drop a NaN operand: every index is in range whatever a record holds.
#include "pt_grid.h"

namespace pt {

__global__ void __launch_bounds__(256) grid_pack_kernel(GridParams G, const float4* __restrict__ sums, const float4* __restrict__ maps,
                                                        float4* __restrict__ coeff, float2* __restrict__ texels) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t rows = (size_t)G.n * 9;
    if (g < rows) {
        coeff[g] = grid_fresh_row(G, (int)(g % 9), sums[g]);
        return;
    }
    const int R = G.R, B = R + 2;
    const size_t t = g - rows;
    if (R == 0 || t >= (size_t)G.n * B * B) return;
    const size_t j = t / ((size_t)B * B);
    const int l = (int)(t - j * B * B);
    const int2 s = grid_border_source(R, l);
    const float4 a = maps[j * R * R + (size_t)s.y * R + s.x];
    texels[t] = make_float2(a.x / G.mapSamples, a.y / G.mapSamples);
}

// The eight corners of a record's cell (include/pt_api.h, steps 4 to 6) from its lowest probe `low` and the fractions f. Inlined twice:
// with `low` in SGPRs the nine coefficient rows of a corner are scalar loads. With STATES a corner whose bit 0 is set adds nothing, the
// live ones also sum their trilinear weights in T, and the end divides the plain mix by T where a corner was left out. With OFFSETS
// the probe stands at fma(i, step, lo) + offset, one rounded add per axis; the cell, the weights and the corner order stay the
// regular grid's. `states` and `offsets` are null in the forms without them.
template <bool MAPS, bool STATES, bool OFFSETS>
PT_DEV float4 grid_corners(const GridParams& G, const float4* __restrict__ coeff, const float2* __restrict__ texels,
                           const unsigned* __restrict__ states, const float4* __restrict__ offsets, const float (&p)[3], const float (&y)[9],
                           const int (&low)[3], const float (&f)[3]) {
    static_assert(MAPS || !OFFSETS, "a grid without maps has no positions to read");
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
        if constexpr (STATES || !MAPS) T = T + tri;
        if constexpr (MAPS) {
            V3 at;
            if constexpr (OFFSETS) {
                const float4 off = offsets[j];
                at = v3(__builtin_fmaf((float)ix, G.step[0], G.lo[0]) + off.x, __builtin_fmaf((float)iy, G.step[1], G.lo[1]) + off.y,
                        __builtin_fmaf((float)iz, G.step[2], G.lo[2]) + off.z);
            } else {
                at = v3(__builtin_fmaf((float)ix, G.step[0], G.lo[0]), __builtin_fmaf((float)iy, G.step[1], G.lo[1]),
                        __builtin_fmaf((float)iz, G.step[2], G.lo[2]));
            }
            const float w = tri * grid_visibility(G, texels + (size_t)j * B2, v3(p[0], p[1], p[2]) - at);
            for (int ch = 0; ch < 3; ch++) num[ch] = __builtin_fmaf(w, e[ch], num[ch]);
            W = W + w;
        }
    }
    if (!MAPS) W = T;                              // the same sum in the same order
    if (MAPS && W >= 1e-6f) return make_float4(num[0] / W, num[1] / W, num[2] / W, W);
    if (!STATES || !skipped) return make_float4(plain[0], plain[1], plain[2], W);
    if (T > 0.0f) return make_float4(plain[0] / T, plain[1] / T, plain[2] / T, W);
    return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

template <bool MAPS, bool STATES, bool OFFSETS>
__global__ void __launch_bounds__(256) grid_lookup_kernel(GridParams G, const float4* __restrict__ coeff, const float2* __restrict__ texels,
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
        out[i] = grid_corners<MAPS, STATES, OFFSETS>(G, coeff, texels, states, offsets, p, y, u, f);
        return;
    }
    out[i] = grid_corners<MAPS, STATES, OFFSETS>(G, coeff, texels, states, offsets, p, y, low, f);
}

static int grid_pack_launch(const GridParams& G, const void* sums, const void* maps, void* packed, hipStream_t stream) {
    const size_t threads = (size_t)G.n * 9 + grid_texels(G);
    hipLaunchKernelGGL(grid_pack_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, G, (const float4*)sums, (const float4*)maps,
                       (float4*)packed, (float2*)((char*)packed + grid_coeff_bytes(G)));
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

static int grid_pack_run(const char* fn, const pt_grid_desc* desc, const void* sums, const void* maps, void* packed, bool host, hipStream_t stream) {
    GridParams G;
    if (int r = grid_params(fn, desc, G)) return r;
    if (!sums) return postfx_fail_fn(-1, fn, "null coeff_sums");
    if (!packed) return postfx_fail_fn(-1, fn, "null packed buffer");
    if (G.R == 0 && maps) return postfx_fail_fn(-1, fn, "maps given although map_res is 0");
    if (G.R != 0 && !maps) return postfx_fail_fn(-1, fn, "null maps although map_res is %d", G.R);
    const size_t sumBytes = grid_coeff_bytes(G), mapBytes = (size_t)G.n * G.R * G.R * sizeof(float4);
    if (!host) {
        if (overlaps(packed, grid_bytes(G), sums, sumBytes) || (maps && overlaps(packed, grid_bytes(G), maps, mapBytes)))
            return postfx_fail_fn(-1, fn, "the packed buffer overlaps an input");
        return grid_pack_launch(G, sums, maps, packed, stream);
    }
    const HostIn in[] = {{sums, sumBytes}, {maps, mapBytes}};
    const HostOut out[] = {{packed, grid_bytes(G)}};
    return postfx_host_form(fn, 0, in, out, [&](char*, char** dIn, char** dOut) { return grid_pack_launch(G, dIn[0], dIn[1], dOut[0], nullptr); });
}

// The instantiation that the grid's maps and the arrays given name. <0, *, 1> does not exist: grid_lookup_run refuses offsets when
// map_res is 0 with the caller's message, and a caller that came another way fails here instead of launching a null kernel.
static int grid_lookup_launch(const GridParams& G, const void* packed, const void* states, const void* offsets, int m, const void* recs, void* out,
                              hipStream_t stream) {
    using Kernel = void (*)(GridParams, const float4*, const float2*, const unsigned*, const float4*, int, const float4*, float4*);
    static const Kernel kKernels[2][2][2] = {{{grid_lookup_kernel<false, false, false>, nullptr}, {grid_lookup_kernel<false, true, false>, nullptr}},
                                             {{grid_lookup_kernel<true, false, false>, grid_lookup_kernel<true, false, true>},
                                              {grid_lookup_kernel<true, true, false>, grid_lookup_kernel<true, true, true>}}};
    const Kernel kernel = kKernels[G.R != 0][states != nullptr][offsets != nullptr];
    if (!kernel) return postfx_fail_fn(-1, "grid_lookup_launch", "offsets given although map_res is 0");
    hipLaunchKernelGGL(kernel, dim3((unsigned)(((size_t)m + 255) / 256)), dim3(256), 0, stream, G, (const float4*)packed,
                       (const float2*)((const char*)packed + grid_coeff_bytes(G)), (const unsigned*)states, (const float4*)offsets, m,
                       (const float4*)recs, (float4*)out);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

enum GridLookupForm { kLookupPlain, kLookupStates, kLookupOffsets };     // the arrays an entry point takes; offsets go with states or without

static int grid_lookup_run(const char* fn, const pt_grid_desc* desc, const void* packed, const void* states, const void* offsets, GridLookupForm form,
                           int m, const void* recs, void* out, bool host, hipStream_t stream) {
    GridParams G;
    if (int r = grid_params(fn, desc, G)) return r;
    if (form == kLookupOffsets && G.R == 0) return postfx_fail_fn(-1, fn, "map_res is 0: a grid without maps has no positions to read");
    if (m < 0) return postfx_fail_fn(-1, fn, "m %d must not be negative", m);
    if (m == 0) return 0;
    if (!packed) return postfx_fail_fn(-1, fn, "null packed buffer");
    if (form == kLookupStates && !states) return postfx_fail_fn(-1, fn, "null states");
    if (form == kLookupOffsets && !offsets) return postfx_fail_fn(-1, fn, "null offsets");
    if (!recs) return postfx_fail_fn(-1, fn, "null records");
    if (!out) return postfx_fail_fn(-1, fn, "null output buffer");
    const size_t recBytes = (size_t)m * 32, outBytes = (size_t)m * 16, stateBytes = (size_t)G.n * 4, offBytes = (size_t)G.n * sizeof(float4);
    if (!host) {
        if (overlaps(out, outBytes, recs, recBytes) || overlaps(out, outBytes, packed, grid_bytes(G)) ||
            (states && overlaps(out, outBytes, states, stateBytes)) || (offsets && overlaps(out, outBytes, offsets, offBytes)))
            return postfx_fail_fn(-1, fn, "the output buffer overlaps an input");
        return grid_lookup_launch(G, packed, states, offsets, m, recs, out, stream);
    }
    const HostIn in[] = {{packed, grid_bytes(G)}, {states, stateBytes}, {offsets, offBytes}, {recs, recBytes}};      // a null array takes no room
    const HostOut o[] = {{out, outBytes}};
    return postfx_host_form(fn, 0, in, o, [&](char*, char** dIn, char** dOut) { return grid_lookup_launch(G, dIn[0], dIn[1], dIn[2], m, dIn[3], dOut[0], nullptr); });
}

}  // namespace pt

using namespace pt;

extern "C" {

size_t pt_grid_packed_bytes(const pt_grid_desc* desc) {
    GridParams G;
    return grid_params("pt_grid_packed_bytes", desc, G) ? 0 : grid_bytes(G);
}

int pt_grid_pack_device(const pt_grid_desc* desc, const void* d_coeff_sums, const void* d_maps, void* d_packed, void* stream) {
    return grid_pack_run("pt_grid_pack", desc, d_coeff_sums, d_maps, d_packed, false, (hipStream_t)stream);
}

int pt_grid_pack(const pt_grid_desc* desc, const float* coeff_sums, const float* maps4, void* packed) {
    return grid_pack_run("pt_grid_pack", desc, coeff_sums, maps4, packed, true, nullptr);
}

int pt_grid_irradiance_device(const pt_grid_desc* desc, const void* d_packed, int m, const void* d_records, void* d_out, void* stream) {
    return grid_lookup_run("pt_grid_irradiance", desc, d_packed, nullptr, nullptr, kLookupPlain, m, d_records, d_out, false, (hipStream_t)stream);
}

int pt_grid_irradiance(const pt_grid_desc* desc, const void* packed, int m, const pt_ray* records, float* out4) {
    return grid_lookup_run("pt_grid_irradiance", desc, packed, nullptr, nullptr, kLookupPlain, m, records, out4, true, nullptr);
}

int pt_grid_irradiance_states_device(const pt_grid_desc* desc, const void* d_packed, const void* d_states, int m, const void* d_records, void* d_out,
                                     void* stream) {
    return grid_lookup_run("pt_grid_irradiance_states", desc, d_packed, d_states, nullptr, kLookupStates, m, d_records, d_out, false, (hipStream_t)stream);
}

int pt_grid_irradiance_states(const pt_grid_desc* desc, const void* packed, const uint32_t* states, int m, const pt_ray* records, float* out4) {
    return grid_lookup_run("pt_grid_irradiance_states", desc, packed, states, nullptr, kLookupStates, m, records, out4, true, nullptr);
}

int pt_grid_irradiance_offsets_device(const pt_grid_desc* desc, const void* d_packed, const void* d_states, const void* d_offsets, int m,
                                      const void* d_records, void* d_out, void* stream) {
    return grid_lookup_run("pt_grid_irradiance_offsets", desc, d_packed, d_states, d_offsets, kLookupOffsets, m, d_records, d_out, false, (hipStream_t)stream);
}

int pt_grid_irradiance_offsets(const pt_grid_desc* desc, const void* packed, const uint32_t* states, const float* offsets4, int m, const pt_ray* records,
                               float* out4) {
    return grid_lookup_run("pt_grid_irradiance_offsets", desc, packed, states, offsets4, kLookupOffsets, m, records, out4, true, nullptr);
}

}  // extern "C"
