// pt_grid.h — what the probe-grid units share (pt_grid.hip: pack and every lookup; pt_grid_live.hip: probe states
// and in-place updates, §30; pt_grid_relocate.hip: probe offsets, §31): the grid a desc names as the kernels read it, the desc's
// checks, the packed buffer's layout, the words pack and update both write (a gutter texel's source, a coefficient row), and the
// Chebyshev visibility of a point from a probe's bordered map.
#pragma once
#include <cmath>

#include "../../include/pt_api.h"
#include "pt_device.h"
#include "pt_postfx_host.h"

namespace pt {

struct GridParams {
    float lo[3], inv[3], step[3], top[3];       // top = (float)max(counts - 2, 0); inv = step = 0 on an axis with one probe
    int counts[3];
    int n;                                      // probes
    int R, power;
    float Rf;
    float scale, mapSamples;                    // the pack's
};

constexpr float kShC0 = 0.2820948f, kShC1 = 0.4886025f, kShC2 = 1.0925484f, kShC3 = 0.3153916f, kShC4 = 0.5462742f;    // include/pt_api.h

PT_DEV bool finite_(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// The Chebyshev visibility of a point at `v` from a probe whose bordered map starts at `map` (include/pt_api.h, step 5).
PT_DEV float grid_visibility(const GridParams& G, const float2* __restrict__ map, V3 v) {
    const float dist = __builtin_sqrtf(dot(v, v));
    const V3 d = dist > 0.0f ? v : v3(0.0f, 0.0f, 1.0f);
    const float s = (__builtin_fabsf(d.x) + __builtin_fabsf(d.y)) + __builtin_fabsf(d.z);
    const float px = d.x / s, py = d.y / s;
    float qx = px, qy = py;
    if (d.z < 0.0f) {
        qx = (1.0f - __builtin_fabsf(py)) * __builtin_copysignf(1.0f, d.x);
        qy = (1.0f - __builtin_fabsf(px)) * __builtin_copysignf(1.0f, d.y);
    }
    const float gx = ((qx + 1.0f) * 0.5f) * G.Rf + 0.5f, gy = ((qy + 1.0f) * 0.5f) * G.Rf + 0.5f;
    const float ix = fminf_(fmaxf_(__builtin_floorf(gx), 0.0f), G.Rf), iy = fminf_(fmaxf_(__builtin_floorf(gy), 0.0f), G.Rf);
    const float wx = gx - ix, wy = gy - iy;
    const float2* row = map + (int)iy * (G.R + 2) + (int)ix;
    const float2 t00 = row[0], t10 = row[1], t01 = row[G.R + 2], t11 = row[G.R + 3];
    const float topM = t00.x + wx * (t10.x - t00.x), topQ = t00.y + wx * (t10.y - t00.y);
    const float botM = t01.x + wx * (t11.x - t01.x), botQ = t01.y + wx * (t11.y - t01.y);
    const float mean = topM + wy * (botM - topM), m2 = topQ + wy * (botQ - topQ);
    float var = m2 - mean * mean;
    var = var > 0.0f ? var : 0.0f;
    const float t = dist - mean;
    const float den = var + t * t;
    const float ratio = den > 0.0f ? var / den : 0.0f;
    float vis = ratio;
    for (int k = 1; k < G.power; k++) vis = vis * ratio;
    return dist <= mean ? 1.0f : vis;
}

// The interior texel (sx, sy) that texel l of a probe's bordered (R + 2)^2 map copies: itself off the gutter, rays.oct_border's rule on it.
PT_DEV int2 grid_border_source(int R, int l) {
    const int B = R + 2;
    int sx = l % B - 1, sy = l / B - 1;
    if (sx < 0) { sx = -1 - sx; sy = R - 1 - sy; } else if (sx > R - 1) { sx = 2 * R - 1 - sx; sy = R - 1 - sy; }
    if (sy < 0) { sy = -1 - sy; sx = R - 1 - sx; } else if (sy > R - 1) { sy = 2 * R - 1 - sy; sx = R - 1 - sx; }
    return make_int2(sx, sy);
}

// The packed word of coefficient row k (0..8) from its query sums c: scaled, then convolved with the cosine lobe of the row's band.
PT_DEV float4 grid_fresh_row(const GridParams& G, int k, float4 c) {
    const float lobe = k == 0 ? 3.14159265358979323846f : (k < 4 ? 2.09439510239319549231f : 0.78539816339744830962f);
    return make_float4((c.x * G.scale) * lobe, (c.y * G.scale) * lobe, (c.z * G.scale) * lobe, 0.0f);
}

// The desc's checks in the header's order; on success G holds what the kernels read.
static inline int grid_params(const char* fn, const pt_grid_desc* d, GridParams& G) {
    if (!d) return postfx_fail_fn(-1, fn, "null desc");
    const int32_t* c3 = d->counts;
    if (c3[0] < 1 || c3[1] < 1 || c3[2] < 1) return postfx_fail_fn(-1, fn, "counts %d x %d x %d must be at least 1 each", c3[0], c3[1], c3[2]);
    const long long n = (long long)c3[0] * c3[1] > (1ll << 22) ? (1ll << 23) : (long long)c3[0] * c3[1] * c3[2];
    if (n > (1ll << 22)) return postfx_fail_fn(-1, fn, "counts %d x %d x %d make more than %d probes", c3[0], c3[1], c3[2], 1 << 22);
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(d->lo[a]) || !std::isfinite(d->hi[a])) return postfx_fail_fn(-1, fn, "corner lo[%d] = %g, hi[%d] = %g is not finite", a, d->lo[a], a, d->hi[a]);
        if (d->counts[a] > 1 && !(d->hi[a] > d->lo[a])) return postfx_fail_fn(-1, fn, "hi[%d] = %g must be above lo[%d] = %g", a, d->hi[a], a, d->lo[a]);
    }
    if (d->sh_samples < 1) return postfx_fail_fn(-1, fn, "sh_samples %d must be at least 1", d->sh_samples);
    const int R = d->map_res;
    if (R != 0 && R != 4 && R != 8 && R != 16 && R != 32) return postfx_fail_fn(-1, fn, "map_res %d must be 0, 4, 8, 16 or 32", R);
    if (R != 0 && d->map_samples < 1) return postfx_fail_fn(-1, fn, "map_samples %d must be at least 1", d->map_samples);
    if (d->power < 1 || d->power > 8) return postfx_fail_fn(-1, fn, "power %d must be 1..8", d->power);
    for (int a = 0; a < 3; a++) {
        const int c = d->counts[a];
        const double span = (double)d->hi[a] - (double)d->lo[a];
        G.lo[a] = d->lo[a];
        G.inv[a] = c > 1 ? (float)((c - 1) / span) : 0.0f;
        G.step[a] = c > 1 ? (float)(span / (c - 1)) : 0.0f;
        G.top[a] = (float)(c > 1 ? c - 2 : 0);
        G.counts[a] = c;
    }
    G.n = (int)n;
    G.R = R; G.Rf = (float)R; G.power = d->power;
    G.scale = (float)(4.0 * 3.14159265358979323846 / (double)d->sh_samples);
    G.mapSamples = (float)d->map_samples;
    return 0;
}

// The checks of a probe list (pt_grid_classify, pt_grid_update, pt_grid_relocate): k against n, NULL indices only for the identity.
static inline int live_list_checks(const char* fn, const GridParams& G, int k, const void* indices) {
    if (k > G.n) return postfx_fail_fn(-1, fn, "k %d lists more than the grid's %d probes", k, G.n);
    if (!indices && k != G.n) return postfx_fail_fn(-1, fn, "null indices need k == %d, the grid's probes, not %d", G.n, k);
    return 0;
}

static inline size_t grid_coeff_bytes(const GridParams& G) { return (size_t)G.n * 9 * sizeof(float4); }
static inline size_t grid_texels(const GridParams& G) { return G.R ? (size_t)G.n * (G.R + 2) * (G.R + 2) : 0; }
static inline size_t grid_bytes(const GridParams& G) { return grid_coeff_bytes(G) + grid_texels(G) * sizeof(float2); }

}  // namespace pt
