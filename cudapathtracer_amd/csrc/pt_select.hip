// pt_select.hip — the selection overlay (pt_select_overlay, include/pt_api.h): up to four selections drawn onto display bytes from the
// ID buffer of pt_render_ids. Entry e selects the pixels whose id word `component` lies in [lo, hi]; a selected pixel with an
// unselected pixel of the image inside its (2 radius + 1)^2 window is an OUTLINE pixel and is blended with the entry's colour at the
// outline alpha, every other selected pixel at the fill alpha. Integer arithmetic only: tests/ids_ref.py restates it in numpy.
//
//   select_overlay_kernel   16x16 pixels per workgroup. The tile and a halo of 4 pixels (the largest radius) are read ONCE from the ID
//                           buffer, one int4 per position, and become one byte each in LDS: bit e says "entry e selects this pixel", and a
//                           position beyond the image has every bit set, so it never makes an outline. A thread whose own byte is 0
//                           is done: it neither reads nor writes its display pixel. The window's AND is separable: one pass ANDs
//                           each row's bytes at |dx| <= j into nibble j of a word (j = 0..4, so one word serves every radius),
//                           every other thread ANDs nine of those words down its column (18 LDS reads a pixel where the square
//                           window takes 81) and blends the entries in order in registers: one dword load, one dword store.
#include <hip/hip_runtime.h>

#include "../../include/pt_api.h"
#include "pt_postfx_host.h"

namespace pt {

constexpr int kSelHalo = 4, kSelTile = 16, kSelSpan = kSelTile + 2 * kSelHalo;

struct SelectK {
    int n;
    int component[4], lo[4], hi[4], radius[4], fillAlpha[4];
    uint32_t colour[4];         // r | g << 8 | b << 16 | outline alpha << 24
};

// (in * (255 - a) + c * a + 127) / 255 on one byte
__device__ inline uint32_t sel_blend(uint32_t in, uint32_t c, uint32_t a) { return (in * (255u - a) + c * a + 127u) / 255u; }

__global__ void __launch_bounds__(256) select_overlay_kernel(int w, int h, const int4* __restrict__ ids, SelectK K, uint32_t* __restrict__ rgba8) {
    __shared__ uint8_t bits[kSelSpan][kSelSpan];
    __shared__ uint32_t rows[kSelSpan][kSelTile];
    const int x0 = blockIdx.x * kSelTile - kSelHalo, y0 = blockIdx.y * kSelTile - kSelHalo;
    for (int i = threadIdx.x; i < kSelSpan * kSelSpan; i += 256) {
        const int lx = i % kSelSpan, ly = i / kSelSpan, x = x0 + lx, y = y0 + ly;
        uint32_t b = 0xfu;                                         // beyond the image: counts as selected by every entry
        if (x >= 0 && x < w && y >= 0 && y < h) {
            const int4 v = ids[(size_t)y * w + x];
            b = 0u;
            for (int e = 0; e < K.n; e++) {
                const int c = K.component[e] == 0 ? v.x : (K.component[e] == 1 ? v.y : v.z);
                if (K.lo[e] <= c && c <= K.hi[e]) b |= 1u << e;
            }
        }
        bits[ly][lx] = (uint8_t)b;
    }
    __syncthreads();
    // the window's AND is separable. Rows first: nibble j of a word holds the AND of the bytes at |dx| <= j in its row
    for (int i = threadIdx.x; i < kSelSpan * kSelTile; i += 256) {
        const int col = i % kSelTile, row = i / kSelTile;
        const uint8_t* b = &bits[row][col + kSelHalo];
        uint32_t run = b[0], word = run;
        for (int j = 1; j <= kSelHalo; j++) {
            run &= (uint32_t)b[-j] & (uint32_t)b[j];
            word |= run << (4 * j);
        }
        rows[row][col] = word;
    }
    __syncthreads();
    const int tx = threadIdx.x & (kSelTile - 1), ty = threadIdx.x / kSelTile;
    const int x = x0 + kSelHalo + tx, y = y0 + kSelHalo + ty;
    if (x >= w || y >= h) return;
    const uint32_t m = bits[ty + kSelHalo][tx + kSelHalo];
    if (m == 0u) return;
    // then columns: nibble j of `within` holds "every pixel at |dx|, |dy| <= j is selected"; the rows at distance k reach nibbles k..4
    uint32_t within = rows[ty + kSelHalo][tx];
    for (int k = 1; k <= kSelHalo; k++)
        within &= (rows[ty + kSelHalo - k][tx] & rows[ty + kSelHalo + k][tx]) | ((1u << (4 * k)) - 1u);
    const size_t p = (size_t)y * w + x;
    const uint32_t px = rgba8[p];
    uint32_t r = px & 0xffu, g = (px >> 8) & 0xffu, bl = (px >> 16) & 0xffu;
    for (int e = 0; e < K.n; e++) {
        if (!((m >> e) & 1u)) continue;
        const bool outline = !((within >> (4 * K.radius[e] + e)) & 1u);
        const uint32_t c = K.colour[e], a = outline ? c >> 24 : (uint32_t)K.fillAlpha[e];
        r = sel_blend(r, c & 0xffu, a); g = sel_blend(g, (c >> 8) & 0xffu, a); bl = sel_blend(bl, (c >> 16) & 0xffu, a);
    }
    rgba8[p] = r | (g << 8) | (bl << 16) | (px & 0xff000000u);
}

// The checks of a list of entries (also pt_preview_set_selection's). n == 0 needs no entries.
int check_select_entries(const char* fn, int n, const pt_select_entry* e) {
    if (n < 0 || n > 4) return postfx_fail_fn(-1, fn, "n %d must be 0..4", n);
    if (n > 0 && !e) return postfx_fail_fn(-1, fn, "null entries");
    for (int i = 0; i < n; i++) {
        if (e[i].component < 0 || e[i].component > 2) return postfx_fail_fn(-1, fn, "entry %d: component %d must be 0 (tri), 1 (material) or 2 (light)", i, e[i].component);
        if (e[i].lo < 0 || e[i].hi < e[i].lo) return postfx_fail_fn(-1, fn, "entry %d: range [%d, %d] must have 0 <= lo <= hi", i, e[i].lo, e[i].hi);
        if (e[i].radius < 1 || e[i].radius > kSelHalo) return postfx_fail_fn(-1, fn, "entry %d: radius %d must be 1..4", i, e[i].radius);
        if (e[i].fill_alpha < 0 || e[i].fill_alpha > 255) return postfx_fail_fn(-1, fn, "entry %d: fill_alpha %d must be 0..255", i, e[i].fill_alpha);
    }
    return 0;
}

// Every check of the overlay, before any HIP call.
static int check_select_args(const char* fn, int w, int h, const void* ids, int n, const pt_select_entry* e, const void* rgba8) {
    if (int r = postfx_check_size(fn, w, h)) return r;
    if (!ids) return postfx_fail_fn(-1, fn, "null ids buffer");
    if (!rgba8) return postfx_fail_fn(-1, fn, "null rgba8 buffer");
    if (int r = check_select_entries(fn, n, e)) return r;
    const size_t px = (size_t)w * h;
    if (overlaps(ids, px * 16, rgba8, px * 4)) return postfx_fail_fn(-1, fn, "ids and rgba8 must not overlap");
    return 0;
}

static int select_launch(int w, int h, const void* ids, int n, const pt_select_entry* e, void* rgba8, hipStream_t stream) {
    if (n == 0) return 0;
    SelectK K = {};
    K.n = n;
    for (int i = 0; i < n; i++) {
        K.component[i] = e[i].component; K.lo[i] = e[i].lo; K.hi[i] = e[i].hi; K.radius[i] = e[i].radius; K.fillAlpha[i] = e[i].fill_alpha;
        K.colour[i] = (uint32_t)e[i].colour[0] | ((uint32_t)e[i].colour[1] << 8) | ((uint32_t)e[i].colour[2] << 16) | ((uint32_t)e[i].colour[3] << 24);
    }
    hipLaunchKernelGGL(select_overlay_kernel, dim3((w + kSelTile - 1) / kSelTile, (h + kSelTile - 1) / kSelTile), dim3(256), 0, stream, w, h,
                       (const int4*)ids, K, (uint32_t*)rgba8);
    POSTFX_HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_select_overlay_device(int w, int h, const void* d_ids, int n, const pt_select_entry* e, void* d_rgba8, void* stream) {
    if (int r = check_select_args("pt_select_overlay", w, h, d_ids, n, e, d_rgba8)) return r;
    return select_launch(w, h, d_ids, n, e, d_rgba8, (hipStream_t)stream);
}

int pt_select_overlay(int w, int h, const int32_t* ids, int n, const pt_select_entry* e, uint8_t* rgba8) {
    if (int r = check_select_args("pt_select_overlay", w, h, ids, n, e, rgba8)) return r;
    if (n == 0) return 0;
    const size_t px = (size_t)w * h;
    const HostIn in[] = {{ids, px * 16}, {rgba8, px * 4}};
    const HostOut out[] = {{rgba8, px * 4, 1}};                   // in place: read back from the slice it was uploaded to
    return postfx_host_form("pt_select_overlay", 0, in, out, [&](char*, char** d, char**) { return select_launch(w, h, d[0], n, e, d[1], nullptr); });
}

}  // extern "C"
