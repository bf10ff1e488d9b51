// pt_query.hip — ray queries (pt_query_closest, pt_query_shadow, pt_query_camera_rays_device; include/pt_api.h): the scene's traversal
// on a caller's own rays. The trace kernels are pt_feature.h's FeatureWave and tile loop, as ids_kernel has them with a PickList:
// "tile" t is rays 64 t .. 64 t + 63, one lane each, four waves per workgroup, persistent over the tiles, the LDS stack overflowing
// into the scene's feature spill area. No camera, no RNG, no seed:
//   query_closest_kernel<SURFACE>  trace_closest (non-counting) with the ray's own max_t; SURFACE adds resolve_hit's record, as a
//                                  template parameter so that the hits-only kernel keeps its own register budget
//   query_shadow_kernel            trace_shadow (non-counting) with the ray's own max_t
//   query_camera_rays_kernel       camera_ray_centre of every pixel as pt_ray records, one thread per pixel
// A ray is two 16-byte loads, a hit one 16-byte store, a surface three, a throughput one. Lanes past n take no ray.
//
// PT_QUERY_REORDER: query_keys_kernel gives ray i the key (octant of d) << 27 | Morton27(o quantised to 9 bits per axis in the scene's
// bounds) and the index i, rocprim sorts the pairs by key, and the trace kernels take perm[i] where they took i. A lane's traversal
// does not depend on what the wave's other lanes hold (trace_closest's and trace_shadow's loop exits are off with Keep{0, 0}, and
// descend_node's wave-wide stack test only chooses between two forms of the same push and pop), so the order changes no output bit.
#include "pt_feature.h"
#include <rocprim/device/device_radix_sort.hpp>

namespace pt {

// The ray of `lane` in tile `tile`: entry i of the order (perm NULL: i itself), or none past n.
PT_DEV bool query_index(const uint32_t* __restrict__ perm, int n, int tile, int lane, uint32_t& r) {
    const int i = tile * 64 + lane;
    if (i >= n) return false;
    r = perm ? perm[i] : (uint32_t)i;
    return true;
}

template <bool SURFACE>
__global__ void __launch_bounds__(256) query_closest_kernel(DeviceScene S, const float4* __restrict__ rays, const uint32_t* __restrict__ perm, int n,
                                                            int nTiles, float4* __restrict__ hits, float4* __restrict__ surfaces, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    FeatureWave W(ldsStack, S, spill);
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        uint32_t r;
        if (!query_index(perm, n, tile, W.lane, r)) continue;
        const QueryRay q = load_ray(rays, r);
        Hit hit;
        trace_closest<false, kStackLds>(S, W.C, q.o, q.d, q.maxT, W.st, hit, W.c);
        float4 oh = make_float4(0.0f, 0.0f, 0.0f, __builtin_bit_cast(float, -1));
        float4 s0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), s1 = s0;
        int4 s2 = make_int4(-1, -1, 0, 0);
        if (hit.tri >= 0) {
            oh = make_float4(hit.t, hit.u, hit.v, __builtin_bit_cast(float, hit.tri));
            if (SURFACE) {
                HitInfo hi; resolve_hit(S, hit, q.o, q.d, hi);
                s0 = make_float4(hi.point.x, hi.point.y, hi.point.z, hi.uvx);
                s1 = make_float4(hi.normal.x, hi.normal.y, hi.normal.z, hi.uvy);
                s2 = make_int4(hi.material, hi.lightInd < 0 ? -1 : hi.lightInd, hi.backface ? 1 : 0, 0);     // (PAttr's lightInd is -51 for no light)
            }
        }
        hits[r] = oh;
        if (SURFACE) {
            float4* s = surfaces + 3 * (size_t)r;
            s[0] = s0; s[1] = s1; *(int4*)(s + 2) = s2;
        }
    }
}

__global__ void __launch_bounds__(256) query_shadow_kernel(DeviceScene S, const float4* __restrict__ rays, const uint32_t* __restrict__ perm, int n,
                                                           int nTiles, float4* __restrict__ throughput, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    FeatureWave W(ldsStack, S, spill);
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        uint32_t r;
        if (!query_index(perm, n, tile, W.lane, r)) continue;
        const QueryRay q = load_ray(rays, r);
        const V3 t = trace_shadow<false, kStackLds>(S, W.C, q.o, q.d, q.maxT, W.st, W.c);
        throughput[r] = make_float4(t.x, t.y, t.z, 0.0f);
    }
}

__global__ void __launch_bounds__(256) query_camera_rays_kernel(CamK cam, int n, float maxT, float4* __restrict__ rays) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    V3 o, d;
    camera_ray_centre(cam, i % cam.w, i / cam.w, o, d);
    rays[2 * (size_t)i] = make_float4(o.x, o.y, o.z, maxT);
    rays[2 * (size_t)i + 1] = make_float4(d.x, d.y, d.z, 0.0f);       // (pad = 0)
}

// Bits 0..8 of v spread to every third bit.
PT_DEV uint32_t spread9(uint32_t v) {
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// One coordinate of an origin as a cell 0..511 of [lo, hi]; outside the bounds: the nearest cell. (A flat scene: ext 0, cell 0.)
PT_DEV uint32_t query_cell(float x, float lo, float hi) {
    const float ext = hi - lo;
    const float c = ext > 0.0f ? (x - lo) / ext * 512.0f : 0.0f;
    return (uint32_t)fminf_(fmaxf_(c, 0.0f), 511.0f);
}

// The sort's input. Only called for a scene whose root is an internal node (the host's test): its record holds both children's boxes.
__global__ void __launch_bounds__(256) query_keys_kernel(DeviceScene S, const float4* __restrict__ rays, int n, uint32_t* __restrict__ keys,
                                                         uint32_t* __restrict__ idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4* node = (const float4*)(S.nodes + S.rootRef);
    const float4 a = node[0], b = node[1], c = node[2];     // left min (a.xyz), left max (a.w, b.xy), right min (b.zw, c.x), right max (c.yzw)
    const QueryRay q = load_ray(rays, (uint32_t)i);
    uint32_t key = 0;
    const float big = 3.402823466e+38f;
    if (__builtin_fabsf(q.o.x) <= big && __builtin_fabsf(q.o.y) <= big && __builtin_fabsf(q.o.z) <= big) {      // (false for NaN and inf)
        const uint32_t cx = query_cell(q.o.x, fminf_(a.x, b.z), fmaxf_(a.w, c.y));
        const uint32_t cy = query_cell(q.o.y, fminf_(a.y, b.w), fmaxf_(b.x, c.z));
        const uint32_t cz = query_cell(q.o.z, fminf_(a.z, c.x), fmaxf_(b.y, c.w));
        const uint32_t octant = (q.d.x < 0.0f ? 1u : 0u) | (q.d.y < 0.0f ? 2u : 0u) | (q.d.z < 0.0f ? 4u : 0u);
        key = (octant << 27) | spread9(cx) | (spread9(cy) << 1) | (spread9(cz) << 2);
    }
    keys[i] = key;
    idx[i] = (uint32_t)i;
}

hipError_t launch_query_closest(const DeviceScene& S, int n, const void* rays, const uint32_t* perm, int blocks, void* hits, void* surfaces,
                                int32_t* spill, hipStream_t stream) {
    const int nTiles = (n + 63) / 64;
    if (surfaces)
        hipLaunchKernelGGL(query_closest_kernel<true>, dim3(blocks), dim3(256), 0, stream, S, (const float4*)rays, perm, n, nTiles, (float4*)hits,
                           (float4*)surfaces, spill);
    else
        hipLaunchKernelGGL(query_closest_kernel<false>, dim3(blocks), dim3(256), 0, stream, S, (const float4*)rays, perm, n, nTiles, (float4*)hits,
                           (float4*)nullptr, spill);
    return hipGetLastError();
}

hipError_t launch_query_shadow(const DeviceScene& S, int n, const void* rays, const uint32_t* perm, int blocks, void* throughput, int32_t* spill,
                               hipStream_t stream) {
    hipLaunchKernelGGL(query_shadow_kernel, dim3(blocks), dim3(256), 0, stream, S, (const float4*)rays, perm, n, (n + 63) / 64, (float4*)throughput, spill);
    return hipGetLastError();
}

hipError_t launch_query_camera_rays(const CamK& cam, int w, int h, float maxT, void* rays, hipStream_t stream) {
    const int n = w * h;
    hipLaunchKernelGGL(query_camera_rays_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, cam, n, maxT, (float4*)rays);
    return hipGetLastError();
}

hipError_t launch_query_keys(const DeviceScene& S, int n, const void* rays, uint32_t* keys, uint32_t* idx, hipStream_t stream) {
    hipLaunchKernelGGL(query_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, S, (const float4*)rays, n, keys, idx);
    return hipGetLastError();
}

// rocprim's radix sort of the (key, index) pairs over the key's 30 bits. temp NULL: only *tempBytes is set, nothing is launched.
hipError_t query_sort(void* temp, size_t* tempBytes, const uint32_t* keysIn, uint32_t* keysOut, const uint32_t* idxIn, uint32_t* idxOut, int n,
                      hipStream_t stream) {
    return rocprim::radix_sort_pairs(temp, *tempBytes, keysIn, keysOut, idxIn, idxOut, (size_t)n, 0u, 30u, stream);
}

}  // namespace pt
