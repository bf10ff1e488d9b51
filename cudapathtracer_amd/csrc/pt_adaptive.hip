// pt_adaptive.hip — the per-round bookkeeping kernels of adaptive sampling (pt_render_adaptive, include/pt_api.h).
//
// A round renders c samples on the live tiles, snapshots the sums (M = S), renders c more and then runs
//   adaptive_error_kernel    H += S - M, the per-pixel error e, the tile's E_T (a 64-lane max), tile_spp, the stop decision;
//   adaptive_compact_kernel  the live list without the stopped tiles, in the same (ascending) order, and its length;
//   adaptive_queue_save_kernel, after each launch: the tile queue's first 8 words, which the next launch's queue init resets —
//                            the host checks both launches of a round from one read-back (pt_render.hip: render_adaptive).
// pt_render_adaptive_moments adds, after each of a round's two launches,
//   adaptive_moments_kernel  d = S - P, Q = Q + d d per rgb channel, P = S on the live tiles: pt_moments.hip's pass on a list.
// The renders are the ordinary megakernels, launched on the list through the tile queue (pt_kernels.hip: queue_init_list_kernel).
// S, M and H are tile-major over the whole frame ([tile][64] float4, lane = ly*8+lx), so one wave per live tile reads 1 KB
// coalesced per buffer. These kernels run once per round: correct and cheap, not clever. Host side: pt_render.hip.
#include "pt_params.h"

namespace pt {

__global__ void __launch_bounds__(256) adaptive_iota_kernel(int n, int* __restrict__ list) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) list[i] = i;
}

// M = S on the live tiles.
__global__ void __launch_bounds__(256) adaptive_snapshot_kernel(const int* __restrict__ list, int nList, const float4* __restrict__ S,
                                                                float4* __restrict__ M) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= nList) return;
    const size_t o = (size_t)list[i] * 64 + lane;
    M[o] = S[o];
}

// One wave per live tile, lane = pixel: moments_update_kernel's arithmetic (pt_moments.hip) in its order (-ffp-contract=off: the
// product is rounded before the add), on the tiles of the list. Q.w = the batches the tile has taken so far. `first`: the first
// launch of round 0, which lists every tile and takes P = Q = 0 without reading them. Lanes outside the image carry zeros along.
__global__ void __launch_bounds__(256) adaptive_moments_kernel(const int* __restrict__ list, int nList, const float4* __restrict__ S,
                                                               float4* __restrict__ P, float4* __restrict__ Q, int first, float batches) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= nList) return;
    const size_t o = (size_t)list[i] * 64 + lane;
    const float4 s = S[o];
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q = p;
    if (!first) { p = P[o]; q = Q[o]; }
    const float dx = s.x - p.x, dy = s.y - p.y, dz = s.z - p.z;
    q.x = q.x + dx * dx; q.y = q.y + dy * dy; q.z = q.z + dz * dz; q.w = batches;
    P[o] = s;
    Q[o] = q;
}

PT_DEV bool finite3(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

// One wave per live tile, lane = pixel. The arithmetic is the header's, in its order (-ffp-contract=off: no fused products).
// keep[i] = 1: list[i] stays live. tileSpp / tileErr are written for every tile of the round, so they end holding the values
// of the last round the tile took part in.
__global__ void __launch_bounds__(256) adaptive_error_kernel(const int* __restrict__ list, int nList, const float4* __restrict__ S,
                                                             const float4* __restrict__ M, float4* __restrict__ H, int n, int w, int h,
                                                             int tilesX, int minSpp, float threshold, int32_t* __restrict__ tileSpp,
                                                             float* __restrict__ tileErr, int32_t* __restrict__ keep) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= nList) return;
    const int tile = list[i];
    const size_t o = (size_t)tile * 64 + lane;
    const float4 s = S[o], m = M[o], h0 = H[o];
    float4 hn;
    hn.x = h0.x + (s.x - m.x); hn.y = h0.y + (s.y - m.y); hn.z = h0.z + (s.z - m.z); hn.w = h0.w;
    H[o] = hn;
    const int x = (tile % tilesX) * 8 + (lane & 7), y = (tile / tilesX) * 8 + (lane >> 3);
    float e = 0.0f;
    if (x < w && y < h && finite3(s.x, s.y, s.z) && finite3(hn.x, hn.y, hn.z)) {
        const float d = __builtin_fabsf(s.x - 2.0f * hn.x) + __builtin_fabsf(s.y - 2.0f * hn.y) + __builtin_fabsf(s.z - 2.0f * hn.z);
        const float inv = 1.0f / (float)n;
        e = (d * inv) / (1e-4f + __builtin_sqrtf((s.x + s.y + s.z) * inv));
        if (e != e) e = 0.0f;
    }
    for (int k = 32; k > 0; k >>= 1) {             // E_T = max(0, e): every e here is >= 0 and not NaN
        const float other = __shfl_xor(e, k, 64);
        e = other > e ? other : e;
    }
    if (lane == 0) {
        tileSpp[tile] = n;
        tileErr[tile] = e;
        keep[i] = (n >= minSpp && e < threshold) ? 0 : 1;
    }
}

// Ordered compaction in one workgroup of 1024 threads: per chunk of 1024 entries a wave ballot, mbcnt for the lane's rank in
// its wave, the waves' counts through LDS. out[] keeps list[]'s order. *outCount = the new length.
__global__ void __launch_bounds__(1024) adaptive_compact_kernel(const int* __restrict__ list, const int32_t* __restrict__ keep, int nList,
                                                                int* __restrict__ out, int* __restrict__ outCount) {
    __shared__ int waveCount[16];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int base = 0;
    for (int i0 = 0; i0 < nList; i0 += 1024) {
        const int i = i0 + tid;
        const bool k = i < nList && keep[i] != 0;
        const unsigned long long b = __ballot(k);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        if (lane == 0) waveCount[wave] = __builtin_popcountll(b);
        __syncthreads();
        int before = 0, total = 0;
        for (int v = 0; v < 16; v++) {
            const int c = waveCount[v];
            before += v < wave ? c : 0;
            total += c;
        }
        if (k) out[base + before + rank] = list[i];
        base += total;
        __syncthreads();                                   // waveCount is rewritten by the next chunk
    }
    if (tid == 0) *outCount = base;
}

// q[0..7] -> save[0..7], read as the waiters read them (relaxed agent-scope atomics: pt_megakernel.h, the queue protocol).
__global__ void adaptive_queue_save_kernel(const int* q, int* __restrict__ save) {
    const int i = threadIdx.x;
    if (i < 8) save[i] = __hip_atomic_load(const_cast<int*>(q) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t launch_adaptive_iota(int n, int* list, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(adaptive_iota_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, list);
    return hipGetLastError();
}
hipError_t launch_adaptive_snapshot(const int* list, int nList, const float4* S, float4* M, hipStream_t stream) {
    if (nList <= 0) return hipSuccess;
    hipLaunchKernelGGL(adaptive_snapshot_kernel, dim3((nList + 3) / 4), dim3(256), 0, stream, list, nList, S, M);
    return hipGetLastError();
}
hipError_t launch_adaptive_moments(const int* list, int nList, const float4* S, float4* P, float4* Q, bool first, int batches,
                                   hipStream_t stream) {
    if (nList <= 0) return hipSuccess;
    hipLaunchKernelGGL(adaptive_moments_kernel, dim3((nList + 3) / 4), dim3(256), 0, stream, list, nList, S, P, Q, first ? 1 : 0, (float)batches);
    return hipGetLastError();
}
hipError_t launch_adaptive_error(const int* list, int nList, const float4* S, const float4* M, float4* H, int n, int w, int h, int tilesX,
                                 int minSpp, float threshold, int32_t* tileSpp, float* tileErr, int32_t* keep, hipStream_t stream) {
    if (nList <= 0) return hipSuccess;
    hipLaunchKernelGGL(adaptive_error_kernel, dim3((nList + 3) / 4), dim3(256), 0, stream, list, nList, S, M, H, n, w, h, tilesX, minSpp,
                       threshold, tileSpp, tileErr, keep);
    return hipGetLastError();
}
hipError_t launch_adaptive_compact(const int* list, const int32_t* keep, int nList, int* out, int* outCount, hipStream_t stream) {
    hipLaunchKernelGGL(adaptive_compact_kernel, dim3(1), dim3(1024), 0, stream, list, keep, nList, out, outCount);
    return hipGetLastError();
}

hipError_t launch_adaptive_queue_save(const int* q, int* save, hipStream_t stream) {
    hipLaunchKernelGGL(adaptive_queue_save_kernel, dim3(1), dim3(64), 0, stream, q, save);
    return hipGetLastError();
}

}  // namespace pt
