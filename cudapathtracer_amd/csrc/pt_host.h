// pt_host.h — what the host translation units behind include/pt_api.h share (pt_api, pt_scene, pt_render, pt_feature_api, pt_probe):
// the error channel, DevBuf, struct pt_scene and the helpers that cross units. Internal: include/pt_api.h never includes it. Host only.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/pt_api.h"
#include "pt_plan.h"

namespace pt {

// ---- errors (pt_api.hip): the message pt_last_error returns, per thread -----------------------
int fail(int code, const char* fmt, ...);
#define HIP_OK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return pt::fail(-2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    int ensure(size_t n) {
        if (n <= bytes) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) return fail(-2, "hipMalloc(%zu) failed: %s", n, hipGetErrorString(e));
        bytes = n;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

// ---- the groups of pt_scene ---------------------------------------------------------------------
struct Device { int id = 0, numCU = 256; hipEvent_t ev0 = nullptr, ev1 = nullptr; };      // ev0 / ev1: around the last render launch
// Options (what pt_set_option stores) and Facts (what the scene knows about itself), the two groups the launch decision reads, are
// in pt_plan.h. Kept: what a scene keeps of the description it was made from (only an update of the whole mesh replaces these). deviceLeaf: the device
// builder's leaf size; -1: the tree was the caller's (pt_scene_create)
struct Kept { int deviceLeaf = -1, nPositions = 0, nNormals = 0, nUvs = 0, nTexels = 0; };
// The last render launch, for pt_scene_flags, the queue-word checks and the counters' entry points.
struct LastLaunch {
    int flat = 0, simple = 0, leafTable = 0, flat2 = 0, lean = 0, refill = 0;      // which instantiation it was (pt_scene_flags)
    int hbm = -1;                // which megakernel it used (-1: none yet)
    bool queued = false;         // the last megakernel launch used the tile queue (only then is its error word that launch's)
    int tiles = 0;               // ... and held this many tiles (the frame's, in list mode: the waiters' exit test)
    int pushed = 0;              // ... of which it queued this many at the start (pt_last_tile_handovers: pushes beyond them are hand-overs)
    int queueStalls = 0;         // launches whose waiters gave up (q[3] != 0) although every tile was finished: not an error, counted (pt_queue_stalls)
    int momentsLaunches = -1;    // render launches of the last pt_render_moments* call (pt_last_moments_launches; -1: none yet)
    float kernelMs = 0.0f; bool evPending = false;      // evPending: ev0/ev1 recorded, elapsed time not read yet
    void forget() { flat = simple = leafTable = flat2 = lean = refill = 0; hbm = -1; }     // after an update: there is no launch on the new records yet
};
struct Update {
    int generation = 0;          // pt_scene_generation: +1 per successful update
    bool hasMotion = false;      // pt_scene_has_motion: the last successful update was a vertex update
    float renumberMs = 0.0f, updateMs = 0.0f;   // host wall clock of the last renumber_by_area / of the last successful update (pt_debug_update_ms)
    DevBuf edit;                 // pt_scene_update_materials / _emission: the edit's table and the kernel's result word
};
// Scene data: the packed records an update rebuilds; the tables, and what the device builder packs from, kept on the device (dynamic
// geometry); the spare halves an update builds into and swaps in on success, with the builder's pool (grown on demand, freed at destroy).
// posCur / posPrev (pt_render_motion): the positions as of the last successful update (or creation) and, while hasMotion, those before
// it. A vertex update copies its positions into posPrev and swaps the pair; 2 x 16 B per vertex, device-built scenes only.
struct Geometry { DevBuf nodes, tris, attrs, lights, leaves; };
struct Data { DevBuf mats, textures, jump, totals, kTris, kNormals, kUvs, kTypes, kLightTris, posCur, posPrev; };
struct Spare { Geometry geo; DevBuf normals, pool; };
struct Work { DevBuf rng, spill, tilebuf, colors, pixcnt, queue, left; };      // render work buffers, grown on demand
struct Wavefront { DevBuf state, ctl, ctr, spill; };                           // wavefront variant
// pt_render_adaptive: sums, snapshot, half sums, live lists; _moments: previous sums, squared batch sums (tile-major); err: the
// device form's tile errors when the caller passes none; out: host-form staging
struct Adaptive { DevBuf S, M, H, list, keep, count, P, Q, err, out; };
// pt_render_moments: sums, previous sums, squared batch sums (tile-major); host-form staging; _tiles, host form: the list on the device
struct Moments { DevBuf S, P, Q, out, list; };
// the feature passes: their own traversal spill area; host-form staging of pt_render_aovs*, pt_render_motion*, pt_render_ids / pt_pick
// and of pt_query_*; a reordered query's keys and indices (in and out halves each) and rocprim's sort workspace
struct Feature { DevBuf spill, aovOut, motionOut, idsOut, queryOut, queryKeys, queryIdx, querySort; };

}  // namespace pt

struct pt_scene {
    pt::Device dev; pt::Options opt; pt::Facts facts; pt::Kept kept; pt::LastLaunch last; pt::Update upd;
    pt::Geometry geo; pt::Data data; pt::Spare spare; pt::Work work; pt::Wavefront wf; pt::Adaptive ad; pt::Moments mo; pt::Feature feat;
};

namespace pt {

// ---- helpers that cross units: pt_render.hip ... ---------------------------------------------------
int resolve_tiles(int w, int h, const pt_tile_range* tiles, TileSpan& t);
CamK cam_to_kernel(const pt_camera& c);
int check_render_args(pt_scene* s, const pt_camera* cam, int spp, int integrator);
// ... pt_api.hip ...
int queue_error(pt_scene* s);
int queue_words_error(pt_scene* s, const int* q, int tiles);
int wait_and_check(pt_scene* s, hipStream_t stream);
// ... and pt_adaptive.hip
hipError_t launch_adaptive_iota(int n, int* list, hipStream_t stream);
hipError_t launch_adaptive_snapshot(const int* list, int nList, const float4* S, float4* M, hipStream_t stream);
hipError_t launch_adaptive_error(const int* list, int nList, const float4* S, const float4* M, float4* H, int n, int w, int h, int tilesX,
                                 int minSpp, float threshold, int32_t* tileSpp, float* tileErr, int32_t* keep, hipStream_t stream);
hipError_t launch_adaptive_compact(const int* list, const int32_t* keep, int nList, int* out, int* outCount, hipStream_t stream);
hipError_t launch_adaptive_queue_save(const int* q, int* save, hipStream_t stream);
hipError_t launch_adaptive_moments(const int* list, int nList, const float4* S, float4* P, float4* Q, bool first, int batches, hipStream_t stream);

// A host form: render(d) into `staging`, where d[i] is output i's slice (NULL for an output the caller left out, whose slice stays
// reserved), then the copies to the host in order.
struct StagedOut { void* host; size_t bytes; };
template <int N, class Render>
static int staged_download(DevBuf& staging, const StagedOut (&out)[N], Render render) {
    size_t total = 0;
    for (const StagedOut& o : out) total += o.bytes;
    if (int r = staging.ensure(total)) return r;
    void* d[N];
    char* at = (char*)staging.p;
    for (int i = 0; i < N; at += out[i++].bytes) d[i] = out[i].host ? at : nullptr;
    if (int r = render(d)) return r;
    for (int i = 0; i < N; i++)
        if (out[i].host) HIP_OK(hipMemcpy(out[i].host, d[i], out[i].bytes, hipMemcpyDeviceToHost));
    return 0;
}

// A ray query's host form: the n rays go up into the head of `staging`, run(dRays, d) works there, d[i] being output i's slice
// behind them (NULL for an output the caller left out, which gets no slice), then the copies to the host in order.
template <int N, class Run>
static int staged_query(DevBuf& staging, int n, const pt_ray* rays, const StagedOut (&out)[N], Run run) {
    const size_t rayBytes = (size_t)n * sizeof(pt_ray);
    size_t total = rayBytes;
    for (const StagedOut& o : out) total += o.host ? o.bytes : 0;
    if (int r = staging.ensure(total)) return r;
    HIP_OK(hipMemcpy(staging.p, rays, rayBytes, hipMemcpyHostToDevice));
    void* d[N];
    char* at = (char*)staging.p + rayBytes;
    for (int i = 0; i < N; i++) { d[i] = out[i].host ? at : nullptr; at += out[i].host ? out[i].bytes : 0; }
    if (int r = run(staging.p, d)) return r;
    for (int i = 0; i < N; i++)
        if (out[i].host) HIP_OK(hipMemcpy(out[i].host, d[i], out[i].bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace pt
