// pt_host.h — what the host translation units behind include/pt_api.h share (pt_api, pt_scene, pt_render, pt_feature_api, pt_probe):
// the error channel, DevBuf, struct pt_scene and the helpers that cross units. Internal: include/pt_api.h never includes it. Host only.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/pt_api.h"
#include "pt_params.h"

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
// Set per scene through pt_set_option (names in quotes; kOptions stores into the int members by pointer-to-member, so an option's
// switch is an int), pt_set_variant and pt_set_culling; the library reads no environment variable. No update resets any of them.
struct Options {
    int variant = 0;             // 0 megakernel, 1 wavefront (pt_set_variant)
    int cull = 0;                // pt_set_culling / "culling": opt-in, not parity-exact by construction
    int schedMask = 31;          // "sched_mask": scheduling checks every schedMask + 1 bounce iterations (tests use 3)
    int sliceAlways = 1;         // "slice_always" 0: slices only once no fresh tile is left
    int sliceIters = 512;        // "slice_iters": time slice of the tile queue (0 = off)
    int lptPrio = 2;             // "lpt_prio": 0 no issue-priority steering, 1 once no fresh tile is left, 2 always (A/B)
    int persistent = 1;          // "persistent" 0: one tile per wave, workgroups launched per 4 tiles (A/B)
    int queueTimeoutMs = 30000;  // "queue_timeout_ms": how long a wait on the tile queue may see no progress (tests use 0-1 to exercise the give-up path)
    int onchipOk = 1;            // "onchip" 0: never pick the LDS-only kernel instantiation (A/B)
    bool wavesHbmOk = true;      // "waves_hbm" 0: scenes in HBM use the 4-waves-per-SIMD kernel too (A/B)
    bool wavesHbmForce = false;  // "waves_hbm" 2: ... and the 6-wave kernel whatever the tile count (tests)
    int nodeKeep = 10, triKeep = 8;       // "node_keep" / "tri_keep" (pt_trace.h: Keep)
    int refill = 1, refillKeep = 6;       // "refill" / "refill_keep": REFILL instantiation of the kernel for scenes in HBM (pt_trace.h: trace_resume)
    bool refillKeepSet = false;           // (unset: the 4-wave kernel of small shares uses kRefillKeepSmall — it is chain-bound and wants its lanes back sooner)
    int flatWanted = 1, simpleWanted = 1, leanWanted = 1;      // "flat" / "simple" / "lean" 0 turns the FLAT kernels / the SIMPLE / the LEAN bounce off (A/B)
    int leafBoxes = 1;           // "leaf_boxes" 0: the FLAT kernels walk the nodes in lockstep instead of testing the leaves' own boxes (A/B)
    int flat2Wanted = 1;         // "flat2" 1 (default): SIMPLE FLAT scenes trace shadow + extension ray in one FLAT pass (DEFER logic step)
    int wfWideWg = 1;            // wavefront trace kernel: 16-wave workgroups for scenes in HBM ("wf_wide_wg")
    int momentsFused = 0;        // "moments_fused" 1: pt_render_moments* renders all its samples in one launch that keeps Q itself, where the kernel has a fused twin
};
// What repack / derive_layout / apply_material_class compute from the scene; an update adopts the staging scene's as a whole.
struct Facts {
    DeviceScene ds{};
    int stackNeed = 0, nInternal = 0, cacheNodes = 0, cacheTris = 0, nTrisPacked = 0, nMats = 0, nLightsPacked = 0;
    int nLeaves = 0;                      // FLAT scenes: the leaf table (pt_trace.h: visited(leaf) == slab(leaf's own box))
    unsigned long long lightTri8 = 0ull;  // a byte per light, for the first 8: 1 + the packed triangle the light is, 0 = none (light_triangles); KParams::lightTri8
    bool armless = false;        // a triangle uses a material type without a dispatch arm (pt_path.h): DEFER is not exact
    bool noLeafTris = false;     // no triangle carries a MAT_LEAF material: a shadow ray is occluded by any hit (order-free)
    bool simpleOk = false;       // scene qualifies for the SIMPLE bounce (diffuse-only, pt_path.h)
    bool leanOk = false;         // ... for the LEAN generic bounce (no MAT_LEAF triangle, no texture / transmission map on any triangle's material)
    bool flatOk = false;         // ... for the FLAT kernels: LDS-resident, at most 128 nodes / triangles (64- or 128-bit masks), checked in derive_layout
};
// ... and what it keeps of the description it was made from (only an update of the whole mesh replaces these). deviceLeaf: the device
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
struct Feature { DevBuf spill, aovOut, motionOut, idsOut; };

}  // namespace pt

struct pt_scene {
    pt::Device dev; pt::Options opt; pt::Facts facts; pt::Kept kept; pt::LastLaunch last; pt::Update upd;
    pt::Geometry geo; pt::Data data; pt::Spare spare; pt::Work work; pt::Wavefront wf; pt::Adaptive ad; pt::Moments mo; pt::Feature feat;
};

namespace pt {

// ---- helpers that cross units: pt_render.hip ... ---------------------------------------------------
int scene_onchip_wg(const pt_scene* s);
bool scene_onchip(const pt_scene* s);
bool hbm_kernel_pays(const pt_scene* s, bool simple, long long tiles);
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

}  // namespace pt
