// pt_api.hip — implementation of the C ABI in include/pt_api.h: scene re-pack + upload, the
// launcher boundary (launch_unidirectional / launch_naive_unidirectional, deviceCode.cuh:8-12)
// and the probe entry points. Host code only; the kernels live in pt_kernels.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pt_api.h"
#include "pt_params.h"
#include "pt_feature_host.h"
#include "pt_bvh_build.h"
#include "xorwow_host.h"

using namespace pt;

static_assert(sizeof(pt_bvh_node) == 48 && sizeof(pt_triangle) == 80 && sizeof(pt_material) == 176 && sizeof(pt_camera) == 112,
              "boundary structs must keep the reference's CUDA layouts (SURVEY.md Appendix A)");
static_assert(offsetof(pt_triangle, emission) == 48 && offsetof(pt_triangle, lightInd) == 64, "Triangle layout");
static_assert(offsetof(pt_material, type) == 32 && offsetof(pt_material, albedo) == 48 && offsetof(pt_material, eta) == 80 &&
              offsetof(pt_material, ior) == 112 && offsetof(pt_material, isSpecular) == 128 && offsetof(pt_material, absorption) == 144 &&
              offsetof(pt_material, priority) == 160, "Material layout");
static_assert(offsetof(pt_camera, forward) == 64 && offsetof(pt_camera, fovScale) == 44, "Camera layout");

// ---- errors ---------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_OK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(-2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
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

struct pt_scene {
    int device = 0;
    DevBuf nodes, tris, attrs, lights, mats, textures, jump, totals, leaves;
    int wfWideWg = 1;                                 // wavefront trace kernel: 16-wave workgroups for scenes in HBM ("wf_wide_wg")
    int nLeaves = 0;                                  // FLAT scenes: the leaf table (pt_trace.h: visited(leaf) == slab(leaf's own box))
    DevBuf rng, spill, tilebuf, colors, pixcnt, queue, left; // work buffers, grown on demand
    DevBuf wfState, wfCtl, wfCtr, wfSpill;            // wavefront variant
    DevBuf aovSpill, aovOut;                          // pt_render_aovs: its own traversal spill area / host-form staging
    DevBuf adS, adM, adH, adList, adKeep, adCount, adOut, adSpp, adErr;   // pt_render_adaptive: sums, snapshot, half sums, live lists; host-form staging
    DevBuf adP, adQ, adSq;                            // pt_render_adaptive_moments: previous sums, squared batch sums (tile-major); host-form staging
    DevBuf moS, moP, moQ, moOut;                      // pt_render_moments: sums, previous sums, squared batch sums (tile-major); host-form staging
    DevBuf moList;                                    // pt_render_moments_tiles, host form: the tile list on the device
    int variant = 0;                                  // 0 megakernel, 1 wavefront (pt_set_variant)
    int numCU = 256;
    DeviceScene ds{};
    int stackNeed = 0, nInternal = 0, cacheNodes = 0, cacheTris = 0;
    int nMats = 0, nLightsPacked = 0, nTexels = 0;
    bool armless = false;        // a triangle uses a material type without a dispatch arm (pt_path.h): DEFER is not exact
    // Everything below is set per scene through pt_set_option (names in quotes; kOptions stores into the int members by
    // pointer-to-member, so an option's switch is an int); the library reads no environment variable.
    int schedMask = 31;          // "sched_mask": scheduling checks every schedMask + 1 bounce iterations (tests use 3)
    int sliceAlways = 1;         // "slice_always" 0: slices only once no fresh tile is left
    bool wavesHbmOk = true;   // "waves_hbm" 0: scenes in HBM use the 4-waves-per-SIMD kernel too (A/B)
    int nodeKeep = 10, triKeep = 8;        // "node_keep" / "tri_keep" (pt_trace.h: Keep)
    int refill = 1, refillKeep = 6;       // "refill" / "refill_keep": REFILL instantiation of the kernel for scenes in HBM (pt_trace.h: trace_resume)
    bool refillKeepSet = false;           // (unset: the 4-wave kernel of small shares uses kRefillKeepSmall — it is chain-bound and wants its lanes back sooner)
    int cull = 0;                         // pt_set_culling / "culling": opt-in, not parity-exact by construction
    unsigned long long lightTri8 = 0ull;          // a byte per light, for the first 8: 1 + the packed triangle the light is, 0 = none (light_triangles); KParams::lightTri8
    int leafBoxes = 1;                            // "leaf_boxes" 0: the FLAT kernels walk the nodes in lockstep instead of testing the leaves' own boxes (A/B)
    int flat2Wanted = 1; int lastLaunchFlat2 = 0;   // "flat2" 1 (default): SIMPLE FLAT scenes trace shadow + extension ray in one FLAT pass (DEFER logic step)
    bool noLeafTris = false;                      // no triangle carries a MAT_LEAF material: a shadow ray is occluded by any hit (order-free)
    int queueTimeoutMs = 30000;                   // "queue_timeout_ms": how long a wait on the tile queue may see no progress (tests use 0-1 to exercise the give-up path)
    int queueStalls = 0;                          // launches whose waiters gave up (q[3] != 0) although every tile was finished: not an error, counted (pt_queue_stalls)
    bool leanOk = false; int leanWanted = 1;      // scene qualifies for the LEAN generic bounce (no MAT_LEAF triangle, no texture / transmission map on any triangle's material) / "lean" 0 turns it off (A/B)
    int lastLaunchLean = 0;
    int momentsFused = 0;                         // "moments_fused" 1: pt_render_moments* renders all its samples in one launch that keeps Q itself, where the kernel has a fused twin
    int lastMomentsLaunches = -1;                 // render launches of the last pt_render_moments* call (pt_last_moments_launches; -1: none yet)
    bool simpleOk = false; int simpleWanted = 1;  // scene qualifies for the SIMPLE bounce (diffuse-only, pt_path.h) / "simple" 0 turns it off (A/B)
    bool flatOk = false; int flatWanted = 1;      // "flat": 0 off, 1 (or 2) on: scenes of at most 128 nodes / triangles (64- or 128-bit masks)   // scene qualifies for the FLAT kernels (checked in repack) / "flat" 0 turns them off (A/B)
    int lastLaunchFlat = 0, lastLaunchSimple = 0, lastLaunchLeafTable = 0;
    bool lastLaunchQueued = false;        // the last megakernel launch used the tile queue (only then is its error word that launch's)
    int lastLaunchTiles = 0;              // ... and held this many tiles (the frame's, in list mode: the waiters' exit test)
    int lastLaunchPushed = 0;             // ... of which it queued this many at the start (pt_last_tile_handovers: pushes beyond them are hand-overs)
    int lastLaunchRefill = 0;             // ... and whether it was a REFILL instantiation
    int lastLaunchHbm = -1;               // which megakernel the last launch used (-1: none yet)
    bool wavesHbmForce = false;           // "waves_hbm" 2: ... and the 6-wave kernel whatever the tile count (tests)
    int onchipOk = 1;            // "onchip" 0: never pick the LDS-only kernel instantiation (A/B)
    int nTrisPacked = 0;
    int sliceIters = 512;        // "slice_iters": time slice of the tile queue (0 = off)
    int lptPrio = 2;             // "lpt_prio": 0 no issue-priority steering, 1 once no fresh tile is left, 2 always (A/B)
    int persistent = 1;          // "persistent" 0: one tile per wave, workgroups launched per 4 tiles (A/B)
    // dynamic geometry (pt_scene_update_*): what the device builder packs from, kept on the device; the spare halves an update builds
    // into and swaps in on success; the builder's pool (grown on demand, freed at destroy)
    int generation = 0;                   // pt_scene_generation: +1 per successful update
    int deviceLeaf = -1;                  // the device builder's leaf size; -1: the tree was the caller's (pt_scene_create)
    int nPositions = 0, nNormals = 0, nUvs = 0;
    DevBuf kTris, kNormals, kUvs, kTypes, kLightTris;
    DevBuf spNodes, spTris, spAttrs, spLights, spLeaves, spNormals;
    DevBuf buildPool;
    // motion (pt_render_motion): the positions as of the last successful update (or creation) and, while hasMotion, those before it.
    // A vertex update copies its positions into posPrev and swaps the pair; 2 x 16 B per vertex, device-built scenes only.
    DevBuf posCur, posPrev;
    bool hasMotion = false;               // pt_scene_has_motion: the last successful update was a vertex update
    DevBuf motionOut;                     // pt_render_motion, host form: staging
    DevBuf idsOut;                        // pt_render_ids, host form, and pt_pick: staging
    DevBuf edit;                          // pt_scene_update_materials / _emission: the edit's table and the kernel's result word
    float renumberMs = 0.0f, updateMs = 0.0f;   // host wall clock of the last renumber_by_area / of the last successful update (pt_debug_update_ms)
    float lastKernelMs = 0.0f;
    bool evPending = false;                            // ev0/ev1 recorded, elapsed time not read yet
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

static int queue_error(pt_scene* s);
static int queue_words_error(pt_scene* s, const int* q, int tiles);

// LDS-resident instantiation: every PNode and PTri in the scene cache, the tree no deeper than the LDS stack, and the
// records the bounce reads (PAttr, PMat, PLight) within their own LDS budget.
// Its workgroups hold ONE copy of the scene each, and a CU has 160 KB of LDS for its 16 waves: workgroups of 4, 8 or 16
// waves get 1, 2 or 4 times the budgets kCacheBytes (PNodes + PTris) and kAttrCacheBytes. Returns the smallest workgroup
// size (in waves) that holds the scene, 0 if none does.
static int scene_onchip_wg(const pt_scene* s) {
    if (!s->onchipOk || s->nTrisPacked <= 0 || s->ds.stackSpill != 0) return 0;
    const size_t geom = (size_t)s->nInternal * 64 + (size_t)s->nTrisPacked * 48, rec = attr_cache_bytes(s->nTrisPacked, s->nMats, s->nLightsPacked);
    // ... and 16 / wg such workgroups must fit a CU's 160 KB with the largest per-wave area any LDS-resident kernel uses (the pair
    // pass scratch, 24 x 256 B, plus the medium stack of the non-SIMPLE kernels): a Cornell box of glass, water and gold at four
    // waves per workgroup was 1 KB over — three workgroups per CU instead of four, 19 % of the frame (round 3)
    const size_t perWave = (size_t)kStackFlat2Rows * 256 + (s->simpleOk && s->simpleWanted ? 0 : (size_t)kMediumMax * 64);
    for (int wg = 4; wg <= 16; wg *= 2)
        if (geom <= (size_t)kCacheBytes * (wg / 4) && (kAttrCacheBytes == 0 || rec <= (size_t)kAttrCacheBytes * (wg / 4)) &&
            geom + rec + (size_t)wg * perWave <= (size_t)160 * 1024 * wg / 16) return wg;
    return 0;
}
static bool scene_onchip(const pt_scene* s) { return scene_onchip_wg(s) > 0; }
// Does a launch of `tiles` tiles get megakernel_hbm — six waves per SIMD, eight with the SIMPLE bounce — and not the general 4-wave
// kernel? A scene in HBM does, with enough tiles to fill those waves: with fewer (a 1/8 shard of a 1080p frame is 4050 tiles for 6144
// slots) the extra slots stay empty and the 4-wave kernel's faster waves win (measured: 1/8 shard 176 vs 185 ms, 1/4 shard equal, 1/2
// shard 602 vs 518 ms on the 263 k-triangle scene). The SIMPLE kernel's eight waves pay from ~3/4 of its 8192 slots on — a 1/4 share of
// a 1080p frame: 201 vs 269 ms — the generic kernel's six from 5/4 of its 6144 (profiles/r02_sched_shards.log).
static bool hbm_kernel_pays(const pt_scene* s, bool simple, long long tiles) {
    if (scene_onchip(s) || !s->wavesHbmOk) return false;
    const long long slots = (long long)s->numCU * 4 * (simple ? kWavesHbmSimple : kWavesHbm);
    return s->wavesHbmForce || tiles * 4 >= slots * (simple ? 3 : 5);
}

extern "C" {

int pt_fail_(int code, const char* msg) { g_err = msg; return code; }     // for the other translation units

int pt_api_version(void) { return PT_API_VERSION; }
const char* pt_last_error(void) { return g_err.c_str(); }

int pt_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(-2, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

void pt_scene_destroy(pt_scene* s) {
    if (!s) return;
    DevBuf* all[] = {&s->nodes, &s->tris, &s->attrs, &s->lights, &s->mats, &s->textures, &s->jump, &s->totals, &s->leaves,
                     &s->rng, &s->spill, &s->tilebuf, &s->colors, &s->pixcnt, &s->queue, &s->left, &s->wfState, &s->wfCtl, &s->wfCtr, &s->wfSpill,
                     &s->aovSpill, &s->aovOut, &s->adS, &s->adM, &s->adH, &s->adList, &s->adKeep, &s->adCount, &s->adOut, &s->adSpp, &s->adErr,
                     &s->adP, &s->adQ, &s->adSq,
                     &s->moS, &s->moP, &s->moQ, &s->moOut, &s->moList,
                     &s->kTris, &s->kNormals, &s->kUvs, &s->kTypes, &s->kLightTris,
                     &s->spNodes, &s->spTris, &s->spAttrs, &s->spLights, &s->spLeaves, &s->spNormals, &s->buildPool,
                     &s->posCur, &s->posPrev, &s->motionOut, &s->idsOut, &s->edit};
    for (DevBuf* b : all) b->release();
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    delete s;
}

static double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static int upload(DevBuf& b, const void* src, size_t bytes) {
    if (int r = b.ensure(std::max<size_t>(bytes, 16))) return r;
    if (bytes) HIP_OK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return 0;
}

// The leaf table of the FLAT kernels replaces the reference's root-to-leaf box walk by a test of each leaf's OWN box.
// That equals the reference's visiting set only if every box contains the boxes
// below it and no box holds a NaN or an infinity (pt_trace.h: inv_is_regular and the monotonicity argument above it). The
// reference's builder nests exactly (a parent's box is the float-wise min / max of its children's, main.cu:20-233), but
// pt_scene_create also takes a caller's own BVH arrays — a refit, loose or corrupt tree must fall back to the walk that
// tests the boxes the caller gave. pn: packed internal nodes, children numbered after their parents.
static bool boxes_nested_and_finite(const std::vector<PNode>& pn, int nInternal) {
    for (int i = 0; i < nInternal; i++) {
        const PNode& p = pn[i];
        for (int a = 0; a < 3; a++)
            if (!(std::isfinite(p.lmin[a]) && std::isfinite(p.lmax[a]) && std::isfinite(p.rmin[a]) && std::isfinite(p.rmax[a]))) return false;
        const int32_t ref[2] = {p.left, p.right};
        for (int k = 0; k < 2; k++) {
            if (ref[k] < 0) continue;                              // a leaf child: its box IS the one the table tests
            if (ref[k] <= i || ref[k] >= nInternal) return false;
            const PNode& c = pn[ref[k]];
            const float* mn = k == 0 ? p.lmin : p.rmin; const float* mx = k == 0 ? p.lmax : p.rmax;
            for (int a = 0; a < 3; a++)
                if (!(mn[a] <= c.lmin[a] && mn[a] <= c.rmin[a] && mx[a] >= c.lmax[a] && mx[a] >= c.rmax[a])) return false;
        }
    }
    return true;
}

// For each light: the packed triangle (position in leaf order, the FLAT kernels' numbering) it was made from, or -1. The pair pass
// leaves that triangle out of the tests of a shadow ray aimed at the light (pt_trace.h: trace_pair_flat), which is exact only if
// the bounce's own test of the ray against the light (PLight a, b - a, c - a) and the pass's test against the triangle (PTri v0, e1,
// e2) see the same operands: checked here bit for bit, on the records as the kernels read them. A light that is no triangle of
// the scene, or whose vertices are in another order, gets -1 and its shadow rays are tested against everything.
// The records are read as the kernels read them: PLight a, b, c ARE the positions' floats, and lightIndOf(idx) is the lightInd of
// original triangle idx (anything outside 0..nLights-1 matches no light), so the table can be made from a description's host
// arrays and from a scene's device records alike.
extern "C++" {
template <class LightIndOf>
static void light_triangles(const PTri* pt, int nT, const PLight* lights, int nLights, int nTriangles, LightIndOf lightIndOf, int32_t* out) {
    for (int i = 0; i < nLights; i++) {
        out[i] = -1;
        const PLight& L = lights[i];
        const float v0[3] = {L.a[0], L.a[1], L.a[2]}, e1[3] = {L.b[0] - L.a[0], L.b[1] - L.a[1], L.b[2] - L.a[2]},
                    e2[3] = {L.c[0] - L.a[0], L.c[1] - L.a[1], L.c[2] - L.a[2]};
        for (int p = 0; p < nT && p < 63; p++) {                 // (the pair pass holds a ray's triangles in one 64-bit mask, and clears bit p as (1 << (p + 1)) >> 1)
            const int idx = (int)(pt[p].idx & 0x7fffffffu);
            if (idx >= nTriangles || lightIndOf(idx) != i) continue;
            if (!memcmp(pt[p].v0, v0, 12) && !memcmp(pt[p].e1, e1, 12) && !memcmp(pt[p].e2, e2, 12)) { out[i] = p; break; }
        }
    }
}
}  // extern "C++"
// ... from a description: a light whose vertex indices are out of range gets -1.
static void light_triangles(const PTri* pt, int nT, const pt_scene_desc* d, int32_t* out) {
    std::vector<PLight> L((size_t)std::max(d->n_lights, 1));
    std::vector<uint8_t> bad((size_t)std::max(d->n_lights, 1), 0);
    for (int i = 0; i < d->n_lights; i++) {
        const pt_triangle& t = d->lights[i];
        L[i] = PLight{};
        if (t.aInd < 0 || t.aInd >= d->n_positions || t.bInd < 0 || t.bInd >= d->n_positions || t.cInd < 0 || t.cInd >= d->n_positions) { bad[i] = 1; continue; }
        const pt_float4 a = d->positions[t.aInd], b = d->positions[t.bInd], c = d->positions[t.cInd];
        L[i].a[0] = a.x; L[i].a[1] = a.y; L[i].a[2] = a.z; L[i].b[0] = b.x; L[i].b[1] = b.y; L[i].b[2] = b.z; L[i].c[0] = c.x; L[i].c[1] = c.y; L[i].c[2] = c.z;
    }
    light_triangles(pt, nT, L.data(), d->n_lights, d->n_triangles, [&](int idx) { const int li = d->triangles[idx].lightInd; return (li >= 0 && li < d->n_lights && bad[li]) ? -1 : li; }, out);
}

// Re-pack the reference's data model for gfx950.
// deviceLeaf < 0: the caller's BVH, packed on the host. deviceLeaf >= 0 (pt_scene_create_from_mesh): the tree is built AND
// packed on the device (pt_bvh_build.hip) with that leaf size; d->bvh / d->bvh_indices are not read.
static int renumber_by_area(pt_scene* s, int nInternal, int rootRef);
static int derive_layout(pt_scene* s, int nInternal, int stackNeed, int rootRef, int nT, int nLights, bool haveLights, int nMats, const PLight* hostLights,
                         const int32_t* lightIndOf, int nLightInd);

// The material table as the kernels read it, and the class word of every row (pt_bvh_build.h: pt_material_class_). Creation and
// pt_scene_update_materials both pack through here; fn names the caller in the message of a refused texture window.
static int pack_materials(const pt_material* materials, int nMats, int nTexels, const char* fn, std::vector<PMat>& mats, std::vector<uint32_t>& matClass) {
    mats.resize((size_t)nMats); matClass.resize((size_t)nMats);
    std::memset(mats.data(), 0, mats.size() * sizeof(PMat));
    for (int i = 0; i < nMats; i++) {
        const pt_material& m = materials[i];
        PMat& p = mats[i];
        p.type = m.type;
        p.flags = (m.hasTexture ? kMatHasTexture : 0) | (m.hasTransMap ? kMatHasTransMap : 0) | (m.isSpecular ? kMatSpecular : 0) | (m.boundary ? kMatBoundary : 0);
        p.priority = m.priority;
        p.texStart = m.startInd; p.texW = m.width; p.texH = m.height;
        if ((m.hasTexture || m.hasTransMap) && m.width > 0 && m.height > 0 &&
            (m.startInd < 0 || (long long)m.startInd + (long long)m.width * m.height > nTexels))
            return fail(-1, "%s: material %d texture window exceeds the texel array", fn, i);
        p.roughness = m.roughness; p.ior = m.ior; p.transmission = m.transmission;
        p.albedo[0] = m.albedo.x; p.albedo[1] = m.albedo.y; p.albedo[2] = m.albedo.z;
        p.eta[0] = m.eta.x; p.eta[1] = m.eta.y; p.eta[2] = m.eta.z;
        p.k[0] = m.k.x; p.k[1] = m.k.y; p.k[2] = m.k.z;
        p.absorption[0] = m.absorption.x; p.absorption[1] = m.absorption.y; p.absorption[2] = m.absorption.z;
        p.albedoOverPi[0] = m.albedo.x / kPi; p.albedoOverPi[1] = m.albedo.y / kPi; p.albedoOverPi[2] = m.albedo.z / kPi;   // cosine_f, reflectors.cuh:10-13
        matClass[i] = pt_material_class_(m);
    }
    return 0;
}

// What a scene decides from its triangles' materials alone, from `used` = the class words of the rows its triangles use, OR-ed:
// all four from scratch, since an edit can clear what another set.
// SIMPLE scenes (pt_path.h): every triangle's material an untextured MAT_DIFFUSE that is neither boundary nor specular, in air
// (material 0) that does not absorb — then the medium stack never changes and the dispatchers have one arm. noLeafTris: no triangle
// carries MAT_LEAF. LEAN (pt_shade.h): additionally no triangle's material samples a texture. armless: pt_bvh_build.h.
static void apply_material_class(pt_scene* s, uint32_t used, const pt_material& air) {
    s->simpleOk = air.absorption.x == 0.0f && air.absorption.y == 0.0f && air.absorption.z == 0.0f && !(used & kRowNotSimple);
    s->noLeafTris = !(used & kTriLeaf);
    s->leanOk = s->noLeafTris && !(used & kRowTextured);
    s->armless = (used & kTriArmless) != 0;
}

// update: the scene is being updated in place (pt_scene_update_mesh): `s` is the staging scene whose buffers are swapped in on
// success; the jump table and the counters stay the live scene's and are not touched here.
static int repack(pt_scene* s, const pt_scene_desc* d, int deviceLeaf = -1, pt_bvh_build_stats* buildStats = nullptr, bool update = false) {
    const bool onDevice = deviceLeaf >= 0;
    const int nT = d->n_triangles, nN = onDevice ? 1 : d->n_nodes;
    if (nT <= 0 || nN <= 0 || !d->triangles || (!onDevice && (!d->bvh || !d->bvh_indices)) || !d->positions || !d->materials)
        return fail(-1, "pt_scene_create: empty scene (the reference aborts with 'No triangles loaded', main.cu:505-508)");
    if (d->n_materials <= 0 || d->n_materials > 256) return fail(-1, "pt_scene_create: %d materials (1..256 supported)", d->n_materials);

    int nInternal = 0, stackNeed = 0, rootRef = 0;
    std::vector<PNode> nodes; std::vector<PTri> tris; std::vector<PAttr> attrs;
    auto pos = [&](int i, const char* what, int tri, bool& ok) -> pt_float4 {
        if (i < 0 || i >= d->n_positions) { ok = false; fail(-1, "pt_scene_create: triangle %d %s index %d out of range", tri, what, i); return pt_float4{0, 0, 0, 0}; }
        return d->positions[i];
    };
    if (!onDevice) {
    // --- internal nodes renumbered BREADTH-FIRST from the root, so PNodes [0, K) are the top of the
    //     tree (the part every ray visits) and can be staged in LDS as one contiguous block ---
    std::vector<int> internalId(nN, -1);
    for (int i = 0; i < nN; i++) {
        const pt_bvh_node& n = d->bvh[i];
        if (n.primCount > 0) {
            if (n.first < 0 || n.first + n.primCount > nT) return fail(-1, "pt_scene_create: leaf %d range [%d,+%d) out of bounds", i, n.first, n.primCount);
        } else {
            if (n.left < 0 || n.right < 0 || n.left >= nN || n.right >= nN) return fail(-1, "pt_scene_create: internal node %d has child out of range", i);
        }
    }
    {
        std::vector<int> queue;
        if (d->bvh[0].primCount <= 0) { queue.push_back(0); internalId[0] = nInternal++; }
        for (size_t q = 0; q < queue.size(); q++) {
            const pt_bvh_node& n = d->bvh[queue[q]];
            for (int c : {n.left, n.right}) {
                if (d->bvh[c].primCount > 0) continue;
                if (internalId[c] >= 0 || (int)queue.size() >= nN) return fail(-1, "pt_scene_create: BVH is not a tree");
                internalId[c] = nInternal++;
                queue.push_back(c);
            }
        }
    }
    // Scenes in HBM: the kernels keep PNodes [0, K) in LDS, so number the internal nodes by how often rays visit them rather
    // than by level — a ray enters a box with a probability proportional to its surface area (the SAH's own estimate), and a
    // child's box lies inside its parent's, so descending area (ties: breadth-first order) still numbers parents first.
    // (Against plain breadth-first numbering: 82 k triangles 765 -> 729 ms at 128 spp, 263 k 387 -> 379 ms at 16 spp, 7.5 % fewer
    // node fetches from global memory; profiles/r03_ab_node_order_area.log)
    if (nInternal > 128) {
        std::vector<float> area((size_t)nInternal, 0.0f);
        for (int i = 0; i < nN; i++) {
            if (internalId[i] < 0) continue;
            const pt_bvh_node& n = d->bvh[i];
            const float dx = n.aabbMAX.x - n.aabbMIN.x, dy = n.aabbMAX.y - n.aabbMIN.y, dz = n.aabbMAX.z - n.aabbMIN.z;
            const float a = dx * dy + dy * dz + dz * dx;
            area[internalId[i]] = std::isfinite(a) ? a : 0.0f;
        }
        std::vector<int> order((size_t)nInternal);
        for (int i = 0; i < nInternal; i++) order[i] = i;
        std::stable_sort(order.begin() + 1, order.end(), [&](int a, int b) { return area[a] > area[b]; });     // the root stays node 0
        std::vector<int> rank((size_t)nInternal);
        for (int k = 0; k < nInternal; k++) rank[order[k]] = k;
        for (int i = 0; i < nN; i++) if (internalId[i] >= 0) internalId[i] = rank[internalId[i]];
    }
    auto childRef = [&](int c) -> int32_t { return d->bvh[c].primCount > 0 ? ~d->bvh[c].first : internalId[c]; };
    nodes.assign(std::max(nInternal, 1), PNode{});
    std::vector<uint8_t> leafEnd(nT, 0);
    for (int i = 0; i < nN; i++) {
        const pt_bvh_node& n = d->bvh[i];
        if (n.primCount > 0) { leafEnd[n.first + n.primCount - 1] = 1; continue; }
        if (internalId[i] < 0) continue;                       // unreachable from the root
        PNode& p = nodes[internalId[i]];
        const pt_bvh_node& L = d->bvh[n.left];
        const pt_bvh_node& R = d->bvh[n.right];
        p.lmin[0] = L.aabbMIN.x; p.lmin[1] = L.aabbMIN.y; p.lmin[2] = L.aabbMIN.z;
        p.lmax[0] = L.aabbMAX.x; p.lmax[1] = L.aabbMAX.y; p.lmax[2] = L.aabbMAX.z;
        p.rmin[0] = R.aabbMIN.x; p.rmin[1] = R.aabbMIN.y; p.rmin[2] = R.aabbMIN.z;
        p.rmax[0] = R.aabbMAX.x; p.rmax[1] = R.aabbMAX.y; p.rmax[2] = R.aabbMAX.z;
        p.left = childRef(n.left); p.right = childRef(n.right); p.pad0 = p.pad1 = 0;
    }
    // stack need = the largest number of internal nodes on a root-to-leaf path (each can leave one
    // far child pending); also rejects cycles.
    {
        std::vector<std::pair<int, int>> st; st.push_back({0, 1});
        size_t visited = 0;
        while (!st.empty()) {
            auto [i, depth] = st.back(); st.pop_back();
            if (++visited > (size_t)nN) return fail(-1, "pt_scene_create: BVH is not a tree");
            if (d->bvh[i].primCount > 0) continue;
            stackNeed = std::max(stackNeed, depth);
            st.push_back({d->bvh[i].left, depth + 1});
            st.push_back({d->bvh[i].right, depth + 1});
        }
    }
    if (stackNeed > 128) return fail(-1, "pt_scene_create: BVH depth %d exceeds the reference's nodeStack[128] (integratorUtilities.cuh:89)", stackNeed);

    // --- triangles in leaf order ---
    tris.resize(nT);
    for (int i = 0; i < nT; i++) {
        int idx = d->bvh_indices[i];
        if (idx < 0 || idx >= nT) return fail(-1, "pt_scene_create: BVHindices[%d] = %d out of range", i, idx);
        const pt_triangle& t = d->triangles[idx];
        bool ok = true;
        pt_float4 a = pos(t.aInd, "a", idx, ok), b = pos(t.bInd, "b", idx, ok), c = pos(t.cInd, "c", idx, ok);
        if (!ok) return -1;
        if (t.materialID < 0 || t.materialID >= d->n_materials) return fail(-1, "pt_scene_create: triangle %d material %d out of range", idx, t.materialID);
        PTri& p = tris[i];
        p.v0[0] = a.x; p.v0[1] = a.y; p.v0[2] = a.z;
        p.e1[0] = b.x - a.x; p.e1[1] = b.y - a.y; p.e1[2] = b.z - a.z;      // trib - tria, integratorUtilities.cuh:13
        p.e2[0] = c.x - a.x; p.e2[1] = c.y - a.y; p.e2[2] = c.z - a.z;      // tric - tria, :14
        p.idx = (uint32_t)idx | (leafEnd[i] ? 0x80000000u : 0u);
        p.material = t.materialID;
        p.flags = pt_tri_flags_(d->materials[t.materialID].type);
    }
    // --- hit attributes by original index ---
    attrs.resize(nT);
    for (int i = 0; i < nT; i++) {
        const pt_triangle& t = d->triangles[i];
        PAttr& a = attrs[i];
        const int ni[3] = {t.naInd, t.nbInd, t.ncInd}, ui[3] = {t.uvaInd, t.uvbInd, t.uvcInd};
        float* nd[3] = {a.n0, a.n1, a.n2}; float* ud[3] = {a.uv0, a.uv1, a.uv2};
        for (int k = 0; k < 3; k++) {
            if (ni[k] < 0 || ni[k] >= d->n_normals || !d->normals) return fail(-1, "pt_scene_create: triangle %d normal index %d out of range (faces without vn must be given a normal by the loader)", i, ni[k]);
            if (ui[k] < 0 || ui[k] >= d->n_uvs || !d->uvs) return fail(-1, "pt_scene_create: triangle %d uv index %d out of range", i, ui[k]);
            nd[k][0] = d->normals[ni[k]].x; nd[k][1] = d->normals[ni[k]].y; nd[k][2] = d->normals[ni[k]].z;
            ud[k][0] = d->uvs[ui[k]].x; ud[k][1] = d->uvs[ui[k]].y;
        }
        a.emission[0] = t.emission.x; a.emission[1] = t.emission.y; a.emission[2] = t.emission.z;
        a.material = t.materialID;
        a.lightInd = (t.lightInd >= 0 && t.lightInd < d->n_lights) ? t.lightInd : -51;
    }
    rootRef = childRef(0);
    }
    // --- lights ---
    std::vector<PLight> lights(std::max(d->n_lights, 1));
    std::memset(lights.data(), 0, lights.size() * sizeof(PLight));
    for (int i = 0; i < d->n_lights; i++) {
        const pt_triangle& t = d->lights[i];
        bool ok = true;
        pt_float4 a = pos(t.aInd, "a", i, ok), b = pos(t.bInd, "b", i, ok), c = pos(t.cInd, "c", i, ok);
        if (!ok) return -1;
        if (t.naInd < 0 || t.naInd >= d->n_normals) return fail(-1, "pt_scene_create: light %d normal index out of range", i);
        PLight& L = lights[i];
        L.a[0] = a.x; L.a[1] = a.y; L.a[2] = a.z; L.b[0] = b.x; L.b[1] = b.y; L.b[2] = b.z; L.c[0] = c.x; L.c[1] = c.y; L.c[2] = c.z;
        L.na[0] = d->normals[t.naInd].x; L.na[1] = d->normals[t.naInd].y; L.na[2] = d->normals[t.naInd].z;
        L.emission[0] = t.emission.x; L.emission[1] = t.emission.y; L.emission[2] = t.emission.z;
        // area = 0.5f * length(cross3(b - a, c - a)) exactly as the kernels used to evaluate it per NEE sample: IEEE
        // subtractions, cross = fma(p, q, -(r * s)), dot = fma(z, z', fma(y, y', x * x')), correctly rounded sqrt
        const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
        const float cx = fmaf(uy, vz, -(uz * vy)), cy = fmaf(uz, vx, -(ux * vz)), cz = fmaf(ux, vy, -(uy * vx));
        L.area = 0.5f * sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
    }
    // --- materials ---
    std::vector<PMat> mats; std::vector<uint32_t> matClass;
    if (int r = pack_materials(d->materials, d->n_materials, d->n_texels, "pt_scene_create", mats, matClass)) return r;
    {
        uint32_t used = 0u;                       // the classes of the rows the triangles use (a device-built scene's builder refuses an index outside the table)
        for (int i = 0; i < nT; i++) {
            const int id = d->triangles[i].materialID;
            if (id >= 0 && id < d->n_materials) used |= matClass[id];
        }
        apply_material_class(s, used, d->materials[0]);
    }
    if (!onDevice) {
        if (int r = upload(s->nodes, nodes.data(), nodes.size() * sizeof(PNode))) return r;
        if (int r = upload(s->tris, tris.data(), tris.size() * sizeof(PTri))) return r;
        if (int r = upload(s->attrs, attrs.data(), attrs.size() * sizeof(PAttr))) return r;
    } else {
        if (int r = s->nodes.ensure((size_t)nT * sizeof(PNode))) return r;
        if (int r = s->tris.ensure((size_t)nT * sizeof(PTri))) return r;
        if (int r = s->attrs.ensure((size_t)nT * sizeof(PAttr))) return r;
        std::vector<int> types(d->n_materials);
        for (int i = 0; i < d->n_materials; i++) types[i] = d->materials[i].type;
        // what the builder packs from stays on the device with the scene: pt_scene_update_vertices rebuilds from it
        if (int r = upload(s->kTris, d->triangles, (size_t)nT * sizeof(pt_triangle))) return r;
        if (int r = upload(s->kNormals, d->normals, d->normals ? (size_t)std::max(d->n_normals, 0) * sizeof(pt_float4) : 0)) return r;
        if (int r = upload(s->kUvs, d->uvs, d->uvs ? (size_t)std::max(d->n_uvs, 0) * sizeof(pt_float2) : 0)) return r;
        if (int r = upload(s->kTypes, types.data(), types.size() * sizeof(int))) return r;
        if (int r = upload(s->kLightTris, d->lights, d->lights ? (size_t)std::max(d->n_lights, 0) * sizeof(pt_triangle) : 0)) return r;
        if (int r = upload(s->posCur, d->positions, (size_t)d->n_positions * sizeof(pt_float4))) return r;      // the motion pass reads them
        s->deviceLeaf = deviceLeaf; s->nPositions = d->n_positions; s->nNormals = d->normals ? std::max(d->n_normals, 0) : 0; s->nUvs = d->uvs ? std::max(d->n_uvs, 0) : 0;
        pt_build_src_ src{};
        src.positions = d->positions; src.n_positions = d->n_positions; src.positions_on_device = 0;
        src.d_triangles = (const pt_triangle*)s->kTris.p; src.n_triangles = nT;
        src.d_normals = (const pt_float4*)s->kNormals.p; src.n_normals = s->nNormals;
        src.d_uvs = (const pt_float2*)s->kUvs.p; src.n_uvs = s->nUvs;
        src.d_mat_types = (const int*)s->kTypes.p; src.n_materials = d->n_materials;
        src.d_light_tris = (const pt_triangle*)s->kLightTris.p; src.n_lights = d->n_lights;
        if (update) { src.pool = &s->buildPool.p; src.pool_bytes = &s->buildPool.bytes; }     // (creation allocates and frees its pool, as it always did)
        int out5[5] = {0, 0, 0, 0, 0};
        if (int r = pt_bvh_build_pack_(&src, deviceLeaf, s->nodes.p, s->tris.p, s->attrs.p, nullptr, out5, buildStats)) return r;
        nInternal = out5[0]; stackNeed = out5[1]; rootRef = out5[2];
        if (out5[3]) s->armless = true;
        if (stackNeed > 128) return fail(-1, "pt_scene_create_from_mesh: BVH depth %d exceeds the reference's nodeStack[128] (integratorUtilities.cuh:89)", stackNeed);
        if (int r = renumber_by_area(s, nInternal, rootRef)) return r;
    }
    if (int r = upload(s->lights, lights.data(), lights.size() * sizeof(PLight))) return r;
    if (int r = upload(s->mats, mats.data(), mats.size() * sizeof(PMat))) return r;
    if (int r = upload(s->textures, d->textures, (size_t)std::max(d->n_texels, 0) * sizeof(float4))) return r;
    s->nTexels = d->n_texels;                 // (what a later material edit checks its texture windows against, as above)
    if (!update) {
        const std::vector<uint32_t>& jt = xorwow_host::jump_table();
        if (int r = upload(s->jump, jt.data(), jt.size() * sizeof(uint32_t))) return r;
        if (int r = s->totals.ensure(16 * sizeof(unsigned long long))) return r;      // 8 counters + 6 diagnostic stamp sums
        HIP_OK(hipMemset(s->totals.p, 0, 16 * sizeof(unsigned long long)));
    }
    std::vector<int32_t> lightInd;                         // (only the scenes the pair kernels can run look at it)
    if (nT <= 128) { lightInd.resize((size_t)nT); for (int i = 0; i < nT; i++) lightInd[i] = d->triangles[i].lightInd; }
    return derive_layout(s, nInternal, stackNeed, rootRef, nT, d->n_lights, d->lights != nullptr, d->n_materials, lights.data(), lightInd.data(), (int)lightInd.size());
}

// Scenes in HBM: the numbering the host re-pack gives the internal nodes (descending surface area of a node's own box — here
// read from its parent's record, the same floats — so that the LDS copy of PNodes [0, K) holds the most-visited ones), applied to
// the records the device builder packed into s->nodes. Through the host: one download and one upload of the internal nodes.
static int renumber_by_area(pt_scene* s, int nInternal, int rootRef) {
    s->renumberMs = 0.0f;
    const double t0 = wall_ms();
        if (nInternal > 128 && rootRef == 0) {
            std::vector<PNode> pn((size_t)nInternal);
            HIP_OK(hipMemcpy(pn.data(), s->nodes.p, (size_t)nInternal * sizeof(PNode), hipMemcpyDeviceToHost));
            std::vector<float> area((size_t)nInternal, 0.0f);
            std::vector<int> bfs; bfs.reserve((size_t)nInternal); bfs.push_back(0);
            std::vector<uint8_t> seen((size_t)nInternal, 0); seen[0] = 1;
            bool tree = true;
            for (size_t q = 0; q < bfs.size() && tree; q++) {
                const PNode& p = pn[bfs[q]];
                const int32_t ref[2] = {p.left, p.right};
                for (int k = 0; k < 2; k++) {
                    if (ref[k] < 0) continue;
                    if (ref[k] >= nInternal || seen[ref[k]]) { tree = false; break; }
                    seen[ref[k]] = 1;
                    const float* mn = k == 0 ? p.lmin : p.rmin; const float* mx = k == 0 ? p.lmax : p.rmax;
                    const float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
                    const float a = dx * dy + dy * dz + dz * dx;
                    area[ref[k]] = std::isfinite(a) ? a : 0.0f;
                    bfs.push_back(ref[k]);
                }
            }
            if (tree && (int)bfs.size() == nInternal) {
                // bfs[k]: k-th node in breadth-first order; sort those positions by area (stable: ties keep breadth-first order)
                std::vector<int> order(bfs);
                std::stable_sort(order.begin() + 1, order.end(), [&](int a, int b) { return area[a] > area[b]; });
                std::vector<int> rank((size_t)nInternal);
                for (int k = 0; k < nInternal; k++) rank[order[k]] = k;
                std::vector<PNode> out((size_t)nInternal);
                for (int i = 0; i < nInternal; i++) {
                    PNode p = pn[i];
                    if (p.left >= 0) p.left = rank[p.left];
                    if (p.right >= 0) p.right = rank[p.right];
                    out[rank[i]] = p;
                }
                HIP_OK(hipMemcpy(s->nodes.p, out.data(), (size_t)nInternal * sizeof(PNode), hipMemcpyHostToDevice));
            }
            s->renumberMs = (float)(wall_ms() - t0);
        }
    return 0;
}

// What creation derives from the packed records in s->nodes / tris / attrs / lights, and an update derives again: the device
// scene's pointers, the LDS cache split, the spill need, whether the FLAT kernels can run it (and then the leaf counts in the
// PNodes' spare words, the leaf table and the lights' triangles). hostLights: the PLight records as uploaded (haveLights: the
// scene has a light list at all); lightIndOf[i]: lightInd of original triangle i (nLightInd entries; read only for scenes of at
// most 128 triangles).
static int derive_layout(pt_scene* s, int nInternal, int stackNeed, int rootRef, int nT, int nLights, bool haveLights, int nMats, const PLight* hostLights,
                         const int32_t* lightIndOf, int nLightInd) {
    std::vector<int32_t> lightTri((size_t)std::max(nLights, 1), -1);      // filled in below for the scenes the pair kernels can run
    s->lightTri8 = 0ull;
    s->nInternal = nInternal;
    s->stackNeed = stackNeed;
    s->ds.nodes = (const PNode*)s->nodes.p; s->ds.tris = (const PTri*)s->tris.p; s->ds.attrs = (const PAttr*)s->attrs.p;
    s->ds.lights = (const PLight*)s->lights.p; s->ds.mats = (const PMat*)s->mats.p; s->ds.textures = (const float4*)s->textures.p;
    s->ds.rootRef = rootRef;
    s->ds.nLights = nLights; s->ds.nTris = nT;
    s->nMats = nMats; s->nLightsPacked = std::max(nLights, 1);
    s->ds.stackSpill = std::max(0, stackNeed - kStackLds);
    // scene cache: everything if it fits the LDS budget, else only the top of the (breadth-first) tree
    s->nTrisPacked = nT;
    if ((size_t)nInternal * 64 + (size_t)nT * 48 <= (size_t)kCacheBytes) { s->cacheNodes = nInternal; s->cacheTris = nT; }
    else { s->cacheNodes = std::min(nInternal, kCacheBytes / 64); s->cacheTris = 0; }
    // FLAT kernels (pt_trace.h): one forward pass over the internal nodes with 64- or 128-bit masks — needs at most 128 of
    // each, every child numbered after its parent (the breadth-first numbering gives that; checked on the packed records)
    // and the triangle count of every leaf child, which goes into the spare words of its PNode.
    s->flatOk = false;
    if (nInternal <= 128 && nT >= 1 && nT <= 128 && scene_onchip_wg(s) > 0) {
        std::vector<PNode> pn((size_t)std::max(nInternal, 1));
        std::vector<PTri> pt((size_t)nT);
        if (nInternal > 0) HIP_OK(hipMemcpy(pn.data(), s->nodes.p, (size_t)nInternal * sizeof(PNode), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(pt.data(), s->tris.p, (size_t)nT * sizeof(PTri), hipMemcpyDeviceToHost));
        auto leafCount = [&](int first) {                      // triangles up to and including the one flagged last
            int k = first;
            while (k < nT) { uint32_t w; memcpy(&w, (const char*)&pt[k] + 36, 4); k++; if (w & 0x80000000u) return k - first; }
            return 0;                                          // runs off the end: not a well-formed leaf
        };
        bool ok = rootRef < 0 ? (~rootRef == 0 && leafCount(0) == nT) : (rootRef == 0);
        std::vector<int> first((size_t)std::max(nInternal, 1), 0);   // first triangle below node i
        for (int i = nInternal - 1; i >= 0 && ok; i--) {          // children come after their parent: bottom-up
            int32_t* ref = &pn[i].left;                         // left, right, pad0, pad1
            int firstOf[2] = {0, 0};
            for (int k = 0; k < 2 && ok; k++) {
                if (ref[k] >= 0) {
                    ok = ref[k] > i && ref[k] < nInternal;
                    if (ok) { ref[2 + k] = pn[ref[k]].pad0 + pn[ref[k]].pad1; firstOf[k] = first[ref[k]]; }
                } else {
                    const int f = ~ref[k]; const int cnt = (ref[k] != kRefNone && f < nT) ? leafCount(f) : 0;
                    ok = cnt >= 1; ref[2 + k] = cnt; firstOf[k] = f;
                }
            }
            // leaf order is left to right: the right subtree's triangles follow the left subtree's
            ok = ok && firstOf[1] == firstOf[0] + ref[2];
            first[i] = firstOf[0];
        }
        if (ok && nInternal > 0) ok = first[0] == 0 && pn[0].pad0 + pn[0].pad1 == nT;
        if (ok && nInternal > 0) HIP_OK(hipMemcpy(s->nodes.p, pn.data(), (size_t)nInternal * sizeof(PNode), hipMemcpyHostToDevice));
        s->flatOk = ok;
        s->nLeaves = 0;
        if (ok && nLights > 0 && haveLights) {
            // the table travels as a kernel argument, a byte per light: the first 8 lights (a scene of at most 64 triangles rarely has
            // more; a light beyond them is simply tested like any other triangle)
            light_triangles(pt.data(), nT, hostLights, nLights, nLightInd, [&](int idx) { return lightIndOf[idx]; }, lightTri.data());
            for (int i = 0; i < nLights && i < 8; i++) s->lightTri8 |= (uint64_t)(lightTri[i] + 1) << (8 * i);
        }
        if (ok && nInternal > 0 && boxes_nested_and_finite(pn, nInternal)) {     // the leaf table: every leaf child's box and triangle range
            std::vector<PLeaf> lf;
            for (int i = 0; i < nInternal; i++) {
                const int32_t* ref = &pn[i].left;
                for (int k = 0; k < 2; k++) {
                    if (ref[k] >= 0) continue;
                    PLeaf L;
                    const float* mn = k == 0 ? pn[i].lmin : pn[i].rmin; const float* mx = k == 0 ? pn[i].lmax : pn[i].rmax;
                    for (int a = 0; a < 3; a++) { L.mn[a] = mn[a]; L.mx[a] = mx[a]; }
                    L.first = ~ref[k]; L.count = ref[2 + k];
                    lf.push_back(L);
                }
            }
            if (int r = upload(s->leaves, lf.data(), lf.size() * sizeof(PLeaf))) return r;
            s->nLeaves = (int)lf.size();
        }
    }
    return 0;
}

static pt_scene* create_scene(const pt_scene_desc* desc, int deviceLeaf, pt_bvh_build_stats* stats) {
    if (!desc) { fail(-1, "pt_scene_create: null desc"); return nullptr; }
    pt_scene* s = new pt_scene();
    if (hipError_t e = hipGetDevice(&s->device); e != hipSuccess) {
        fail(-2, "pt_scene_create: no usable HIP device (%s); the path has no CPU fallback", hipGetErrorString(e));
        delete s;
        return nullptr;
    }
    if (repack(s, desc, deviceLeaf, stats) != 0) { pt_scene_destroy(s); return nullptr; }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, s->device) == hipSuccess && prop.multiProcessorCount > 0) s->numCU = prop.multiProcessorCount;
    }
    if (hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess) { fail(-2, "hipEventCreate failed"); pt_scene_destroy(s); return nullptr; }
    return s;
}

pt_scene* pt_scene_create(const pt_scene_desc* desc) { return create_scene(desc, -1, nullptr); }

pt_scene* pt_scene_create_from_mesh(const pt_scene_desc* desc, int max_leaf_size, pt_bvh_build_stats* stats) {
    if (max_leaf_size < 0) { fail(-1, "pt_scene_create_from_mesh: negative leaf size"); return nullptr; }
    return create_scene(desc, max_leaf_size, stats);
}

// ---- dynamic geometry: pt_scene_update_* ---------------------------------------------------------------------------------
// An update fills a STAGING scene — a default pt_scene on the caller's stack that borrows the live scene's spare buffers and the
// builder's pool — through the code creation runs (repack, or the builder + renumber_by_area + derive_layout), and only a
// complete one is swapped into the live scene. The buffers swapped out become the spares of the next update.
static void stage_begin(pt_scene* s, pt_scene& t) {
    auto take = [](DevBuf& from) { DevBuf b = from; from = DevBuf{}; return b; };
    t.device = s->device; t.numCU = s->numCU;
    t.nodes = take(s->spNodes); t.tris = take(s->spTris); t.attrs = take(s->spAttrs); t.lights = take(s->spLights); t.leaves = take(s->spLeaves);
    t.kNormals = take(s->spNormals); t.buildPool = take(s->buildPool);
}
static void stage_end(pt_scene* s, pt_scene& t) {
    s->spNodes = t.nodes; s->spTris = t.tris; s->spAttrs = t.attrs; s->spLights = t.lights; s->spLeaves = t.leaves;
    s->spNormals = t.kNormals; s->buildPool = t.buildPool;
    DevBuf* rest[] = {&t.mats, &t.textures, &t.kTris, &t.kUvs, &t.kTypes, &t.kLightTris, &t.posCur};     // an update of the whole mesh: the old ones (or, failed, the new ones)
    for (DevBuf* b : rest) b->release();
}
// mesh: materials, textures and the builder's inputs are the staging scene's too (pt_scene_update_mesh); otherwise only the
// geometry and, if the update brought normals, those.
static void adopt_geometry(pt_scene* s, pt_scene& t, bool mesh, bool normals) {
    std::swap(s->nodes, t.nodes); std::swap(s->tris, t.tris); std::swap(s->attrs, t.attrs); std::swap(s->lights, t.lights); std::swap(s->leaves, t.leaves);
    if (mesh || normals) std::swap(s->kNormals, t.kNormals);
    if (mesh) {
        std::swap(s->mats, t.mats); std::swap(s->textures, t.textures);
        std::swap(s->kTris, t.kTris); std::swap(s->kUvs, t.kUvs); std::swap(s->kTypes, t.kTypes); std::swap(s->kLightTris, t.kLightTris);
        std::swap(s->posCur, t.posCur); s->hasMotion = false;        // the topology may have changed: no previous positions, no motion
        s->deviceLeaf = t.deviceLeaf; s->nPositions = t.nPositions; s->nNormals = t.nNormals; s->nUvs = t.nUvs; s->nTexels = t.nTexels;
    }
    s->ds = t.ds;
    s->ds.nodes = (const PNode*)s->nodes.p; s->ds.tris = (const PTri*)s->tris.p; s->ds.attrs = (const PAttr*)s->attrs.p;
    s->ds.lights = (const PLight*)s->lights.p; s->ds.mats = (const PMat*)s->mats.p; s->ds.textures = (const float4*)s->textures.p;
    s->stackNeed = t.stackNeed; s->nInternal = t.nInternal; s->cacheNodes = t.cacheNodes; s->cacheTris = t.cacheTris;
    s->nMats = t.nMats; s->nLightsPacked = t.nLightsPacked; s->nTrisPacked = t.nTrisPacked; s->nLeaves = t.nLeaves; s->lightTri8 = t.lightTri8;
    s->armless = t.armless; s->simpleOk = t.simpleOk; s->noLeafTris = t.noLeafTris; s->leanOk = t.leanOk; s->flatOk = t.flatOk;
    // pt_scene_flags describes the last launch: there is none on this geometry yet
    s->lastLaunchFlat = s->lastLaunchSimple = s->lastLaunchLeafTable = s->lastLaunchFlat2 = s->lastLaunchLean = s->lastLaunchRefill = 0;
    s->lastLaunchHbm = -1;
    s->renumberMs = t.renumberMs;
    s->generation++;
}

// The per-frame path: everything but the positions (and the normals, if given) is the scene's own device copy.
static int update_vertices_staged(pt_scene* s, pt_scene& t, const void* pos, const void* nrm, bool onDevice, pt_bvh_build_stats* stats) {
    const int nT = s->nTrisPacked, nL = s->ds.nLights;
    if (int r = t.nodes.ensure((size_t)nT * sizeof(PNode))) return r;
    if (int r = t.tris.ensure((size_t)nT * sizeof(PTri))) return r;
    if (int r = t.attrs.ensure((size_t)nT * sizeof(PAttr))) return r;
    if (int r = t.lights.ensure((size_t)std::max(nL, 1) * sizeof(PLight))) return r;
    const void* normals = s->kNormals.p;
    if (nrm) {
        const size_t bytes = (size_t)s->nNormals * sizeof(pt_float4);
        if (int r = t.kNormals.ensure(std::max<size_t>(bytes, 16))) return r;
        if (bytes) HIP_OK(hipMemcpy(t.kNormals.p, nrm, bytes, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        normals = t.kNormals.p;
    }
    pt_build_src_ src{};
    src.positions = (const pt_float4*)pos; src.n_positions = s->nPositions; src.positions_on_device = onDevice ? 1 : 0;
    src.d_triangles = (const pt_triangle*)s->kTris.p; src.n_triangles = nT;
    src.d_normals = (const pt_float4*)normals; src.n_normals = s->nNormals;
    src.d_uvs = (const pt_float2*)s->kUvs.p; src.n_uvs = s->nUvs;
    src.d_mat_types = (const int*)s->kTypes.p; src.n_materials = s->nMats;
    src.d_light_tris = (const pt_triangle*)s->kLightTris.p; src.n_lights = nL;
    src.pool = &t.buildPool.p; src.pool_bytes = &t.buildPool.bytes;
    int out5[5] = {0, 0, 0, 0, 0};
    if (int r = pt_bvh_build_pack_(&src, s->deviceLeaf, t.nodes.p, t.tris.p, t.attrs.p, t.lights.p, out5, stats)) return r;
    const int nInternal = out5[0], stackNeed = out5[1], rootRef = out5[2];
    if (stackNeed > 128) return fail(-1, "pt_scene_update_vertices: BVH depth %d exceeds the reference's nodeStack[128] (integratorUtilities.cuh:89)", stackNeed);
    // what creation decides from the triangles' materials alone stands: neither changed
    t.armless = s->armless; t.simpleOk = s->simpleOk; t.noLeafTris = s->noLeafTris; t.leanOk = s->leanOk;
    if (int r = renumber_by_area(&t, nInternal, rootRef)) return r;
    std::vector<PLight> hostLights((size_t)std::max(nL, 1));
    std::vector<int32_t> lightInd;
    if (nT <= 128) {                       // the scenes whose lights' triangles derive_layout looks for: read the records the device made
        HIP_OK(hipMemcpy(hostLights.data(), t.lights.p, hostLights.size() * sizeof(PLight), hipMemcpyDeviceToHost));
        std::vector<PAttr> at((size_t)nT);
        HIP_OK(hipMemcpy(at.data(), t.attrs.p, at.size() * sizeof(PAttr), hipMemcpyDeviceToHost));
        lightInd.resize((size_t)nT);
        for (int i = 0; i < nT; i++) lightInd[i] = at[i].lightInd;
    }
    return derive_layout(&t, nInternal, stackNeed, rootRef, nT, nL, nL > 0, s->nMats, hostLights.data(), lightInd.data(), (int)lightInd.size());
}

static int update_vertices(pt_scene* s, const void* pos, int nPos, const void* nrm, int nNrm, bool onDevice, pt_bvh_build_stats* stats, const char* fn) {
    if (!s) return fail(-1, "%s: null scene", fn);
    if (!pos) return fail(-1, "%s: null positions", fn);
    if (s->deviceLeaf < 0)
        return fail(-1, "%s: the scene's tree was the caller's (pt_scene_create): only a scene that went through the device builder "
                        "(pt_scene_create_from_mesh, or one pt_scene_update_mesh) keeps what a vertex update rebuilds from", fn);
    if (nPos != s->nPositions) return fail(-1, "%s: %d positions, the scene has %d", fn, nPos, s->nPositions);
    if (nrm && nNrm != s->nNormals) return fail(-1, "%s: %d normals, the scene has %d", fn, nNrm, s->nNormals);
    const double t0 = wall_ms();
    HIP_OK(hipDeviceSynchronize());        // a frame boundary: nothing of the old geometry is in flight
    pt_scene t;
    stage_begin(s, t);
    int r = update_vertices_staged(s, t, pos, nrm, onDevice, stats);
    // the new positions go into the spare of the pair, and only once the build has taken them: a refused update touches neither
    const size_t posBytes = (size_t)nPos * sizeof(pt_float4);
    if (r == 0) r = s->posPrev.ensure(std::max<size_t>(posBytes, 16));
    if (r == 0) {
        const hipError_t e = hipMemcpy(s->posPrev.p, pos, posBytes, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
        if (e != hipSuccess) { s->hasMotion = false; r = fail(-2, "%s: copying the positions failed: %s", fn, hipGetErrorString(e)); }
    }
    if (r == 0) {
        std::swap(s->posCur, s->posPrev); s->hasMotion = true;
        adopt_geometry(s, t, false, nrm != nullptr);
    }
    stage_end(s, t);
    if (r == 0) s->updateMs = (float)(wall_ms() - t0);
    if (r == 0 && stats) stats->total_ms = s->updateMs;
    return r;
}

int pt_scene_update_vertices(pt_scene* s, const pt_float4* positions, int n_positions, const pt_float4* normals, int n_normals, pt_bvh_build_stats* stats) {
    return update_vertices(s, positions, n_positions, normals, n_normals, false, stats, "pt_scene_update_vertices");
}
int pt_scene_update_vertices_device(pt_scene* s, const void* d_positions, int n_positions, const void* d_normals, int n_normals, pt_bvh_build_stats* stats) {
    return update_vertices(s, d_positions, n_positions, d_normals, n_normals, true, stats, "pt_scene_update_vertices_device");
}

int pt_scene_update_mesh(pt_scene* s, const pt_scene_desc* d, int max_leaf_size, pt_bvh_build_stats* stats) {
    if (!s) return fail(-1, "pt_scene_update_mesh: null scene");
    if (!d) return fail(-1, "pt_scene_update_mesh: null desc");
    if (max_leaf_size < 0) return fail(-1, "pt_scene_update_mesh: negative leaf size");
    if (d->n_triangles <= 0 || d->n_positions <= 0 || !d->triangles || !d->positions || !d->materials)
        return fail(-1, "pt_scene_update_mesh: empty scene (triangles, positions and materials are needed)");
    if ((d->n_lights > 0 && !d->lights) || (d->n_normals > 0 && !d->normals) || (d->n_uvs > 0 && !d->uvs) || (d->n_texels > 0 && !d->textures))
        return fail(-1, "pt_scene_update_mesh: an array with a positive count is NULL");
    const double t0 = wall_ms();
    HIP_OK(hipDeviceSynchronize());        // a frame boundary: nothing of the old geometry is in flight
    pt_scene t;
    stage_begin(s, t);
    const int r = repack(&t, d, max_leaf_size, stats, true);
    if (r == 0) adopt_geometry(s, t, true, true);
    stage_end(s, t);
    if (r == 0) s->updateMs = (float)(wall_ms() - t0);
    if (r == 0 && stats) stats->total_ms = s->updateMs;
    return r;
}

// ---- material and emission edits: pt_scene_update_materials / pt_scene_update_emission --------------------------------------------
// Neither touches the tree, the geometry records' geometry, the leaf table, lightTri8 or the cache split: derive_layout reads a
// material only through scene_onchip_wg's per-wave area (a medium stack unless the scene is SIMPLE), and that cannot decide whether
// a scene small enough for the FLAT kernels is LDS-resident: at 16 waves the largest such scene fits with the medium stacks.
static_assert(kAttrCacheBytes > 0 && 128 * 64 + 128 * 48 + 4 * kAttrCacheBytes + 16 * (kStackFlat2Rows * 256 + kMediumMax * 64) <= 160 * 1024,
              "a material edit would have to derive flatOk again");

// The end of a successful edit: one generation on, and the previous positions describe a step the viewer has already seen.
static void edit_done(pt_scene* s, double t0) {
    s->hasMotion = false;
    // pt_scene_flags describes the last launch: there is none on these records yet
    s->lastLaunchFlat = s->lastLaunchSimple = s->lastLaunchLeafTable = s->lastLaunchFlat2 = s->lastLaunchLean = s->lastLaunchRefill = 0;
    s->lastLaunchHbm = -1;
    s->generation++;
    s->updateMs = (float)(wall_ms() - t0);
}

int pt_scene_update_materials(pt_scene* s, const pt_material* materials, int n_materials) {
    const char* fn = "pt_scene_update_materials";
    if (!s) return fail(-1, "%s: null scene", fn);
    if (!materials) return fail(-1, "%s: null materials", fn);
    if (n_materials != s->nMats) return fail(-1, "%s: %d materials, the scene has %d", fn, n_materials, s->nMats);
    std::vector<PMat> mats; std::vector<uint32_t> matClass;
    if (int r = pack_materials(materials, n_materials, s->nTexels, fn, mats, matClass)) return r;
    const double t0 = wall_ms();
    HIP_OK(hipDeviceSynchronize());        // a frame boundary: nothing that reads the old table is in flight
    // the edit buffer: the kernel's result word, then the class of every row
    const size_t classOff = 256, classBytes = matClass.size() * sizeof(uint32_t);
    if (int r = s->edit.ensure(classOff + classBytes)) return r;
    uint32_t* dUsed = (uint32_t*)s->edit.p;
    uint32_t* dClass = (uint32_t*)((char*)s->edit.p + classOff);
    HIP_OK(hipMemset(dUsed, 0, sizeof(uint32_t)));
    HIP_OK(hipMemcpy(dClass, matClass.data(), classBytes, hipMemcpyHostToDevice));
    if (int r = pt_edit_materials_(s->tris.p, s->nTrisPacked, dClass, n_materials, dUsed)) return r;
    uint32_t used = 0u;
    HIP_OK(hipMemcpy(&used, dUsed, sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(s->mats.p, mats.data(), mats.size() * sizeof(PMat), hipMemcpyHostToDevice));
    if (s->deviceLeaf >= 0) {              // what the next vertex update packs the triangles' flags from
        std::vector<int> types((size_t)n_materials);
        for (int i = 0; i < n_materials; i++) types[i] = materials[i].type;
        HIP_OK(hipMemcpy(s->kTypes.p, types.data(), types.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    apply_material_class(s, used, materials[0]);
    edit_done(s, t0);
    return 0;
}

int pt_scene_update_emission(pt_scene* s, int n, const int32_t* light_indices, const pt_float4* emission) {
    const char* fn = "pt_scene_update_emission";
    if (!s) return fail(-1, "%s: null scene", fn);
    if (n < 0) return fail(-1, "%s: negative count", fn);
    if (n > 0 && (!light_indices || !emission)) return fail(-1, "%s: null %s", fn, !light_indices ? "light_indices" : "emission");
    const int nL = s->ds.nLights, nT = s->nTrisPacked;
    for (int k = 0; k < n; k++)
        if (light_indices[k] < 0 || light_indices[k] >= nL) return fail(-1, "%s: light index %d (entry %d) out of range, the scene has %d lights", fn, light_indices[k], k, nL);
    // the edit as a table by light: the new emission and whether the light is edited at all (a repeated index: the last entry stands)
    std::vector<pt_float4> table((size_t)std::max(nL, 1));
    std::vector<int32_t> on((size_t)std::max(nL, 1), 0);
    std::memset(table.data(), 0, table.size() * sizeof(pt_float4));
    for (int k = 0; k < n; k++) { table[light_indices[k]] = emission[k]; on[light_indices[k]] = 1; }
    const double t0 = wall_ms();
    HIP_OK(hipDeviceSynchronize());        // a frame boundary
    if (n > 0) {
        const size_t tableBytes = table.size() * sizeof(pt_float4), onBytes = on.size() * sizeof(int32_t);
        if (int r = s->edit.ensure(tableBytes + onBytes)) return r;
        pt_float4* dTable = (pt_float4*)s->edit.p;
        int32_t* dOn = (int32_t*)((char*)s->edit.p + tableBytes);
        HIP_OK(hipMemcpy(dTable, table.data(), tableBytes, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dOn, on.data(), onBytes, hipMemcpyHostToDevice));
        const bool kept = s->deviceLeaf >= 0;       // ... and what the next vertex update packs attributes and lights from
        if (int r = pt_edit_emission_(s->attrs.p, nT, s->lights.p, nL, dTable, dOn, kept ? (pt_triangle*)s->kTris.p : nullptr,
                                      kept ? (pt_triangle*)s->kLightTris.p : nullptr))
            return r;
        HIP_OK(hipDeviceSynchronize());
    }
    edit_done(s, t0);
    return 0;
}

int pt_scene_generation(pt_scene* s) { return s ? s->generation : fail(-1, "pt_scene_generation: null scene"); }

int pt_scene_has_motion(pt_scene* s) { return s ? (s->hasMotion ? 1 : 0) : fail(-1, "pt_scene_has_motion: null scene"); }

int pt_debug_update_ms(pt_scene* s, float* out3) {
    if (!s || !out3) return fail(-1, "pt_debug_update_ms: null argument");
    out3[0] = s->renumberMs; out3[1] = s->updateMs; out3[2] = 0.0f;
    return 0;
}

// what: 0 PNodes (64 B each), 1 PTris (48 B), 2 PAttrs (80 B), 3 PLights (64 B), 4 PMats (96 B). Returns the record count (or < 0);
// copies min(count * size, capacity) bytes. For tests: the device re-layout must equal the host one.
int pt_debug_packed(pt_scene* s, int what, void* dst, size_t capacity) {
    if (!s) return fail(-1, "null scene");
    const void* src = what == 0 ? s->nodes.p : what == 1 ? s->tris.p : what == 2 ? s->attrs.p : what == 3 ? s->lights.p : what == 4 ? s->mats.p : nullptr;
    const size_t rec = what == 0 ? sizeof(PNode) : what == 1 ? sizeof(PTri) : what == 2 ? sizeof(PAttr) : what == 3 ? sizeof(PLight) : sizeof(PMat);
    const int count = what == 0 ? s->nInternal : what == 3 ? s->ds.nLights : what == 4 ? s->nMats : s->nTrisPacked;
    if (!src) return fail(-1, "pt_debug_packed: unknown array %d", what);
    const size_t bytes = std::min((size_t)count * rec, capacity);
    if (dst && bytes) HIP_OK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return count;
}

// Host only: light_triangles on the triangles in the leaf order desc->bvh_indices gives, packed as repack packs them.
int pt_light_triangles(const pt_scene_desc* d, int32_t* out) {
    if (!d || !out) return fail(-1, "null argument");
    if (d->n_triangles <= 0 || !d->triangles || !d->bvh_indices || !d->positions || (d->n_lights > 0 && !d->lights)) return fail(-1, "pt_light_triangles: empty scene");
    std::vector<PTri> pt((size_t)d->n_triangles);
    for (int i = 0; i < d->n_triangles; i++) {
        const int idx = d->bvh_indices[i];
        if (idx < 0 || idx >= d->n_triangles) return fail(-1, "pt_light_triangles: BVHindices[%d] = %d out of range", i, idx);
        const pt_triangle& t = d->triangles[idx];
        if (t.aInd < 0 || t.aInd >= d->n_positions || t.bInd < 0 || t.bInd >= d->n_positions || t.cInd < 0 || t.cInd >= d->n_positions)
            return fail(-1, "pt_light_triangles: triangle %d position index out of range", idx);
        const pt_float4 a = d->positions[t.aInd], b = d->positions[t.bInd], c = d->positions[t.cInd];
        PTri& p = pt[i];
        p.v0[0] = a.x; p.v0[1] = a.y; p.v0[2] = a.z;
        p.e1[0] = b.x - a.x; p.e1[1] = b.y - a.y; p.e1[2] = b.z - a.z;
        p.e2[0] = c.x - a.x; p.e2[1] = c.y - a.y; p.e2[2] = c.z - a.z;
        p.idx = (uint32_t)idx; p.material = t.materialID; p.flags = 0u;
    }
    light_triangles(pt.data(), d->n_triangles, d, out);
    return 0;
}

// ---- helpers ----------------------------------------------------------------------------------
static int resolve_tiles(int w, int h, const pt_tile_range* tiles, TileSpan& t) {
    if (w <= 0 || h <= 0) return fail(-1, "bad image size %dx%d", w, h);
    t.tilesX = (w + 7) / 8;
    int total = t.tilesX * ((h + 7) / 8);
    if (!tiles) { t.first = 0; t.stride = 1; t.count = total; return 0; }
    t.first = tiles->first; t.stride = tiles->stride; t.count = tiles->count;
    if (t.count < 0 || t.stride < 1 || t.first < 0) return fail(-1, "bad tile range {first %d, stride %d, count %d}", t.first, t.stride, t.count);
    if (t.count > 0 && (long long)t.first + (long long)(t.count - 1) * t.stride >= total)
        return fail(-1, "tile range {first %d, stride %d, count %d} exceeds the %d tiles of a %dx%d image", t.first, t.stride, t.count, total, w, h);
    return 0;
}

static CamK cam_to_kernel(const pt_camera& c) {
    CamK k;
    k.origin = V3{c.cameraOrigin.x, c.cameraOrigin.y, c.cameraOrigin.z};
    k.forward = V3{c.forward.x, c.forward.y, c.forward.z};
    k.right = V3{c.right.x, c.right.y, c.right.z};
    k.up = V3{c.up.x, c.up.y, c.up.z};
    k.w = c.w; k.h = c.h; k.aperture = c.aperture; k.focalDist = c.focalDist; k.fovScale = c.fovScale; k.jitter = c.antiAliasJitterDist;
    return k;
}

static int check_render_args(pt_scene* s, const pt_camera* cam, int spp, int integrator) {
    if (!s || !cam) return fail(-1, "null scene or camera");
    if (spp < 0) return fail(-1, "negative sample count");
    if (integrator != PT_UNIDIRECTIONAL && integrator != PT_NAIVE_UNIDIRECTIONAL)
        return fail(-3, "integrator %d is out of scope: only UNIDIRECTIONAL (0) and NAIVE_UNIDIRECTIONAL (2) are on this path", integrator);
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != s->device) return fail(-1, "scene lives on HIP device %d but the current device is %d", s->device, dev);
    return 0;
}

// The wavefront variant of render_tiles: logic / trace kernel pairs until no path is alive.
static int render_tiles_wavefront(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int maxDepth, int integrator, int useMIS,
                                  const TileSpan& t, void* d_tiles, uint32_t* d_pixcnt, bool count, hipStream_t stream) {
    if (s->armless) return fail(-3, "the wavefront variant needs every material to have a dispatch arm (pt_path.h); use the megakernel");
    WfParams W;
    W.n = t.count * 64; W.w = w; W.h = h; W.tileFirst = t.first; W.tileStride = t.stride; W.tilesX = t.tilesX;
    W.nodeKeep = s->nodeKeep; W.triKeep = s->triKeep;
    if (int r = s->wfState.ensure(wf_state_bytes(W.n))) return r;
    if (int r = s->wfCtl.ensure(64)) return r;
    wf_carve(W, s->wfState.p);
    W.qctl = (uint32_t*)s->wfCtl.p;
    W.rng = (uint32_t*)s->rng.p; W.out = (float4*)d_tiles;
    W.pathCtr = nullptr;
    if (count) {
        if (int r = s->wfCtr.ensure((size_t)W.n * 8 * sizeof(uint32_t))) return r;
        W.pathCtr = (uint32_t*)s->wfCtr.p;
    }
    // the trace kernel has its own LDS budget (no medium stacks, smaller traversal stack): the whole scene if it fits 12 KB, else
    // the top of the tree — in 16-wave workgroups, two per CU, that share 48 KB of it (`wf_wide_wg` 0: the 4-wave shape)
    int wfNodes, wfTris, wgWaves = 4;
    if ((size_t)s->nInternal * 64 + (size_t)s->ds.nTris * 48 <= (size_t)kWfCacheBytes) { wfNodes = s->nInternal; wfTris = s->ds.nTris; }
    else if (s->wfWideWg == 2 || (s->wfWideWg == 1 && (W.n + 1023) / 1024 >= s->numCU * 2)) { wgWaves = 16; wfNodes = std::min(s->nInternal, (80 * 1024 - 16 * kWfStackLds * 256) / 64); wfTris = 0; }
    else { wfNodes = std::min(s->nInternal, kWfCacheBytes / 64); wfTris = 0; }
    const int blocks = std::max(1, std::min(s->numCU * (32 / wgWaves), (W.n + 64 * wgWaves - 1) / (64 * wgWaves)));
    const int spillPerLane = std::max(0, s->stackNeed - kWfStackLds);
    int32_t* spill = nullptr;
    if (spillPerLane > 0) {
        if (int r = s->wfSpill.ensure((size_t)blocks * wgWaves * spillPerLane * 64 * sizeof(int32_t))) return r;
        spill = (int32_t*)s->wfSpill.p;
    }
    const CamK ck = cam_to_kernel(*cam);
    const bool wfSimple = s->simpleOk && s->simpleWanted && !count;        // the SIMPLE bounce (pt_path.h) in the logic kernel: diffuse-only scenes, timed launches
    s->lastLaunchSimple = wfSimple ? 1 : 0;
    HIP_OK(hipMemsetAsync(W.qctl, 0, 16, stream));
    HIP_OK(hipEventRecord(s->ev0, stream));
    HIP_OK(launch_wf_init(W, spp, stream));
    // Paths end at different iterations; the host polls the queue length every 16 iterations.
    const long long cap = (long long)std::max(spp, 1) * 4200 + 64;
    bool finished = false;
    for (long long it = 0; it < cap; it++) {
        HIP_OK(launch_wf_logic(integrator, count, wfSimple, W, s->ds, ck, maxDepth, useMIS, (int)(it & 1), stream));
        if ((it & 15) == 15) {
            uint32_t queued = 0;
            HIP_OK(hipMemcpyAsync(&queued, W.qctl + (it & 1) * 2, 4, hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            if (queued == 0) { finished = true; break; }
        }
        HIP_OK(launch_wf_trace(count, wgWaves, blocks, W, s->ds, wfNodes, wfTris, spill, spillPerLane, (int)(it & 1), stream));
    }
    if (!finished) return fail(-4, "wavefront render did not terminate within %lld iterations", cap);
    HIP_OK(launch_wf_finish(W, stream));
    if (count) HIP_OK(launch_wf_counters(W, d_pixcnt, (unsigned long long*)s->totals.p, stream));
    HIP_OK(hipEventRecord(s->ev1, stream));
    s->evPending = true;
    return 0;
}

// rng init + megakernel on `stream`; d_tiles holds t.count*64 float4.
// List mode (list != null: adaptive sampling): t is the whole frame and the launch renders the `live` tiles that the device
// array `list` names, through the tile queue whatever "persistent" says; the kernel is picked by `live`. The RNG states, the
// accumulator and `left` stay indexed by tile number, so every buffer is sized for the whole frame.
// Fused (render_moments with "moments_fused"): the launch is to keep the squared batch sums itself, batches of c samples, in the
// tile-major buffers P and Q. If the kernel this launch gets has no fused twin, or the scene renders with the wavefront variant,
// nothing is rendered and `launched` stays false; `seeded` then says whether the streams have been seeded on `stream` already.
struct FusedMoments { float4* P; float4* Q; int c; bool launched, seeded; };
static int render_tiles(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int maxDepth, int integrator, int useMIS,
                        uint64_t seed, const TileSpan& t, void* d_tiles, uint32_t* d_pixcnt, bool count, hipStream_t stream, bool continueStreams,
                        const int* list = nullptr, int live = -1, FusedMoments* fused = nullptr) {
    if (t.count == 0) return 0;
    if (fused && s->variant == 1) return 0;
    if (!list) live = t.count;
    if (list && (count || s->variant != 0 || t.first != 0 || t.stride != 1 || live < 0 || live > t.count)) return fail(-1, "render_tiles: bad tile list");
    // the reference keys the stream by the camera's image size (y*w+x with the launch's w, deviceCode.cu:59)
    if (int r = s->rng.ensure((size_t)t.count * 384 * sizeof(uint32_t))) return r;
    // continueStreams: a later chunk of a progressive render keeps the per-pixel XORWOW states the
    // previous chunk stored (the reference reloads / stores them around every sample, deviceCode.cu:294, 541)
    if (!continueStreams) HIP_OK(launch_rng_init((const uint32_t*)s->jump.p, seed, w, h, t, (uint32_t*)s->rng.p, stream));
    if (fused) fused->seeded = !continueStreams;
    if (s->variant == 1) return render_tiles_wavefront(s, cam, w, h, spp, maxDepth, integrator, useMIS, t, d_tiles, d_pixcnt, count, stream);
    // First the selector fields of the launch, then the kernel they choose (pt_kernels.hip: megakernel_choose), then everything that is
    // sized for THAT kernel: its LDS stack length lays out the spill area, its launch bounds give the workgroup and the grid.
    const bool onchip = scene_onchip(s);
    // the SIMPLE bounce for a scene in HBM: diffuse-only scenes, timed launches with the resumable traversal
    const bool simpleTimed = s->simpleOk && s->simpleWanted && s->refill && !s->cull && !s->armless;
    const bool simpleHbm = !onchip && s->wavesHbmOk && simpleTimed && !count;
    const bool hbm = hbm_kernel_pays(s, simpleHbm, live);
    KParams P = {};                                         // (its padding too: pt_params.h)
    P.onchip = onchip ? 1 : 0;
    P.hbm = hbm ? 1 : 0;
    P.cull = (s->cull && hbm) ? 1 : 0;
    P.refill = (s->refill && !P.cull && !s->armless && !onchip) ? 1 : 0;
    P.flat = 0;                                             // 1: FLAT with 64-bit masks, 2: with 128-bit masks
    if (onchip && s->flatOk && s->flatWanted) {
        P.flat = (s->nInternal <= 64 && s->nTrisPacked <= 64) ? 1 : 2;     // 65..128: +17-20 % over the stack walk with the leaf-box form (profiles/r02_flat_crossover.jsonl)
    }
    // the instantiations that have the SIMPLE bounce: FLAT, the production kernel for scenes in HBM and its 4-wave form (small shares)
    P.simple = ((P.flat && s->simpleOk && s->simpleWanted) || simpleHbm) ? 1 : 0;
    if (P.flat == 1 && s->noLeafTris && !s->armless && s->flat2Wanted && integrator == PT_UNIDIRECTIONAL && !count && useMIS) P.flat = 3;   // ... and the pair form of FLAT
    // the LEAN generic bounce exists for the three timed kernels generic scenes run: the pair form of FLAT, the kernel for scenes in HBM
    // and its 4-wave form (both REFILL)
    P.lean = (s->leanOk && s->leanWanted && !s->armless && !P.simple && !count && !P.cull && (P.flat == 3 || (!onchip && P.refill))) ? 1 : 0;
    const MkRow* row = megakernel_choose(integrator, count, true, P, false);      // (syncShadow: outside the pair form of FLAT no kernel defers the shadow ray)
    if (!row) return fail(-1, "render_tiles: no megakernel is built for this launch");
    const int spillEntries = hbm ? std::max(0, s->stackNeed - row->f.stackEntries) : s->ds.stackSpill;
    const int wgWaves = row->f.wgWaves ? row->f.wgWaves : (onchip ? scene_onchip_wg(s) : 4);
    int blocks = megakernel_blocks(t.count, wgWaves);
    if (spillEntries > 0)
        if (int r = s->spill.ensure((size_t)blocks * wgWaves * spillEntries * 64 * sizeof(int32_t))) return r;
    P.S = s->ds;
    P.cam = cam_to_kernel(*cam);
    P.w = w; P.h = h; P.spp = spp; P.maxDepth = maxDepth; P.useMIS = useMIS;
    P.tileFirst = t.first; P.tileStride = t.stride; P.tileCount = t.count; P.tilesX = t.tilesX;
    P.cacheNodes = s->cacheNodes; P.cacheTris = s->cacheTris;
    if (onchip) { P.cacheNodes = s->nInternal; P.cacheTris = s->nTrisPacked; }      // the whole scene, in workgroups large enough to hold it
    P.cacheAttrs = P.cacheMats = P.cacheLights = 0;
    P.nLeaves = 0; P.leaves = nullptr;
    P.lightTri8 = s->lightTri8;
    if (onchip && kAttrCacheBytes > 0) { P.cacheAttrs = s->nTrisPacked; P.cacheMats = s->nMats; P.cacheLights = s->nLightsPacked; }   // the bounce's records in LDS as well
    if (onchip && kAttrCacheBytes > 0 && s->flatOk && s->leafBoxes && s->nLeaves > 0) { P.nLeaves = s->nLeaves; P.leaves = (const PLeaf*)s->leaves.p; }
    P.wgWaves = wgWaves;
    if (hbm && s->cacheTris == 0) P.cacheNodes = std::min(s->nInternal, (simpleHbm ? kCacheBytesHbmSimple : kCacheBytesHbm) / 64);     // its workgroups share a larger copy of the top of the tree
    P.gnodeFrom = P.cacheNodes;
    if (count && !onchip && s->wavesHbmOk && s->cacheTris == 0) {
        // a counting launch stands in for the timed launch of the same tiles (bench.py): count a node fetch as "global" against THAT
        // instantiation's LDS copy of the tree top — the SIMPLE production kernel holds 768 nodes, this counting kernel 704 (or 192)
        P.gnodeFrom = hbm_kernel_pays(s, simpleTimed, t.count) ? std::min(s->nInternal, (simpleTimed ? kCacheBytesHbmSimple : kCacheBytesHbm) / 64) : s->cacheNodes;
    }
    P.S.stackSpill = spillEntries;
    P.refillKeep = (hbm || s->refillKeepSet) ? s->refillKeep : kRefillKeepSmall;      // re-swept on the round's kernels: 6 for the 8-wave kernel, 10 for the 4-wave one (1/8 shares +5.5 % / +6 %, profiles/r03_shards_hbm_final.log)
    P.nodeKeep = s->nodeKeep; P.triKeep = s->triKeep;
    s->lastLaunchLean = P.lean;
    s->lastLaunchRefill = P.refill; s->lastLaunchFlat = (P.flat && !count) ? 1 : 0;
    s->lastLaunchSimple = (P.simple && !count) ? 1 : 0;
    s->lastLaunchFlat2 = (P.flat == 3) ? 1 : 0;
    s->lastLaunchLeafTable = (P.flat && !count && P.nLeaves > 0) ? 1 : 0;
    s->lastLaunchHbm = hbm ? 1 : 0;
    P.wavesPerSimd = row->f.wavesPerSimd;
    P.queue = nullptr; P.queueMask = 0; P.left = nullptr; P.gridBlocks = 0;
    P.lptPrio = s->lptPrio; P.sliceIters = s->sliceIters; P.schedMask = s->schedMask; P.sliceAlways = s->sliceAlways ? 1 : 0;
    P.queueTimeout = (unsigned long long)s->queueTimeoutMs * 100000ull;        // ms -> ticks of the 100 MHz steady counter (hipDeviceAttributeWallClockRate)
    if (s->persistent || list) {
        int cap = 256;
        while (cap < t.count) cap <<= 1;
        if (int r = s->queue.ensure((size_t)(kQueueHeader + 2 * cap) * sizeof(int))) return r;
        if (int r = s->left.ensure((size_t)t.count * 64 * sizeof(int))) return r;
        P.queue = (int*)s->queue.p; P.queueMask = cap - 1; P.left = (int*)s->left.p;
        P.gridBlocks = s->numCU * P.wavesPerSimd * 4 / wgWaves;      // n waves per SIMD = 4n waves per CU, in workgroups of wgWaves
    }
    s->lastLaunchQueued = P.queue != nullptr;
    s->lastLaunchTiles = t.count;
    s->lastLaunchPushed = live;
    P.rng = (uint32_t*)s->rng.p; P.out = (float4*)d_tiles; P.pixCounters = d_pixcnt;
    P.totals = count ? (unsigned long long*)s->totals.p : nullptr;
#ifdef PT_STAMPS
    P.totals = (unsigned long long*)s->totals.p;           // the diagnostic build sums its stamps for timed launches too
#endif
    P.spill = spillEntries > 0 ? (int32_t*)s->spill.p : nullptr;
    MomentsK M = {nullptr, nullptr, 0, 0.0f};
    if (fused) {
        row = megakernel_choose(integrator, count, true, P, true);     // the twin: its counterpart's facts, so everything sized above stands
        if (!row || (row->key & kMkBuiltOnly)) return 0;                    // the caller renders in batches
        M.P = fused->P; M.Q = fused->Q; M.c = fused->c; M.rc = 1.0f / (float)fused->c;
        fused->launched = true;
    }
    HIP_OK(hipEventRecord(s->ev0, stream));            // HIP events on the launch stream, around the megakernel only
    HIP_OK(launch_megakernel(*row, P, live, list, stream, fused ? &M : nullptr));
    HIP_OK(hipEventRecord(s->ev1, stream));
    s->evPending = true;
    return 0;
}

int pt_render_tiles_device(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int maxDepth, int integrator, int useMIS,
                           uint64_t seed, const pt_tile_range* tiles, void* d_tile_rgba, int count_work, void* stream) {
    if (int r = check_render_args(s, cam, spp, integrator)) return r;
    if (!d_tile_rgba) return fail(-1, "null tile buffer");
    TileSpan t;
    if (int r = resolve_tiles(w, h, tiles, t)) return r;
    return render_tiles(s, cam, w, h, spp, maxDepth, integrator, useMIS, seed, t, d_tile_rgba, nullptr, count_work != 0, (hipStream_t)stream, false);
}

int pt_untile_device(int w, int h, const pt_tile_range* tiles, const void* d_tile_rgba, void* d_colors, void* stream) {
    TileSpan t;
    if (int r = resolve_tiles(w, h, tiles, t)) return r;
    HIP_OK(launch_untile(w, h, t, (const float4*)d_tile_rgba, (float4*)d_colors, (hipStream_t)stream));
    return 0;
}
int pt_tile_device(int w, int h, const pt_tile_range* tiles, const void* d_colors, void* d_tile_rgba, void* stream) {
    TileSpan t;
    if (int r = resolve_tiles(w, h, tiles, t)) return r;
    HIP_OK(launch_tile(w, h, t, (const float4*)d_colors, (float4*)d_tile_rgba, (hipStream_t)stream));
    return 0;
}

// scan-line DEVICE accumulator in / out, blocking; the body of both reference launchers.
static int launch_on_colors(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int maxDepth, int integrator, int useMIS,
                            uint64_t seed, const pt_tile_range* tiles, void* d_colors, uint32_t* d_pixcnt, bool count) {
    if (int r = check_render_args(s, cam, spp, integrator)) return r;
    TileSpan t;
    if (int r = resolve_tiles(w, h, tiles, t)) return r;
    if (int r = s->tilebuf.ensure(std::max<size_t>((size_t)t.count * 64 * sizeof(float4), 16))) return r;
    HIP_OK(launch_tile(w, h, t, (const float4*)d_colors, (float4*)s->tilebuf.p, nullptr));
    if (int r = render_tiles(s, cam, w, h, spp, maxDepth, integrator, useMIS, seed, t, s->tilebuf.p, d_pixcnt, count, nullptr, false)) return r;
    HIP_OK(launch_untile(w, h, t, (const float4*)s->tilebuf.p, (float4*)d_colors, nullptr));
    HIP_OK(hipDeviceSynchronize());                 // cudaDeviceSynchronize, deviceCode.cu:608
    return queue_error(s);                          // a tile-queue timeout means an incomplete frame: never report success
}

// The reference's launchers with their progressive hook (deviceCode.cu:568-606): the sample loop runs
// in chunks of `chunk_spp`; after every chunk `d_colors` holds the sum over `samples_done` samples and
// `progress(samples_done, user)` is called on the calling thread (the reference writes render.bmp /
// renderCSV.csv there every >= 5 s; file I/O stays outside this ABI). The per-pixel streams continue
// across chunks, so the final image is bit-identical to the one-shot launcher. A non-zero return
// from `progress` stops the render after that chunk.
int pt_launch_progressive(int integrator, int maxDepth, pt_camera camera, pt_scene* s, int numSample, int useMIS, int w, int h,
                          void* d_colors, int chunk_spp, pt_progress_fn progress, void* user) {
    if (int r = check_render_args(s, &camera, numSample, integrator)) return r;
    if (chunk_spp <= 0) return fail(-1, "chunk_spp must be positive");
    TileSpan t;
    if (int r = resolve_tiles(w, h, nullptr, t)) return r;
    if (int r = s->tilebuf.ensure(std::max<size_t>((size_t)t.count * 64 * sizeof(float4), 16))) return r;
    HIP_OK(launch_tile(w, h, t, (const float4*)d_colors, (float4*)s->tilebuf.p, nullptr));
    for (int done = 0; done < numSample;) {
        const int n = std::min(chunk_spp, numSample - done);
        if (int r = render_tiles(s, &camera, w, h, n, maxDepth, integrator, useMIS, 103033ull, t, s->tilebuf.p, nullptr, false, nullptr, done > 0)) return r;
        HIP_OK(launch_untile(w, h, t, (const float4*)s->tilebuf.p, (float4*)d_colors, nullptr));
        HIP_OK(hipDeviceSynchronize());
        if (int r = queue_error(s)) return r;
        done += n;
        if (progress && progress(done, user) != 0) break;
    }
    return 0;
}

int pt_launch_unidirectional(int maxDepth, pt_camera camera, pt_scene* scene, int numSample, int useMIS, int w, int h, void* d_colors) {
    return launch_on_colors(scene, &camera, w, h, numSample, maxDepth, PT_UNIDIRECTIONAL, useMIS, 103033ull, nullptr, d_colors, nullptr, false);
}
int pt_launch_naive_unidirectional(int maxDepth, pt_camera camera, pt_scene* scene, int numSample, int useMIS, int w, int h, void* d_colors) {
    return launch_on_colors(scene, &camera, w, h, numSample, maxDepth, PT_NAIVE_UNIDIRECTIONAL, useMIS, 103033ull, nullptr, d_colors, nullptr, false);
}

static int render_host(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int maxDepth, int integrator, int useMIS, uint64_t seed,
                       const pt_tile_range* tiles, float* out, uint32_t* outCounters, bool count) {
    if (!out) return fail(-1, "null output buffer");
    if (int r = check_render_args(s, cam, spp, integrator)) return r;
    TileSpan t;
    if (int r = resolve_tiles(w, h, tiles, t)) return r;
    size_t px = (size_t)w * h;
    if (int r = s->colors.ensure(px * sizeof(float4))) return r;
    HIP_OK(hipMemcpy(s->colors.p, out, px * sizeof(float4), hipMemcpyHostToDevice));
    uint32_t* dpc = nullptr;
    if (outCounters) {
        if (int r = s->pixcnt.ensure(std::max<size_t>((size_t)t.count * 512 * sizeof(uint32_t), 16))) return r;
        dpc = (uint32_t*)s->pixcnt.p;
    }
    if (int r = launch_on_colors(s, cam, w, h, spp, maxDepth, integrator, useMIS, seed, tiles, s->colors.p, dpc, count)) return r;
    HIP_OK(hipMemcpy(out, s->colors.p, px * sizeof(float4), hipMemcpyDeviceToHost));
    if (outCounters) {
        std::vector<uint32_t> tmp((size_t)t.count * 512);
        HIP_OK(hipMemcpy(tmp.data(), dpc, tmp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int lt = 0; lt < t.count; lt++) {
            int tile = t.first + lt * t.stride;
            for (int lane = 0; lane < 64; lane++) {
                int x = (tile % t.tilesX) * 8 + (lane & 7), y = (tile / t.tilesX) * 8 + (lane >> 3);
                if (x >= w || y >= h) continue;
                for (int k = 0; k < 8; k++) outCounters[((size_t)y * w + x) * 8 + k] = tmp[(size_t)lt * 512 + k * 64 + lane];
            }
        }
    }
    return 0;
}

// pt_render runs the kernels the bench times; pt_render_counted the counting instantiations (same image, per-pixel
// and total work counters on the side, no time slices).
int pt_render(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int maxDepth, int integrator, int useMIS, uint64_t seed,
              const pt_tile_range* tiles, float* out) {
    return render_host(s, cam, w, h, spp, maxDepth, integrator, useMIS, seed, tiles, out, nullptr, false);
}
int pt_render_counted(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int maxDepth, int integrator, int useMIS, uint64_t seed,
                      const pt_tile_range* tiles, float* out, uint32_t* outCounters) {
    return render_host(s, cam, w, h, spp, maxDepth, integrator, useMIS, seed, tiles, out, outCounters, true);
}

}  // extern "C"

namespace pt {      // pt_adaptive.hip
hipError_t launch_adaptive_iota(int n, int* list, hipStream_t stream);
hipError_t launch_adaptive_snapshot(const int* list, int nList, const float4* S, float4* M, hipStream_t stream);
hipError_t launch_adaptive_error(const int* list, int nList, const float4* S, const float4* M, float4* H, int n, int w, int h, int tilesX,
                                 int minSpp, float threshold, int32_t* tileSpp, float* tileErr, int32_t* keep, hipStream_t stream);
hipError_t launch_adaptive_compact(const int* list, const int32_t* keep, int nList, int* out, int* outCount, hipStream_t stream);
hipError_t launch_adaptive_queue_save(const int* q, int* save, hipStream_t stream);
hipError_t launch_adaptive_moments(const int* list, int nList, const float4* S, float4* P, float4* Q, bool first, int batches, hipStream_t stream);
}

// What one round of pt_render_adaptive reads back: the new live count and the first 8 queue words after each of its two launches.
struct RoundWords { int count, pad[7]; int q[2][8]; };
static_assert(sizeof(RoundWords) == 96, "pt_api.h states the read-back's size");

// Argument checks of pt_render_adaptive[_device], all before the first HIP call: image size, params, NULL pointers, the scene.
// moments: pt_render_adaptive_moments[_device], which also wants equal batches (after the params' own checks) and outSq.
static int check_adaptive_args(pt_scene* s, const pt_camera* cam, int w, int h, int integrator, const pt_adaptive_params* p,
                               const void* out, const void* tileSpp, const void* outSq = nullptr, bool moments = false) {
    if (w <= 0 || h <= 0) return fail(-1, "pt_render_adaptive: image size %d x %d must be positive", w, h);
    if ((long long)w * h > 0x7fffffffll) return fail(-1, "pt_render_adaptive: image of %d x %d pixels is too large", w, h);
    if (!p) return fail(-1, "pt_render_adaptive: null params");
    if (p->max_spp < 2) return fail(-1, "pt_render_adaptive: max_spp %d must be at least 2", p->max_spp);
    if (p->min_spp < 0 || p->min_spp > p->max_spp) return fail(-1, "pt_render_adaptive: min_spp %d must lie in 0..max_spp (%d)", p->min_spp, p->max_spp);
    if (p->chunk_spp < 1) return fail(-1, "pt_render_adaptive: chunk_spp %d must be positive", p->chunk_spp);
    if (!(p->threshold >= 0.0f)) return fail(-1, "pt_render_adaptive: threshold %g must be a number >= 0", (double)p->threshold);
    if (moments && p->max_spp % (2 * p->chunk_spp) != 0)
        return fail(-1, "pt_render_adaptive_moments: max_spp %d must be a multiple of 2 * chunk_spp (%d), so that every batch has chunk_spp samples",
                    p->max_spp, 2 * p->chunk_spp);
    if (integrator != PT_UNIDIRECTIONAL && integrator != PT_NAIVE_UNIDIRECTIONAL)
        return fail(-3, "pt_render_adaptive: integrator %d is out of scope: only UNIDIRECTIONAL (0) and NAIVE_UNIDIRECTIONAL (2) are on this path", integrator);
    if (!cam) return fail(-1, "pt_render_adaptive: null camera");
    if (!out || !tileSpp || (moments && !outSq)) return fail(-1, "pt_render_adaptive: null output buffer");
    if (!s) return fail(-1, "pt_render_adaptive: null scene");
    if (s->variant != 0) return fail(-1, "pt_render_adaptive: the wavefront variant has no tile queue; select the megakernel (pt_set_variant 0)");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != s->device) return fail(-1, "scene lives on HIP device %d but the current device is %d", s->device, dev);
    return 0;
}

// The schedule of include/pt_api.h. Every buffer is the scene's, sized for the whole frame (the tile number indexes it); dOut,
// dSpp and dErr are device buffers. Once per round one read-back on `stream` brings the new live count and the queue words that
// each of the round's two launches left (the second launch re-initialises the queue, so the first one's words are saved on the
// device before it does): both launches are checked as queue_error checks a pt_render launch.
// With dSq (pt_render_adaptive_moments: a device buffer, scan-line) every launch is followed by the moments pass on its list and
// Q is untiled into dSq at the end; nothing else changes, so the other outputs are pt_render_adaptive's.
static int render_adaptive(pt_scene* s, const pt_camera* cam, int w, int h, int maxDepth, int integrator, int useMIS, uint64_t seed,
                           const pt_adaptive_params& p, float4* dOut, int32_t* dSpp, float* dErr, pt_adaptive_stats* stats, hipStream_t stream,
                           float4* dSq = nullptr) {
    TileSpan t;
    if (int r = resolve_tiles(w, h, nullptr, t)) return r;
    const int T = t.count;
    const size_t tileBytes = (size_t)T * 64 * sizeof(float4);
    if (int r = s->adS.ensure(tileBytes)) return r;
    if (int r = s->adM.ensure(tileBytes)) return r;
    if (int r = s->adH.ensure(tileBytes)) return r;
    if (int r = s->adList.ensure((size_t)2 * T * sizeof(int))) return r;
    if (int r = s->adKeep.ensure((size_t)T * sizeof(int32_t))) return r;
    if (int r = s->adCount.ensure(sizeof(RoundWords))) return r;
    if (dSq) {
        if (int r = s->adP.ensure(tileBytes)) return r;
        if (int r = s->adQ.ensure(tileBytes)) return r;
    }
    if (!dErr) {
        if (int r = s->adErr.ensure((size_t)T * sizeof(float))) return r;
        dErr = (float*)s->adErr.p;
    }
    float4* S = (float4*)s->adS.p;
    int* lists[2] = {(int*)s->adList.p, (int*)s->adList.p + T};
    HIP_OK(hipMemsetAsync(s->adS.p, 0, tileBytes, stream));           // this call writes the sums: they start at 0
    HIP_OK(hipMemsetAsync(s->adH.p, 0, tileBytes, stream));
    HIP_OK(launch_adaptive_iota(T, lists[0], stream));               // round 0: every tile, in the order of a full frame
    int n = 0, live = T, cur = 0, rounds = 0;
    while (live > 0) {
        const int c = std::min(p.chunk_spp, (p.max_spp - n) / 2);
        if (c == 0) break;
        RoundWords* dw = (RoundWords*)s->adCount.p;
        for (int half = 0; half < 2; half++) {
            // (round 0's first launch seeds the streams of every tile, as pt_render does; every later launch continues them)
            if (int r = render_tiles(s, cam, w, h, c, maxDepth, integrator, useMIS, seed, t, S, nullptr, false, stream, rounds > 0 || half > 0,
                                     lists[cur], live)) return r;
            HIP_OK(launch_adaptive_queue_save((const int*)s->queue.p, dw->q[half], stream));
            if (dSq)                                                  // (every half-round renders chunk_spp samples: the entry point checked)
                HIP_OK(launch_adaptive_moments(lists[cur], live, S, (float4*)s->adP.p, (float4*)s->adQ.p, rounds == 0 && half == 0,
                                               2 * rounds + half + 1, stream));
            if (half == 0) HIP_OK(launch_adaptive_snapshot(lists[cur], live, S, (float4*)s->adM.p, stream));
        }
        n += 2 * c;
        HIP_OK(launch_adaptive_error(lists[cur], live, S, (const float4*)s->adM.p, (float4*)s->adH.p, n, w, h, t.tilesX, p.min_spp, p.threshold,
                                     dSpp, dErr, (int32_t*)s->adKeep.p, stream));
        HIP_OK(launch_adaptive_compact(lists[cur], (const int32_t*)s->adKeep.p, live, lists[cur ^ 1], &dw->count, stream));
        RoundWords hw;
        HIP_OK(hipMemcpyAsync(&hw, dw, sizeof(hw), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        for (int half = 0; half < 2; half++)                          // both launches left every listed tile finished (or report -4)
            if (int r = queue_words_error(s, hw.q[half], T)) return r;
        const int next = hw.count;
        if (next < 0 || next > live) return fail(-2, "pt_render_adaptive: the live list grew from %d to %d tiles", live, next);
        live = next; cur ^= 1; rounds++;
    }
    HIP_OK(launch_untile(w, h, t, S, dOut, stream));
    if (dSq) HIP_OK(launch_untile(w, h, t, (const float4*)s->adQ.p, dSq, stream));
    if (stats) {
        std::vector<int32_t> spp(T);
        HIP_OK(hipMemcpyAsync(spp.data(), dSpp, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        stats->rounds = rounds; stats->tiles_at_max = 0; stats->pixel_samples = 0;
        for (int tile = 0; tile < T; tile++) {
            const int x0 = (tile % t.tilesX) * 8, y0 = (tile / t.tilesX) * 8;
            const long long px = (long long)std::min(8, w - x0) * std::min(8, h - y0);
            stats->pixel_samples += px * spp[tile];
            stats->tiles_at_max += spp[tile] == n ? 1 : 0;
        }
    }
    HIP_OK(hipStreamSynchronize(stream));
    return 0;
}

extern "C" {

int pt_render_adaptive_device(pt_scene* s, const pt_camera* cam, int w, int h, int max_depth, int integrator, int use_mis, uint64_t seed,
                              const pt_adaptive_params* params, void* d_rgba_sum, void* d_tile_spp, void* d_tile_err, pt_adaptive_stats* stats,
                              void* stream) {
    if (int r = check_adaptive_args(s, cam, w, h, integrator, params, d_rgba_sum, d_tile_spp)) return r;
    return render_adaptive(s, cam, w, h, max_depth, integrator, use_mis, seed, *params, (float4*)d_rgba_sum, (int32_t*)d_tile_spp,
                           (float*)d_tile_err, stats, (hipStream_t)stream);
}

int pt_render_adaptive(pt_scene* s, const pt_camera* cam, int w, int h, int max_depth, int integrator, int use_mis, uint64_t seed,
                       const pt_adaptive_params* params, float* out_rgba_sum, int32_t* out_tile_spp, float* out_tile_err, pt_adaptive_stats* stats) {
    if (int r = check_adaptive_args(s, cam, w, h, integrator, params, out_rgba_sum, out_tile_spp)) return r;
    const size_t px = (size_t)w * h, T = (size_t)((w + 7) / 8) * ((h + 7) / 8);
    if (int r = s->adOut.ensure(px * sizeof(float4))) return r;
    if (int r = s->adSpp.ensure(T * sizeof(int32_t))) return r;
    if (int r = s->adErr.ensure(T * sizeof(float))) return r;
    if (int r = render_adaptive(s, cam, w, h, max_depth, integrator, use_mis, seed, *params, (float4*)s->adOut.p, (int32_t*)s->adSpp.p,
                                (float*)s->adErr.p, stats, nullptr)) return r;
    HIP_OK(hipMemcpy(out_rgba_sum, s->adOut.p, px * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out_tile_spp, s->adSpp.p, T * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_tile_err) HIP_OK(hipMemcpy(out_tile_err, s->adErr.p, T * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int pt_render_adaptive_moments_device(pt_scene* s, const pt_camera* cam, int w, int h, int max_depth, int integrator, int use_mis, uint64_t seed,
                                      const pt_adaptive_params* params, void* d_rgba_sum, void* d_sq_sum, void* d_tile_spp, void* d_tile_err,
                                      pt_adaptive_stats* stats, void* stream) {
    if (int r = check_adaptive_args(s, cam, w, h, integrator, params, d_rgba_sum, d_tile_spp, d_sq_sum, true)) return r;
    return render_adaptive(s, cam, w, h, max_depth, integrator, use_mis, seed, *params, (float4*)d_rgba_sum, (int32_t*)d_tile_spp,
                           (float*)d_tile_err, stats, (hipStream_t)stream, (float4*)d_sq_sum);
}

int pt_render_adaptive_moments(pt_scene* s, const pt_camera* cam, int w, int h, int max_depth, int integrator, int use_mis, uint64_t seed,
                               const pt_adaptive_params* params, float* out_rgba_sum, float* out_sq_sum, int32_t* out_tile_spp,
                               float* out_tile_err, pt_adaptive_stats* stats) {
    if (int r = check_adaptive_args(s, cam, w, h, integrator, params, out_rgba_sum, out_tile_spp, out_sq_sum, true)) return r;
    const size_t px = (size_t)w * h, T = (size_t)((w + 7) / 8) * ((h + 7) / 8);
    if (int r = s->adOut.ensure(px * sizeof(float4))) return r;
    if (int r = s->adSq.ensure(px * sizeof(float4))) return r;
    if (int r = s->adSpp.ensure(T * sizeof(int32_t))) return r;
    if (int r = s->adErr.ensure(T * sizeof(float))) return r;
    if (int r = render_adaptive(s, cam, w, h, max_depth, integrator, use_mis, seed, *params, (float4*)s->adOut.p, (int32_t*)s->adSpp.p,
                                (float*)s->adErr.p, stats, nullptr, (float4*)s->adSq.p)) return r;
    HIP_OK(hipMemcpy(out_rgba_sum, s->adOut.p, px * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out_sq_sum, s->adSq.p, px * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out_tile_spp, s->adSpp.p, T * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_tile_err) HIP_OK(hipMemcpy(out_tile_err, s->adErr.p, T * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

namespace pt {      // pt_moments.hip
hipError_t launch_moments_update(int nTiles, const float4* S, float4* P, float4* Q, bool first, int batches, hipStream_t stream);
}

// Argument checks of pt_render_moments[_device], all before the first HIP call: image size, the sample counts, the integrator,
// NULL pointers (camera and the outputs), the camera's size, then the scene.
static int check_moments_args(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int batchSpp, int integrator, const void* outS,
                              const void* outQ) {
    if (w <= 0 || h <= 0) return fail(-1, "pt_render_moments: image size %d x %d must be positive", w, h);
    if ((long long)((w + 7) / 8) * ((h + 7) / 8) * 64 > 0x7fffffffll) return fail(-1, "pt_render_moments: image of %d x %d pixels is too large", w, h);
    if (spp <= 0) return fail(-1, "pt_render_moments: spp %d must be positive", spp);
    if (batchSpp <= 0) return fail(-1, "pt_render_moments: batch_spp %d must be positive", batchSpp);
    if (spp % batchSpp != 0) return fail(-1, "pt_render_moments: spp %d must be a multiple of batch_spp %d", spp, batchSpp);
    if (spp / batchSpp < 2) return fail(-1, "pt_render_moments: spp %d / batch_spp %d must give at least 2 batches", spp, batchSpp);
    if (integrator != PT_UNIDIRECTIONAL && integrator != PT_NAIVE_UNIDIRECTIONAL)
        return fail(-3, "pt_render_moments: integrator %d is out of scope: only UNIDIRECTIONAL (0) and NAIVE_UNIDIRECTIONAL (2) are on this path", integrator);
    if (!cam) return fail(-1, "pt_render_moments: null camera");
    if (cam->w != w || cam->h != h) return fail(-1, "pt_render_moments: the camera is %d x %d, the image %d x %d", cam->w, cam->h, w, h);
    if (!outS || !outQ) return fail(-1, "pt_render_moments: null output buffer");
    if (!s) return fail(-1, "pt_render_moments: null scene");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != s->device) return fail(-1, "scene lives on HIP device %d but the current device is %d", s->device, dev);
    return 0;
}

// B = spp / c ordinary launches of c samples into the scene's own zeroed accumulator, the first seeding the streams as pt_render
// does and the others continuing them; after each the bookkeeping pass, a wait, and the check pt_render makes of its launch (the
// tile queue's words; the wavefront variant checks itself). A batch that fails ends the call. dS, dQ: device, scan-line.
// With a list (pt_render_moments_tiles: `live` tiles, a device array, ascending) every launch renders the listed tiles through the
// tile queue, as render_adaptive's do. The streams are still seeded for the whole frame and the bookkeeping pass and the untile
// still cover it: S stays 0 where nothing was rendered, so Q.rgb does too. An empty list launches no render at all.
static int render_moments(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int c, int maxDepth, int integrator, int useMIS,
                          uint64_t seed, float4* dS, float4* dQ, hipStream_t stream, bool listed = false, const int* list = nullptr, int live = -1) {
    TileSpan t;
    if (int r = resolve_tiles(w, h, nullptr, t)) return r;
    const int T = t.count, B = spp / c;
    const size_t tileBytes = (size_t)T * 64 * sizeof(float4);
    if (int r = s->moS.ensure(tileBytes)) return r;
    if (int r = s->moP.ensure(tileBytes)) return r;
    if (int r = s->moQ.ensure(tileBytes)) return r;
    float4 *S = (float4*)s->moS.p, *P = (float4*)s->moP.p, *Q = (float4*)s->moQ.p;
    s->lastMomentsLaunches = 0;
    HIP_OK(hipMemsetAsync(S, 0, tileBytes, stream));                  // this call writes the sums: they start at 0
    if (listed && live == 0) HIP_OK(launch_moments_update(T, S, P, Q, true, B, stream));    // the zero frame: Q = (0, 0, 0, B)
    // "moments_fused": ONE launch of all spp samples whose lanes do the bookkeeping themselves at every c-th sample of their pixel
    // (pt_megakernel.h: MOMENTS) except the last, from P = Q = 0; then the same check and wait as after a batch, and ONE bookkeeping
    // pass: the last batch's boundary (S is final then) and Q.w. Same bits as the loop below. Where the launch's kernel has no fused twin (render_tiles says so and renders nothing) the loop below runs instead.
    bool seeded = false, ranFused = false;
    if (s->momentsFused && !(listed && live == 0) && spp < (1 << 22)) {        // (the kernel's boundary test is exact below 2^22 samples)
        HIP_OK(hipMemsetAsync(P, 0, tileBytes, stream));
        HIP_OK(hipMemsetAsync(Q, 0, tileBytes, stream));
        FusedMoments fused = {P, Q, c, false, false};
        if (int r = render_tiles(s, cam, w, h, spp, maxDepth, integrator, useMIS, seed, t, S, nullptr, false, stream, false, listed ? list : nullptr, live, &fused)) return r;
        seeded = fused.seeded;                                         // (the streams are seeded already: the first batch below must not seed them again)
        if (fused.launched) {
            s->lastMomentsLaunches = 1; ranFused = true;
            int q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const bool queued = s->queue.p && s->lastLaunchQueued;
            if (queued) HIP_OK(hipMemcpyAsync(q, s->queue.p, sizeof(q), hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            if (queued)
                if (int r = queue_words_error(s, q, s->lastLaunchTiles)) return r;
            HIP_OK(launch_moments_update(T, S, P, Q, false, B, stream));      // the last batch's boundary, and Q.w, for the whole frame
        }
    }
    for (int j = 0; j < B && !(listed && live == 0) && !ranFused; j++) {
        if (int r = render_tiles(s, cam, w, h, c, maxDepth, integrator, useMIS, seed, t, S, nullptr, false, stream, j > 0 || seeded, listed ? list : nullptr, live)) return r;
        s->lastMomentsLaunches = j + 1;
        HIP_OK(launch_moments_update(T, S, P, Q, j == 0, B, stream));
        int q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const bool queued = s->queue.p && s->variant == 0 && s->lastLaunchQueued;
        if (queued) HIP_OK(hipMemcpyAsync(q, s->queue.p, sizeof(q), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        if (queued)
            if (int r = queue_words_error(s, q, s->lastLaunchTiles)) return r;
    }
    HIP_OK(launch_untile(w, h, t, S, dS, stream));
    HIP_OK(launch_untile(w, h, t, Q, dQ, stream));
    HIP_OK(hipStreamSynchronize(stream));
    return 0;
}

// What the list forms check before check_moments_args: the image size (the tile count derives from it), the count and the list.
static int check_moments_list_args(int w, int h, const void* list, int count) {
    if (w <= 0 || h <= 0) return fail(-1, "pt_render_moments_tiles: image size %d x %d must be positive", w, h);
    const long long T = (long long)((w + 7) / 8) * ((h + 7) / 8);
    if (count < 0 || count > T) return fail(-1, "pt_render_moments_tiles: count %d must lie in 0..%lld, the frame's tiles", count, T);
    if (count > 0 && !list) return fail(-1, "pt_render_moments_tiles: null tile list");
    return 0;
}
static int check_moments_list_variant(pt_scene* s) {
    if (s->variant != 0) return fail(-1, "pt_render_moments_tiles: the wavefront variant has no tile queue; select the megakernel (pt_set_variant 0)");
    return 0;
}

extern "C" {

int pt_render_moments_tiles_device(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int batch_spp, int max_depth, int integrator,
                                   int use_mis, uint64_t seed, const void* d_tile_list, int count, void* d_rgba_sum, void* d_sq_sum,
                                   void* stream) {
    if (int r = check_moments_list_args(w, h, d_tile_list, count)) return r;
    if (int r = check_moments_args(s, cam, w, h, spp, batch_spp, integrator, d_rgba_sum, d_sq_sum)) return r;
    if (int r = check_moments_list_variant(s)) return r;
    return render_moments(s, cam, w, h, spp, batch_spp, max_depth, integrator, use_mis, seed, (float4*)d_rgba_sum, (float4*)d_sq_sum,
                          (hipStream_t)stream, true, (const int*)d_tile_list, count);
}

int pt_render_moments_tiles(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int batch_spp, int max_depth, int integrator, int use_mis,
                            uint64_t seed, const int32_t* tile_list, int count, float* out_rgba_sum, float* out_sq_sum) {
    if (int r = check_moments_list_args(w, h, tile_list, count)) return r;
    const int T = ((w + 7) / 8) * ((h + 7) / 8);
    for (int i = 0; i < count; i++)
        if (tile_list[i] < 0 || tile_list[i] >= T || (i > 0 && tile_list[i] <= tile_list[i - 1]))
            return fail(-1, "pt_render_moments_tiles: tile_list[%d] = %d: the list must be strictly ascending within 0..%d", i, tile_list[i], T - 1);
    if (int r = check_moments_args(s, cam, w, h, spp, batch_spp, integrator, out_rgba_sum, out_sq_sum)) return r;
    if (int r = check_moments_list_variant(s)) return r;
    const size_t bytes = (size_t)w * h * sizeof(float4);
    if (int r = s->moOut.ensure(2 * bytes)) return r;
    if (int r = s->moList.ensure((size_t)std::max(count, 1) * sizeof(int))) return r;
    if (count > 0) HIP_OK(hipMemcpy(s->moList.p, tile_list, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
    char* d = (char*)s->moOut.p;
    if (int r = render_moments(s, cam, w, h, spp, batch_spp, max_depth, integrator, use_mis, seed, (float4*)d, (float4*)(d + bytes), nullptr, true,
                               (const int*)s->moList.p, count)) return r;
    HIP_OK(hipMemcpy(out_rgba_sum, d, bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out_sq_sum, d + bytes, bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

extern "C" {

int pt_render_moments_device(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int batch_spp, int max_depth, int integrator,
                             int use_mis, uint64_t seed, void* d_rgba_sum, void* d_sq_sum, void* stream) {
    if (int r = check_moments_args(s, cam, w, h, spp, batch_spp, integrator, d_rgba_sum, d_sq_sum)) return r;
    return render_moments(s, cam, w, h, spp, batch_spp, max_depth, integrator, use_mis, seed, (float4*)d_rgba_sum, (float4*)d_sq_sum,
                          (hipStream_t)stream);
}

int pt_render_moments(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int batch_spp, int max_depth, int integrator, int use_mis,
                      uint64_t seed, float* out_rgba_sum, float* out_sq_sum) {
    if (int r = check_moments_args(s, cam, w, h, spp, batch_spp, integrator, out_rgba_sum, out_sq_sum)) return r;
    const size_t bytes = (size_t)w * h * sizeof(float4);
    if (int r = s->moOut.ensure(2 * bytes)) return r;
    char* d = (char*)s->moOut.p;
    if (int r = render_moments(s, cam, w, h, spp, batch_spp, max_depth, integrator, use_mis, seed, (float4*)d, (float4*)(d + bytes), nullptr)) return r;
    HIP_OK(hipMemcpy(out_rgba_sum, d, bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out_sq_sum, d + bytes, bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

// The feature passes (pt_aov.hip, pt_motion.hip, pt_motion_chain.hip, pt_ids.hip; their launchers and block counts: pt_feature_host.h).

// The traversal spill area of a feature pass of `blocks` workgroups: the passes' own (a render in flight on this scene keeps s->spill),
// shared among them, since all run on the caller's stream, one after the other. NULL for a scene whose stack never leaves the LDS.
static int feature_spill(pt_scene* s, int blocks, int32_t** spill) {
    *spill = nullptr;
    if (s->ds.stackSpill > 0) {
        if (int r = s->aovSpill.ensure((size_t)blocks * 4 * s->ds.stackSpill * 64 * sizeof(int32_t))) return r;
        *spill = (int32_t*)s->aovSpill.p;
    }
    return 0;
}

// The host form of a feature pass: render(d) into `staging`, where d[i] is output i's slice (NULL for an output the caller left out,
// whose slice stays reserved), then the copies to the host in order.
struct HostOut { void* host; size_t bytes; };
template <int N, class Render>
static int feature_download(DevBuf& staging, const HostOut (&out)[N], Render render) {
    size_t total = 0;
    for (const HostOut& o : out) total += o.bytes;
    if (int r = staging.ensure(total)) return r;
    void* d[N];
    char* at = (char*)staging.p;
    for (int i = 0; i < N; at += out[i++].bytes) d[i] = out[i].host ? at : nullptr;
    if (int r = render(d)) return r;
    for (int i = 0; i < N; i++)
        if (out[i].host) HIP_OK(hipMemcpy(out[i].host, d[i], out[i].bytes, hipMemcpyDeviceToHost));
    return 0;
}

// Argument checks of the AOV pass, all before the first HIP call (the device check comes last).
static int check_aov_args(pt_scene* s, const pt_camera* cam, int w, int h, int aovSpp, const void* a, const void* nd) {
    if (w <= 0 || h <= 0) return fail(-1, "pt_render_aovs: image size %d x %d must be positive", w, h);
    if ((long long)w * h > 0x7fffffffll) return fail(-1, "pt_render_aovs: image of %d x %d pixels is too large", w, h);
    if (aovSpp <= 0) return fail(-1, "pt_render_aovs: aov_spp %d must be positive", aovSpp);
    if (!cam) return fail(-1, "pt_render_aovs: null camera");
    if (cam->w != w || cam->h != h) return fail(-1, "pt_render_aovs: the camera is %d x %d, the image %d x %d", cam->w, cam->h, w, h);
    if (!a || !nd) return fail(-1, "pt_render_aovs: null output buffer");
    if (!s) return fail(-1, "pt_render_aovs: null scene");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != s->device) return fail(-1, "scene lives on HIP device %d but the current device is %d", s->device, dev);
    return 0;
}

static int render_aovs(pt_scene* s, const pt_camera* cam, int w, int h, int aovSpp, uint64_t seed, void* dA, void* dN, hipStream_t stream) {
    const int blocks = feature_blocks(feature_tiles(w, h).nTiles, s->numCU, kAovWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    HIP_OK(launch_aov(s->ds, cam_to_kernel(*cam), (const uint32_t*)s->jump.p, seed, w, h, aovSpp, blocks, (float4*)dA, (float4*)dN, spill, stream));
    return 0;
}

extern "C" {

int pt_render_aovs_device(pt_scene* s, const pt_camera* cam, int w, int h, int aov_spp, uint64_t seed, void* d_albedo, void* d_normal_depth,
                          void* stream) {
    if (int r = check_aov_args(s, cam, w, h, aov_spp, d_albedo, d_normal_depth)) return r;
    return render_aovs(s, cam, w, h, aov_spp, seed, d_albedo, d_normal_depth, (hipStream_t)stream);
}

int pt_render_aovs(pt_scene* s, const pt_camera* cam, int w, int h, int aov_spp, uint64_t seed, float* out_albedo, float* out_normal_depth) {
    if (int r = check_aov_args(s, cam, w, h, aov_spp, out_albedo, out_normal_depth)) return r;
    const size_t bytes = (size_t)w * h * sizeof(float4);
    return feature_download(s->aovOut, {{out_albedo, bytes}, {out_normal_depth, bytes}, {nullptr, 0}},
                            [&](void* const* d) { return render_aovs(s, cam, w, h, aov_spp, seed, d[0], d[1], nullptr); });
}

// The chain pass (pt_aov.hip: aov_chain_kernel): max_links, then the checks it shares with the first-hit pass, all before any HIP call.
static int check_aov_chain_args(pt_scene* s, const pt_camera* cam, int w, int h, int aovSpp, int maxLinks, const void* a, const void* nd) {
    if (maxLinks < 0 || maxLinks > 16) return fail(-1, "pt_render_aovs_chain: max_links %d must be 0..16", maxLinks);
    return check_aov_args(s, cam, w, h, aovSpp, a, nd);
}

static int render_aovs_chain(pt_scene* s, const pt_camera* cam, int w, int h, int aovSpp, int maxLinks, uint64_t seed, void* dA, void* dN, void* dL,
                             hipStream_t stream) {
    const int blocks = feature_blocks(feature_tiles(w, h).nTiles, s->numCU, kAovChainWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    HIP_OK(launch_aov_chain(s->ds, cam_to_kernel(*cam), (const uint32_t*)s->jump.p, seed, w, h, aovSpp, maxLinks, blocks, (float4*)dA, (float4*)dN,
                            (float*)dL, spill, stream));
    return 0;
}

int pt_render_aovs_chain_device(pt_scene* s, const pt_camera* cam, int w, int h, int aov_spp, int max_links, uint64_t seed, void* d_albedo,
                                void* d_normal_depth, void* d_links, void* stream) {
    if (int r = check_aov_chain_args(s, cam, w, h, aov_spp, max_links, d_albedo, d_normal_depth)) return r;
    return render_aovs_chain(s, cam, w, h, aov_spp, max_links, seed, d_albedo, d_normal_depth, d_links, (hipStream_t)stream);
}

int pt_render_aovs_chain(pt_scene* s, const pt_camera* cam, int w, int h, int aov_spp, int max_links, uint64_t seed, float* out_albedo,
                         float* out_normal_depth, float* out_links) {
    if (int r = check_aov_chain_args(s, cam, w, h, aov_spp, max_links, out_albedo, out_normal_depth)) return r;
    const size_t bytes = (size_t)w * h * sizeof(float4), lbytes = (size_t)w * h * sizeof(float);
    return feature_download(s->aovOut, {{out_albedo, bytes}, {out_normal_depth, bytes}, {out_links, lbytes}},
                            [&](void* const* d) { return render_aovs_chain(s, cam, w, h, aov_spp, max_links, seed, d[0], d[1], d[2], nullptr); });
}

// The centre pass (pt_aov.hip: aov_centre_kernel, aov_centre_chain_kernel): one unjittered pinhole ray per pixel, no seed.
static int check_aov_centre_args(pt_scene* s, const pt_camera* cam, int w, int h, int maxLinks, const void* a, const void* nd) {
    if (maxLinks < 0 || maxLinks > 16) return fail(-1, "pt_render_aovs_centre: max_links %d must be 0..16", maxLinks);
    return check_aov_args(s, cam, w, h, 1, a, nd);
}

// max_links 0 without a links buffer is the first-hit kernel; everything else the chain kernel (bit-identical where both apply).
static int render_aovs_centre(pt_scene* s, const pt_camera* cam, int w, int h, int maxLinks, void* dA, void* dN, void* dL, hipStream_t stream) {
    const bool chain = maxLinks > 0 || dL;
    const int blocks = feature_blocks(feature_tiles(w, h).nTiles, s->numCU, chain ? kAovChainWavesPerSimd : kAovCentreWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    if (chain) HIP_OK(launch_aov_centre_chain(s->ds, cam_to_kernel(*cam), w, h, maxLinks, blocks, (float4*)dA, (float4*)dN, (float*)dL, spill, stream));
    else HIP_OK(launch_aov_centre(s->ds, cam_to_kernel(*cam), w, h, blocks, (float4*)dA, (float4*)dN, spill, stream));
    return 0;
}

int pt_render_aovs_centre_device(pt_scene* s, const pt_camera* cam, int w, int h, int max_links, void* d_albedo, void* d_normal_depth, void* d_links,
                                 void* stream) {
    if (int r = check_aov_centre_args(s, cam, w, h, max_links, d_albedo, d_normal_depth)) return r;
    return render_aovs_centre(s, cam, w, h, max_links, d_albedo, d_normal_depth, d_links, (hipStream_t)stream);
}

int pt_render_aovs_centre(pt_scene* s, const pt_camera* cam, int w, int h, int max_links, float* out_albedo, float* out_normal_depth,
                          float* out_links) {
    if (int r = check_aov_centre_args(s, cam, w, h, max_links, out_albedo, out_normal_depth)) return r;
    const size_t bytes = (size_t)w * h * sizeof(float4), lbytes = (size_t)w * h * sizeof(float);
    return feature_download(s->aovOut, {{out_albedo, bytes}, {out_normal_depth, bytes}, {out_links, lbytes}},
                            [&](void* const* d) { return render_aovs_centre(s, cam, w, h, max_links, d[0], d[1], d[2], nullptr); });
}

// The motion pass (pt_motion.hip: motion_kernel): the centre pass's checks, the guide outputs both or neither, and the motion output.
static int check_motion_args(pt_scene* s, const pt_camera* cam, int w, int h, const void* a, const void* nd, const void* mv) {
    if ((a != nullptr) != (nd != nullptr)) return fail(-1, "pt_render_motion: albedo and normal_depth must be both NULL or both set");
    if (!mv) return fail(-1, "pt_render_motion: null motion output");
    return check_aov_centre_args(s, cam, w, h, 0, mv, mv);
}

static int render_motion(pt_scene* s, const pt_camera* cam, int w, int h, void* dA, void* dN, void* dM, hipStream_t stream) {
    const int blocks = feature_blocks(feature_tiles(w, h).nTiles, s->numCU, kMotionWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    const bool moving = s->hasMotion && s->deviceLeaf >= 0;
    HIP_OK(launch_motion(s->ds, s->kTris.p, s->posCur.p, moving ? s->posPrev.p : nullptr, s->nPositions, cam_to_kernel(*cam), w, h, blocks, (float4*)dA,
                         (float4*)dN, (float4*)dM, spill, stream));
    return 0;
}

int pt_render_motion_device(pt_scene* s, const pt_camera* cam, int w, int h, void* d_albedo, void* d_normal_depth, void* d_motion, void* stream) {
    if (int r = check_motion_args(s, cam, w, h, d_albedo, d_normal_depth, d_motion)) return r;
    return render_motion(s, cam, w, h, d_albedo, d_normal_depth, d_motion, (hipStream_t)stream);
}

int pt_render_motion(pt_scene* s, const pt_camera* cam, int w, int h, float* out_albedo, float* out_normal_depth, float* out_motion) {
    if (int r = check_motion_args(s, cam, w, h, out_albedo, out_normal_depth, out_motion)) return r;
    const size_t bytes = (size_t)w * h * sizeof(float4);
    return feature_download(s->motionOut, {{out_albedo, bytes}, {out_normal_depth, bytes}, {out_motion, bytes}},
                            [&](void* const* d) { return render_motion(s, cam, w, h, d[0], d[1], d[2], nullptr); });
}

// The motion pass through mirrors and glass (pt_motion_chain.hip: motion_chain_kernel). Its own checks, every message under its own
// name, all before any HIP call (the device check comes last).
static int check_motion_chain_args(pt_scene* s, const pt_camera* cam, int w, int h, int maxLinks, const void* a, const void* nd, const void* l,
                                   const void* mv) {
    if (maxLinks < 0 || maxLinks > 16) return fail(-1, "pt_render_motion_chain: max_links %d must be 0..16", maxLinks);
    if ((a != nullptr) != (nd != nullptr)) return fail(-1, "pt_render_motion_chain: albedo and normal_depth must be both NULL or both set");
    if (l && !a) return fail(-1, "pt_render_motion_chain: links needs albedo and normal_depth");
    if (!mv) return fail(-1, "pt_render_motion_chain: null motion output");
    if (w <= 0 || h <= 0) return fail(-1, "pt_render_motion_chain: image size %d x %d must be positive", w, h);
    if ((long long)w * h > 0x7fffffffll) return fail(-1, "pt_render_motion_chain: image of %d x %d pixels is too large", w, h);
    if (!cam) return fail(-1, "pt_render_motion_chain: null camera");
    if (cam->w != w || cam->h != h) return fail(-1, "pt_render_motion_chain: the camera is %d x %d, the image %d x %d", cam->w, cam->h, w, h);
    if (!s) return fail(-1, "pt_render_motion_chain: null scene");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != s->device)
        return fail(-1, "pt_render_motion_chain: scene lives on HIP device %d but the current device is %d", s->device, dev);
    return 0;
}

static int render_motion_chain(pt_scene* s, const pt_camera* cam, int w, int h, int maxLinks, void* dA, void* dN, void* dL, void* dM,
                               hipStream_t stream) {
    const int blocks = feature_blocks(feature_tiles(w, h).nTiles, s->numCU, kMotionChainWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    const bool moving = s->hasMotion && s->deviceLeaf >= 0;
    HIP_OK(launch_motion_chain(s->ds, s->kTris.p, s->posCur.p, moving ? s->posPrev.p : nullptr, s->nPositions, cam_to_kernel(*cam), w, h, maxLinks,
                               blocks, (float4*)dA, (float4*)dN, (float*)dL, (float4*)dM, spill, stream));
    return 0;
}

int pt_render_motion_chain_device(pt_scene* s, const pt_camera* cam, int w, int h, int max_links, void* d_albedo, void* d_normal_depth,
                                  void* d_links, void* d_motion, void* stream) {
    if (int r = check_motion_chain_args(s, cam, w, h, max_links, d_albedo, d_normal_depth, d_links, d_motion)) return r;
    return render_motion_chain(s, cam, w, h, max_links, d_albedo, d_normal_depth, d_links, d_motion, (hipStream_t)stream);
}

int pt_render_motion_chain(pt_scene* s, const pt_camera* cam, int w, int h, int max_links, float* out_albedo, float* out_normal_depth,
                           float* out_links, float* out_motion) {
    if (int r = check_motion_chain_args(s, cam, w, h, max_links, out_albedo, out_normal_depth, out_links, out_motion)) return r;
    const size_t bytes = (size_t)w * h * sizeof(float4), lbytes = (size_t)w * h * sizeof(float);
    return feature_download(s->motionOut, {{out_albedo, bytes}, {out_normal_depth, bytes}, {out_motion, bytes}, {out_links, lbytes}},
                            [&](void* const* d) { return render_motion_chain(s, cam, w, h, max_links, d[0], d[1], d[3], d[2], nullptr); });
}

// The ID pass and the pick queries (pt_ids.hip: ids_kernel, ids_chain_kernel). Every message under the caller's name, all before any
// HIP call (the device check comes last).
static int check_ids_args(const char* fn, pt_scene* s, const pt_camera* cam, int w, int h, int maxLinks, const void* ids, const int32_t* xy = nullptr,
                          int n = 0) {
    if (maxLinks < 0 || maxLinks > 16) return fail(-1, "%s: max_links %d must be 0..16", fn, maxLinks);
    if (w <= 0 || h <= 0) return fail(-1, "%s: image size %d x %d must be positive", fn, w, h);
    if ((long long)w * h > 0x7fffffffll) return fail(-1, "%s: image of %d x %d pixels is too large", fn, w, h);
    if (!cam) return fail(-1, "%s: null camera", fn);
    if (cam->w != w || cam->h != h) return fail(-1, "%s: the camera is %d x %d, the image %d x %d", fn, cam->w, cam->h, w, h);
    if (!ids) return fail(-1, "%s: null ids output", fn);
    for (int k = 0; k < n; k++)
        if (xy[2 * k] < 0 || xy[2 * k] >= w || xy[2 * k + 1] < 0 || xy[2 * k + 1] >= h)
            return fail(-1, "%s: pixel %d is (%d, %d), outside the %d x %d image", fn, k, xy[2 * k], xy[2 * k + 1], w, h);
    if (!s) return fail(-1, "%s: null scene", fn);
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != s->device) return fail(-1, "%s: scene lives on HIP device %d but the current device is %d", fn, s->device, dev);
    return 0;
}

// xy NULL: the image. xy set: nPick pixels (device memory), and dHit their (point, depth) records.
static int render_ids(pt_scene* s, const pt_camera* cam, int w, int h, int maxLinks, const int32_t* xy, int nPick, void* dIds, void* dHit,
                      hipStream_t stream) {
    const int nTiles = xy ? (nPick + 63) / 64 : feature_tiles(w, h).nTiles;
    const int blocks = feature_blocks(nTiles, s->numCU, maxLinks > 0 ? kIdsChainWavesPerSimd : kIdsWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    HIP_OK(launch_ids(s->ds, cam_to_kernel(*cam), w, h, maxLinks, xy, nPick, blocks, (int4*)dIds, (float4*)dHit, spill, stream));
    return 0;
}

int pt_render_ids_device(pt_scene* s, const pt_camera* cam, int w, int h, int max_links, void* d_ids, void* stream) {
    if (int r = check_ids_args("pt_render_ids", s, cam, w, h, max_links, d_ids)) return r;
    return render_ids(s, cam, w, h, max_links, nullptr, 0, d_ids, nullptr, (hipStream_t)stream);
}

int pt_render_ids(pt_scene* s, const pt_camera* cam, int w, int h, int max_links, int32_t* out_ids) {
    if (int r = check_ids_args("pt_render_ids", s, cam, w, h, max_links, out_ids)) return r;
    return feature_download(s->idsOut, {{out_ids, (size_t)w * h * sizeof(int4)}},
                            [&](void* const* d) { return render_ids(s, cam, w, h, max_links, nullptr, 0, d[0], nullptr, nullptr); });
}

int pt_pick(pt_scene* s, const pt_camera* cam, int w, int h, int n, const int32_t* xy, int max_links, int32_t* out_ids, float* out_hit) {
    if (n <= 0) return fail(-1, "pt_pick: n %d must be positive", n);
    if (!xy) return fail(-1, "pt_pick: null pixel list");
    if (!out_hit) return fail(-1, "pt_pick: null hit output");
    if (int r = check_ids_args("pt_pick", s, cam, w, h, max_links, out_ids, xy, n)) return r;
    // staging: the list, then the two outputs, each slice a multiple of 16 bytes
    const size_t xyBytes = ((size_t)n * 8 + 15) & ~(size_t)15, recBytes = (size_t)n * 16;
    if (int r = s->idsOut.ensure(xyBytes + 2 * recBytes)) return r;
    char* d = (char*)s->idsOut.p;
    HIP_OK(hipMemcpy(d, xy, (size_t)n * 8, hipMemcpyHostToDevice));
    if (int r = render_ids(s, cam, w, h, max_links, (const int32_t*)d, n, d + xyBytes, d + xyBytes + recBytes, nullptr)) return r;
    HIP_OK(hipMemcpy(out_ids, d + xyBytes, recBytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out_hit, d + xyBytes + recBytes, recBytes, hipMemcpyDeviceToHost));
    return 0;
}

int pt_has_experimental(void) { return 0; }     // always: the experimental variants were removed; kept for callers that ask

int pt_set_variant(pt_scene* s, int variant) {
    if (!s) return fail(-1, "null scene");
    if (variant != 0 && variant != 1) return fail(-1, "unknown variant %d (0 = megakernel, 1 = wavefront)", variant);
    s->variant = variant;
    return 0;
}

int pt_get_counters(pt_scene* s, pt_counters* out) {
    if (!s || !out) return fail(-1, "null argument");
    HIP_OK(hipMemcpy(out, s->totals.p, sizeof(pt_counters), hipMemcpyDeviceToHost));
    return 0;
}
int pt_reset_counters(pt_scene* s) {
    if (!s) return fail(-1, "null scene");
    HIP_OK(hipMemset(s->totals.p, 0, 16 * sizeof(unsigned long long)));
    return 0;
}
// Diagnostic builds only: the eight diagnostic sums behind the counters (-DPT_STAMPS: six per-phase s_memtime /
// wall-clock sums; -DPT_UTIL: wave- and lane-level trip counts of the traversal loops); zeros otherwise.
int pt_debug_stamps(pt_scene* s, unsigned long long* out8) {
    if (!s || !out8) return fail(-1, "null argument");
    HIP_OK(hipMemcpy(out8, (unsigned long long*)s->totals.p + 8, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

// The tile queue's waits are bounded (pt_kernels.hip); a wait that ran out leaves q[3] != 0 and an
// unfinished frame. Read where the host waits for the kernel anyway.
static int queue_error(pt_scene* s) {
    if (!s->queue.p || s->variant != 0 || !s->lastLaunchQueued) return 0;     // (an error word left by an earlier queued launch is not this launch's)
    int q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpy(q, s->queue.p, sizeof(q), hipMemcpyDeviceToHost) != hipSuccess) return fail(-2, "tile queue read-back failed");
    return queue_words_error(s, q, s->lastLaunchTiles);
}
// q: the first 8 header words that a queued launch of `tiles` tiles (the frame's, in list mode) left behind.
static int queue_words_error(pt_scene* s, const int* q, int tiles) {
    if (q[3] != 0) {
        // A waiter saw no progress for the whole bound (bit 0: a stall, recorded; the waiters stayed), or gave up for good after four
        // more (bit 1; bit 2: a push found no slot). The frame is complete iff every tile has been finished (each wave counts its tile
        // in q[2] after its last state store, and the kernel has ended); only an unfinished tile is an error.
        if (q[2] >= tiles) { s->queueStalls++; return 0; }
        return fail(-4, "megakernel tile queue timed out (code %d): %d of %d tiles finished, %d pops and %d pushes claimed; the first stalled waiter saw %d finished after %.1f M ticks "
                        "of the device's steady counter without progress: the frame is incomplete", q[3], q[2], tiles, q[0], q[1], q[6], (double)q[7] * 1.048576);
    }
    return 0;
}

// How often did a tile change hands in the last megakernel launch? The ring starts with every tile of the launch pushed once
// (q[1] = its tiles, in list mode the listed ones); every further push is a wave yielding its tile at the end of a time slice for
// another wave to continue.
int pt_last_tile_handovers(pt_scene* s) {
    if (!s) return fail(-1, "null scene");
    if (!s->queue.p || s->variant != 0 || !s->lastLaunchQueued) return 0;
    int q[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpy(q, s->queue.p, sizeof(q), hipMemcpyDeviceToHost));
    return std::max(0, q[1] - s->lastLaunchPushed);
}

// The 16 header words of the tile queue after the last queued launch (tests: the words' layout — q[4] / q[5], the issue-priority
// steering's sums, are back at zero when the kernel has ended, q[8..9] hold the wait bound in ticks, q[3] the stall / error bits).
int pt_debug_queue_header(pt_scene* s, int* out16) {
    if (!s || !out16) return fail(-1, "null argument");
    for (int i = 0; i < kQueueHeader; i++) out16[i] = 0;
    if (!s->queue.p || s->variant != 0 || !s->lastLaunchQueued) return 0;
    HIP_OK(hipMemcpy(out16, s->queue.p, kQueueHeader * sizeof(int), hipMemcpyDeviceToHost));
    return 1;
}

// Render launches of the last pt_render_moments* call on this scene: 1 when it ran fused, B in batches, 0 for an empty list.
int pt_last_moments_launches(pt_scene* s) { return s ? s->lastMomentsLaunches : -1; }

// Launches of this scene whose queue waiters gave up (no progress for "queue_timeout_ms") although the frame was complete.
int pt_queue_stalls(pt_scene* s) { return s ? s->queueStalls : 0; }

int pt_set_culling(pt_scene* s, int on) {
    if (!s) return fail(-1, "null scene");
    s->cull = on != 0;
    return 0;
}

// Per-scene kernel-selection and scheduling options (round 1 read these from the environment of the host process; an
// environment variable must not be able to change what a library renders, so they are explicit calls now). Only
// "culling" can reach the image (pt_set_culling); every other option selects between instantiations / schedules that
// are bit-identical by construction and by test.
namespace {
// One row per option: its name and range, and where its value lives — an int member of pt_scene, or a set / get pair where a
// plain store is not enough. A row with neither is an option of a variant that was removed: the name is still
// known, and `off`, the value that meant "not that variant", is the only one it accepts and the one it reads back.
struct Option {
    const char* name; int lo, hi;
    int pt_scene::*field;
    int (*set)(pt_scene*, int);          // returns an error code
    int (*get)(const pt_scene*);
    int off;
};
int removed(const char* name, int v) {
    return fail(-3, "pt_set_option: %s = %d selected an experimental variant that lost its measurement and was removed (DESIGN.md §6 has the results "
                    "and the commit that last held the code)", name, v);
}
const Option kOptions[] = {
    {"flat", 0, 2, &pt_scene::flatWanted}, {"onchip", 0, 1, &pt_scene::onchipOk},
    {"waves_hbm", 0, 2, nullptr,
     [](pt_scene* s, int v) { s->wavesHbmOk = v != 0; s->wavesHbmForce = s->wavesHbmOk && v == 2; return 0; },
     [](const pt_scene* s) { return s->wavesHbmForce ? 2 : (s->wavesHbmOk ? 1 : 0); }},
    {"refill", 0, 2, nullptr,            // (2 was REFILL for LDS-resident scenes: removed)
     [](pt_scene* s, int v) { if (v == 2) return removed("refill", v); s->refill = v; return 0; },
     [](const pt_scene* s) { return s->refill; }},
    {"refill_keep", 0, 15, nullptr,
     [](pt_scene* s, int v) { s->refillKeep = v; s->refillKeepSet = true; return 0; },
     [](const pt_scene* s) { return s->refillKeep; }},
    {"node_keep", 0, 15, &pt_scene::nodeKeep}, {"tri_keep", 0, 15, &pt_scene::triKeep},
    {"defer_shadow", 0, 1, nullptr, nullptr, nullptr, 0},
    {"slice_iters", 0, 1 << 30, &pt_scene::sliceIters}, {"slice_always", 0, 1, &pt_scene::sliceAlways},
    {"sched_mask", 0, 1 << 20, nullptr,
     [](pt_scene* s, int v) { if (((v + 1) & v) != 0) return fail(-1, "pt_set_option: sched_mask must be 2^k - 1"); s->schedMask = v; return 0; },
     [](const pt_scene* s) { return s->schedMask; }},
    {"lpt_prio", 0, 2, &pt_scene::lptPrio}, {"persistent", 0, 1, &pt_scene::persistent},
    {"xcd_bands", 0, 1, nullptr, nullptr, nullptr, 0},
    {"culling", 0, 1, &pt_scene::cull},
    {"spec", 0, 2, nullptr, nullptr, nullptr, 2},
    {"simple", 0, 1, &pt_scene::simpleWanted}, {"flat2", 0, 1, &pt_scene::flat2Wanted}, {"leaf_boxes", 0, 1, &pt_scene::leafBoxes},
    {"wide", 0, 1, nullptr, nullptr, nullptr, 0}, {"compact", 0, 1, nullptr, nullptr, nullptr, 0},
    {"wf_wide_wg", 0, 2, &pt_scene::wfWideWg}, {"lean", 0, 1, &pt_scene::leanWanted},
    {"queue_timeout_ms", 0, 1 << 22, &pt_scene::queueTimeoutMs}, {"moments_fused", 0, 1, &pt_scene::momentsFused},
};
const Option* find_option(const char* name) {
    if (name) for (const Option& o : kOptions) if (!strcmp(o.name, name)) return &o;
    return nullptr;
}
}  // namespace

int pt_set_option(pt_scene* s, const char* name, int v) {
    // (the name and the value are checked before the scene: what the library accepts can be asked without a device)
    const Option* o = find_option(name);
    if (!o) return fail(-1, "pt_set_option: unknown option '%s'", name ? name : "(null)");
    if (v < o->lo || v > o->hi) return fail(-1, "pt_set_option: %s = %d is outside [%d, %d]", name, v, o->lo, o->hi);
    if (!s) return fail(-1, "pt_set_option: null scene");
    if (o->set) return o->set(s, v);
    if (!o->field) return v == o->off ? 0 : removed(name, v);
    s->*(o->field) = v;
    return 0;
}

int pt_get_option(pt_scene* s, const char* name, int* out) {
    const Option* o = find_option(name);
    if (!o) return fail(-1, "pt_get_option: unknown option '%s'", name ? name : "(null)");
    if (!s || !out) return fail(-1, "pt_get_option: null argument");
    *out = o->get ? o->get(s) : (o->field ? s->*(o->field) : o->off);
    return 0;
}

int pt_scene_flags(pt_scene* s) {
    if (!s) return 0;
    const bool onchip = scene_onchip(s);
    const bool pers = s->persistent != 0;
    // the kernel the last launch used; before any launch, the one a frame with tiles enough for any kernel would get
    const bool hbm = s->lastLaunchHbm >= 0 ? s->lastLaunchHbm == 1 : hbm_kernel_pays(s, false, 1ll << 40);
    return (onchip ? 1 : 0) | (pers ? 2 : 0) | ((pers && s->sliceIters > 0) ? 4 : 0) | (hbm ? 8 : 0) | ((s->cull && hbm) ? 16 : 0) | (s->lastLaunchRefill ? 32 : 0) | (s->lastLaunchFlat ? 64 : 0) | (s->lastLaunchSimple ? 128 : 0) | (s->lastLaunchFlat2 ? 256 : 0) | (s->lastLaunchLeafTable ? 512 : 0) | (s->lastLaunchLean ? 1024 : 0);
}

float pt_last_kernel_ms(pt_scene* s) {
    if (!s) return -1.0f;
    if (s->evPending) {                                // waits for the last megakernel launch to finish
        if (hipEventSynchronize(s->ev1) != hipSuccess || hipEventElapsedTime(&s->lastKernelMs, s->ev0, s->ev1) != hipSuccess) return -1.0f;
        s->evPending = false;
        if (queue_error(s)) return -1.0f;
    }
    return s->lastKernelMs;
}

// device-memory helpers for novum_host.cpp (which stays free of HIP headers)
int pt_host_alloc_zero_(void** p, size_t bytes) {
    HIP_OK(hipMalloc(p, std::max<size_t>(bytes, 16)));
    HIP_OK(hipMemset(*p, 0, bytes));
    return 0;
}
int pt_host_download_(void* d, void* h, size_t bytes) {
    HIP_OK(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
    return 0;
}
int pt_host_download_free_(void* d, void* h, size_t bytes) {
    hipError_t e = hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(-2, "hipMemcpy D2H failed: %s", hipGetErrorString(e));
    return 0;
}

// ---- probes -------------------------------------------------------------------------------------
struct Scratch {      // RAII device scratch for the probe entry points
    std::vector<void*> ptrs;
    ~Scratch() { for (void* p : ptrs) (void)hipFree(p); }
    void* get(size_t bytes, const void* init = nullptr) {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        if (init && bytes) { if (hipMemcpy(p, init, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr; }
        return p;
    }
};
#define SCRATCH(var, type, bytes, init)                              \
    type* var = (type*)sc.get(bytes, init);                          \
    if (!var) return fail(-2, "probe: device scratch allocation failed")

static int jump_device(Scratch& sc, const uint32_t*& dj) {
    const std::vector<uint32_t>& jt = xorwow_host::jump_table();
    dj = (const uint32_t*)sc.get(jt.size() * 4, jt.data());
    return dj ? 0 : fail(-2, "probe: device scratch allocation failed");
}

int pt_probe_rng(uint64_t seed, int n, const uint32_t* subseq, int nDraws, uint32_t* outState6, uint32_t* outU32, float* outUni) {
    if (n <= 0 || nDraws < 0) return fail(-1, "bad sizes");
    Scratch sc;
    const uint32_t* dj; if (int r = jump_device(sc, dj)) return r;
    SCRATCH(dsub, uint32_t, (size_t)n * 4, subseq);
    SCRATCH(dst, uint32_t, (size_t)n * 24, nullptr);
    SCRATCH(du, uint32_t, (size_t)n * nDraws * 4, nullptr);
    SCRATCH(df, float, (size_t)n * nDraws * 4, nullptr);
    HIP_OK(launch_probe_rng(dj, seed, n, dsub, nDraws, dst, du, df, nullptr));
    HIP_OK(hipDeviceSynchronize());
    if (outState6) HIP_OK(hipMemcpy(outState6, dst, (size_t)n * 24, hipMemcpyDeviceToHost));
    if (outU32 && nDraws) HIP_OK(hipMemcpy(outU32, du, (size_t)n * nDraws * 4, hipMemcpyDeviceToHost));
    if (outUni && nDraws) HIP_OK(hipMemcpy(outUni, df, (size_t)n * nDraws * 4, hipMemcpyDeviceToHost));
    return 0;
}

// The moments pass of pt_render_adaptive_moments alone, as a round runs it: `live` tiles (the first of the frame, ascending) of a
// w x h frame's tile-major S, P and Q, one warm-up launch and then `reps` launches between two HIP events. *out_ms: their mean.
int pt_probe_adaptive_moments(int w, int h, int live, int reps, float* out_ms) {
    if (w <= 0 || h <= 0) return fail(-1, "pt_probe_adaptive_moments: image size %d x %d must be positive", w, h);
    const long long T = (long long)((w + 7) / 8) * ((h + 7) / 8);
    if (T * 64 > 0x7fffffffll) return fail(-1, "pt_probe_adaptive_moments: image of %d x %d pixels is too large", w, h);
    if (live < 1 || live > T) return fail(-1, "pt_probe_adaptive_moments: live %d must lie in 1..%lld, the frame's tiles", live, T);
    if (reps < 1) return fail(-1, "pt_probe_adaptive_moments: reps %d must be positive", reps);
    if (!out_ms) return fail(-1, "pt_probe_adaptive_moments: null output");
    Scratch sc;
    const size_t tileBytes = (size_t)T * 64 * sizeof(float4);
    SCRATCH(S, float4, tileBytes, nullptr);
    SCRATCH(P, float4, tileBytes, nullptr);
    SCRATCH(Q, float4, tileBytes, nullptr);
    SCRATCH(list, int, (size_t)live * sizeof(int), nullptr);
    HIP_OK(hipMemset(S, 0, tileBytes));
    HIP_OK(launch_adaptive_iota(live, list, nullptr));
    HIP_OK(launch_adaptive_moments(list, live, S, P, Q, true, 1, nullptr));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_OK(hipEventCreate(&e0));
    hipError_t e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
    for (int k = 0; k < reps && e == hipSuccess; k++) e = launch_adaptive_moments(list, live, S, P, Q, false, k + 2, nullptr);
    if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(-2, "pt_probe_adaptive_moments: %s", hipGetErrorString(e));
    *out_ms = ms / (float)reps;
    return 0;
}

int pt_probe_math(int n, const float* x, float* oSin, float* oCos, float* oExp, float* oRsqrt, float* oPow5) {
    if (n <= 0) return fail(-1, "bad sizes");
    Scratch sc;
    SCRATCH(dx, float, (size_t)n * 4, x);
    float* d[5]; float* outs[5] = {oSin, oCos, oExp, oRsqrt, oPow5};
    for (int k = 0; k < 5; k++) { d[k] = (float*)sc.get((size_t)n * 4); if (!d[k]) return fail(-2, "probe: device scratch allocation failed"); }
    HIP_OK(launch_probe_math(n, dx, d[0], d[1], d[2], d[3], d[4], nullptr));
    HIP_OK(hipDeviceSynchronize());
    for (int k = 0; k < 5; k++) if (outs[k]) HIP_OK(hipMemcpy(outs[k], d[k], (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int pt_probe_rcp_exhaustive(unsigned long long* out3, uint32_t* first_bad) {
    if (!out3) return fail(-1, "bad arguments");
    Scratch sc;
    SCRATCH(dout, unsigned long long, 32, nullptr);
    SCRATCH(dfb, uint32_t, 16, nullptr);
    HIP_OK(hipMemset(dout, 0, 32));
    HIP_OK(hipMemset(dfb, 0xff, 16));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(launch_probe_rcp_exhaustive(dout, dfb, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out3, dout, 24, hipMemcpyDeviceToHost));
    if (first_bad) HIP_OK(hipMemcpy(first_bad, dfb, 4, hipMemcpyDeviceToHost));
    return 0;
}

int pt_probe_camera_rays(const pt_camera* cam, uint64_t seed, int n, const int32_t* xy, float* outRays6) {
    if (!cam || n <= 0) return fail(-1, "bad arguments");
    Scratch sc;
    const uint32_t* dj; if (int r = jump_device(sc, dj)) return r;
    std::vector<uint32_t> sub(n);
    for (int i = 0; i < n; i++) sub[i] = (uint32_t)(xy[2 * i + 1] * cam->w + xy[2 * i]);
    SCRATCH(dsub, uint32_t, (size_t)n * 4, sub.data());
    SCRATCH(dst, uint32_t, (size_t)n * 24, nullptr);
    SCRATCH(du, uint32_t, 16, nullptr);
    SCRATCH(df, float, 16, nullptr);
    SCRATCH(dxy, int, (size_t)n * 8, xy);
    SCRATCH(dout, float, (size_t)n * 24, nullptr);
    HIP_OK(launch_probe_rng(dj, seed, n, dsub, 0, dst, du, df, nullptr));
    HIP_OK(launch_probe_camera(dst, cam_to_kernel(*cam), n, dxy, dout, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(outRays6, dout, (size_t)n * 24, hipMemcpyDeviceToHost));
    return 0;
}

int pt_probe_centre_rays(const pt_camera* cam, int n, const int32_t* xy, float* outRays6) {
    if (!cam || n <= 0 || !xy || !outRays6) return fail(-1, "pt_probe_centre_rays: bad arguments");
    Scratch sc;
    SCRATCH(dxy, int, (size_t)n * 8, xy);
    SCRATCH(dout, float, (size_t)n * 24, nullptr);
    HIP_OK(launch_probe_centre(cam_to_kernel(*cam), n, dxy, dout, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(outRays6, dout, (size_t)n * 24, hipMemcpyDeviceToHost));
    return 0;
}

static int probe_spill(pt_scene* s, int n, int32_t*& spill) {
    spill = nullptr;
    if (s->ds.stackSpill > 0) {
        if (int r = s->spill.ensure((size_t)probe_trace_blocks(n) * s->ds.stackSpill * 64 * sizeof(int32_t))) return r;
        spill = (int32_t*)s->spill.p;
    }
    return 0;
}

int pt_probe_trace_closest(pt_scene* s, int n, const float* rays6, int32_t* outI, float* outF, pt_counters* counters) {
    if (!s || n <= 0) return fail(-1, "bad arguments");
    Scratch sc;
    SCRATCH(dr, float, (size_t)n * 24, rays6);
    SCRATCH(di, int32_t, (size_t)n * 16, nullptr);
    SCRATCH(df, float, (size_t)n * 48, nullptr);
    SCRATCH(dt, unsigned long long, 64, nullptr);
    HIP_OK(hipMemset(dt, 0, 64));
    int32_t* spill; if (int r = probe_spill(s, n, spill)) return r;
    HIP_OK(launch_probe_closest(s->ds, n, dr, di, df, dt, spill, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(outI, di, (size_t)n * 16, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(outF, df, (size_t)n * 48, hipMemcpyDeviceToHost));
    if (counters) HIP_OK(hipMemcpy(counters, dt, 64, hipMemcpyDeviceToHost));
    return 0;
}

int pt_probe_trace_shadow(pt_scene* s, int n, const float* rays6, const float* maxT, float* outThr3, pt_counters* counters) {
    if (!s || n <= 0) return fail(-1, "bad arguments");
    Scratch sc;
    SCRATCH(dr, float, (size_t)n * 24, rays6);
    SCRATCH(dm, float, (size_t)n * 4, maxT);
    SCRATCH(df, float, (size_t)n * 12, nullptr);
    SCRATCH(dt, unsigned long long, 64, nullptr);
    HIP_OK(hipMemset(dt, 0, 64));
    int32_t* spill; if (int r = probe_spill(s, n, spill)) return r;
    HIP_OK(launch_probe_shadow(s->ds, n, dr, dm, df, dt, spill, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(outThr3, df, (size_t)n * 12, hipMemcpyDeviceToHost));
    if (counters) HIP_OK(hipMemcpy(counters, dt, 64, hipMemcpyDeviceToHost));
    return 0;
}

int pt_probe_bsdf_sample(pt_scene* s, int n, const int32_t* material, const float* wi3, const int32_t* backface, float etaI, float etaT,
                         uint64_t seed, const uint32_t* subseq, float* out8) {
    (void)etaT;      // the reference's sample_f_eval never reads etaT (reflectors.cuh:588-629)
    if (!s || n <= 0) return fail(-1, "bad arguments");
    Scratch sc;
    const uint32_t* dj; if (int r = jump_device(sc, dj)) return r;
    SCRATCH(dsub, uint32_t, (size_t)n * 4, subseq);
    SCRATCH(dst, uint32_t, (size_t)n * 24, nullptr);
    SCRATCH(du, uint32_t, 16, nullptr);
    SCRATCH(dfu, float, 16, nullptr);
    SCRATCH(dm, int, (size_t)n * 4, material);
    SCRATCH(dw, float, (size_t)n * 12, wi3);
    SCRATCH(db, int, (size_t)n * 4, backface);
    SCRATCH(dout, float, (size_t)n * 32, nullptr);
    HIP_OK(launch_probe_rng(dj, seed, n, dsub, 0, dst, du, dfu, nullptr));
    HIP_OK(launch_probe_bsdf_sample(s->ds, n, dm, dw, db, etaI, dst, dout, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out8, dout, (size_t)n * 32, hipMemcpyDeviceToHost));
    return 0;
}

int pt_probe_bsdf_eval(pt_scene* s, int n, const int32_t* material, const float* wi3, const float* wo3, float etaI, float etaT, float* out4) {
    (void)etaT;
    if (!s || n <= 0) return fail(-1, "bad arguments");
    Scratch sc;
    SCRATCH(dm, int, (size_t)n * 4, material);
    SCRATCH(dwi, float, (size_t)n * 12, wi3);
    SCRATCH(dwo, float, (size_t)n * 12, wo3);
    SCRATCH(dout, float, (size_t)n * 16, nullptr);
    HIP_OK(launch_probe_bsdf_eval(s->ds, n, dm, dwi, dwo, etaI, dout, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out4, dout, (size_t)n * 16, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
