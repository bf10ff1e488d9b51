// pt_plan.h — which megakernel a launch gets and how that launch is sized, as pure functions (pt_plan.hip) of what a scene knows about
// itself (Facts), its options, the chip's CU count and what the launch is asked for: no HIP call, no pt_scene, no error channel, no
// allocation, so tests/launch_plan_driver.hip walks them without a GPU. render_tiles (pt_render.hip) is their one caller on the launch
// path: plan_launch, then megakernel_choose (pt_kernels.hip) on the plan's selectors, then size_launch for the row that was chosen.
#pragma once
#include "pt_params.h"

namespace pt {

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
    int nBoxes = 0, nBoxGroups = 0, boxAxis = 0;   // ... and the timed pair kernels' table of its distinct boxes, behind it in the same buffer: records, groups of
                                          // records that share their interval on boxAxis, and that axis (pt_box_table.h); nBoxes 0: none
    unsigned long long lightTri8 = 0ull;  // a byte per light, for the first 8: 1 + the packed triangle the light is, 0 = none (light_triangles); KParams::lightTri8
    bool armless = false;        // a triangle uses a material type without a dispatch arm (pt_path.h): DEFER is not exact
    bool noLeafTris = false;     // no triangle carries a MAT_LEAF material: a shadow ray is occluded by any hit (order-free)
    bool simpleOk = false;       // scene qualifies for the SIMPLE bounce (diffuse-only, pt_path.h)
    bool leanOk = false;         // ... for the LEAN generic bounce (no MAT_LEAF triangle, no texture / transmission map on any triangle's material)
    bool flatOk = false;         // ... for the FLAT kernels: LDS-resident, at most 128 nodes / triangles (64- or 128-bit masks), checked in derive_layout
};

// The smallest workgroup (in waves) whose LDS holds the whole scene, 0 if none does; and whether a launch of `tiles` tiles of a scene
// in HBM gets megakernel_hbm (pt_plan.hip has the measurements behind both).
int scene_onchip_wg(const Facts& F, const Options& O);
bool scene_onchip(const Facts& F, const Options& O);
bool hbm_kernel_pays(const Facts& F, const Options& O, int numCU, bool simple, long long tiles);

// What a launch is asked for. live: the tiles it renders (a list's length, or the launch's tile count).
struct LaunchAsk { int integrator; bool count; int useMIS; int live; };
// What is decided for it: the selector fields megakernel_choose reads, and two facts about the TIMED launch of the same tiles, which
// a counting launch stands in for: whether that one has the SIMPLE bounce, and whether it gets the kernel for scenes in HBM.
struct LaunchPlan {
    int onchipWg;                // waves per workgroup of an LDS-resident scene, 0: the scene is not resident
    bool hbm, cull, refill;
    int flat;                    // 1: FLAT with 64-bit masks, 2: with 128-bit masks, 3: the pair form
    bool simple, lean;
    bool simpleTimed, timedHbm;
};
LaunchPlan plan_launch(const Facts& F, const Options& O, int numCU, const LaunchAsk& ask);
// A zeroed KParams (its padding too: pt_params.h) with the plan's selectors in it: what megakernel_choose takes.
KParams plan_selectors(const LaunchPlan& plan);

// What the launch's buffers must hold: traversal-stack entries per lane in the global spill area (0: none), the workgroups that area
// is laid out for, and the tile queue's ring capacity (0: no queue, one tile per wave).
struct LaunchSizes { int spillEntries, blocks, queueCap; };
// Everything of the launch that is sized for `row`, the kernel megakernel_choose returned for plan_selectors(plan): fills every field
// of P that is neither a device pointer nor the request's own camera and image (cam, w, h, spp, maxDepth). t: the launch's tiles;
// listed: they come as a list (adaptive sampling), so the launch goes through the tile queue whatever "persistent" says.
LaunchSizes size_launch(const Facts& F, const Options& O, int numCU, const LaunchAsk& ask, const TileSpan& t, bool listed,
                        const LaunchPlan& plan, const MkRow& row, KParams& P);

}  // namespace pt
