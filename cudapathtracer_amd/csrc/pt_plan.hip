// pt_plan.hip — the decision and the sizing of a megakernel launch (pt_plan.h). Host code only, and pure: tests/test_mk_choice.py
// links this unit into a driver without a GPU and compares every plan with the record of what render_tiles decided before the
// decision moved here (tests/golden/launch_plan_parent.json).
#include <algorithm>

#include "../../include/pt_api.h"
#include "pt_plan.h"

namespace pt {

// LDS-resident instantiation: every PNode and PTri in the scene cache, the tree no deeper than the LDS stack, and the
// records the bounce reads (PAttr, PMat, PLight) within their own LDS budget.
// Its workgroups hold ONE copy of the scene each, and a CU has 160 KB of LDS for its 16 waves: workgroups of 4, 8 or 16
// waves get 1, 2 or 4 times the budgets kCacheBytes (PNodes + PTris) and kAttrCacheBytes. Returns the smallest workgroup
// size (in waves) that holds the scene, 0 if none does.
int scene_onchip_wg(const Facts& F, const Options& O) {
    if (!O.onchipOk || F.nTrisPacked <= 0 || F.ds.stackSpill != 0) return 0;
    const size_t geom = (size_t)F.nInternal * 64 + (size_t)F.nTrisPacked * 48, rec = attr_cache_bytes(F.nTrisPacked, F.nMats, F.nLightsPacked);
    // ... and 16 / wg such workgroups must fit a CU's 160 KB with the largest per-wave area any LDS-resident kernel uses (the pair
    // pass scratch, 24 x 256 B, plus the medium stack of the non-SIMPLE kernels): a Cornell box of glass, water and gold at four
    // waves per workgroup was 1 KB over — three workgroups per CU instead of four, 19 % of the frame (round 3)
    const size_t perWave = (size_t)kStackFlat2Rows * 256 + (F.simpleOk && O.simpleWanted ? 0 : (size_t)kMediumMax * 64);
    for (int wg = 4; wg <= 16; wg *= 2)
        if (geom <= (size_t)kCacheBytes * (wg / 4) && (kAttrCacheBytes == 0 || rec <= (size_t)kAttrCacheBytes * (wg / 4)) &&
            geom + rec + (size_t)wg * perWave <= (size_t)160 * 1024 * wg / 16) return wg;
    return 0;
}
bool scene_onchip(const Facts& F, const Options& O) { return scene_onchip_wg(F, O) > 0; }
// Does a launch of `tiles` tiles get megakernel_hbm — six waves per SIMD, eight with the SIMPLE bounce — and not the general 4-wave
// kernel? A scene in HBM does, with enough tiles to fill those waves: with fewer (a 1/8 shard of a 1080p frame is 4050 tiles for 6144
// slots) the extra slots stay empty and the 4-wave kernel's faster waves win (measured: 1/8 shard 176 vs 185 ms, 1/4 shard equal, 1/2
// shard 602 vs 518 ms on the 263 k-triangle scene). The SIMPLE kernel's eight waves pay from ~3/4 of its 8192 slots on — a 1/4 share of
// a 1080p frame: 201 vs 269 ms — the generic kernel's six from 5/4 of its 6144 (profiles/r02_sched_shards.log).
bool hbm_kernel_pays(const Facts& F, const Options& O, int numCU, bool simple, long long tiles) {
    if (scene_onchip(F, O) || !O.wavesHbmOk) return false;
    const long long slots = (long long)numCU * 4 * (simple ? kWavesHbmSimple : kWavesHbm);
    return O.wavesHbmForce || tiles * 4 >= slots * (simple ? 3 : 5);
}

// The selector fields of a launch. The kernel they choose (pt_kernels.hip: megakernel_choose) is what size_launch sizes everything for.
LaunchPlan plan_launch(const Facts& F, const Options& O, int numCU, const LaunchAsk& ask) {
    LaunchPlan p = {};
    p.onchipWg = scene_onchip_wg(F, O);
    const bool onchip = p.onchipWg > 0;
    // the SIMPLE bounce for a scene in HBM: diffuse-only scenes, timed launches with the resumable traversal
    p.simpleTimed = F.simpleOk && O.simpleWanted && O.refill && !O.cull && !F.armless;
    const bool simpleHbm = !onchip && O.wavesHbmOk && p.simpleTimed && !ask.count;
    // a counting launch stands in for the timed launch of the same tiles (bench.py), which may get another kernel than it does: a
    // counting kernel has no SIMPLE bounce, so its slots fill by the generic rule (hbm_kernel_pays says no to every `simple` where
    // simpleHbm's other conditions fail, so a timed launch's two answers are one)
    p.timedHbm = hbm_kernel_pays(F, O, numCU, p.simpleTimed, ask.live);
    p.hbm = ask.count ? hbm_kernel_pays(F, O, numCU, false, ask.live) : p.timedHbm;
    p.cull = O.cull && p.hbm;
    p.refill = O.refill && !p.cull && !F.armless && !onchip;
    p.flat = 0;
    if (onchip && F.flatOk && O.flatWanted) {
        p.flat = (F.nInternal <= 64 && F.nTrisPacked <= 64) ? 1 : 2;     // 65..128: +17-20 % over the stack walk with the leaf-box form (profiles/r02_flat_crossover.jsonl)
    }
    // the instantiations that have the SIMPLE bounce: FLAT, the production kernel for scenes in HBM and its 4-wave form (small shares)
    p.simple = (p.flat && F.simpleOk && O.simpleWanted) || simpleHbm;
    if (p.flat == 1 && F.noLeafTris && !F.armless && O.flat2Wanted && ask.integrator == PT_UNIDIRECTIONAL && !ask.count && ask.useMIS) p.flat = 3;   // ... and the pair form of FLAT
    // the LEAN generic bounce exists for the three timed kernels generic scenes run: the pair form of FLAT, the kernel for scenes in HBM
    // and its 4-wave form (both REFILL)
    p.lean = F.leanOk && O.leanWanted && !F.armless && !p.simple && !ask.count && !p.cull && (p.flat == 3 || (!onchip && p.refill));
    return p;
}

KParams plan_selectors(const LaunchPlan& plan) {
    KParams P = {};
    P.onchip = plan.onchipWg > 0 ? 1 : 0;
    P.hbm = plan.hbm ? 1 : 0;
    P.cull = plan.cull ? 1 : 0;
    P.refill = plan.refill ? 1 : 0;
    P.flat = plan.flat;
    P.simple = plan.simple ? 1 : 0;
    P.lean = plan.lean ? 1 : 0;
    return P;
}

// The row's LDS stack length lays out the spill area, its launch bounds give the workgroup and the grid.
LaunchSizes size_launch(const Facts& F, const Options& O, int numCU, const LaunchAsk& ask, const TileSpan& t, bool listed,
                        const LaunchPlan& plan, const MkRow& row, KParams& P) {
    const bool onchip = plan.onchipWg > 0;
    LaunchSizes z = {};
    z.spillEntries = plan.hbm ? std::max(0, F.stackNeed - row.f.stackEntries) : F.ds.stackSpill;
    P.wgWaves = row.f.wgWaves ? row.f.wgWaves : (onchip ? plan.onchipWg : 4);
    P.wavesPerSimd = row.f.wavesPerSimd;
    z.blocks = megakernel_blocks(t.count, P.wgWaves);
    P.S = F.ds;
    P.S.stackSpill = z.spillEntries;
    P.useMIS = ask.useMIS;
    P.tileFirst = t.first; P.tileStride = t.stride; P.tileCount = t.count; P.tilesX = t.tilesX;
    P.cacheNodes = F.cacheNodes; P.cacheTris = F.cacheTris;
    P.lightTri8 = F.lightTri8;
    if (onchip) { P.cacheNodes = F.nInternal; P.cacheTris = F.nTrisPacked; }      // the whole scene, in workgroups large enough to hold it
    if (onchip && kAttrCacheBytes > 0) { P.cacheAttrs = F.nTrisPacked; P.cacheMats = F.nMats; P.cacheLights = F.nLightsPacked; }   // the bounce's records in LDS as well
    if (onchip && kAttrCacheBytes > 0 && F.flatOk && O.leafBoxes && F.nLeaves > 0) P.nLeaves = F.nLeaves;       // (the caller points P.leaves at the table)
    if (P.nLeaves > 0 && plan.flat == 3) P.pad0 = F.nBoxes | (F.nBoxGroups << 8) | (F.boxAxis << 16);      // the pair kernels' box table (pt_params.h; the caller points P.pad1 at it)
    // (a scene in HBM has no FLAT form, so its kernel has the SIMPLE bounce exactly when it is the SIMPLE production kernel)
    if (plan.hbm && F.cacheTris == 0) P.cacheNodes = std::min(F.nInternal, (plan.simple ? kCacheBytesHbmSimple : kCacheBytesHbm) / 64);     // its workgroups share a larger copy of the top of the tree
    P.gnodeFrom = P.cacheNodes;
    if (ask.count && !onchip && F.cacheTris == 0) {
        // a counting launch stands in for the timed launch of the same tiles (bench.py): count a node fetch as "global" against THAT
        // instantiation's LDS copy of the tree top — the SIMPLE production kernel holds 768 nodes, this counting kernel 704 (or 192)
        P.gnodeFrom = plan.timedHbm ? std::min(F.nInternal, (plan.simpleTimed ? kCacheBytesHbmSimple : kCacheBytesHbm) / 64) : F.cacheNodes;
    }
    P.refillKeep = (plan.hbm || O.refillKeepSet) ? O.refillKeep : kRefillKeepSmall;      // re-swept on the round's kernels: 6 for the 8-wave kernel, 10 for the 4-wave one (1/8 shares +5.5 % / +6 %, profiles/r03_shards_hbm_final.log)
    P.nodeKeep = O.nodeKeep; P.triKeep = O.triKeep;
    P.lptPrio = O.lptPrio; P.sliceIters = O.sliceIters; P.schedMask = O.schedMask; P.sliceAlways = O.sliceAlways ? 1 : 0;
    P.queueTimeout = (unsigned long long)O.queueTimeoutMs * 100000ull;        // ms -> ticks of the 100 MHz steady counter (hipDeviceAttributeWallClockRate)
    if (O.persistent || listed) {
        z.queueCap = 256;
        while (z.queueCap < t.count) z.queueCap <<= 1;
        P.queueMask = z.queueCap - 1;
        P.gridBlocks = numCU * P.wavesPerSimd * 4 / P.wgWaves;      // n waves per SIMD = 4n waves per CU, in workgroups of wgWaves
    }
    return z;
}

}  // namespace pt
