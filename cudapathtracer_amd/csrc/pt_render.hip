// pt_render.hip — the launcher boundary (launch_unidirectional / launch_naive_unidirectional, deviceCode.cuh:8-12): the choice and
// the launch of the render kernels, pt_render*, adaptive sampling and the moments renders. Host code only; the kernels live in
// pt_kernels.hip.
#include "pt_host.h"

using namespace pt;

namespace pt {

// LDS-resident instantiation: every PNode and PTri in the scene cache, the tree no deeper than the LDS stack, and the
// records the bounce reads (PAttr, PMat, PLight) within their own LDS budget.
// Its workgroups hold ONE copy of the scene each, and a CU has 160 KB of LDS for its 16 waves: workgroups of 4, 8 or 16
// waves get 1, 2 or 4 times the budgets kCacheBytes (PNodes + PTris) and kAttrCacheBytes. Returns the smallest workgroup
// size (in waves) that holds the scene, 0 if none does.
int scene_onchip_wg(const pt_scene* s) {
    if (!s->opt.onchipOk || s->facts.nTrisPacked <= 0 || s->facts.ds.stackSpill != 0) return 0;
    const size_t geom = (size_t)s->facts.nInternal * 64 + (size_t)s->facts.nTrisPacked * 48, rec = attr_cache_bytes(s->facts.nTrisPacked, s->facts.nMats, s->facts.nLightsPacked);
    // ... and 16 / wg such workgroups must fit a CU's 160 KB with the largest per-wave area any LDS-resident kernel uses (the pair
    // pass scratch, 24 x 256 B, plus the medium stack of the non-SIMPLE kernels): a Cornell box of glass, water and gold at four
    // waves per workgroup was 1 KB over — three workgroups per CU instead of four, 19 % of the frame (round 3)
    const size_t perWave = (size_t)kStackFlat2Rows * 256 + (s->facts.simpleOk && s->opt.simpleWanted ? 0 : (size_t)kMediumMax * 64);
    for (int wg = 4; wg <= 16; wg *= 2)
        if (geom <= (size_t)kCacheBytes * (wg / 4) && (kAttrCacheBytes == 0 || rec <= (size_t)kAttrCacheBytes * (wg / 4)) &&
            geom + rec + (size_t)wg * perWave <= (size_t)160 * 1024 * wg / 16) return wg;
    return 0;
}
bool scene_onchip(const pt_scene* s) { return scene_onchip_wg(s) > 0; }
// Does a launch of `tiles` tiles get megakernel_hbm — six waves per SIMD, eight with the SIMPLE bounce — and not the general 4-wave
// kernel? A scene in HBM does, with enough tiles to fill those waves: with fewer (a 1/8 shard of a 1080p frame is 4050 tiles for 6144
// slots) the extra slots stay empty and the 4-wave kernel's faster waves win (measured: 1/8 shard 176 vs 185 ms, 1/4 shard equal, 1/2
// shard 602 vs 518 ms on the 263 k-triangle scene). The SIMPLE kernel's eight waves pay from ~3/4 of its 8192 slots on — a 1/4 share of
// a 1080p frame: 201 vs 269 ms — the generic kernel's six from 5/4 of its 6144 (profiles/r02_sched_shards.log).
bool hbm_kernel_pays(const pt_scene* s, bool simple, long long tiles) {
    if (scene_onchip(s) || !s->opt.wavesHbmOk) return false;
    const long long slots = (long long)s->dev.numCU * 4 * (simple ? kWavesHbmSimple : kWavesHbm);
    return s->opt.wavesHbmForce || tiles * 4 >= slots * (simple ? 3 : 5);
}

// ---- helpers ----------------------------------------------------------------------------------
int resolve_tiles(int w, int h, const pt_tile_range* tiles, TileSpan& t) {
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

CamK cam_to_kernel(const pt_camera& c) {
    CamK k;
    k.origin = V3{c.cameraOrigin.x, c.cameraOrigin.y, c.cameraOrigin.z};
    k.forward = V3{c.forward.x, c.forward.y, c.forward.z};
    k.right = V3{c.right.x, c.right.y, c.right.z};
    k.up = V3{c.up.x, c.up.y, c.up.z};
    k.w = c.w; k.h = c.h; k.aperture = c.aperture; k.focalDist = c.focalDist; k.fovScale = c.fovScale; k.jitter = c.antiAliasJitterDist;
    return k;
}

int check_render_args(pt_scene* s, const pt_camera* cam, int spp, int integrator) {
    if (!s || !cam) return fail(-1, "null scene or camera");
    if (spp < 0) return fail(-1, "negative sample count");
    if (integrator != PT_UNIDIRECTIONAL && integrator != PT_NAIVE_UNIDIRECTIONAL)
        return fail(-3, "integrator %d is out of scope: only UNIDIRECTIONAL (0) and NAIVE_UNIDIRECTIONAL (2) are on this path", integrator);
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != s->dev.id) return fail(-1, "scene lives on HIP device %d but the current device is %d", s->dev.id, dev);
    return 0;
}
}  // namespace pt

// One call of render_tiles: rng init + megakernel on `stream`; d_tiles holds t.count*64 float4.
// List mode (list != null: adaptive sampling): t is the whole frame and the launch renders the `live` tiles that the device
// array `list` names, through the tile queue whatever "persistent" says; the kernel is picked by `live`. The RNG states, the
// accumulator and `left` stay indexed by tile number, so every buffer is sized for the whole frame.
// Fused (render_moments with "moments_fused"): the launch is to keep the squared batch sums itself, batches of c samples, in the
// tile-major buffers P and Q. If the kernel this launch gets has no fused twin, or the scene renders with the wavefront variant,
// nothing is rendered and `launched` stays false; `seeded` then says whether the streams have been seeded on `stream` already.
struct RenderRequest {
    const pt_camera* cam; int w, h, spp, maxDepth, integrator, useMIS; uint64_t seed; TileSpan t; void* d_tiles;
    uint32_t* d_pixcnt = nullptr; bool count = false; hipStream_t stream = nullptr;
    bool continueStreams = false; const int* list = nullptr; int live = -1;
    bool fused = false; float4 *P = nullptr, *Q = nullptr; int c = 0; bool launched = false, seeded = false;
};

// The wavefront variant of render_tiles: logic / trace kernel pairs until no path is alive.
static int render_tiles_wavefront(pt_scene* s, const RenderRequest& rq) {
    const pt_camera* cam = rq.cam; const TileSpan& t = rq.t; void* d_tiles = rq.d_tiles; uint32_t* d_pixcnt = rq.d_pixcnt; hipStream_t stream = rq.stream;
    const int w = rq.w, h = rq.h, spp = rq.spp, maxDepth = rq.maxDepth, integrator = rq.integrator, useMIS = rq.useMIS; const bool count = rq.count;
    if (s->facts.armless) return fail(-3, "the wavefront variant needs every material to have a dispatch arm (pt_path.h); use the megakernel");
    WfParams W;
    W.n = t.count * 64; W.w = w; W.h = h; W.tileFirst = t.first; W.tileStride = t.stride; W.tilesX = t.tilesX;
    W.nodeKeep = s->opt.nodeKeep; W.triKeep = s->opt.triKeep;
    if (int r = s->wf.state.ensure(wf_state_bytes(W.n))) return r;
    if (int r = s->wf.ctl.ensure(64)) return r;
    wf_carve(W, s->wf.state.p);
    W.qctl = (uint32_t*)s->wf.ctl.p;
    W.rng = (uint32_t*)s->work.rng.p; W.out = (float4*)d_tiles;
    W.pathCtr = nullptr;
    if (count) {
        if (int r = s->wf.ctr.ensure((size_t)W.n * 8 * sizeof(uint32_t))) return r;
        W.pathCtr = (uint32_t*)s->wf.ctr.p;
    }
    // the trace kernel has its own LDS budget (no medium stacks, smaller traversal stack): the whole scene if it fits 12 KB, else
    // the top of the tree — in 16-wave workgroups, two per CU, that share 48 KB of it (`wf_wide_wg` 0: the 4-wave shape)
    int wfNodes, wfTris, wgWaves = 4;
    if ((size_t)s->facts.nInternal * 64 + (size_t)s->facts.ds.nTris * 48 <= (size_t)kWfCacheBytes) { wfNodes = s->facts.nInternal; wfTris = s->facts.ds.nTris; }
    else if (s->opt.wfWideWg == 2 || (s->opt.wfWideWg == 1 && (W.n + 1023) / 1024 >= s->dev.numCU * 2)) { wgWaves = 16; wfNodes = std::min(s->facts.nInternal, (80 * 1024 - 16 * kWfStackLds * 256) / 64); wfTris = 0; }
    else { wfNodes = std::min(s->facts.nInternal, kWfCacheBytes / 64); wfTris = 0; }
    const int blocks = std::max(1, std::min(s->dev.numCU * (32 / wgWaves), (W.n + 64 * wgWaves - 1) / (64 * wgWaves)));
    const int spillPerLane = std::max(0, s->facts.stackNeed - kWfStackLds);
    int32_t* spill = nullptr;
    if (spillPerLane > 0) {
        if (int r = s->wf.spill.ensure((size_t)blocks * wgWaves * spillPerLane * 64 * sizeof(int32_t))) return r;
        spill = (int32_t*)s->wf.spill.p;
    }
    const CamK ck = cam_to_kernel(*cam);
    const bool wfSimple = s->facts.simpleOk && s->opt.simpleWanted && !count;        // the SIMPLE bounce (pt_path.h) in the logic kernel: diffuse-only scenes, timed launches
    s->last.simple = wfSimple ? 1 : 0;
    HIP_OK(hipMemsetAsync(W.qctl, 0, 16, stream));
    HIP_OK(hipEventRecord(s->dev.ev0, stream));
    HIP_OK(launch_wf_init(W, spp, stream));
    // Paths end at different iterations; the host polls the queue length every 16 iterations.
    const long long cap = (long long)std::max(spp, 1) * 4200 + 64;
    bool finished = false;
    for (long long it = 0; it < cap; it++) {
        HIP_OK(launch_wf_logic(integrator, count, wfSimple, W, s->facts.ds, ck, maxDepth, useMIS, (int)(it & 1), stream));
        if ((it & 15) == 15) {
            uint32_t queued = 0;
            HIP_OK(hipMemcpyAsync(&queued, W.qctl + (it & 1) * 2, 4, hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            if (queued == 0) { finished = true; break; }
        }
        HIP_OK(launch_wf_trace(count, wgWaves, blocks, W, s->facts.ds, wfNodes, wfTris, spill, spillPerLane, (int)(it & 1), stream));
    }
    if (!finished) return fail(-4, "wavefront render did not terminate within %lld iterations", cap);
    HIP_OK(launch_wf_finish(W, stream));
    if (count) HIP_OK(launch_wf_counters(W, d_pixcnt, (unsigned long long*)s->data.totals.p, stream));
    HIP_OK(hipEventRecord(s->dev.ev1, stream));
    s->last.evPending = true;
    return 0;
}

static int render_tiles(pt_scene* s, RenderRequest& rq) {
    const pt_camera* cam = rq.cam; const TileSpan& t = rq.t; void* d_tiles = rq.d_tiles; uint32_t* d_pixcnt = rq.d_pixcnt; hipStream_t stream = rq.stream;
    const int w = rq.w, h = rq.h, spp = rq.spp, maxDepth = rq.maxDepth, integrator = rq.integrator, useMIS = rq.useMIS; const bool count = rq.count;
    const uint64_t seed = rq.seed; const bool continueStreams = rq.continueStreams, fused = rq.fused; const int* list = rq.list; int live = rq.live;
    if (t.count == 0) return 0;
    if (fused && s->opt.variant == 1) return 0;
    if (!list) live = t.count;
    if (list && (count || s->opt.variant != 0 || t.first != 0 || t.stride != 1 || live < 0 || live > t.count)) return fail(-1, "render_tiles: bad tile list");
    // the reference keys the stream by the camera's image size (y*w+x with the launch's w, deviceCode.cu:59)
    if (int r = s->work.rng.ensure((size_t)t.count * 384 * sizeof(uint32_t))) return r;
    // continueStreams: a later chunk of a progressive render keeps the per-pixel XORWOW states the
    // previous chunk stored (the reference reloads / stores them around every sample, deviceCode.cu:294, 541)
    if (!continueStreams) HIP_OK(launch_rng_init((const uint32_t*)s->data.jump.p, seed, w, h, t, (uint32_t*)s->work.rng.p, stream));
    if (fused) rq.seeded = !continueStreams;
    if (s->opt.variant == 1) return render_tiles_wavefront(s, rq);
    // First the selector fields of the launch, then the kernel they choose (pt_kernels.hip: megakernel_choose), then everything that is
    // sized for THAT kernel: its LDS stack length lays out the spill area, its launch bounds give the workgroup and the grid.
    const bool onchip = scene_onchip(s);
    // the SIMPLE bounce for a scene in HBM: diffuse-only scenes, timed launches with the resumable traversal
    const bool simpleTimed = s->facts.simpleOk && s->opt.simpleWanted && s->opt.refill && !s->opt.cull && !s->facts.armless;
    const bool simpleHbm = !onchip && s->opt.wavesHbmOk && simpleTimed && !count;
    const bool hbm = hbm_kernel_pays(s, simpleHbm, live);
    KParams P = {};                                         // (its padding too: pt_params.h)
    P.onchip = onchip ? 1 : 0;
    P.hbm = hbm ? 1 : 0;
    P.cull = (s->opt.cull && hbm) ? 1 : 0;
    P.refill = (s->opt.refill && !P.cull && !s->facts.armless && !onchip) ? 1 : 0;
    P.flat = 0;                                             // 1: FLAT with 64-bit masks, 2: with 128-bit masks
    if (onchip && s->facts.flatOk && s->opt.flatWanted) {
        P.flat = (s->facts.nInternal <= 64 && s->facts.nTrisPacked <= 64) ? 1 : 2;     // 65..128: +17-20 % over the stack walk with the leaf-box form (profiles/r02_flat_crossover.jsonl)
    }
    // the instantiations that have the SIMPLE bounce: FLAT, the production kernel for scenes in HBM and its 4-wave form (small shares)
    P.simple = ((P.flat && s->facts.simpleOk && s->opt.simpleWanted) || simpleHbm) ? 1 : 0;
    if (P.flat == 1 && s->facts.noLeafTris && !s->facts.armless && s->opt.flat2Wanted && integrator == PT_UNIDIRECTIONAL && !count && useMIS) P.flat = 3;   // ... and the pair form of FLAT
    // the LEAN generic bounce exists for the three timed kernels generic scenes run: the pair form of FLAT, the kernel for scenes in HBM
    // and its 4-wave form (both REFILL)
    P.lean = (s->facts.leanOk && s->opt.leanWanted && !s->facts.armless && !P.simple && !count && !P.cull && (P.flat == 3 || (!onchip && P.refill))) ? 1 : 0;
    const MkRow* row = megakernel_choose(integrator, count, true, P, false);      // (syncShadow: outside the pair form of FLAT no kernel defers the shadow ray)
    if (!row) return fail(-1, "render_tiles: no megakernel is built for this launch");
    const int spillEntries = hbm ? std::max(0, s->facts.stackNeed - row->f.stackEntries) : s->facts.ds.stackSpill;
    const int wgWaves = row->f.wgWaves ? row->f.wgWaves : (onchip ? scene_onchip_wg(s) : 4);
    int blocks = megakernel_blocks(t.count, wgWaves);
    if (spillEntries > 0)
        if (int r = s->work.spill.ensure((size_t)blocks * wgWaves * spillEntries * 64 * sizeof(int32_t))) return r;
    P.S = s->facts.ds;
    P.cam = cam_to_kernel(*cam);
    P.w = w; P.h = h; P.spp = spp; P.maxDepth = maxDepth; P.useMIS = useMIS;
    P.tileFirst = t.first; P.tileStride = t.stride; P.tileCount = t.count; P.tilesX = t.tilesX;
    P.cacheNodes = s->facts.cacheNodes; P.cacheTris = s->facts.cacheTris;
    if (onchip) { P.cacheNodes = s->facts.nInternal; P.cacheTris = s->facts.nTrisPacked; }      // the whole scene, in workgroups large enough to hold it
    P.cacheAttrs = P.cacheMats = P.cacheLights = 0;
    P.nLeaves = 0; P.leaves = nullptr;
    P.lightTri8 = s->facts.lightTri8;
    if (onchip && kAttrCacheBytes > 0) { P.cacheAttrs = s->facts.nTrisPacked; P.cacheMats = s->facts.nMats; P.cacheLights = s->facts.nLightsPacked; }   // the bounce's records in LDS as well
    if (onchip && kAttrCacheBytes > 0 && s->facts.flatOk && s->opt.leafBoxes && s->facts.nLeaves > 0) { P.nLeaves = s->facts.nLeaves; P.leaves = (const PLeaf*)s->geo.leaves.p; }
    P.wgWaves = wgWaves;
    if (hbm && s->facts.cacheTris == 0) P.cacheNodes = std::min(s->facts.nInternal, (simpleHbm ? kCacheBytesHbmSimple : kCacheBytesHbm) / 64);     // its workgroups share a larger copy of the top of the tree
    P.gnodeFrom = P.cacheNodes;
    if (count && !onchip && s->opt.wavesHbmOk && s->facts.cacheTris == 0) {
        // a counting launch stands in for the timed launch of the same tiles (bench.py): count a node fetch as "global" against THAT
        // instantiation's LDS copy of the tree top — the SIMPLE production kernel holds 768 nodes, this counting kernel 704 (or 192)
        P.gnodeFrom = hbm_kernel_pays(s, simpleTimed, t.count) ? std::min(s->facts.nInternal, (simpleTimed ? kCacheBytesHbmSimple : kCacheBytesHbm) / 64) : s->facts.cacheNodes;
    }
    P.S.stackSpill = spillEntries;
    P.refillKeep = (hbm || s->opt.refillKeepSet) ? s->opt.refillKeep : kRefillKeepSmall;      // re-swept on the round's kernels: 6 for the 8-wave kernel, 10 for the 4-wave one (1/8 shares +5.5 % / +6 %, profiles/r03_shards_hbm_final.log)
    P.nodeKeep = s->opt.nodeKeep; P.triKeep = s->opt.triKeep;
    s->last.lean = P.lean;
    s->last.refill = P.refill; s->last.flat = (P.flat && !count) ? 1 : 0;
    s->last.simple = (P.simple && !count) ? 1 : 0;
    s->last.flat2 = (P.flat == 3) ? 1 : 0;
    s->last.leafTable = (P.flat && !count && P.nLeaves > 0) ? 1 : 0;
    s->last.hbm = hbm ? 1 : 0;
    P.wavesPerSimd = row->f.wavesPerSimd;
    P.queue = nullptr; P.queueMask = 0; P.left = nullptr; P.gridBlocks = 0;
    P.lptPrio = s->opt.lptPrio; P.sliceIters = s->opt.sliceIters; P.schedMask = s->opt.schedMask; P.sliceAlways = s->opt.sliceAlways ? 1 : 0;
    P.queueTimeout = (unsigned long long)s->opt.queueTimeoutMs * 100000ull;        // ms -> ticks of the 100 MHz steady counter (hipDeviceAttributeWallClockRate)
    if (s->opt.persistent || list) {
        int cap = 256;
        while (cap < t.count) cap <<= 1;
        if (int r = s->work.queue.ensure((size_t)(kQueueHeader + 2 * cap) * sizeof(int))) return r;
        if (int r = s->work.left.ensure((size_t)t.count * 64 * sizeof(int))) return r;
        P.queue = (int*)s->work.queue.p; P.queueMask = cap - 1; P.left = (int*)s->work.left.p;
        P.gridBlocks = s->dev.numCU * P.wavesPerSimd * 4 / wgWaves;      // n waves per SIMD = 4n waves per CU, in workgroups of wgWaves
    }
    s->last.queued = P.queue != nullptr;
    s->last.tiles = t.count;
    s->last.pushed = live;
    P.rng = (uint32_t*)s->work.rng.p; P.out = (float4*)d_tiles; P.pixCounters = d_pixcnt;
    P.totals = count ? (unsigned long long*)s->data.totals.p : nullptr;
#ifdef PT_STAMPS
    P.totals = (unsigned long long*)s->data.totals.p;           // the diagnostic build sums its stamps for timed launches too
#endif
    P.spill = spillEntries > 0 ? (int32_t*)s->work.spill.p : nullptr;
    MomentsK M = {nullptr, nullptr, 0, 0.0f};
    if (fused) {
        row = megakernel_choose(integrator, count, true, P, true);     // the twin: its counterpart's facts, so everything sized above stands
        if (!row || (row->key & kMkBuiltOnly)) return 0;                    // the caller renders in batches
        M.P = rq.P; M.Q = rq.Q; M.c = rq.c; M.rc = 1.0f / (float)rq.c;
        rq.launched = true;
    }
    HIP_OK(hipEventRecord(s->dev.ev0, stream));            // HIP events on the launch stream, around the megakernel only
    HIP_OK(launch_megakernel(*row, P, live, list, stream, fused ? &M : nullptr));
    HIP_OK(hipEventRecord(s->dev.ev1, stream));
    s->last.evPending = true;
    return 0;
}

int pt_render_tiles_device(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int maxDepth, int integrator, int useMIS,
                           uint64_t seed, const pt_tile_range* tiles, void* d_tile_rgba, int count_work, void* stream) {
    if (int r = check_render_args(s, cam, spp, integrator)) return r;
    if (!d_tile_rgba) return fail(-1, "null tile buffer");
    TileSpan t;
    if (int r = resolve_tiles(w, h, tiles, t)) return r;
    RenderRequest rq; rq.cam = cam; rq.w = w; rq.h = h; rq.spp = spp; rq.maxDepth = maxDepth; rq.integrator = integrator; rq.useMIS = useMIS; rq.seed = seed;
    rq.t = t; rq.d_tiles = d_tile_rgba; rq.count = count_work != 0; rq.stream = (hipStream_t)stream;
    return render_tiles(s, rq);
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
    if (int r = s->work.tilebuf.ensure(std::max<size_t>((size_t)t.count * 64 * sizeof(float4), 16))) return r;
    HIP_OK(launch_tile(w, h, t, (const float4*)d_colors, (float4*)s->work.tilebuf.p, nullptr));
    RenderRequest rq; rq.cam = cam; rq.w = w; rq.h = h; rq.spp = spp; rq.maxDepth = maxDepth; rq.integrator = integrator; rq.useMIS = useMIS; rq.seed = seed;
    rq.t = t; rq.d_tiles = s->work.tilebuf.p; rq.d_pixcnt = d_pixcnt; rq.count = count;
    if (int r = render_tiles(s, rq)) return r;
    HIP_OK(launch_untile(w, h, t, (const float4*)s->work.tilebuf.p, (float4*)d_colors, nullptr));
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
    if (int r = s->work.tilebuf.ensure(std::max<size_t>((size_t)t.count * 64 * sizeof(float4), 16))) return r;
    HIP_OK(launch_tile(w, h, t, (const float4*)d_colors, (float4*)s->work.tilebuf.p, nullptr));
    RenderRequest rq; rq.cam = &camera; rq.w = w; rq.h = h; rq.maxDepth = maxDepth; rq.integrator = integrator; rq.useMIS = useMIS; rq.seed = 103033ull;
    rq.t = t; rq.d_tiles = s->work.tilebuf.p;
    for (int done = 0; done < numSample;) {
        const int n = std::min(chunk_spp, numSample - done);
        rq.spp = n; rq.continueStreams = done > 0;
        if (int r = render_tiles(s, rq)) return r;
        HIP_OK(launch_untile(w, h, t, (const float4*)s->work.tilebuf.p, (float4*)d_colors, nullptr));
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
    if (int r = s->work.colors.ensure(px * sizeof(float4))) return r;
    HIP_OK(hipMemcpy(s->work.colors.p, out, px * sizeof(float4), hipMemcpyHostToDevice));
    uint32_t* dpc = nullptr;
    if (outCounters) {
        if (int r = s->work.pixcnt.ensure(std::max<size_t>((size_t)t.count * 512 * sizeof(uint32_t), 16))) return r;
        dpc = (uint32_t*)s->work.pixcnt.p;
    }
    if (int r = launch_on_colors(s, cam, w, h, spp, maxDepth, integrator, useMIS, seed, tiles, s->work.colors.p, dpc, count)) return r;
    HIP_OK(hipMemcpy(out, s->work.colors.p, px * sizeof(float4), hipMemcpyDeviceToHost));
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
    if (s->opt.variant != 0) return fail(-1, "pt_render_adaptive: the wavefront variant has no tile queue; select the megakernel (pt_set_variant 0)");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != s->dev.id) return fail(-1, "scene lives on HIP device %d but the current device is %d", s->dev.id, dev);
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
    if (int r = s->ad.S.ensure(tileBytes)) return r;
    if (int r = s->ad.M.ensure(tileBytes)) return r;
    if (int r = s->ad.H.ensure(tileBytes)) return r;
    if (int r = s->ad.list.ensure((size_t)2 * T * sizeof(int))) return r;
    if (int r = s->ad.keep.ensure((size_t)T * sizeof(int32_t))) return r;
    if (int r = s->ad.count.ensure(sizeof(RoundWords))) return r;
    if (dSq) {
        if (int r = s->ad.P.ensure(tileBytes)) return r;
        if (int r = s->ad.Q.ensure(tileBytes)) return r;
    }
    if (!dErr) {
        if (int r = s->ad.err.ensure((size_t)T * sizeof(float))) return r;
        dErr = (float*)s->ad.err.p;
    }
    float4* S = (float4*)s->ad.S.p;
    int* lists[2] = {(int*)s->ad.list.p, (int*)s->ad.list.p + T};
    HIP_OK(hipMemsetAsync(s->ad.S.p, 0, tileBytes, stream));           // this call writes the sums: they start at 0
    HIP_OK(hipMemsetAsync(s->ad.H.p, 0, tileBytes, stream));
    HIP_OK(launch_adaptive_iota(T, lists[0], stream));               // round 0: every tile, in the order of a full frame
    int n = 0, live = T, cur = 0, rounds = 0;
    RenderRequest rq; rq.cam = cam; rq.w = w; rq.h = h; rq.maxDepth = maxDepth; rq.integrator = integrator; rq.useMIS = useMIS; rq.seed = seed;
    rq.t = t; rq.d_tiles = S; rq.stream = stream;
    while (live > 0) {
        const int c = std::min(p.chunk_spp, (p.max_spp - n) / 2);
        if (c == 0) break;
        RoundWords* dw = (RoundWords*)s->ad.count.p;
        for (int half = 0; half < 2; half++) {
            // (round 0's first launch seeds the streams of every tile, as pt_render does; every later launch continues them)
            rq.spp = c; rq.continueStreams = rounds > 0 || half > 0; rq.list = lists[cur]; rq.live = live;
            if (int r = render_tiles(s, rq)) return r;
            HIP_OK(launch_adaptive_queue_save((const int*)s->work.queue.p, dw->q[half], stream));
            if (dSq)                                                  // (every half-round renders chunk_spp samples: the entry point checked)
                HIP_OK(launch_adaptive_moments(lists[cur], live, S, (float4*)s->ad.P.p, (float4*)s->ad.Q.p, rounds == 0 && half == 0,
                                               2 * rounds + half + 1, stream));
            if (half == 0) HIP_OK(launch_adaptive_snapshot(lists[cur], live, S, (float4*)s->ad.M.p, stream));
        }
        n += 2 * c;
        HIP_OK(launch_adaptive_error(lists[cur], live, S, (const float4*)s->ad.M.p, (float4*)s->ad.H.p, n, w, h, t.tilesX, p.min_spp, p.threshold,
                                     dSpp, dErr, (int32_t*)s->ad.keep.p, stream));
        HIP_OK(launch_adaptive_compact(lists[cur], (const int32_t*)s->ad.keep.p, live, lists[cur ^ 1], &dw->count, stream));
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
    if (dSq) HIP_OK(launch_untile(w, h, t, (const float4*)s->ad.Q.p, dSq, stream));
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
    return staged_download(s->ad.out, {{out_rgba_sum, px * sizeof(float4)}, {out_tile_spp, T * sizeof(int32_t)}, {out_tile_err, T * sizeof(float)}}, [&](void* const* d) {
        return render_adaptive(s, cam, w, h, max_depth, integrator, use_mis, seed, *params, (float4*)d[0], (int32_t*)d[1], (float*)d[2], stats, nullptr);
    });
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
    const StagedOut out[] = {{out_rgba_sum, px * sizeof(float4)}, {out_sq_sum, px * sizeof(float4)}, {out_tile_spp, T * sizeof(int32_t)}, {out_tile_err, T * sizeof(float)}};
    return staged_download(s->ad.out, out, [&](void* const* d) {
        return render_adaptive(s, cam, w, h, max_depth, integrator, use_mis, seed, *params, (float4*)d[0], (int32_t*)d[2], (float*)d[3], stats, nullptr, (float4*)d[1]);
    });
}

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
    if (hipGetDevice(&dev) != hipSuccess || dev != s->dev.id) return fail(-1, "scene lives on HIP device %d but the current device is %d", s->dev.id, dev);
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
    if (int r = s->mo.S.ensure(tileBytes)) return r;
    if (int r = s->mo.P.ensure(tileBytes)) return r;
    if (int r = s->mo.Q.ensure(tileBytes)) return r;
    float4 *S = (float4*)s->mo.S.p, *P = (float4*)s->mo.P.p, *Q = (float4*)s->mo.Q.p;
    s->last.momentsLaunches = 0;
    HIP_OK(hipMemsetAsync(S, 0, tileBytes, stream));                  // this call writes the sums: they start at 0
    if (listed && live == 0) HIP_OK(launch_moments_update(T, S, P, Q, true, B, stream));    // the zero frame: Q = (0, 0, 0, B)
    // "moments_fused": ONE launch of all spp samples whose lanes do the bookkeeping themselves at every c-th sample of their pixel
    // (pt_megakernel.h: MOMENTS) except the last, from P = Q = 0; then the same check and wait as after a batch, and ONE bookkeeping
    // pass: the last batch's boundary (S is final then) and Q.w. Same bits as the loop below. Where the launch's kernel has no fused twin (render_tiles says so and renders nothing) the loop below runs instead.
    bool seeded = false, ranFused = false;
    RenderRequest rq; rq.cam = cam; rq.w = w; rq.h = h; rq.maxDepth = maxDepth; rq.integrator = integrator; rq.useMIS = useMIS; rq.seed = seed;
    rq.t = t; rq.d_tiles = S; rq.stream = stream; rq.list = listed ? list : nullptr; rq.live = live;
    if (s->opt.momentsFused && !(listed && live == 0) && spp < (1 << 22)) {        // (the kernel's boundary test is exact below 2^22 samples)
        HIP_OK(hipMemsetAsync(P, 0, tileBytes, stream));
        HIP_OK(hipMemsetAsync(Q, 0, tileBytes, stream));
        rq.spp = spp; rq.fused = true; rq.P = P; rq.Q = Q; rq.c = c;
        if (int r = render_tiles(s, rq)) return r;
        rq.fused = false;
        seeded = rq.seeded;                                            // (the streams are seeded already: the first batch below must not seed them again)
        if (rq.launched) {
            s->last.momentsLaunches = 1; ranFused = true;
            if (int r = wait_and_check(s, stream)) return r;
            HIP_OK(launch_moments_update(T, S, P, Q, false, B, stream));      // the last batch's boundary, and Q.w, for the whole frame
        }
    }
    for (int j = 0; j < B && !(listed && live == 0) && !ranFused; j++) {
        rq.spp = c; rq.continueStreams = j > 0 || seeded;
        if (int r = render_tiles(s, rq)) return r;
        s->last.momentsLaunches = j + 1;
        HIP_OK(launch_moments_update(T, S, P, Q, j == 0, B, stream));
        if (int r = wait_and_check(s, stream)) return r;
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
    if (s->opt.variant != 0) return fail(-1, "pt_render_moments_tiles: the wavefront variant has no tile queue; select the megakernel (pt_set_variant 0)");
    return 0;
}

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
    if (int r = s->mo.list.ensure((size_t)std::max(count, 1) * sizeof(int))) return r;
    if (count > 0) HIP_OK(hipMemcpy(s->mo.list.p, tile_list, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
    return staged_download(s->mo.out, {{out_rgba_sum, bytes}, {out_sq_sum, bytes}}, [&](void* const* d) {
        return render_moments(s, cam, w, h, spp, batch_spp, max_depth, integrator, use_mis, seed, (float4*)d[0], (float4*)d[1], nullptr, true,
                              (const int*)s->mo.list.p, count);
    });
}

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
    return staged_download(s->mo.out, {{out_rgba_sum, bytes}, {out_sq_sum, bytes}}, [&](void* const* d) {
        return render_moments(s, cam, w, h, spp, batch_spp, max_depth, integrator, use_mis, seed, (float4*)d[0], (float4*)d[1], nullptr);
    });
}
