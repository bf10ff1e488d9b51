// pt_render.hip — the launcher boundary (launch_unidirectional / launch_naive_unidirectional, deviceCode.cuh:8-12): the launch of
// the render kernels, pt_render*, adaptive sampling and the moments renders. Host code only; the kernels live in pt_kernels.hip,
// the decision which of them a launch gets and how it is sized in pt_plan.hip.
#include "pt_host.h"

using namespace pt;

namespace pt {

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

// prefix: the entry point's name and ": ", or ""
static int check_integrator(int integrator, const char* prefix) {
    if (integrator != PT_UNIDIRECTIONAL && integrator != PT_NAIVE_UNIDIRECTIONAL)
        return fail(-3, "%sintegrator %d is out of scope: only UNIDIRECTIONAL (0) and NAIVE_UNIDIRECTIONAL (2) are on this path", prefix, integrator);
    return 0;
}
static int check_device(const pt_scene* s) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != s->dev.id) return fail(-1, "scene lives on HIP device %d but the current device is %d", s->dev.id, dev);
    return 0;
}

int check_render_args(pt_scene* s, const pt_camera* cam, int spp, int integrator) {
    if (!s || !cam) return fail(-1, "null scene or camera");
    if (spp < 0) return fail(-1, "negative sample count");
    if (int r = check_integrator(integrator, "")) return r;
    return check_device(s);
}
}  // namespace pt

// One call of render_tiles: rng init + megakernel on `stream`; d_tiles holds t.count*64 float4.
// List mode (list != null: adaptive sampling): t is the whole frame and the launch renders the `live` tiles that the device
// array `list` names, through the tile queue whatever "persistent" says; the kernel is picked by `live`. The RNG states, the
// accumulator and `left` stay indexed by tile number, so every buffer is sized for the whole frame.
// Fused (render_moments with "moments_fused"): the launch is to keep the squared batch sums itself, batches of c samples, in the
// tile-major buffers P and Q. If the kernel this launch gets has no fused twin, or the scene renders with the wavefront variant,
// nothing is rendered and `launched` stays false; `seeded` then says whether the streams have been seeded on `stream` already.
// The constructor takes what every caller sets; a caller assigns its own extras (spp, stream, list, count, ...) after it.
struct RenderRequest {
    const pt_camera* cam; int w, h, maxDepth, integrator, useMIS; uint64_t seed; TileSpan t; void* d_tiles;
    int spp = 0; uint32_t* d_pixcnt = nullptr; bool count = false; hipStream_t stream = nullptr;
    bool continueStreams = false; const int* list = nullptr; int live = -1;
    bool fused = false; float4 *P = nullptr, *Q = nullptr; int c = 0; bool launched = false, seeded = false;
    RenderRequest(const pt_camera* cam, int w, int h, int maxDepth, int integrator, int useMIS, uint64_t seed, const TileSpan& t, void* d_tiles)
        : cam(cam), w(w), h(h), maxDepth(maxDepth), integrator(integrator), useMIS(useMIS), seed(seed), t(t), d_tiles(d_tiles) {}
};

// The wavefront variant of render_tiles: logic / trace kernel pairs until no path is alive.
static int render_tiles_wavefront(pt_scene* s, const RenderRequest& rq) {
    if (s->facts.armless) return fail(-3, "the wavefront variant needs every material to have a dispatch arm (pt_path.h); use the megakernel");
    WfParams W;
    W.n = rq.t.count * 64; W.w = rq.w; W.h = rq.h; W.tileFirst = rq.t.first; W.tileStride = rq.t.stride; W.tilesX = rq.t.tilesX;
    W.nodeKeep = s->opt.nodeKeep; W.triKeep = s->opt.triKeep;
    if (int r = s->wf.state.ensure(wf_state_bytes(W.n))) return r;
    if (int r = s->wf.ctl.ensure(64)) return r;
    wf_carve(W, s->wf.state.p);
    W.qctl = (uint32_t*)s->wf.ctl.p;
    W.rng = (uint32_t*)s->work.rng.p; W.out = (float4*)rq.d_tiles;
    W.pathCtr = nullptr;
    if (rq.count) {
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
    const CamK ck = cam_to_kernel(*rq.cam);
    const bool wfSimple = s->facts.simpleOk && s->opt.simpleWanted && !rq.count;        // the SIMPLE bounce (pt_path.h) in the logic kernel: diffuse-only scenes, timed launches
    s->last.simple = wfSimple ? 1 : 0;
    HIP_OK(hipMemsetAsync(W.qctl, 0, 16, rq.stream));
    HIP_OK(hipEventRecord(s->dev.ev0, rq.stream));
    HIP_OK(launch_wf_init(W, rq.spp, rq.stream));
    // Paths end at different iterations; the host polls the queue length every 16 iterations.
    const long long cap = (long long)std::max(rq.spp, 1) * 4200 + 64;
    bool finished = false;
    for (long long it = 0; it < cap; it++) {
        HIP_OK(launch_wf_logic(rq.integrator, rq.count, wfSimple, W, s->facts.ds, ck, rq.maxDepth, rq.useMIS, (int)(it & 1), rq.stream));
        if ((it & 15) == 15) {
            uint32_t queued = 0;
            HIP_OK(hipMemcpyAsync(&queued, W.qctl + (it & 1) * 2, 4, hipMemcpyDeviceToHost, rq.stream));
            HIP_OK(hipStreamSynchronize(rq.stream));
            if (queued == 0) { finished = true; break; }
        }
        HIP_OK(launch_wf_trace(rq.count, wgWaves, blocks, W, s->facts.ds, wfNodes, wfTris, spill, spillPerLane, (int)(it & 1), rq.stream));
    }
    if (!finished) return fail(-4, "wavefront render did not terminate within %lld iterations", cap);
    HIP_OK(launch_wf_finish(W, rq.stream));
    if (rq.count) HIP_OK(launch_wf_counters(W, rq.d_pixcnt, (unsigned long long*)s->data.totals.p, rq.stream));
    HIP_OK(hipEventRecord(s->dev.ev1, rq.stream));
    s->last.evPending = true;
    return 0;
}

static int render_tiles(pt_scene* s, RenderRequest& rq) {
    const TileSpan& t = rq.t;
    if (t.count == 0) return 0;
    if (rq.fused && s->opt.variant == 1) return 0;
    const int live = rq.list ? rq.live : t.count;
    if (rq.list && (rq.count || s->opt.variant != 0 || t.first != 0 || t.stride != 1 || live < 0 || live > t.count)) return fail(-1, "render_tiles: bad tile list");
    // the reference keys the stream by the camera's image size (y*w+x with the launch's w, deviceCode.cu:59)
    if (int r = s->work.rng.ensure((size_t)t.count * 384 * sizeof(uint32_t))) return r;
    // continueStreams: a later chunk of a progressive render keeps the per-pixel XORWOW states the
    // previous chunk stored (the reference reloads / stores them around every sample, deviceCode.cu:294, 541)
    if (!rq.continueStreams) HIP_OK(launch_rng_init((const uint32_t*)s->data.jump.p, rq.seed, rq.w, rq.h, t, (uint32_t*)s->work.rng.p, rq.stream));
    if (rq.fused) rq.seeded = !rq.continueStreams;
    if (s->opt.variant == 1) return render_tiles_wavefront(s, rq);

    // The decision, the kernel it chooses, and everything that is sized for that kernel (pt_plan.hip)
    const LaunchAsk ask = {rq.integrator, rq.count, rq.useMIS, live};
    const LaunchPlan plan = plan_launch(s->facts, s->opt, s->dev.numCU, ask);
    KParams P = plan_selectors(plan);
    const MkRow* row = megakernel_choose(rq.integrator, rq.count, true, P, false);      // (syncShadow: outside the pair form of FLAT no kernel defers the shadow ray)
    if (!row) return fail(-1, "render_tiles: no megakernel is built for this launch");
    const LaunchSizes z = size_launch(s->facts, s->opt, s->dev.numCU, ask, t, rq.list != nullptr, plan, *row, P);

    // The buffers the sizes name, and the launch's pointers
    if (z.spillEntries > 0)
        if (int r = s->work.spill.ensure((size_t)z.blocks * P.wgWaves * z.spillEntries * 64 * sizeof(int32_t))) return r;
    if (z.queueCap > 0) {
        if (int r = s->work.queue.ensure((size_t)(kQueueHeader + 2 * z.queueCap) * sizeof(int))) return r;
        if (int r = s->work.left.ensure((size_t)t.count * 64 * sizeof(int))) return r;
        P.queue = (int*)s->work.queue.p; P.left = (int*)s->work.left.p;
    }
    P.cam = cam_to_kernel(*rq.cam);
    P.w = rq.w; P.h = rq.h; P.spp = rq.spp; P.maxDepth = rq.maxDepth;
    if (P.nLeaves > 0) P.leaves = (const PLeaf*)s->geo.leaves.p;
    if (P.pad0 > 0) P.pad1 = P.leaves + s->facts.nLeaves;       // the box table follows the leaf table (pt_scene.hip: derive_layout)
    P.rng = (uint32_t*)s->work.rng.p; P.out = (float4*)rq.d_tiles; P.pixCounters = rq.d_pixcnt;
    P.totals = rq.count ? (unsigned long long*)s->data.totals.p : nullptr;
#ifdef PT_STAMPS
    P.totals = (unsigned long long*)s->data.totals.p;           // the diagnostic build sums its stamps for timed launches too
#endif
    P.spill = z.spillEntries > 0 ? (int32_t*)s->work.spill.p : nullptr;

    s->last.lean = P.lean; s->last.refill = P.refill; s->last.hbm = P.hbm;
    s->last.flat = (P.flat && !rq.count) ? 1 : 0;
    s->last.simple = (P.simple && !rq.count) ? 1 : 0;
    s->last.flat2 = (P.flat == 3) ? 1 : 0;
    s->last.leafTable = (P.flat && !rq.count && P.nLeaves > 0) ? 1 : 0;
    s->last.queued = P.queue != nullptr;
    s->last.tiles = t.count;
    s->last.pushed = live;

    MomentsK M = {nullptr, nullptr, 0, 0.0f};
    if (rq.fused) {
        row = megakernel_choose(rq.integrator, rq.count, true, P, true);     // the twin: its counterpart's facts, so everything sized above stands
        if (!row || (row->key & kMkBuiltOnly)) return 0;                    // the caller renders in batches
        M.P = rq.P; M.Q = rq.Q; M.c = rq.c; M.rc = 1.0f / (float)rq.c;
        rq.launched = true;
    }
    HIP_OK(hipEventRecord(s->dev.ev0, rq.stream));            // HIP events on the launch stream, around the megakernel only
    HIP_OK(launch_megakernel(*row, P, live, rq.list, rq.stream, rq.fused ? &M : nullptr));
    HIP_OK(hipEventRecord(s->dev.ev1, rq.stream));
    s->last.evPending = true;
    return 0;
}

int pt_render_tiles_device(pt_scene* s, const pt_camera* cam, int w, int h, int spp, int maxDepth, int integrator, int useMIS,
                           uint64_t seed, const pt_tile_range* tiles, void* d_tile_rgba, int count_work, void* stream) {
    if (int r = check_render_args(s, cam, spp, integrator)) return r;
    if (!d_tile_rgba) return fail(-1, "null tile buffer");
    TileSpan t;
    if (int r = resolve_tiles(w, h, tiles, t)) return r;
    RenderRequest rq(cam, w, h, maxDepth, integrator, useMIS, seed, t, d_tile_rgba);
    rq.spp = spp; rq.count = count_work != 0; rq.stream = (hipStream_t)stream;
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
    RenderRequest rq(cam, w, h, maxDepth, integrator, useMIS, seed, t, s->work.tilebuf.p);
    rq.spp = spp; rq.d_pixcnt = d_pixcnt; rq.count = count;
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
    RenderRequest rq(&camera, w, h, maxDepth, integrator, useMIS, 103033ull, t, s->work.tilebuf.p);
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
    if (int r = check_integrator(integrator, "pt_render_adaptive: ")) return r;
    if (!cam) return fail(-1, "pt_render_adaptive: null camera");
    if (!out || !tileSpp || (moments && !outSq)) return fail(-1, "pt_render_adaptive: null output buffer");
    if (!s) return fail(-1, "pt_render_adaptive: null scene");
    if (s->opt.variant != 0) return fail(-1, "pt_render_adaptive: the wavefront variant has no tile queue; select the megakernel (pt_set_variant 0)");
    return check_device(s);
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
    RenderRequest rq(cam, w, h, maxDepth, integrator, useMIS, seed, t, S);
    rq.stream = stream;
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
    if (int r = check_integrator(integrator, "pt_render_moments: ")) return r;
    if (!cam) return fail(-1, "pt_render_moments: null camera");
    if (cam->w != w || cam->h != h) return fail(-1, "pt_render_moments: the camera is %d x %d, the image %d x %d", cam->w, cam->h, w, h);
    if (!outS || !outQ) return fail(-1, "pt_render_moments: null output buffer");
    if (!s) return fail(-1, "pt_render_moments: null scene");
    return check_device(s);
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
    RenderRequest rq(cam, w, h, maxDepth, integrator, useMIS, seed, t, S);
    rq.stream = stream; rq.list = listed ? list : nullptr; rq.live = live;
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
