// pt_api.hip — the parts of the C ABI in include/pt_api.h that are neither a scene's making (pt_scene.hip), a render (pt_render.hip,
// pt_feature_api.hip) nor a probe (pt_probe.hip): the error channel, the counters, the tile queue's words, the options. Host code only.
#include <cstdarg>
#include <cstdio>
#include <string>

#include "pt_host.h"

using namespace pt;

// ---- errors ---------------------------------------------------------------------------------
static thread_local std::string g_err;
namespace pt {
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}

// q: the first 8 header words that a queued launch of `tiles` tiles (the frame's, in list mode) left behind.
int queue_words_error(pt_scene* s, const int* q, int tiles) {
    if (q[3] != 0) {
        // A waiter saw no progress for the whole bound (bit 0: a stall, recorded; the waiters stayed), or gave up for good after four
        // more (bit 1; bit 2: a push found no slot). The frame is complete iff every tile has been finished (each wave counts its tile
        // in q[2] after its last state store, and the kernel has ended); only an unfinished tile is an error.
        if (q[2] >= tiles) { s->last.queueStalls++; return 0; }
        return fail(-4, "megakernel tile queue timed out (code %d): %d of %d tiles finished, %d pops and %d pushes claimed; the first stalled waiter saw %d finished after %.1f M ticks "
                        "of the device's steady counter without progress: the frame is incomplete", q[3], q[2], tiles, q[0], q[1], q[6], (double)q[7] * 1.048576);
    }
    return 0;
}

// The tile queue's waits are bounded (pt_kernels.hip); a wait that ran out leaves q[3] != 0 and an
// unfinished frame. Read where the host waits for the kernel anyway.
int queue_error(pt_scene* s) {
    if (!s->work.queue.p || s->opt.variant != 0 || !s->last.queued) return 0;     // (an error word left by an earlier queued launch is not this launch's)
    int q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpy(q, s->work.queue.p, sizeof(q), hipMemcpyDeviceToHost) != hipSuccess) return fail(-2, "tile queue read-back failed");
    return queue_words_error(s, q, s->last.tiles);
}
// The same check where the host has work in flight on `stream`: the words travel on it, ahead of the wait.
int wait_and_check(pt_scene* s, hipStream_t stream) {
    int q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool queued = s->work.queue.p && s->opt.variant == 0 && s->last.queued;
    if (queued) HIP_OK(hipMemcpyAsync(q, s->work.queue.p, sizeof(q), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    return queued ? queue_words_error(s, q, s->last.tiles) : 0;
}
}  // namespace pt

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

int pt_has_experimental(void) { return 0; }     // always: the experimental variants were removed; kept for callers that ask

int pt_set_variant(pt_scene* s, int variant) {
    if (!s) return fail(-1, "null scene");
    if (variant != 0 && variant != 1) return fail(-1, "unknown variant %d (0 = megakernel, 1 = wavefront)", variant);
    s->opt.variant = variant;
    return 0;
}

int pt_get_counters(pt_scene* s, pt_counters* out) {
    if (!s || !out) return fail(-1, "null argument");
    HIP_OK(hipMemcpy(out, s->data.totals.p, sizeof(pt_counters), hipMemcpyDeviceToHost));
    return 0;
}
int pt_reset_counters(pt_scene* s) {
    if (!s) return fail(-1, "null scene");
    HIP_OK(hipMemset(s->data.totals.p, 0, 16 * sizeof(unsigned long long)));
    return 0;
}
// Diagnostic builds only: the eight diagnostic sums behind the counters (-DPT_STAMPS: six per-phase s_memtime /
// wall-clock sums; -DPT_UTIL: wave- and lane-level trip counts of the traversal loops); zeros otherwise.
int pt_debug_stamps(pt_scene* s, unsigned long long* out8) {
    if (!s || !out8) return fail(-1, "null argument");
    HIP_OK(hipMemcpy(out8, (unsigned long long*)s->data.totals.p + 8, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

// How often did a tile change hands in the last megakernel launch? The ring starts with every tile of the launch pushed once
// (q[1] = its tiles, in list mode the listed ones); every further push is a wave yielding its tile at the end of a time slice for
// another wave to continue.
int pt_last_tile_handovers(pt_scene* s) {
    if (!s) return fail(-1, "null scene");
    if (!s->work.queue.p || s->opt.variant != 0 || !s->last.queued) return 0;
    int q[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpy(q, s->work.queue.p, sizeof(q), hipMemcpyDeviceToHost));
    return std::max(0, q[1] - s->last.pushed);
}

// The 16 header words of the tile queue after the last queued launch (tests: the words' layout — q[4] / q[5], the issue-priority
// steering's sums, are back at zero when the kernel has ended, q[8..9] hold the wait bound in ticks, q[3] the stall / error bits).
int pt_debug_queue_header(pt_scene* s, int* out16) {
    if (!s || !out16) return fail(-1, "null argument");
    for (int i = 0; i < kQueueHeader; i++) out16[i] = 0;
    if (!s->work.queue.p || s->opt.variant != 0 || !s->last.queued) return 0;
    HIP_OK(hipMemcpy(out16, s->work.queue.p, kQueueHeader * sizeof(int), hipMemcpyDeviceToHost));
    return 1;
}

// Render launches of the last pt_render_moments* call on this scene: 1 when it ran fused, B in batches, 0 for an empty list.
int pt_last_moments_launches(pt_scene* s) { return s ? s->last.momentsLaunches : -1; }

// Launches of this scene whose queue waiters gave up (no progress for "queue_timeout_ms") although the frame was complete.
int pt_queue_stalls(pt_scene* s) { return s ? s->last.queueStalls : 0; }

int pt_set_culling(pt_scene* s, int on) {
    if (!s) return fail(-1, "null scene");
    s->opt.cull = on != 0;
    return 0;
}

// Per-scene kernel-selection and scheduling options (round 1 read these from the environment of the host process; an
// environment variable must not be able to change what a library renders, so they are explicit calls now). Only
// "culling" can reach the image (pt_set_culling); every other option selects between instantiations / schedules that
// are bit-identical by construction and by test.
namespace {
// One row per option: its name and range, and where its value lives — an int member of the scene's Options, or a set / get pair where a
// plain store is not enough. A row with neither is an option of a variant that was removed: the name is still
// known, and `off`, the value that meant "not that variant", is the only one it accepts and the one it reads back.
struct Option {
    const char* name; int lo, hi;
    int Options::*field;
    int (*set)(pt_scene*, int);          // returns an error code
    int (*get)(const pt_scene*);
    int off;
};
int removed(const char* name, int v) {
    return fail(-3, "pt_set_option: %s = %d selected an experimental variant that lost its measurement and was removed (DESIGN.md §6 has the results "
                    "and the commit that last held the code)", name, v);
}
const Option kOptions[] = {
    {"flat", 0, 2, &Options::flatWanted}, {"onchip", 0, 1, &Options::onchipOk},
    {"waves_hbm", 0, 2, nullptr,
     [](pt_scene* s, int v) { s->opt.wavesHbmOk = v != 0; s->opt.wavesHbmForce = s->opt.wavesHbmOk && v == 2; return 0; },
     [](const pt_scene* s) { return s->opt.wavesHbmForce ? 2 : (s->opt.wavesHbmOk ? 1 : 0); }},
    {"refill", 0, 2, nullptr,            // (2 was REFILL for LDS-resident scenes: removed)
     [](pt_scene* s, int v) { if (v == 2) return removed("refill", v); s->opt.refill = v; return 0; },
     [](const pt_scene* s) { return s->opt.refill; }},
    {"refill_keep", 0, 15, nullptr,
     [](pt_scene* s, int v) { s->opt.refillKeep = v; s->opt.refillKeepSet = true; return 0; },
     [](const pt_scene* s) { return s->opt.refillKeep; }},
    {"node_keep", 0, 15, &Options::nodeKeep}, {"tri_keep", 0, 15, &Options::triKeep},
    {"defer_shadow", 0, 1, nullptr, nullptr, nullptr, 0},
    {"slice_iters", 0, 1 << 30, &Options::sliceIters}, {"slice_always", 0, 1, &Options::sliceAlways},
    {"sched_mask", 0, 1 << 20, nullptr,
     [](pt_scene* s, int v) { if (((v + 1) & v) != 0) return fail(-1, "pt_set_option: sched_mask must be 2^k - 1"); s->opt.schedMask = v; return 0; },
     [](const pt_scene* s) { return s->opt.schedMask; }},
    {"lpt_prio", 0, 2, &Options::lptPrio}, {"persistent", 0, 1, &Options::persistent},
    {"xcd_bands", 0, 1, nullptr, nullptr, nullptr, 0},
    {"culling", 0, 1, &Options::cull},
    {"spec", 0, 2, nullptr, nullptr, nullptr, 2},
    {"simple", 0, 1, &Options::simpleWanted}, {"flat2", 0, 1, &Options::flat2Wanted}, {"leaf_boxes", 0, 1, &Options::leafBoxes},
    {"wide", 0, 1, nullptr, nullptr, nullptr, 0}, {"compact", 0, 1, nullptr, nullptr, nullptr, 0},
    {"wf_wide_wg", 0, 2, &Options::wfWideWg}, {"lean", 0, 1, &Options::leanWanted},
    {"queue_timeout_ms", 0, 1 << 22, &Options::queueTimeoutMs}, {"moments_fused", 0, 1, &Options::momentsFused},
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
    s->opt.*(o->field) = v;
    return 0;
}

int pt_get_option(pt_scene* s, const char* name, int* out) {
    const Option* o = find_option(name);
    if (!o) return fail(-1, "pt_get_option: unknown option '%s'", name ? name : "(null)");
    if (!s || !out) return fail(-1, "pt_get_option: null argument");
    *out = o->get ? o->get(s) : (o->field ? s->opt.*(o->field) : o->off);
    return 0;
}

int pt_scene_flags(pt_scene* s) {
    if (!s) return 0;
    const bool onchip = scene_onchip(s->facts, s->opt);
    const bool pers = s->opt.persistent != 0;
    // the kernel the last launch used; before any launch, the one a frame with tiles enough for any kernel would get
    const bool hbm = s->last.hbm >= 0 ? s->last.hbm == 1 : hbm_kernel_pays(s->facts, s->opt, s->dev.numCU, false, 1ll << 40);
    return (onchip ? 1 : 0) | (pers ? 2 : 0) | ((pers && s->opt.sliceIters > 0) ? 4 : 0) | (hbm ? 8 : 0) | ((s->opt.cull && hbm) ? 16 : 0) | (s->last.refill ? 32 : 0) | (s->last.flat ? 64 : 0) | (s->last.simple ? 128 : 0) | (s->last.flat2 ? 256 : 0) | (s->last.leafTable ? 512 : 0) | (s->last.lean ? 1024 : 0);
}

float pt_last_kernel_ms(pt_scene* s) {
    if (!s) return -1.0f;
    if (s->last.evPending) {                                // waits for the last megakernel launch to finish
        if (hipEventSynchronize(s->dev.ev1) != hipSuccess || hipEventElapsedTime(&s->last.kernelMs, s->dev.ev0, s->dev.ev1) != hipSuccess) return -1.0f;
        s->last.evPending = false;
        if (queue_error(s)) return -1.0f;
    }
    return s->last.kernelMs;
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

}  // extern "C"
