// pt_feature_api.hip — the host side of the feature passes behind include/pt_api.h: their checks, launches and entry points, pt_pick.
// (The kernels: pt_aov.hip, pt_motion.hip, pt_motion_chain.hip, pt_ids.hip; their launchers and block counts: pt_feature_host.h.)
#include "pt_host.h"
#include "pt_feature_host.h"

using namespace pt;

// The traversal spill area of a feature pass of `blocks` workgroups: the passes' own (a render in flight on this scene keeps s->work.spill),
// shared among them, since all run on the caller's stream, one after the other. NULL for a scene whose stack never leaves the LDS.
static int feature_spill(pt_scene* s, int blocks, int32_t** spill) {
    *spill = nullptr;
    if (s->facts.ds.stackSpill > 0) {
        if (int r = s->feat.spill.ensure((size_t)blocks * 4 * s->facts.ds.stackSpill * 64 * sizeof(int32_t))) return r;
        *spill = (int32_t*)s->feat.spill.p;
    }
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
    if (hipGetDevice(&dev) != hipSuccess || dev != s->dev.id) return fail(-1, "scene lives on HIP device %d but the current device is %d", s->dev.id, dev);
    return 0;
}

static int render_aovs(pt_scene* s, const pt_camera* cam, int w, int h, int aovSpp, uint64_t seed, void* dA, void* dN, hipStream_t stream) {
    const int blocks = feature_blocks(feature_tiles(w, h).nTiles, s->dev.numCU, kAovWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    HIP_OK(launch_aov(s->facts.ds, cam_to_kernel(*cam), (const uint32_t*)s->data.jump.p, seed, w, h, aovSpp, blocks, (float4*)dA, (float4*)dN, spill, stream));
    return 0;
}

int pt_render_aovs_device(pt_scene* s, const pt_camera* cam, int w, int h, int aov_spp, uint64_t seed, void* d_albedo, void* d_normal_depth,
                          void* stream) {
    if (int r = check_aov_args(s, cam, w, h, aov_spp, d_albedo, d_normal_depth)) return r;
    return render_aovs(s, cam, w, h, aov_spp, seed, d_albedo, d_normal_depth, (hipStream_t)stream);
}

int pt_render_aovs(pt_scene* s, const pt_camera* cam, int w, int h, int aov_spp, uint64_t seed, float* out_albedo, float* out_normal_depth) {
    if (int r = check_aov_args(s, cam, w, h, aov_spp, out_albedo, out_normal_depth)) return r;
    const size_t bytes = (size_t)w * h * sizeof(float4);
    return staged_download(s->feat.aovOut, {{out_albedo, bytes}, {out_normal_depth, bytes}, {nullptr, 0}},
                            [&](void* const* d) { return render_aovs(s, cam, w, h, aov_spp, seed, d[0], d[1], nullptr); });
}

// The chain pass (pt_aov.hip: aov_chain_kernel): max_links, then the checks it shares with the first-hit pass, all before any HIP call.
static int check_aov_chain_args(pt_scene* s, const pt_camera* cam, int w, int h, int aovSpp, int maxLinks, const void* a, const void* nd) {
    if (maxLinks < 0 || maxLinks > 16) return fail(-1, "pt_render_aovs_chain: max_links %d must be 0..16", maxLinks);
    return check_aov_args(s, cam, w, h, aovSpp, a, nd);
}

static int render_aovs_chain(pt_scene* s, const pt_camera* cam, int w, int h, int aovSpp, int maxLinks, uint64_t seed, void* dA, void* dN, void* dL,
                             hipStream_t stream) {
    const int blocks = feature_blocks(feature_tiles(w, h).nTiles, s->dev.numCU, kAovChainWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    HIP_OK(launch_aov_chain(s->facts.ds, cam_to_kernel(*cam), (const uint32_t*)s->data.jump.p, seed, w, h, aovSpp, maxLinks, blocks, (float4*)dA, (float4*)dN,
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
    return staged_download(s->feat.aovOut, {{out_albedo, bytes}, {out_normal_depth, bytes}, {out_links, lbytes}},
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
    const int blocks = feature_blocks(feature_tiles(w, h).nTiles, s->dev.numCU, chain ? kAovChainWavesPerSimd : kAovCentreWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    if (chain) HIP_OK(launch_aov_centre_chain(s->facts.ds, cam_to_kernel(*cam), w, h, maxLinks, blocks, (float4*)dA, (float4*)dN, (float*)dL, spill, stream));
    else HIP_OK(launch_aov_centre(s->facts.ds, cam_to_kernel(*cam), w, h, blocks, (float4*)dA, (float4*)dN, spill, stream));
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
    return staged_download(s->feat.aovOut, {{out_albedo, bytes}, {out_normal_depth, bytes}, {out_links, lbytes}},
                            [&](void* const* d) { return render_aovs_centre(s, cam, w, h, max_links, d[0], d[1], d[2], nullptr); });
}

// The motion pass (pt_motion.hip: motion_kernel): the centre pass's checks, the guide outputs both or neither, and the motion output.
static int check_motion_args(pt_scene* s, const pt_camera* cam, int w, int h, const void* a, const void* nd, const void* mv) {
    if ((a != nullptr) != (nd != nullptr)) return fail(-1, "pt_render_motion: albedo and normal_depth must be both NULL or both set");
    if (!mv) return fail(-1, "pt_render_motion: null motion output");
    return check_aov_centre_args(s, cam, w, h, 0, mv, mv);
}

static int render_motion(pt_scene* s, const pt_camera* cam, int w, int h, void* dA, void* dN, void* dM, hipStream_t stream) {
    const int blocks = feature_blocks(feature_tiles(w, h).nTiles, s->dev.numCU, kMotionWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    const bool moving = s->upd.hasMotion && s->kept.deviceLeaf >= 0;
    HIP_OK(launch_motion(s->facts.ds, s->data.kTris.p, s->data.posCur.p, moving ? s->data.posPrev.p : nullptr, s->kept.nPositions, cam_to_kernel(*cam), w, h, blocks, (float4*)dA,
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
    return staged_download(s->feat.motionOut, {{out_albedo, bytes}, {out_normal_depth, bytes}, {out_motion, bytes}},
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
    if (hipGetDevice(&dev) != hipSuccess || dev != s->dev.id)
        return fail(-1, "pt_render_motion_chain: scene lives on HIP device %d but the current device is %d", s->dev.id, dev);
    return 0;
}

static int render_motion_chain(pt_scene* s, const pt_camera* cam, int w, int h, int maxLinks, void* dA, void* dN, void* dL, void* dM,
                               hipStream_t stream) {
    const int blocks = feature_blocks(feature_tiles(w, h).nTiles, s->dev.numCU, kMotionChainWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    const bool moving = s->upd.hasMotion && s->kept.deviceLeaf >= 0;
    HIP_OK(launch_motion_chain(s->facts.ds, s->data.kTris.p, s->data.posCur.p, moving ? s->data.posPrev.p : nullptr, s->kept.nPositions, cam_to_kernel(*cam), w, h, maxLinks,
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
    return staged_download(s->feat.motionOut, {{out_albedo, bytes}, {out_normal_depth, bytes}, {out_motion, bytes}, {out_links, lbytes}},
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
    if (hipGetDevice(&dev) != hipSuccess || dev != s->dev.id) return fail(-1, "%s: scene lives on HIP device %d but the current device is %d", fn, s->dev.id, dev);
    return 0;
}

// xy NULL: the image. xy set: nPick pixels (device memory), and dHit their (point, depth) records.
static int render_ids(pt_scene* s, const pt_camera* cam, int w, int h, int maxLinks, const int32_t* xy, int nPick, void* dIds, void* dHit,
                      hipStream_t stream) {
    const int nTiles = xy ? (nPick + 63) / 64 : feature_tiles(w, h).nTiles;
    const int blocks = feature_blocks(nTiles, s->dev.numCU, maxLinks > 0 ? kIdsChainWavesPerSimd : kIdsWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    HIP_OK(launch_ids(s->facts.ds, cam_to_kernel(*cam), w, h, maxLinks, xy, nPick, blocks, (int4*)dIds, (float4*)dHit, spill, stream));
    return 0;
}

int pt_render_ids_device(pt_scene* s, const pt_camera* cam, int w, int h, int max_links, void* d_ids, void* stream) {
    if (int r = check_ids_args("pt_render_ids", s, cam, w, h, max_links, d_ids)) return r;
    return render_ids(s, cam, w, h, max_links, nullptr, 0, d_ids, nullptr, (hipStream_t)stream);
}

int pt_render_ids(pt_scene* s, const pt_camera* cam, int w, int h, int max_links, int32_t* out_ids) {
    if (int r = check_ids_args("pt_render_ids", s, cam, w, h, max_links, out_ids)) return r;
    return staged_download(s->feat.idsOut, {{out_ids, (size_t)w * h * sizeof(int4)}},
                            [&](void* const* d) { return render_ids(s, cam, w, h, max_links, nullptr, 0, d[0], nullptr, nullptr); });
}

int pt_pick(pt_scene* s, const pt_camera* cam, int w, int h, int n, const int32_t* xy, int max_links, int32_t* out_ids, float* out_hit) {
    if (n <= 0) return fail(-1, "pt_pick: n %d must be positive", n);
    if (!xy) return fail(-1, "pt_pick: null pixel list");
    if (!out_hit) return fail(-1, "pt_pick: null hit output");
    if (int r = check_ids_args("pt_pick", s, cam, w, h, max_links, out_ids, xy, n)) return r;
    // staging: the list, then the two outputs, each slice a multiple of 16 bytes
    const size_t xyBytes = ((size_t)n * 8 + 15) & ~(size_t)15, recBytes = (size_t)n * 16;
    if (int r = s->feat.idsOut.ensure(xyBytes + 2 * recBytes)) return r;
    char* d = (char*)s->feat.idsOut.p;
    HIP_OK(hipMemcpy(d, xy, (size_t)n * 8, hipMemcpyHostToDevice));
    if (int r = render_ids(s, cam, w, h, max_links, (const int32_t*)d, n, d + xyBytes, d + xyBytes + recBytes, nullptr)) return r;
    HIP_OK(hipMemcpy(out_ids, d + xyBytes, recBytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out_hit, d + xyBytes + recBytes, recBytes, hipMemcpyDeviceToHost));
    return 0;
}
