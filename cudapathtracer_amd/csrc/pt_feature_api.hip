// pt_feature_api.hip — the host side of the feature passes behind include/pt_api.h: their checks, launches and entry points, pt_pick,
// and the ray queries. (The kernels: pt_aov.hip, pt_motion.hip, pt_motion_chain.hip, pt_ids.hip, pt_query.hip, pt_query_guides.hip,
// pt_radiance.hip, pt_radiance_moments.hip, pt_irradiance.hip, pt_sh.hip, pt_distance.hip; their launchers and block counts: pt_feature_host.h; the host forms' staging: pt_host.h.)
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

// Ray queries (pt_query.hip: query_closest_kernel, query_shadow_kernel, query_camera_rays_kernel, query_keys_kernel). Every message
// under the caller's name, all before any HIP call; n == 0 returns before the scene is looked at (the device check comes last).
static int check_query_args(const char* fn, pt_scene* s, int n, const void* rays, const void* out, uint32_t flags) {
    if (!s) return fail(-1, "%s: null scene", fn);
    if (!rays) return fail(-1, "%s: null rays", fn);
    if (!out) return fail(-1, "%s: null output buffer", fn);
    if (n < 0 || n > (1 << 28)) return fail(-1, "%s: n %d must be 0..%d", fn, n, 1 << 28);
    if (flags & ~PT_QUERY_REORDER) return fail(-1, "%s: unknown flag bits 0x%x", fn, flags & ~PT_QUERY_REORDER);
    return 0;
}

static int check_query_device(const char* fn, pt_scene* s) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != s->dev.id) return fail(-1, "%s: scene lives on HIP device %d but the current device is %d", fn, s->dev.id, dev);
    return 0;
}

// PT_QUERY_REORDER: *perm = the rays' order by key (the sorted indices), or NULL where the call takes the unordered path: without
// the flag, for at most one tile of rays, and for a scene whose root is a leaf (it has no record to read the bounds from).
static int query_order(pt_scene* s, int n, const void* dRays, uint32_t flags, const uint32_t** perm, hipStream_t stream) {
    *perm = nullptr;
    if (!(flags & PT_QUERY_REORDER) || n <= 64 || s->facts.ds.rootRef < 0) return 0;
    const size_t half = ((size_t)n * sizeof(uint32_t) + 255) & ~(size_t)255;
    if (int r = s->feat.queryKeys.ensure(2 * half)) return r;
    if (int r = s->feat.queryIdx.ensure(2 * half)) return r;
    uint32_t* keys = (uint32_t*)s->feat.queryKeys.p;
    uint32_t* idx = (uint32_t*)s->feat.queryIdx.p;
    uint32_t* keysOut = (uint32_t*)((char*)keys + half);
    uint32_t* idxOut = (uint32_t*)((char*)idx + half);
    size_t tempBytes = 0;
    HIP_OK(query_sort(nullptr, &tempBytes, keys, keysOut, idx, idxOut, n, stream));
    if (int r = s->feat.querySort.ensure(std::max<size_t>(tempBytes, 256))) return r;
    HIP_OK(launch_query_keys(s->facts.ds, n, dRays, keys, idx, stream));
    HIP_OK(query_sort(s->feat.querySort.p, &tempBytes, keys, keysOut, idx, idxOut, n, stream));
    *perm = idxOut;
    return 0;
}

static int query_closest(pt_scene* s, int n, const void* dRays, void* dHits, void* dSurf, uint32_t flags, hipStream_t stream) {
    const int blocks = feature_blocks((n + 63) / 64, s->dev.numCU, dSurf ? kQuerySurfaceWavesPerSimd : kQueryClosestWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    const uint32_t* perm;
    if (int r = query_order(s, n, dRays, flags, &perm, stream)) return r;
    HIP_OK(launch_query_closest(s->facts.ds, n, dRays, perm, blocks, dHits, dSurf, spill, stream));
    return 0;
}

static int query_shadow(pt_scene* s, int n, const void* dRays, void* dThr, uint32_t flags, hipStream_t stream) {
    const int blocks = feature_blocks((n + 63) / 64, s->dev.numCU, kQueryShadowWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    const uint32_t* perm;
    if (int r = query_order(s, n, dRays, flags, &perm, stream)) return r;
    HIP_OK(launch_query_shadow(s->facts.ds, n, dRays, perm, blocks, dThr, spill, stream));
    return 0;
}

int pt_query_closest_device(pt_scene* s, int n, const void* d_rays, void* d_hits, void* d_surfaces, uint32_t flags, void* stream) {
    if (int r = check_query_args("pt_query_closest", s, n, d_rays, d_hits, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device("pt_query_closest", s)) return r;
    return query_closest(s, n, d_rays, d_hits, d_surfaces, flags, (hipStream_t)stream);
}

int pt_query_shadow_device(pt_scene* s, int n, const void* d_rays, void* d_throughput, uint32_t flags, void* stream) {
    if (int r = check_query_args("pt_query_shadow", s, n, d_rays, d_throughput, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device("pt_query_shadow", s)) return r;
    return query_shadow(s, n, d_rays, d_throughput, flags, (hipStream_t)stream);
}

// The host forms (here and below): pt_host.h's staged_query on the scene's queryOut, the rays at its head, the outputs behind them.
int pt_query_closest(pt_scene* s, int n, const pt_ray* rays, pt_ray_hit* hits, pt_ray_surface* surfaces, uint32_t flags) {
    if (int r = check_query_args("pt_query_closest", s, n, rays, hits, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device("pt_query_closest", s)) return r;
    return staged_query(s->feat.queryOut, n, rays, {{hits, (size_t)n * sizeof(pt_ray_hit)}, {surfaces, (size_t)n * sizeof(pt_ray_surface)}},
                        [&](const void* dRays, void* const* d) { return query_closest(s, n, dRays, d[0], d[1], flags, nullptr); });
}

int pt_query_shadow(pt_scene* s, int n, const pt_ray* rays, float* throughput4, uint32_t flags) {
    if (int r = check_query_args("pt_query_shadow", s, n, rays, throughput4, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device("pt_query_shadow", s)) return r;
    return staged_query(s->feat.queryOut, n, rays, {{throughput4, (size_t)n * sizeof(float4)}},
                        [&](const void* dRays, void* const* d) { return query_shadow(s, n, dRays, d[0], flags, nullptr); });
}

// Radiance queries (pt_radiance.hip: radiance_kernel; pt_radiance_moments.hip: radiance_moments_kernel). Every message under the
// caller's name, all before any HIP call; n == 0 returns before the scene or anything else is looked at.
static int check_radiance_args(const char* fn, pt_scene* s, int n, const void* rays, const void* out, int spp, int integrator, uint32_t firstStream,
                               uint32_t flags) {
    if (n < 0 || n > (1 << 28)) return fail(-1, "%s: n %d must be 0..%d", fn, n, 1 << 28);
    if (n == 0) return 0;
    if (!s) return fail(-1, "%s: null scene", fn);
    if (!rays) return fail(-1, "%s: null rays", fn);
    if (!out) return fail(-1, "%s: null output buffer", fn);
    if (spp < 1 || spp > (1 << 22)) return fail(-1, "%s: spp %d must be 1..%d", fn, spp, 1 << 22);
    if (integrator != PT_UNIDIRECTIONAL && integrator != PT_NAIVE_UNIDIRECTIONAL)
        return fail(-1, "%s: integrator %d is out of scope: only UNIDIRECTIONAL (0) and NAIVE_UNIDIRECTIONAL (2) are on this path", fn, integrator);
    if (flags & PT_QUERY_REORDER) return fail(-1, "%s: PT_QUERY_REORDER is not taken here: a path leaves its first ray's order at once", fn);
    if (flags & ~PT_QUERY_STREAM_PAD) return fail(-1, "%s: unknown flag bits 0x%x", fn, flags & ~PT_QUERY_STREAM_PAD);
    if (!(flags & PT_QUERY_STREAM_PAD) && (unsigned long long)firstStream + (unsigned long long)n > (1ull << 31))
        return fail(-1, "%s: streams %u .. %llu pass 2^31", fn, firstStream, (unsigned long long)firstStream + (unsigned long long)n - 1ull);
    return 0;
}

// The scene's material class picks the instantiation as the render launch picks its bounce (pt_plan.hip: launch_plan): SIMPLE for a
// scene that qualifies unless the "simple" option is 0, else LEAN likewise. No other option is read. batchSpp 0 and dSq NULL:
// radiance_kernel; else radiance_moments_kernel of the same class, at its own waves per SIMD.
static int query_radiance(pt_scene* s, int n, const void* dRays, int spp, int batchSpp, int maxDepth, int integrator, int useMIS, uint64_t seed,
                          uint32_t firstStream, void* dOut, void* dSq, uint32_t flags, hipStream_t stream) {
    const bool simple = s->facts.simpleOk && s->opt.simpleWanted;
    const bool lean = s->facts.leanOk && s->opt.leanWanted && !s->facts.armless && !simple;
    const bool moments = batchSpp != 0 || dSq;
    const int waves = moments ? radiance_moments_waves_per_simd(integrator, simple, lean) : radiance_waves_per_simd(integrator, simple, lean);
    const int blocks = feature_blocks((n + 63) / 64, s->dev.numCU, waves);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    const uint32_t* jump = (const uint32_t*)s->data.jump.p;
    const bool pad = (flags & PT_QUERY_STREAM_PAD) != 0;
    if (moments)
        HIP_OK(launch_radiance_moments(s->facts.ds, integrator, simple, lean, n, dRays, jump, seed, firstStream, pad, spp, batchSpp, maxDepth, useMIS,
                                       blocks, dOut, dSq, spill, stream));
    else
        HIP_OK(launch_radiance(s->facts.ds, integrator, simple, lean, n, dRays, jump, seed, firstStream, pad, spp, maxDepth, useMIS, blocks, dOut, spill,
                               stream));
    return 0;
}

int pt_query_radiance_device(pt_scene* s, int n, const void* d_rays, int spp, int max_depth, int integrator, int use_mis, uint64_t seed,
                             uint32_t first_stream, void* d_rgba_sum, unsigned flags, void* stream) {
    if (int r = check_radiance_args("pt_query_radiance", s, n, d_rays, d_rgba_sum, spp, integrator, first_stream, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device("pt_query_radiance", s)) return r;
    return query_radiance(s, n, d_rays, spp, 0, max_depth, integrator, use_mis, seed, first_stream, d_rgba_sum, nullptr, flags, (hipStream_t)stream);
}

int pt_query_radiance(pt_scene* s, int n, const pt_ray* rays, int spp, int max_depth, int integrator, int use_mis, uint64_t seed,
                      uint32_t first_stream, float* out_rgba_sum, unsigned flags) {
    if (int r = check_radiance_args("pt_query_radiance", s, n, rays, out_rgba_sum, spp, integrator, first_stream, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device("pt_query_radiance", s)) return r;
    return staged_query(s->feat.queryOut, n, rays, {{out_rgba_sum, (size_t)n * sizeof(float4)}}, [&](const void* dRays, void* const* d) {
        return query_radiance(s, n, dRays, spp, 0, max_depth, integrator, use_mis, seed, first_stream, d[0], nullptr, flags, nullptr);
    });
}

// pt_query_radiance_moments: pt_query_radiance's checks in its order, then the batches' and the second output. (n == 0: the callers return.)
static int check_radiance_moments_args(pt_scene* s, int n, const void* rays, const void* out, const void* sq, int spp, int batchSpp, int integrator,
                                       uint32_t firstStream, uint32_t flags) {
    const char* fn = "pt_query_radiance_moments";
    if (int r = check_radiance_args(fn, s, n, rays, out, spp, integrator, firstStream, flags)) return r;
    if (n == 0) return 0;
    if (batchSpp < 1) return fail(-1, "%s: batch_spp %d must be positive", fn, batchSpp);
    if (spp % batchSpp != 0) return fail(-1, "%s: spp %d is not a multiple of batch_spp %d", fn, spp, batchSpp);
    if (spp / batchSpp < 2) return fail(-1, "%s: %d batch(es): a variance needs at least 2", fn, spp / batchSpp);
    if (!sq) return fail(-1, "%s: null sq_sum buffer", fn);
    return 0;
}

int pt_query_radiance_moments_device(pt_scene* s, int n, const void* d_rays, int spp, int batch_spp, int max_depth, int integrator, int use_mis,
                                     uint64_t seed, uint32_t first_stream, void* d_rgba_sum, void* d_sq_sum, unsigned flags, void* stream) {
    if (int r = check_radiance_moments_args(s, n, d_rays, d_rgba_sum, d_sq_sum, spp, batch_spp, integrator, first_stream, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device("pt_query_radiance_moments", s)) return r;
    return query_radiance(s, n, d_rays, spp, batch_spp, max_depth, integrator, use_mis, seed, first_stream, d_rgba_sum, d_sq_sum, flags,
                          (hipStream_t)stream);
}

int pt_query_radiance_moments(pt_scene* s, int n, const pt_ray* rays, int spp, int batch_spp, int max_depth, int integrator, int use_mis, uint64_t seed,
                              uint32_t first_stream, float* out_rgba_sum, float* out_sq_sum, unsigned flags) {
    if (int r = check_radiance_moments_args(s, n, rays, out_rgba_sum, out_sq_sum, spp, batch_spp, integrator, first_stream, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device("pt_query_radiance_moments", s)) return r;
    const size_t bytes = (size_t)n * sizeof(float4);
    return staged_query(s->feat.queryOut, n, rays, {{out_rgba_sum, bytes}, {out_sq_sum, bytes}}, [&](const void* dRays, void* const* d) {
        return query_radiance(s, n, dRays, spp, batch_spp, max_depth, integrator, use_mis, seed, first_stream, d[0], d[1], flags, nullptr);
    });
}

// Irradiance queries (pt_irradiance.hip: irradiance_kernel, irradiance_rays_kernel). Every message under the caller's name, all before
// any HIP call, in the header's order; n == 0 returns before the scene or anything else is looked at. walk: pt_query_irradiance's
// checks; else pt_query_irradiance_rays_device's, which has no samples, integrator or sums (`out` is its rays buffer).
static int check_irradiance_args(const char* fn, bool walk, pt_scene* s, int n, const void* recs, const void* out, const void* sq, int lanes,
                                 int sppLane, int integrator, uint32_t firstStream, uint32_t flags) {
    if (n < 0 || (long long)n * lanes > (1ll << 28)) return fail(-1, "%s: n %d at %d lanes must be 0..%d lanes in all", fn, n, lanes, 1 << 28);
    if (n == 0) return 0;
    if (!s) return fail(-1, "%s: null scene", fn);
    if (!recs) return fail(-1, "%s: null records", fn);
    if (!out) return fail(-1, "%s: null output buffer", fn);
    if (lanes < 1 || lanes > 64 || (lanes & (lanes - 1))) return fail(-1, "%s: lanes %d must be a power of two in 1..64", fn, lanes);
    if (walk) {
        if (sppLane < 1 || (long long)lanes * sppLane > (1ll << 22))
            return fail(-1, "%s: spp_lane %d at %d lanes must be 1..%d samples a record", fn, sppLane, lanes, 1 << 22);
        if (integrator != PT_UNIDIRECTIONAL && integrator != PT_NAIVE_UNIDIRECTIONAL)
            return fail(-1, "%s: integrator %d is out of scope: only UNIDIRECTIONAL (0) and NAIVE_UNIDIRECTIONAL (2) are on this path", fn, integrator);
        if (sq && lanes == 1) return fail(-1, "%s: sq_sum needs lanes >= 2: a lane's sum is one batch", fn);
    }
    if (flags & PT_QUERY_REORDER) return fail(-1, "%s: PT_QUERY_REORDER is not taken here: a path leaves its first ray's order at once", fn);
    if (flags & ~PT_QUERY_STREAM_PAD) return fail(-1, "%s: unknown flag bits 0x%x", fn, flags & ~PT_QUERY_STREAM_PAD);
    const unsigned long long end = (unsigned long long)firstStream + (unsigned long long)n * (unsigned)lanes;
    if (!(flags & PT_QUERY_STREAM_PAD) && end > (1ull << 31)) return fail(-1, "%s: streams %u .. %llu pass 2^31", fn, firstStream, end - 1ull);
    return 0;
}

static int log2_lanes(int lanes) { return __builtin_ctz((unsigned)lanes); }

// The material class picks the instantiation as query_radiance picks it, from the same two options.
static int query_irradiance(pt_scene* s, int n, const void* dRecs, int lanes, int sppLane, int maxDepth, int integrator, int useMIS, uint64_t seed,
                            uint32_t firstStream, void* dOut, void* dSq, uint32_t flags, hipStream_t stream) {
    const bool simple = s->facts.simpleOk && s->opt.simpleWanted;
    const bool lean = s->facts.leanOk && s->opt.leanWanted && !s->facts.armless && !simple;
    const int log2L = log2_lanes(lanes);
    const int blocks = feature_blocks(irradiance_tiles(n, log2L), s->dev.numCU, irradiance_waves_per_simd(integrator, simple, lean));
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    HIP_OK(launch_irradiance(s->facts.ds, integrator, simple, lean, n, dRecs, log2L, (const uint32_t*)s->data.jump.p, seed, firstStream,
                             (flags & PT_QUERY_STREAM_PAD) != 0, sppLane, maxDepth, useMIS, blocks, dOut, dSq, spill, stream));
    return 0;
}

int pt_query_irradiance_device(pt_scene* s, int n, const void* d_records, int lanes, int spp_lane, int max_depth, int integrator, int use_mis,
                               uint64_t seed, uint32_t first_stream, void* d_rgba_sum, void* d_sq_sum, unsigned flags, void* stream) {
    const char* fn = "pt_query_irradiance";
    if (int r = check_irradiance_args(fn, true, s, n, d_records, d_rgba_sum, d_sq_sum, lanes, spp_lane, integrator, first_stream, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device(fn, s)) return r;
    return query_irradiance(s, n, d_records, lanes, spp_lane, max_depth, integrator, use_mis, seed, first_stream, d_rgba_sum, d_sq_sum, flags,
                            (hipStream_t)stream);
}

int pt_query_irradiance(pt_scene* s, int n, const pt_ray* records, int lanes, int spp_lane, int max_depth, int integrator, int use_mis, uint64_t seed,
                        uint32_t first_stream, float* out_rgba_sum, float* out_sq_sum, unsigned flags) {
    const char* fn = "pt_query_irradiance";
    if (int r = check_irradiance_args(fn, true, s, n, records, out_rgba_sum, out_sq_sum, lanes, spp_lane, integrator, first_stream, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device(fn, s)) return r;
    const size_t bytes = (size_t)n * sizeof(float4);
    return staged_query(s->feat.queryOut, n, records, {{out_rgba_sum, bytes}, {out_sq_sum, bytes}}, [&](const void* dRecs, void* const* d) {
        return query_irradiance(s, n, dRecs, lanes, spp_lane, max_depth, integrator, use_mis, seed, first_stream, d[0], d[1], flags, nullptr);
    });
}

int pt_query_irradiance_rays_device(pt_scene* s, int n, const void* d_records, int lanes, uint64_t seed, uint32_t first_stream,
                                    const void* d_draw_offset, void* d_rays, unsigned flags, void* stream) {
    const char* fn = "pt_query_irradiance_rays_device";
    if (int r = check_irradiance_args(fn, false, s, n, d_records, d_rays, nullptr, lanes, 1, PT_UNIDIRECTIONAL, first_stream, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device(fn, s)) return r;
    HIP_OK(launch_irradiance_rays(n, d_records, log2_lanes(lanes), (const uint32_t*)s->data.jump.p, seed, first_stream,
                                  (flags & PT_QUERY_STREAM_PAD) != 0, d_draw_offset, d_rays, (hipStream_t)stream));
    return 0;
}

// SH queries (pt_sh.hip: sh_kernel, sh_reduce_kernel, sh_rays_kernel). Every message under the caller's name, all before any HIP
// call, in the header's order; n == 0 returns before the scene or anything else is looked at. walk: pt_query_sh's checks; else
// pt_query_sh_rays_device's, which has no samples, integrator or workspace (`out` is its rays buffer). needWork: the device form,
// whose caller brings the workspace.
static int check_sh_args(const char* fn, bool walk, pt_scene* s, int n, const void* recs, const void* out, int lanes, int sppLane, int integrator,
                         uint32_t firstStream, uint32_t flags, bool needWork, const void* work) {
    if (n < 0 || (long long)n * lanes > (1ll << 28)) return fail(-1, "%s: n %d at %d lanes must be 0..%d lanes in all", fn, n, lanes, 1 << 28);
    if (n == 0) return 0;
    if (!s) return fail(-1, "%s: null scene", fn);
    if (!recs) return fail(-1, "%s: null records", fn);
    if (!out) return fail(-1, "%s: null output buffer", fn);
    if (lanes < 1 || lanes > 4096 || (lanes & (lanes - 1))) return fail(-1, "%s: lanes %d must be a power of two in 1..4096", fn, lanes);
    if (walk) {
        if (sppLane < 1 || (long long)lanes * sppLane > (1ll << 22))
            return fail(-1, "%s: spp_lane %d at %d lanes must be 1..%d samples a record", fn, sppLane, lanes, 1 << 22);
        if (integrator != PT_UNIDIRECTIONAL && integrator != PT_NAIVE_UNIDIRECTIONAL)
            return fail(-1, "%s: integrator %d is out of scope: only UNIDIRECTIONAL (0) and NAIVE_UNIDIRECTIONAL (2) are on this path", fn, integrator);
    }
    if (flags & PT_QUERY_REORDER) return fail(-1, "%s: PT_QUERY_REORDER is not taken here: a path leaves its first ray's order at once", fn);
    if (flags & ~PT_QUERY_STREAM_PAD) return fail(-1, "%s: unknown flag bits 0x%x", fn, flags & ~PT_QUERY_STREAM_PAD);
    const unsigned long long end = (unsigned long long)firstStream + (unsigned long long)n * (unsigned)lanes;
    if (!(flags & PT_QUERY_STREAM_PAD) && end > (1ull << 31)) return fail(-1, "%s: streams %u .. %llu pass 2^31", fn, firstStream, end - 1ull);
    if (needWork && lanes > 64 && !work) return fail(-1, "%s: lanes %d needs a workspace of pt_query_sh_workspace_bytes", fn, lanes);
    return 0;
}

size_t pt_query_sh_workspace_bytes(int n, int lanes) { return n > 0 && lanes > 64 ? (size_t)n * (size_t)(lanes / 64) * 9 * sizeof(float4) : 0; }

// The material class picks the instantiation as query_radiance picks it, from the same two options. More than 64 lanes: the walk
// leaves a tile's sums in dWork and the second stage of the tree follows on the same stream.
static int query_sh(pt_scene* s, int n, const void* dRecs, int lanes, int sppLane, int maxDepth, int integrator, int useMIS, uint64_t seed,
                    uint32_t firstStream, void* dOut, void* dWork, uint32_t flags, hipStream_t stream) {
    const bool simple = s->facts.simpleOk && s->opt.simpleWanted;
    const bool lean = s->facts.leanOk && s->opt.leanWanted && !s->facts.armless && !simple;
    const int log2L = log2_lanes(lanes);
    const int blocks = feature_blocks(irradiance_tiles(n, log2L), s->dev.numCU, sh_waves_per_simd(integrator, simple, lean));
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    HIP_OK(launch_sh(s->facts.ds, integrator, simple, lean, n, dRecs, log2L, (const uint32_t*)s->data.jump.p, seed, firstStream,
                     (flags & PT_QUERY_STREAM_PAD) != 0, sppLane, maxDepth, useMIS, blocks, dOut, dWork, spill, stream));
    if (lanes > 64) HIP_OK(launch_sh_reduce(n, log2L, dWork, dOut, stream));
    return 0;
}

int pt_query_sh_device(pt_scene* s, int n, const void* d_records, int lanes, int spp_lane, int max_depth, int integrator, int use_mis, uint64_t seed,
                       uint32_t first_stream, void* d_coeffs, void* d_workspace, unsigned flags, void* stream) {
    const char* fn = "pt_query_sh";
    if (int r = check_sh_args(fn, true, s, n, d_records, d_coeffs, lanes, spp_lane, integrator, first_stream, flags, true, d_workspace)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device(fn, s)) return r;
    return query_sh(s, n, d_records, lanes, spp_lane, max_depth, integrator, use_mis, seed, first_stream, d_coeffs, d_workspace, flags,
                    (hipStream_t)stream);
}

// The host form's workspace lies in the staging buffer behind the coefficients: the buffer is grown for all three before
// staged_query lays out the first two.
int pt_query_sh(pt_scene* s, int n, const pt_ray* records, int lanes, int spp_lane, int max_depth, int integrator, int use_mis, uint64_t seed,
                uint32_t first_stream, float* out_coeffs, unsigned flags) {
    const char* fn = "pt_query_sh";
    if (int r = check_sh_args(fn, true, s, n, records, out_coeffs, lanes, spp_lane, integrator, first_stream, flags, false, nullptr)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device(fn, s)) return r;
    const size_t bytes = (size_t)n * 9 * sizeof(float4);
    if (int r = s->feat.queryOut.ensure((size_t)n * sizeof(pt_ray) + bytes + pt_query_sh_workspace_bytes(n, lanes))) return r;
    return staged_query(s->feat.queryOut, n, records, {{out_coeffs, bytes}}, [&](const void* dRecs, void* const* d) {
        return query_sh(s, n, dRecs, lanes, spp_lane, max_depth, integrator, use_mis, seed, first_stream, d[0], (char*)d[0] + bytes, flags, nullptr);
    });
}

int pt_query_sh_rays_device(pt_scene* s, int n, const void* d_records, int lanes, uint64_t seed, uint32_t first_stream, const void* d_draw_offset,
                            void* d_rays, unsigned flags, void* stream) {
    const char* fn = "pt_query_sh_rays_device";
    if (int r = check_sh_args(fn, false, s, n, d_records, d_rays, lanes, 1, PT_UNIDIRECTIONAL, first_stream, flags, false, nullptr)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device(fn, s)) return r;
    HIP_OK(launch_sh_rays(n, d_records, log2_lanes(lanes), (const uint32_t*)s->data.jump.p, seed, first_stream, (flags & PT_QUERY_STREAM_PAD) != 0,
                          d_draw_offset, d_rays, (hipStream_t)stream));
    return 0;
}

// Distance probes (pt_distance.hip: distance_kernel, distance_rays_kernel). Every message under the caller's name, all before any HIP
// call, in the header's order, which is pt_query_sh's; n == 0 returns before the scene or anything else is looked at. walk:
// pt_query_distance's checks; else pt_query_distance_rays_device's, which has no samples (`out` is its rays buffer).
static int check_distance_args(const char* fn, bool walk, pt_scene* s, int n, const void* recs, const void* out, int res, int sppLane,
                               uint32_t firstStream, uint32_t flags) {
    const long long lanes = (long long)res * res;
    if (n < 0 || (n > 0 && lanes > (1ll << 28)) || (long long)n * lanes > (1ll << 28)) return fail(-1, "%s: n %d at res %d must be 0..%d lanes in all", fn, n, res, 1 << 28);
    if (n == 0) return 0;
    if (!s) return fail(-1, "%s: null scene", fn);
    if (!recs) return fail(-1, "%s: null records", fn);
    if (!out) return fail(-1, "%s: null output buffer", fn);
    if (res != 4 && res != 8 && res != 16 && res != 32) return fail(-1, "%s: res %d must be 4, 8, 16 or 32", fn, res);
    if (walk && (sppLane < 1 || lanes * sppLane > (1ll << 22)))
        return fail(-1, "%s: spp_lane %d at res %d must be 1..%d samples a record", fn, sppLane, res, 1 << 22);
    if (flags & PT_QUERY_REORDER) return fail(-1, "%s: PT_QUERY_REORDER is not taken here: the library makes the rays itself", fn);
    const uint32_t known = PT_QUERY_STREAM_PAD | PT_QUERY_TEXEL_CENTRE;
    if (flags & ~known) return fail(-1, "%s: unknown flag bits 0x%x", fn, flags & ~known);
    const bool centre = (flags & PT_QUERY_TEXEL_CENTRE) != 0;
    if (walk && centre && sppLane != 1) return fail(-1, "%s: PT_QUERY_TEXEL_CENTRE has one sample a texel: spp_lane %d must be 1", fn, sppLane);
    const unsigned long long end = (unsigned long long)firstStream + (unsigned long long)n * (unsigned long long)lanes;
    if (!centre && !(flags & PT_QUERY_STREAM_PAD) && end > (1ull << 31)) return fail(-1, "%s: streams %u .. %llu pass 2^31", fn, firstStream, end - 1ull);
    return 0;
}

static int query_distance(pt_scene* s, int n, const void* dRecs, int res, int sppLane, uint64_t seed, uint32_t firstStream, void* dMaps, uint32_t flags,
                          hipStream_t stream) {
    const bool centre = (flags & PT_QUERY_TEXEL_CENTRE) != 0;
    const int log2R = log2_lanes(res);
    const int blocks = feature_blocks(irradiance_tiles(n, 2 * log2R), s->dev.numCU, centre ? kDistanceCentreWavesPerSimd : kDistanceWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    HIP_OK(launch_distance(s->facts.ds, n, dRecs, log2R, (const uint32_t*)s->data.jump.p, seed, firstStream, (flags & PT_QUERY_STREAM_PAD) != 0, centre,
                           sppLane, blocks, dMaps, spill, stream));
    return 0;
}

int pt_query_distance_device(pt_scene* s, int n, const void* d_records, int res, int spp_lane, uint64_t seed, uint32_t first_stream, void* d_maps,
                             uint32_t flags, void* stream) {
    const char* fn = "pt_query_distance";
    if (int r = check_distance_args(fn, true, s, n, d_records, d_maps, res, spp_lane, first_stream, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device(fn, s)) return r;
    return query_distance(s, n, d_records, res, spp_lane, seed, first_stream, d_maps, flags, (hipStream_t)stream);
}

int pt_query_distance(pt_scene* s, int n, const pt_ray* records, int res, int spp_lane, uint64_t seed, uint32_t first_stream, float* maps4,
                      uint32_t flags) {
    const char* fn = "pt_query_distance";
    if (int r = check_distance_args(fn, true, s, n, records, maps4, res, spp_lane, first_stream, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device(fn, s)) return r;
    return staged_query(s->feat.queryOut, n, records, {{maps4, (size_t)n * res * res * sizeof(float4)}}, [&](const void* dRecs, void* const* d) {
        return query_distance(s, n, dRecs, res, spp_lane, seed, first_stream, d[0], flags, nullptr);
    });
}

int pt_query_distance_rays_device(pt_scene* s, int n, const void* d_records, int res, uint64_t seed, uint32_t first_stream, const void* d_skip,
                                  void* d_rays, uint32_t flags, void* stream) {
    const char* fn = "pt_query_distance_rays_device";
    if (int r = check_distance_args(fn, false, s, n, d_records, d_rays, res, 1, first_stream, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device(fn, s)) return r;
    HIP_OK(launch_distance_rays(n, d_records, log2_lanes(res), (const uint32_t*)s->data.jump.p, seed, first_stream, (flags & PT_QUERY_STREAM_PAD) != 0,
                                (flags & PT_QUERY_TEXEL_CENTRE) != 0, d_skip, d_rays, (hipStream_t)stream));
    return 0;
}

// Guide queries (pt_query_guides.hip: query_guides_kernel, query_guides_chain_kernel). Every message under pt_query_guides, all
// before any HIP call; n == 0 returns once the arguments have passed (the device check comes last).
static int check_guides_args(pt_scene* s, int n, const void* rays, int maxLinks, const void* a, const void* nd, uint32_t flags) {
    const char* fn = "pt_query_guides";
    if (n < 0 || n > (1 << 28)) return fail(-1, "%s: n %d must be 0..%d", fn, n, 1 << 28);
    if (!s) return fail(-1, "%s: null scene", fn);
    if (!rays) return fail(-1, "%s: null rays", fn);
    if (!a || !nd) return fail(-1, "%s: null output buffer", fn);
    if (maxLinks < 0 || maxLinks > 16) return fail(-1, "%s: max_links %d must be 0..16", fn, maxLinks);
    if (flags) return fail(-1, "%s: flags 0x%x: the word is reserved and must be 0", fn, flags);
    return 0;
}

static int query_guides(pt_scene* s, int n, const void* dRays, int maxLinks, void* dA, void* dN, void* dL, hipStream_t stream) {
    const int blocks = feature_blocks((n + 63) / 64, s->dev.numCU, maxLinks > 0 ? kQueryGuidesChainWavesPerSimd : kQueryGuidesWavesPerSimd);
    int32_t* spill;
    if (int r = feature_spill(s, blocks, &spill)) return r;
    HIP_OK(launch_query_guides(s->facts.ds, n, dRays, maxLinks, blocks, dA, dN, (float*)dL, spill, stream));
    return 0;
}

int pt_query_guides_device(pt_scene* s, int n, const void* d_rays, int max_links, void* d_albedo, void* d_normal_depth, void* d_links, unsigned flags,
                           void* stream) {
    if (int r = check_guides_args(s, n, d_rays, max_links, d_albedo, d_normal_depth, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device("pt_query_guides", s)) return r;
    return query_guides(s, n, d_rays, max_links, d_albedo, d_normal_depth, d_links, (hipStream_t)stream);
}

int pt_query_guides(pt_scene* s, int n, const pt_ray* rays, int max_links, float* out_albedo, float* out_normal_depth, float* out_links, unsigned flags) {
    if (int r = check_guides_args(s, n, rays, max_links, out_albedo, out_normal_depth, flags)) return r;
    if (n == 0) return 0;
    if (int r = check_query_device("pt_query_guides", s)) return r;
    const size_t bytes = (size_t)n * sizeof(float4);
    return staged_query(s->feat.queryOut, n, rays, {{out_albedo, bytes}, {out_normal_depth, bytes}, {out_links, (size_t)n * sizeof(float)}},
                        [&](const void* dRays, void* const* d) { return query_guides(s, n, dRays, max_links, d[0], d[1], d[2], nullptr); });
}

int pt_query_camera_rays_device(const pt_camera* cam, int w, int h, float max_t, void* d_rays, void* stream) {
    if (!cam) return fail(-1, "pt_query_camera_rays_device: null camera");
    if (w <= 0 || h <= 0) return fail(-1, "pt_query_camera_rays_device: image size %d x %d must be positive", w, h);
    if ((long long)w * h > (1ll << 28)) return fail(-1, "pt_query_camera_rays_device: image of %d x %d pixels is too large", w, h);
    if (cam->w != w || cam->h != h) return fail(-1, "pt_query_camera_rays_device: the camera is %d x %d, the image %d x %d", cam->w, cam->h, w, h);
    if (!d_rays) return fail(-1, "pt_query_camera_rays_device: null rays buffer");
    HIP_OK(launch_query_camera_rays(cam_to_kernel(*cam), w, h, max_t, d_rays, (hipStream_t)stream));
    return 0;
}
