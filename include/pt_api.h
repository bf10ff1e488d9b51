/* pt_api.h — C ABI of the MI355X-native unidirectional path tracer (libptamd.so).
 *
 * Drop-in boundary for ONE hot path of DanielQ-51/cudapathtracer: the integrator launchers
 *     launch_unidirectional / launch_naive_unidirectional        (deviceCode.cuh:8-12,
 *                                                                 bodies deviceCode.cu:544-620, 207-283)
 * and the kernels under them (initRNG deviceCode.cu:53-61, Li_unidirectional :285-542,
 * Li_naive_unidirectional :158-205). Everything here is plain C: pointers, sizes, PODs whose
 * byte layouts equal the reference's CUDA structs, no torch / HIP types.
 *
 * The reference passes eleven raw device pointers per launch; here the scene arguments are
 * bundled once into an opaque `pt_scene` (which re-packs them for gfx950) and the
 * launchers take that handle. Errors: every entry point returns 0 on success or a negative
 * code, never throws or exits (the reference's launchers return void and print,
 * deviceCode.cu:611-619); pt_last_error() holds the message for the calling thread.
 *
 * `novum_*` entry points are the host side the reference keeps in main.cu/objects.cuh (config
 * parser, OBJ reader, SAH BVH builder, material table, camera, finalise) restated in plain C++.
 */
#ifndef PT_API_H
#define PT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_API_VERSION 1
#define PT_TILE_DIM 8          /* one wave64 renders one 8x8-pixel tile */
#define PT_TILE_PIXELS 64

/* ---- PODs with the reference's layouts ------------------------------------------------- */
typedef struct pt_float4 { float x, y, z, w; } __attribute__((aligned(16))) pt_float4;   /* CUDA float4 */
typedef struct pt_float2 { float x, y; } __attribute__((aligned(8))) pt_float2;           /* CUDA float2 */

/* objects.cuh:12-20 — 48 B. Leaf: left = right = -1, first/primCount index BVHindices.
 * Internal: primCount = 0, first = -1. Root is node 0 (main.cu:133-233). */
typedef struct pt_bvh_node {
    pt_float4 aabbMIN, aabbMAX;
    int32_t left, right, first, primCount;
} pt_bvh_node;

/* objects.cuh:159-172 — 80 B. lightInd = index into the light list or -51 (main.cu:1054-1056). */
typedef struct pt_triangle {
    int32_t aInd, bInd, cInd;
    int32_t naInd, nbInd, ncInd;
    int32_t uvaInd, uvbInd, uvcInd;
    int32_t materialID;
    pt_float4 emission;
    int32_t lightInd, triInd;
} pt_triangle;

/* objects.cuh:605-638 — 176 B. `type` is MaterialType (objects.cuh:595-603). */
typedef struct pt_material {
    uint8_t hasTexture; int32_t startInd, width, height;
    uint8_t hasTransMap; int32_t tstartInd, twidth, theight;
    int32_t type;
    pt_float4 albedo;
    float roughness;
    pt_float4 eta, k;
    float ior, metallic, specular, transmission;
    uint8_t isSpecular, boundary, thinWalled;
    pt_float4 absorption;
    int32_t priority;
} pt_material;

/* objects.cuh:199-219 — 112 B, passed by value to the reference's kernels. */
typedef struct pt_camera {
    pt_float4 cameraOrigin;
    int32_t w, h;
    float xRot, yRot, zRot;
    float aperture, focalDist, fovScale;
    float antiAliasJitterDist;
    pt_float4 forward, right, up;
} pt_camera;

enum { PT_MAT_DIFFUSE = 0, PT_MAT_METAL = 1, PT_MAT_SMOOTHDIELECTRIC = 2, PT_MAT_MICROFACETDIELECTRIC = 3,
       PT_MAT_LEAF = 4, PT_MAT_FLOWER = 5, PT_MAT_DELTAMIRROR = 6 };          /* objects.cuh:595-603 */
enum { PT_UNIDIRECTIONAL = 0, PT_NAIVE_UNIDIRECTIONAL = 2 };                  /* objects.cuh:570-576 */

/* What initRender uploads before the launch (main.cu:469-557), as HOST arrays. */
typedef struct pt_scene_desc {
    const pt_float4* positions; int32_t n_positions;       /* Vertices.positions */
    const pt_float4* normals;   int32_t n_normals;         /* Vertices.normals   */
    const pt_float2* uvs;       int32_t n_uvs;             /* Vertices.uvs       */
    const pt_triangle* triangles; int32_t n_triangles;     /* `scene`            */
    const pt_triangle* lights;    int32_t n_lights;        /* `lights` (copies of the emissive triangles) */
    const pt_bvh_node* bvh;       int32_t n_nodes;         /* `BVH`              */
    const int32_t* bvh_indices;                            /* `BVHindices`, n_triangles entries */
    const pt_material* materials; int32_t n_materials;     /* `materials`        */
    const pt_float4* textures;    int32_t n_texels;        /* `textures`         */
} pt_scene_desc;

typedef struct pt_scene pt_scene;      /* opaque: device-resident, re-packed scene */

/* A rank's share of the framebuffer: tiles {first + i*stride : 0 <= i < count} of the row-major
 * grid of ceil(w/8) x ceil(h/8) 8x8-pixel tiles. NULL means every tile. */
typedef struct pt_tile_range { int32_t first, stride, count; } pt_tile_range;

/* Work counters of SURVEY.md §8(d), summed over every render since pt_reset_counters. */
typedef struct pt_counters {
    uint64_t rays_closest, rays_shadow, node_pops, box_tests, tri_tests, hits, rng_draws, iterations;
} pt_counters;

/* ---- library ------------------------------------------------------------------------- */
int pt_api_version(void);
const char* pt_last_error(void);
int pt_device_count(void);                 /* number of HIP devices, < 0 on error */

/* ---- scene --------------------------------------------------------------------------- */
/* Re-packs and uploads the scene to the CURRENT HIP device. NULL on error. Replaces the
 * cudaMalloc/cudaMemcpy block main.cu:469-557. */
pt_scene* pt_scene_create(const pt_scene_desc* desc);
void pt_scene_destroy(pt_scene* scene);

/* ---- launchers (the hot path) -------------------------------------------------------- */
/* launch_unidirectional (integrator 0, useMIS as at main.cu:565) / launch_naive_unidirectional
 * (integrator 2): seeds one XORWOW stream per pixel keyed by the GLOBAL index y*w+x
 * (deviceCode.cu:59-60), runs `spp` samples per pixel with the stream continuing across
 * samples, and ADDS the radiance sum into `out_rgba_sum` (w*h float4, row-major, y = 0 is the
 * bottom row; `colors[pixelIdx] += Li`, deviceCode.cu:540). Host-buffer, blocking form. Only
 * pixels of tiles in `tiles` are touched. */
int pt_render(pt_scene* scene, const pt_camera* camera, int w, int h, int spp, int max_depth,
              int integrator, int use_mis, uint64_t seed, const pt_tile_range* tiles, float* out_rgba_sum);

/* Device-resident forms, asynchronous on `stream` (a hipStream_t, NULL = default stream).
 * d_tile_rgba: count*64 float4, tile-major ([local tile][ly*8+lx]); += semantics.
 * A pt_scene owns its work buffers (per-pixel RNG states, tile queue, traversal spill area): launches on ONE
 * scene must be ordered (same stream, or synchronised); different scenes are independent. */
int pt_render_tiles_device(pt_scene* scene, const pt_camera* camera, int w, int h, int spp, int max_depth,
                           int integrator, int use_mis, uint64_t seed, const pt_tile_range* tiles,
                           void* d_tile_rgba, int count_work, void* stream);
/* scan-line `colors` (w*h float4) <- tile-major buffer, for the tiles of `tiles`. */
int pt_untile_device(int w, int h, const pt_tile_range* tiles, const void* d_tile_rgba, void* d_colors, void* stream);
/* tile-major buffer <- scan-line `colors` (to continue an accumulation). */
int pt_tile_device(int w, int h, const pt_tile_range* tiles, const void* d_colors, void* d_tile_rgba, void* stream);

/* The reference's own call shape with the scene bundled (deviceCode.cuh:8-12): d_colors is the
 * zero-initialised DEVICE accumulator of main.cu:337-339; blocking; seed 103033
 * (deviceCode.cu:552); vertNum/triNum/lightNum live in the scene. */
int pt_launch_unidirectional(int maxDepth, pt_camera camera, pt_scene* scene, int numSample, int useMIS, int w, int h, void* d_colors);
int pt_launch_naive_unidirectional(int maxDepth, pt_camera camera, pt_scene* scene, int numSample, int useMIS, int w, int h, void* d_colors);

/* The launchers with the reference's progressive hook (the `elapsed >= saveIntervalSeconds` block
 * inside the sample loop, deviceCode.cu:574-604 / 237-267). The samples run in chunks of
 * chunk_spp; after each chunk d_colors holds the sum over samples_done samples and
 * progress(samples_done, user) runs on the calling thread (write a preview there — the reference
 * writes render.bmp + renderCSV.csv; this ABI does no file I/O). Per-pixel streams continue across
 * chunks: the final d_colors is bit-identical to pt_launch_[naive_]unidirectional. A non-zero
 * return from progress ends the render after that chunk. integrator: 0 or 2. */
typedef int (*pt_progress_fn)(int samples_done, void* user);
int pt_launch_progressive(int integrator, int maxDepth, pt_camera camera, pt_scene* scene, int numSample, int useMIS, int w, int h,
                          void* d_colors, int chunk_spp, pt_progress_fn progress, void* user);

/* The same image from the COUNTING instantiations of the kernels (stack walk everywhere, no time slices), plus the
 * per-pixel counters (w*h x 8 uint32: rays_closest, rays_shadow, node_pops, box_tests, tri_tests, hits, rng_draws,
 * iterations; out_counters may be NULL) and the totals of pt_get_counters, for parity checks. pt_render itself runs
 * the kernels that bench.py times and leaves the counters alone. */
int pt_render_counted(pt_scene* scene, const pt_camera* camera, int w, int h, int spp, int max_depth,
                      int integrator, int use_mis, uint64_t seed, const pt_tile_range* tiles,
                      float* out_rgba_sum, uint32_t* out_counters);

/* Kernel organisation used by every later render of this scene: 0 = megakernel (default: one wave
 * per 8x8 tile, all samples and bounces inside one launch), 1 = wavefront (stream-compacted: path
 * state in HBM, one logic + one traversal launch per bounce; BASELINE config 5's divergence A/B).
 * Results are bit-identical. */
int pt_set_variant(pt_scene* scene, int variant);

int pt_get_counters(pt_scene* scene, pt_counters* out);
int pt_reset_counters(pt_scene* scene);
/* Device time (ms) of the most recent megakernel launch on this scene, from HIP events recorded
 * on the launch stream around that kernel alone; waits for the launch to finish. Returns -1 (and
 * sets pt_last_error) if that launch did not complete its frame — the tile queue's bounded waits
 * ran out. The blocking launchers return -4 in that case themselves; a caller of the asynchronous
 * pt_render_tiles_device MUST check here (or through any later blocking launcher) before it uses
 * the tile buffer. */
float pt_last_kernel_ms(pt_scene* scene);
/* Tile hand-overs of the last megakernel launch (call after it has completed): how many times a wave yielded its tile at
 * the end of a time slice for another wave to continue (0 without time slices); after pt_render_adaptive, in its last launch,
 * which rendered the tiles still live. For tests and scheduling measurements. */
int pt_last_tile_handovers(pt_scene* scene);
/* How many launches of this scene had their queue waiters give up — no tile finished or handed over for "queue_timeout_ms"
 * (option, default 30 000) — although every tile was finished in the end. Not an error: waiters hold no tile, the frame is
 * complete and exact; it says the device stalled (seen with several persistent kernels co-resident on one device). A launch
 * that ends with unfinished tiles IS an error (-4). */
int pt_queue_stalls(pt_scene* scene);
/* Render launches of the last pt_render_moments / _device / _tiles / _tiles_device call on this scene: 1 if it ran fused
 * (option "moments_fused"), spp / batch_spp if it rendered in batches, 0 for an empty tile list; -1 before any such call and
 * for a NULL scene. For tests and measurements. */
int pt_last_moments_launches(pt_scene* scene);
/* Debug: the 16 header words of the tile queue after the last queued launch of this scene (1: copied, 0: the last launch used no
 * queue). [0] pops claimed, [1] pushes claimed, [2] tiles finished, [3] stall / error bits (1: a waiter recorded a stall and kept
 * waiting, 2: a waiter gave up for good, 4: a push found no slot), [4] / [5] the issue-priority steering's sums (zero once the kernel
 * has ended), [6] / [7] what the first stalled waiter saw, [8..9] the wait bound in ticks of the 100 MHz steady counter. */
int pt_debug_queue_header(pt_scene* scene, int* out16);
/* Which instantiation the launcher picks for this scene: bit 0 = ONCHIP (whole packed scene in the LDS cache),
 * bit 1 = persistent waves on the tile queue, bit 2 = time slices on, bit 3 = the 6-waves-per-SIMD kernel for scenes in HBM
 * (as used by the last launch; it needs enough tiles), bit 4 = opt-in culling, bit 5 = the last launch used a REFILL
 * instantiation (scenes in HBM: finished lanes shade and return while the others keep tracing), bit 6 = it used the FLAT
 * closest-hit traversal (LDS-resident scenes with at most 64 nodes and triangles), bit 7 = it used the SIMPLE bounce
 * (every triangle an untextured MAT_DIFFUSE: one arm per dispatcher, no medium stack), bit 8 = the pair form of FLAT
 * (shadow + extension ray in one pass), bit 9 = the FLAT launch decided the visited leaves from the leaves' own boxes (the
 * scene's boxes are finite and nested, checked at pt_scene_create; a caller's loose or refit tree takes the lockstep walk
 * over the boxes as given), bit 10 = it used the LEAN generic bounce. For labelling measurements. */
int pt_scene_flags(pt_scene* scene);
/* Opt-in (default off): skip BVH children whose box lies beyond the best hit so far / beyond a shadow ray's max_t.
 * The reference has no such test and its results are the contract, so the default kernels do not have it either: a
 * triangle inside a skipped box can still produce a smaller t (different roundings, grazing incidence), and one such
 * hit shifts the pixel's whole RNG stream. Measured on the 263 k-triangle scene: 13 of 2 073 600 pixels differ after
 * 4.6e9 rays, at 1.2-1.6x the speed. A renderer's trade-off, not the reference's image. Applies to the
 * kernel for scenes that do not fit the LDS cache; flag bit 4 of pt_scene_flags reports it. */
int pt_set_culling(pt_scene* scene, int on);
/* Per-scene kernel-selection and scheduling options, by name. The library reads NO environment variable: what a
 * process renders cannot be steered from its environment. Only "culling" (= pt_set_culling) can reach the image; all
 * other options choose between instantiations / schedules whose results are bit-identical (tests/test_gpu_parity.py
 * drives every one of them against the oracle). They exist for A/B measurements and for the tests.
 *   "flat" 0|1            FLAT closest-hit traversal for LDS-resident scenes of at most 128 nodes and triangles (1; 2 = 1)
 *   "wf_wide_wg" 0|1|2    wavefront variant, scenes in HBM: the trace kernel in 16-wave workgroups sharing 48 KB of the tree top (1: when
 *                         the launch has enough paths to fill them, 2: always)
 *   "leaf_boxes" 0|1      FLAT kernels test each leaf's own box instead of walking the nodes in lockstep (1)
 *   "flat2" 0|1           FLAT scenes (<= 64 triangles, no MAT_LEAF triangle), MIS integrator: shadow ray and next extension
 *                         ray in one FLAT pass (1)
 *   "simple" 0|1          with FLAT: the diffuse-only bounce for scenes whose triangles are all untextured MAT_DIFFUSE (1)
 *   "lean" 0|1            the generic bounce without its leaf arms and texture fetches for scenes that have neither a MAT_LEAF
 *                         triangle nor a textured material — glass, mirrors, metals (1)
 *   "onchip" 0|1          LDS-resident instantiation when the scene fits (1)
 *   "waves_hbm" 0|1|2     the 6-waves-per-SIMD kernel for scenes in HBM: never / when the launch has enough tiles / always (1)
 *   "refill" 0|1          resumable traversal for scenes in HBM (1)
 *   "refill_keep", "node_keep", "tri_keep" 0..15   loop-exit thresholds in sixteenths (6, 10, 8; re-swept in round 3: profiles/r03_sweep_keep.log — while "refill_keep" is unset the 4-wave kernel of small shares uses 10)
 *   "slice_iters" n       bounce iterations a wave keeps a tile before it queues it again, 0 = until finished (512)
 *   "slice_always" 0|1    time slices from the first tile on (1)
 *   "sched_mask" 2^k-1    a wave looks at the queue every sched_mask + 1 iterations (31)
 *   "lpt_prio" 0|1|2      issue-priority steering: off / once no fresh tile is left / always (2)
 *   "persistent" 0|1      persistent waves on the tile queue (1)
 *   "queue_timeout_ms" n  how long a wait on the tile queue may see no progress before the waiters leave (30 000)
 *   "moments_fused" 0|1   pt_render_moments and its _device / _tiles forms render all spp samples in ONE megakernel launch whose
 *                         lanes keep the squared batch sums themselves, at every batch_spp-th sample of their pixel, instead of
 *                         spp / batch_spp launches with a bookkeeping pass between them: the same two buffers in every bit.
 *                         Where the launch's kernel has no fused form in the dispatch — culling, "refill" 0, the wavefront
 *                         variant, the SIMPLE pair kernel of diffuse-only LDS-resident scenes
 *                          — the call renders in batches as without the option;
 *                         pt_last_moments_launches tells which it was (0)
 * Retired options — experimental variants that were built, proven bit-identical, measured SLOWER and then removed (DESIGN.md §6
 * keeps their results and names the commit that last held their code). Their names are still known; each accepts only the value
 * that meant "off", which is also what pt_get_option reads back, and returns -3 for any other value in its range:
 *   "wide" 0 (was: 4-wide collapsed tree), "compact" 0 (32-byte quantised nodes), "spec" 2 (speculative descent),
 *   "defer_shadow" 0 (pair walk in the 4-wave kernel), "xcd_bands" 0 (one band of tiles per XCD); and "refill" refuses 2
 *   (resumable traversal for LDS-resident scenes too).
 * Returns 0, or < 0 for an unknown name / a value out of range. */
int pt_set_option(pt_scene* scene, const char* name, int value);
int pt_get_option(pt_scene* scene, const char* name, int* value);
/* Always 0: no build holds the retired variants any more. Kept so that callers that ask before an A/B keep linking. */
int pt_has_experimental(void);
/* Eight more sums since the last pt_reset_counters. Normal build: out8[0] = internal-node fetches of counting launches
 * that went to global memory (node index beyond the LDS scene cache) — with tri_tests, the L1 line-access count behind
 * bench.py's roofline for scenes in HBM; the rest zero. Diagnostic builds:
 * -DPT_STAMPS: s_memtime spent in regeneration, closest-hit traversal, bounce logic (incl. the shadow ray), then the
 * sum of wave lifetimes, ~(earliest start) and the latest end on the 100 MHz wall clock, 0, and — timed (non-counting)
 * launches, which this build sums as well — 64 x the logic steps of all waves; such a launch also leaves the rays IT traced
 * in pt_get_counters' rays_closest / rays_shadow and the lanes that were busy at logic-step entry in `iterations`
 * (tools/stamps.py, tools/lane_occupancy.py).
 * -DPT_UTIL (counting launches): {trips of a wave, trips summed over its lanes} through the node loop and the
 * triangle loop of the closest-hit traversal, then of the shadow traversal (tools/lane_util.py). */
int pt_debug_stamps(pt_scene* scene, unsigned long long* out8);

/* ---- multi-GPU: the framebuffer sharded by screen tile over the GPUs of one node -------------
 * The reference is single-GPU (one launch_unidirectional per frame, main.cu:565). A pixel depends only on (scene,
 * camera, global pixel index, seed), so device r of N renders the 8x8 tiles {t : t mod N == r} of a replicated scene
 * — no data-path collective — and ONE gather (RCCL send/recv over xGMI, or hipMemcpyPeerAsync) brings the tile
 * buffers to device 0, which de-interleaves them. One host thread per device inside the call; blocking; the result
 * is bit-identical to pt_render for any N. This is what a C++ host (the reference's main.cu) binds to use 8 GPUs. */
#define PT_MULTI_MAX_DEVICES 16
typedef struct pt_multi pt_multi;          /* opaque: one scene replica, stream and communicator per device */
typedef struct pt_multi_stats {
    int32_t n_devices;
    int32_t gather;                        /* transport the gather used: 0 none (one device), 1 RCCL, 2 peer copies */
    float kernel_ms[PT_MULTI_MAX_DEVICES]; /* per device: its megakernel, HIP events on its stream */
    float render_ms, gather_ms, total_ms;  /* host wall clock: upload + render (max over devices), gather, whole call */
} pt_multi_stats;
/* Tile ownership of `rank` among `world` devices (interleaved). */
void pt_rank_tiles(int w, int h, int rank, int world, pt_tile_range* out);
/* Replicates the scene on n_devices HIP devices (device_ids NULL = 0 .. n_devices-1). NULL on error. */
pt_multi* pt_multi_create(const pt_scene_desc* desc, int n_devices, const int* device_ids);
void pt_multi_destroy(pt_multi* m);
/* "gather": 0 auto (RCCL, else peer copies), 1 RCCL, 2 hipMemcpyPeerAsync; "self_gather" 1: with ONE device, still send
 * the tile buffer through the collective (to itself) — a plumbing check for one-GPU machines; "same_device" 1 (default):
 * ranks that share a device (rehearsals only) issue to ONE stream of that device, so their persistent kernels — each
 * sized to fill the chip — run in stream order, 0: every rank its own stream, the kernels co-reside (both bit-identical;
 * the host threads run concurrently either way); any pt_set_option name: applied to every replica. */
int pt_multi_set_option(pt_multi* m, const char* name, int value);
int pt_multi_set_variant(pt_multi* m, int variant);
/* pt_render over all devices of `m`: host buffer in / out with `+=` semantics like pt_render. stats may be NULL. */
int pt_multi_render(pt_multi* m, const pt_camera* camera, int w, int h, int spp, int max_depth, int integrator, int use_mis,
                    uint64_t seed, float* out_rgba_sum, pt_multi_stats* stats);
/* One-shot form: create, render, destroy. */
int pt_render_multi(const pt_scene_desc* desc, int n_devices, const int* device_ids, const pt_camera* camera, int w, int h, int spp,
                    int max_depth, int integrator, int use_mis, uint64_t seed, float* out_rgba_sum, pt_multi_stats* stats);

/* ---- feature buffers and denoiser (opt-in post-process; not part of the reference's image) ----------------------
 * First-hit feature buffers, scan-line w*h float4 each, y = 0 the bottom row (as pt_render).
 * out_albedo:       rgb = mean albedo over the rays that hit, w = coverage (hits / aov_spp; 0 = nothing hit)
 * out_normal_depth: xyz = mean of resolve_hit's normal over the hits (NOT renormalised; it faces the camera ray),
 *                   w = mean hit distance t
 * Ray k (0 <= k < aov_spp) of pixel (x, y) is camera_ray drawn from a FRESH XORWOW stream keyed (seed + k, y*w + x).
 * Ray 0 is therefore exactly the first camera ray of that pixel's beauty render with `seed`. The closest hit is the
 * probe's (max_t 999999), the albedo what the bounce reads at that hit: the material's albedo, or the bilinear texture
 * sample for textured materials, for every material type (emitters included). FIRST HIT ONLY: mirrors and glass report
 * their own albedo; no specular chain is followed. Sums run in k order in f32, then one IEEE division by the hit count;
 * a pixel with no hit is all zeros. The pass seeds its own streams and never touches the scene's per-pixel RNG states,
 * tile accumulator or counters: it may run between the chunks of pt_launch_progressive. Arguments are checked before
 * any HIP call (w, h, aov_spp > 0; camera->w / h equal to w / h; no NULL pointer). */
int pt_render_aovs(pt_scene* scene, const pt_camera* camera, int w, int h, int aov_spp, uint64_t seed,
                   float* out_albedo, float* out_normal_depth);                       /* host buffers, blocking */
int pt_render_aovs_device(pt_scene* scene, const pt_camera* camera, int w, int h, int aov_spp, uint64_t seed,
                          void* d_albedo, void* d_normal_depth, void* stream);       /* device buffers, async */

/* Feature buffers that follow mirrors and glass to the surface behind them. Same buffers, layout, rays (ray k of pixel (x, y)
 * from the fresh stream keyed (seed + k, y*w + x)), closest hit (max_t 999999), sums in k order and final division as
 * pt_render_aovs, but after its first hit each ray follows a deterministic CHAIN of at most max_links (0..16) specular links:
 *   LINK RULE. The ray is in its chain while the material at its hit has isSpecular set and is a delta mirror (type 6) or a
 *   smooth dielectric (type 2). A mirror reflects; a dielectric refracts, or reflects on total internal reflection. A hit on
 *   any other material ends the chain there.
 *   DIRECTION ARITHMETIC, every operation rounded once to f32 in the order written, left to right, nothing fused. d is the
 *   unit ray direction, n resolve_hit's normal at the hit (it faces the ray), dn = d.x*n.x + d.y*n.y + d.z*n.z:
 *     reflect:     r = d - (2*dn)*n                                   (per component: d.c - (2*dn)*n.c)
 *     dielectric:  cosI = min(max(-dn, EPS), 1); eta = backface ? ior : 1/ior; k = 1 - (eta*eta)*(1 - cosI*cosI);
 *                  k < 0: reflect as above; otherwise r = eta*d + (eta*cosI - sqrtf(k))*n   (per component: eta*d.c + (..)*n.c)
 *     next ray:    d' = r / sqrtf(r.x*r.x + r.y*r.y + r.z*r.z)  (three IEEE divisions);
 *                  o' = point + n*EPS after a reflection, point - n*EPS after a refraction (EPS = 1e-5: the beauty path's offsets).
 *   RESULT OF A RAY whose chain ends on a non-specular surface after L links: that surface's albedo (material's albedo, or the
 *   texture sample: no tint is multiplied at a mirror or an interface, as the path multiplies none), resolve_hit's normal there,
 *   depth = the f32 sum of the links' t in link order (t0, + t1, + t2 ...), links = L. For a planar mirror, camera ray * depth is
 *   the virtual image point, so pt_temporal_accumulate's reprojection holds through it.
 *   FALLBACK: a ray whose chain leaves the scene, or that is still on a specular surface after max_links links, reports its
 *   FIRST hit's albedo, normal and t, with links = 0. A ray whose first ray misses contributes nothing, as in pt_render_aovs.
 *   DELIBERATE SIMPLIFICATIONS: the medium stack and priorities are ignored (an interface the beauty path would pass straight
 *   through, such as a nested lower-priority dielectric, is refracted); there is no Fresnel branch choice (refraction is always
 *   followed where it exists); there is no absorption. The guide is a feature buffer, not radiance.
 * out_links (w*h floats, may be NULL): the mean link count over the rays that hit (integer sum, converted to f32, divided by the
 * hit count), 0 where nothing hit. The coverage channel is bit-identical to pt_render_aovs'; a pixel whose rays all hit a
 * non-specular surface first is bit-identical to pt_render_aovs in all eight floats; max_links = 0 is pt_render_aovs bit for bit
 * with links all 0. Like pt_render_aovs the pass touches no RNG state, accumulator or counter of the scene. Arguments are checked
 * before any HIP call (those of pt_render_aovs, and max_links in 0..16: -1 with a message). */
int pt_render_aovs_chain(pt_scene* scene, const pt_camera* camera, int w, int h, int aov_spp, int max_links, uint64_t seed,
                         float* out_albedo, float* out_normal_depth, float* out_links /* w*h floats, may be NULL */);
int pt_render_aovs_chain_device(pt_scene* scene, const pt_camera* camera, int w, int h, int aov_spp, int max_links, uint64_t seed,
                                void* d_albedo, void* d_normal_depth, void* d_links /* may be NULL */, void* stream);

/* Feature buffers through PIXEL CENTRES: one ray per pixel that no random draw reaches, so the pass has no aov_spp and no seed and
 * seeds no stream. cam0 is *camera with antiAliasJitterDist = 0 and aperture = 0, everything else unchanged (focalDist included);
 * the centre ray of pixel (x, y) is camera_ray(cam0, x, y). In f32, every operation rounded once in the order written, nothing
 * fused:
 *   u = (2 ((float)x / (float)w) - 1) aspect fovScale, aspect = (float)w / (float)h;  v = (2 ((float)y / (float)h) - 1) fovScale;
 *   focal = origin + right (u focalDist) + up (v focalDist) + forward focalDist;  o = origin + 0 (a -0 component becomes +0, as
 *   camera_ray's lens sum makes it);  d = normalize(focal - o).
 * The buffers are bit-identical, in all eight floats and in links, to pt_render_aovs_chain(scene, &cam0, w, h, aov_spp = 1,
 * max_links, any seed, ...), so for max_links = 0 to pt_render_aovs(scene, &cam0, w, h, 1, any seed, ...) as well: layout, closest
 * hit (max_t 999999), link rule, direction arithmetic, fallback, "no hit is all zeros" and coverage (0 or 1) are those functions'.
 * The antiAliasJitterDist and aperture of *camera play no part. Because the ray depends on the pixel only through x / w and y / h,
 * the centre ray of pixel (X, Y) of pt_camera_scaled(camera, s) IS the centre ray of pixel (sX, sY) of camera: see
 * pt_guide_subsample. Like the other feature passes this one touches no RNG state, accumulator or counter of the scene. Arguments
 * are checked before any HIP call (those of pt_render_aovs, and max_links in 0..16: -1 with a message). */
int pt_render_aovs_centre(pt_scene* scene, const pt_camera* camera, int w, int h, int max_links,
                          float* out_albedo, float* out_normal_depth, float* out_links /* w*h floats, may be NULL */);
int pt_render_aovs_centre_device(pt_scene* scene, const pt_camera* camera, int w, int h, int max_links,
                                 void* d_albedo, void* d_normal_depth, void* d_links /* may be NULL */, void* stream);

/* Edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) on albedo-demodulated colour, guided by the buffers
 * above. The contract, per pixel p (all buffers w*h float4):
 *   m_p = S_p / spp. p PASSES THROUGH (output = S_p bit for bit, all four channels) if its coverage is 0 or any of m_p.rgb
 *   is NaN / Inf (so novum_finalise still paints those); pass-through pixels are never taps.
 *   a_p = albedo_p per channel where >= 0.01, else 1; e_p = m_p / a_p. L = mean luminance (0.2126, 0.7152, 0.0722) of e
 *   over the filtered pixels. Iteration i (step s = 2^i): e'_p = sum_q w e_q / sum_q w over q = p + s (dx, dy),
 *   dx, dy in -2..2, inside the image and not pass-through; w = h(dx) h(dy) w_c w_n w_z with h = (1, 4, 6, 4, 1) / 16,
 *   w_c = exp(-|e_p - e_q|^2 / (sigma_color^2 L^2 2^-i + 1e-20)), w_n = max(0, n_p . n_q)^sigma_normal on the
 *   normalised mean normals (0 if either normal is zero), w_z = exp(-|z_p - z_q| / (sigma_depth z_p)); the centre tap
 *   weighs h(0)^2. Output: rgb = spp a_p e_p with the last iteration's e_p, w = S_p.w.
 * Multi-GPU frames are denoised after the gather: the taps cross shard boundaries. */
typedef struct pt_denoise_params {
    int32_t iterations;          /* default 5: steps 1, 2, 4, 8, 16 (0..16) */
    float sigma_color;           /* relative to the image's mean demodulated luminance (> 0) */
    float sigma_normal;          /* exponent on the normals' cosine (>= 0) */
    float sigma_depth;           /* relative depth difference (> 0) */
                                 /* defaults 5, 1.0, 64, 0.02: DESIGN.md "Feature buffers and denoiser" */
} pt_denoise_params;
void   pt_denoise_defaults(pt_denoise_params* out);
/* device workspace of pt_denoise_device: 3 * w*h float4 (two colour buffers, the guide) + 8 B per 256 pixels
 * (rounded up to 16 B) + 16 B; 0 if w or h <= 0 */
size_t pt_denoise_workspace_bytes(int w, int h);
/* in: the radiance SUM of `spp` samples (what pt_render / the launchers leave). out: the same units, so novum_finalise /
 * novum_save_bmp apply unchanged. out may alias in. params NULL = pt_denoise_defaults. */
int pt_denoise(int w, int h, const float* rgba_sum, int spp, const float* albedo, const float* normal_depth,
               const pt_denoise_params* params, float* out_rgba_sum);                                  /* host, blocking */
int pt_denoise_device(int w, int h, const void* d_rgba_sum, int spp, const void* d_albedo, const void* d_normal_depth,
                      const pt_denoise_params* params, void* d_workspace, void* d_out, void* stream);  /* async */

/* ---- adaptive sampling: 8x8 tiles stop when their error estimate converges ------------------
 * The per-pixel stopping criterion of Dammertz et al., "A hierarchical automatic stopping condition for Monte Carlo
 * global illumination" (2009), section 2.1, applied per tile. A pixel's samples are one XORWOW stream keyed by the pixel,
 * so a tile that stops after n samples holds exactly the sums of pt_render(spp = n) over its pixels, bit for bit.
 *
 * Schedule and estimator. All arithmetic is f32 with IEEE rounding and no contraction, evaluated left to right:
 *   n = 0; live = every tile of the ceil(w/8) x ceil(h/8) grid, ascending
 *   loop:
 *     c = min(chunk_spp, (max_spp - n) / 2)  (integer division); stop if c == 0 or live is empty
 *     render c samples on live -> S;  M = S;  render c samples on live -> S
 *     H = H + (S - M)  per rgb channel (H starts at 0);  n = n + 2c
 *     per in-image pixel of a live tile:
 *       d = |S.r - 2H.r| + |S.g - 2H.g| + |S.b - 2H.b|;  inv = 1.0f / (float)n
 *       e = (d * inv) / (1e-4f + sqrtf((S.r + S.g + S.b) * inv))
 *       e = 0 if any rgb channel of S or H is non-finite, or if e is NaN (such a pixel never holds its tile back)
 *     E_T = max(0, e over the tile's in-image pixels)
 *     a live tile stops, with tile_spp = n, if n >= min_spp and E_T < threshold; the others stay live, in ascending order
 *   tiles still live at the end get tile_spp = n
 * Round 0 renders the whole frame (streams seeded as in pt_render); later rounds render only the live tiles.
 *
 * Outputs. out_rgba_sum: w*h float4 scan-line, y = 0 the bottom row, each pixel the sum over its own tile_spp samples;
 * w is 0. This call WRITES the sums, it does not add to them (unlike pt_render): the estimator must see this render's
 * samples alone. out_tile_spp / out_tile_err: one entry per tile, row-major over the tile grid (tile = ty * ceil(w/8) + tx,
 * the numbering of pt_tile_range); out_tile_err holds E_T of the last round the tile took part in and may be NULL.
 * stats (may be NULL): rounds run, tiles whose tile_spp is the largest n the schedule reached, and the sum over in-image
 * pixels of their sample counts.
 * Both forms block; the device form enqueues all its work and read-backs on `stream`: once per round, one copy of 96 bytes
 * (the live count and the tile queue's words after each of the round's two launches, both of which are checked: a launch that
 * left a listed tile unfinished fails the call with -4, a stall counts in pt_queue_stalls). Arguments are checked
 * before any HIP call: image size, params, NULL pointers (camera and the outputs), then the scene. The megakernel only:
 * with the wavefront variant selected (pt_set_variant) the call fails with -1 and leaves the outputs untouched. Every
 * launch uses the tile queue whatever the "persistent" option says; all other options apply as usual. */
typedef struct pt_adaptive_params {
    int32_t min_spp;             /* no tile stops before it has this many samples (0 <= min_spp <= max_spp) */
    int32_t max_spp;             /* no tile gets more (>= 2; an odd budget ends at max_spp - 1) */
    int32_t chunk_spp;           /* c: samples per half-round (>= 1) */
    float threshold;             /* a tile stops when E_T < threshold; 0 = never early (uniform max_spp); NaN / < 0 rejected */
} pt_adaptive_params;
typedef struct pt_adaptive_stats {
    int32_t rounds;              /* rounds run (each renders 2c samples on the live tiles) */
    int32_t tiles_at_max;        /* tiles that ran to the end of the schedule */
    long long pixel_samples;     /* sum of tile_spp over in-image pixels */
} pt_adaptive_stats;
int pt_render_adaptive(pt_scene* scene, const pt_camera* camera, int w, int h, int max_depth, int integrator, int use_mis,
                       uint64_t seed, const pt_adaptive_params* params, float* out_rgba_sum, int32_t* out_tile_spp,
                       float* out_tile_err, pt_adaptive_stats* stats);                                   /* host buffers */
int pt_render_adaptive_device(pt_scene* scene, const pt_camera* camera, int w, int h, int max_depth, int integrator, int use_mis,
                              uint64_t seed, const pt_adaptive_params* params, void* d_rgba_sum, void* d_tile_spp,
                              void* d_tile_err, pt_adaptive_stats* stats, void* stream);                /* device buffers */

/* ---- per-pixel variance: a frame plus its sum of squared batch sums; the variance-guided denoiser ------------------
 * pt_render_moments renders `spp` samples per pixel as B = spp / batch_spp batches of c = batch_spp samples (c >= 1, spp a
 * multiple of c, B >= 2) on the whole frame. All arithmetic is f32 with IEEE rounding and no contraction, left to right:
 *   batch j = 1..B renders c samples per pixel; the streams are seeded as in pt_render before batch 1 and continue afterwards,
 *   so after batch j the accumulator S_j is bit-identical to pt_render(spp = j c) into a zeroed buffer;
 *   after each batch, per pixel and rgb channel: d = S_j - S_{j-1} (S_0 = 0), Q = Q + d d (Q_0 = 0; the product is rounded
 *   before the add). Q.w = (float)B. No special case for NaN / Inf: they propagate into Q.
 * Outputs, both w*h float4 scan-line, y = 0 the bottom row: out_rgba_sum = S_B (pt_render(spp) bit for bit), out_sq_sum = Q.
 * This call WRITES both (like pt_render_adaptive, unlike pt_render). It never touches the counters, and a later pt_render of
 * the same scene is unaffected (it re-seeds). Both forms block; the device form enqueues its work on `stream`. After every
 * batch the host waits and checks the launch as pt_render checks its own: an unfinished frame fails the call with -4 (no
 * further batch is launched), a stall counts in pt_queue_stalls. Both variants (pt_set_variant 0 and 1) and every option
 * apply. Arguments are checked before any HIP call: image size, spp, batch_spp, the integrator, NULL camera, camera->w / h
 * equal to w / h, NULL outputs, then the scene. Multi-GPU frames are out of scope. */
int pt_render_moments(pt_scene* scene, const pt_camera* camera, int w, int h, int spp, int batch_spp, int max_depth, int integrator,
                      int use_mis, uint64_t seed, float* out_rgba_sum, float* out_sq_sum);              /* host buffers */
int pt_render_moments_device(pt_scene* scene, const pt_camera* camera, int w, int h, int spp, int batch_spp, int max_depth,
                             int integrator, int use_mis, uint64_t seed, void* d_rgba_sum, void* d_sq_sum,
                             void* stream);                                                              /* device buffers */

/* pt_denoise's a-trous filter with a variance-guided colour weight (after SVGF: Schied et al., HPG 2017). The contract is
 * pt_denoise's except for what is listed here (p a pixel, q a tap):
 *   B = batches (>= 2, a divisor of spp; Q.w is not read). Per rgb channel, in f32, left to right,
 *     var_c = max(0, Q_c - S_c S_c / B) / (B - 1) * B / (spp spp)     (the variance of the pixel's MEAN; max(0, NaN) is NaN)
 *     V_p = var_r / (a_r a_r) + var_g / (a_g a_g) + var_b / (a_b a_b)  with pt_denoise's demodulation albedo a.
 *   p PASSES THROUGH under pt_denoise's rule, and also if V_p is NaN / Inf. Pass-through pixels are never taps (neither of
 *   the 5x5 nor of the 3x3 below).
 *   Iteration i (step s = 2^i): Vt_p = the 3x3 binomial ((1, 2, 1) x (1, 2, 1) / 16, stride 1) of the current V around p,
 *   where a neighbour outside the image or pass-through contributes V_p itself;
 *     w_c = exp(-|e_p - e_q|_2 / (sigma_var sqrt(Vt_p) + 1e-3 L + 1e-20))
 *   (L as in pt_denoise; the second term keeps the quotient defined where the variance is 0: identical samples, e.g. inside
 *   the emitter; the third where L is 0 as well: a black frame). w_n, w_z, h and the centre weight h(0)^2 are pt_denoise's.
 *     e'_p = sum_q w e_q / sum_q w,   V'_p = sum_q w^2 V_q / (sum_q w)^2     (a pixel with a zero normal keeps e_p and V_p)
 *   Output as pt_denoise: rgb = spp a_p e_p, w = S_p.w; out may alias rgba_sum; host and device form are bit-identical. */
typedef struct pt_denoise_var_params {
    int32_t iterations;          /* default 3: steps 1, 2, 4 (0..16) */
    float sigma_var;             /* colour tolerance in standard deviations of the pixel's mean (> 0) */
    float sigma_normal;          /* exponent on the normals' cosine (>= 0) */
    float sigma_depth;           /* relative depth difference (> 0) */
                                 /* defaults 3, 6.0, 64, 0.02: DESIGN.md "Variance buffers and the variance-guided denoiser" */
} pt_denoise_var_params;
void   pt_denoise_var_defaults(pt_denoise_var_params* out);
/* device workspace of pt_denoise_var_device: pt_denoise_device's layout and size (the variance travels in the colour
 * buffers' w): 3 * w*h float4 + 8 B per 256 pixels (rounded up to 16 B) + 16 B; 0 if w or h <= 0 */
size_t pt_denoise_var_workspace_bytes(int w, int h);
/* rgba_sum, sq_sum: what pt_render_moments wrote (spp samples in `batches` batches). params NULL = pt_denoise_var_defaults. */
int pt_denoise_var(int w, int h, const float* rgba_sum, const float* sq_sum, int spp, int batches, const float* albedo,
                   const float* normal_depth, const pt_denoise_var_params* params, float* out_rgba_sum);        /* host, blocking */
int pt_denoise_var_device(int w, int h, const void* d_rgba_sum, const void* d_sq_sum, int spp, int batches, const void* d_albedo,
                          const void* d_normal_depth, const pt_denoise_var_params* params, void* d_workspace, void* d_out,
                          void* stream);                                                                          /* async */

/* ---- temporal accumulation with reprojection (the history stage of SVGF: Schied et al., HPG 2017) ------------------
 * Two opt-in post-processes on buffers, stateless like pt_denoise*: the caller keeps the history between frames. In these two the
 * scene is static and only the camera moves; the _motion forms (below, "motion") take a buffer that says where the surfaces of a
 * scene updated in place were before. One sample count per frame is assumed: the history length N counts FRAMES, not samples.
 *
 * The history: hist is w*h float4 = (e.r, e.g, e.b, V) in pt_denoise_var's working format: e the albedo-demodulated mean
 * radiance, V the variance of that mean; V = -1 marks a PASS-THROUGH pixel, whose rgb holds the raw mean m. hist_len is w*h
 * float: the number of frames blended into the pixel, 0 = none.
 *
 * pt_temporal_accumulate, per pixel p = (x, y) of this frame. All arithmetic is f32 with IEEE rounding (division and sqrtf
 * included) and no contraction, left to right:
 *   1. This frame: m, a, e_cur, V_cur and the pass-through rule are pt_denoise_var's from (S, Q, spp, batches, albedo). A
 *      pass-through pixel writes (m.rgb, -1) and length 0.
 *   2. No history given (prev_normal_depth, hist, hist_len all NULL: the first frame): write (e_cur, V_cur) and length 1.
 *   3. Reprojection. The unjittered ray of pixel x passes through x, not x + 0.5 (camera_ray's jitter is centred on 0). With
 *      cam's fields and aspect = (float)w / (float)h:
 *        u = (2 (x / w) - 1) aspect fovScale,  v = (2 (y / h) - 1) fovScale,  t = right u + up v + forward,
 *        d = t / sqrtf(t . t),  P = origin + d z_p   with z_p = normal_depth_p.w.
 *      With cam_prev's fields (primed): q = P - origin', z_c = q . forward'; unless z_c > 0 the pixel has no history;
 *        x' = ((q . right' / z_c) / (aspect' fovScale') + 1) w / 2,  y' = ((q . up' / z_c) / fovScale' + 1) h / 2,
 *      and the expected previous depth is z' = sqrtf(q . q). The thin-lens camera uses the same centre ray: its lens sample is
 *      ignored (the feature buffers' depth belongs to a ray from the lens, so history is rejected more often out of focus).
 *      IDENTITY: if cam_prev is NULL or its 112 bytes equal cam's, then x' = x, y' = y, z' = z_p exactly and the only tap is
 *      (x, y) with weight 1: a still camera does not depend on rounding in the projection.
 *   4. Taps k = (floor(x') + {0, 1}, floor(y') + {0, 1}) in the order (0,0), (1,0), (0,1), (1,1), with the bilinear weights
 *      (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy, fx = x' - floor(x'). A tap is VALID if it is inside the image,
 *      hist_k.w >= 0, |z_prev(k) - z'| <= depth_tol z', and n_p . n_prev(k) >= normal_tol on the normals of normal_depth and
 *      prev_normal_depth normalised as pt_denoise normalises them (a zero normal on either side: invalid). Invalid taps are
 *      skipped, never weighted by 0. W = sum of the weights of the valid taps. W < 0.01: no history. Otherwise e_h, V_h, N_h =
 *      (sum of weight times the tap's e, V, hist_len) / W.
 *   5. Blend: N = min(N_h + 1, max_history), alpha = 1 / N, e = e_h + alpha (e_cur - e_h),
 *      V = ((1 - alpha) (1 - alpha)) V_h + (alpha alpha) V_cur   (a blend of independent estimates; every frame brings its own
 *      variance from pt_render_moments). Write (e, V) and N. With no history: (e_cur, V_cur) and length 1.
 * out_hist / out_hist_len must not overlap hist / hist_len (the gather reads neighbours): rejected with -1; a viewer
 * ping-pongs two pairs. Arguments are checked before any HIP call: image size, spp, batches (>= 2, a divisor of spp), NULL
 * camera, camera (and cam_prev) w / h equal to w / h, NULL buffers and outputs, the three history pointers all NULL or all
 * set, aliasing, params. Host and device form are bit-identical; the device form needs no workspace.
 * Multi-GPU frames: accumulate after the gather, as for the denoisers. */
typedef struct pt_temporal_params {
    int32_t max_history;         /* N is capped here: alpha never falls below 1 / max_history (>= 1) */
    float depth_tol;             /* relative depth difference a tap may have (> 0, finite) */
    float normal_tol;            /* smallest cosine between the unit normals (0 < normal_tol <= 1) */
                                 /* defaults 32, 0.10, 0.9: DESIGN.md "Temporal accumulation" */
} pt_temporal_params;
void pt_temporal_defaults(pt_temporal_params* out);
/* rgba_sum, sq_sum: this frame's pt_render_moments (spp samples in `batches` batches); albedo, normal_depth: this frame's
 * pt_render_aovs; prev_normal_depth: the previous frame's normal_depth. params NULL = pt_temporal_defaults. */
int pt_temporal_accumulate(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* rgba_sum, const float* sq_sum,
                           int spp, int batches, const float* albedo, const float* normal_depth, const float* prev_normal_depth,
                           const float* hist, const float* hist_len, const pt_temporal_params* params, float* out_hist,
                           float* out_hist_len);                                                                 /* host, blocking */
int pt_temporal_accumulate_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_rgba_sum,
                                  const void* d_sq_sum, int spp, int batches, const void* d_albedo, const void* d_normal_depth,
                                  const void* d_prev_normal_depth, const void* d_hist, const void* d_hist_len,
                                  const pt_temporal_params* params, void* d_out_hist, void* d_out_hist_len, void* stream);  /* async */

/* pt_denoise_var's filter on a history buffer: the contract is pt_denoise_var's from its prepare stage on, with (e_p, V_p)
 * read from hist instead of derived from S and Q. p PASSES THROUGH if hist_p.w < 0 or any of hist_p is NaN / Inf; pass-through
 * pixels are never taps. albedo and normal_depth are the current frame's. Output: the per-pixel radiance MEAN, rgb = a_p e_p
 * with the last iteration's e_p, w = 0; a pass-through pixel returns hist_p.rgb bit for bit (w = 0), so novum_finalise(.., 1)
 * paints NaN / Inf as before. The history itself stays unfiltered: feeding a filtered iteration back into it, as SVGF does, is
 * out of scope. out may alias hist. Workspace: pt_denoise_var_device's size and layout. params NULL = pt_denoise_var_defaults. */
size_t pt_denoise_hist_workspace_bytes(int w, int h);
int pt_denoise_hist(int w, int h, const float* hist, const float* albedo, const float* normal_depth,
                    const pt_denoise_var_params* params, float* out_rgba_mean);                                  /* host, blocking */
int pt_denoise_hist_device(int w, int h, const void* d_hist, const void* d_albedo, const void* d_normal_depth,
                           const pt_denoise_var_params* params, void* d_workspace, void* d_out, void* stream);   /* async */

/* ---- render scale: a low-resolution frame upsampled by full-resolution guides ------------------------------------------------
 * pt_camera_scaled: *out = *cam with w and h divided by `scale`; nothing else in the struct depends on the size. -1 unless
 * 1 <= scale <= 8 and scale divides cam->w and cam->h (and on a NULL pointer). Host only. The unjittered ray of pixel X of the
 * scaled camera passes through display coordinate scale * X (camera_ray's jitter is centred on 0, and (float)w / (float)h is
 * the same number for both sizes), so low-res pixel X sits exactly on display pixel scale * X.
 *
 * pt_upsample: a stateless post-process like pt_denoise*. In: the low-res frame of the scaled camera, wl x hl = (w / s) x (h / s)
 * float4 each: rgba_sum, sq_sum (pt_render_moments, spp samples in `batches` batches), albedo_lo, normal_depth_lo
 * (pt_render_aovs); and the display camera's albedo and normal_depth, w x h float4. Out: cur, w x h float4 in pt_denoise_var's
 * working format (rgb = e, w = V; V = -1 marks a PASS-THROUGH pixel whose rgb holds a raw mean): what pt_temporal_accumulate_cur
 * and pt_denoise_hist read. Re-modulated by the full-resolution albedo there, texture and material edges come back at display
 * resolution. Per display pixel p = (x, y), in f32 with IEEE rounding and no contraction, left to right:
 *   1. X0 = x / s, Y0 = y / s (integer division); fx = (float)(x - s X0) / (float)s, fy likewise.
 *   2. Taps k = (X0 + dx, Y0 + dy) in the order (0,0), (1,0), (0,1), (1,1) with the bilinear weights b_k = (1 - fx)(1 - fy),
 *      fx (1 - fy), (1 - fx) fy, fx fy. A tap is a CANDIDATE if b_k > 0 and it lies inside the low-res image; USABLE if it is a
 *      candidate and its working pixel (m_k, e_k, V_k: pt_denoise_var's from S_k, Q_k, albedo_lo_k, spp, batches) is not
 *      pass-through. Tap (0,0) is always a candidate.
 *   3. n_p, z_p from normal_depth_p and n_k, z_k from normal_depth_lo_k, normalised as pt_denoise normalises them.
 *      w_k = b_k max(0, n_p . n_k)^sigma_normal exp(-|z_p - z_k| / (sigma_depth z_p)), formed as pt_denoise_var forms w_n w_z
 *      (one exp2 of sigma_normal log2(n_p . n_k) - |z_p - z_k| (log2(e) / (sigma_depth z_p))); 0 if either normal is zero. A usable
 *      tap whose w_k is not > 0 (0 or NaN) is skipped, never multiplied in: its values may be NaN.
 *   4. W = sum of w_k over the usable, non-skipped taps, in tap order. W >= 1e-4: e = sum w_k e_k / W, V = sum (w_k w_k) V_k / (W W).
 *   5. FALLBACK otherwise: (e_k, V_k) of the usable tap with the largest b_k (the first in tap order wins a tie), bit for bit.
 *   6. PASS-THROUGH if !(albedo_p.w > 0) (nothing hit at display resolution) or if no tap is usable: (m_k.rgb, -1) of the
 *      candidate tap with the largest b_k, the first on ties (m = S / spp, the raw mean).
 * V is a pixel's own variance: neighbouring display pixels share taps, so their errors are correlated and a later filter's
 * sum w^2 V rule understates what it leaves. Arguments are checked before any HIP call: image size, 2 <= scale
 * <= 8 dividing w and h, spp, batches (>= 2, a divisor of spp), NULL pointers, the output overlapping an input, params. Host and
 * device form are bit-identical; the device form is asynchronous on `stream` and needs no workspace. */
typedef struct pt_upsample_params {
    float sigma_normal;          /* exponent on the normals' cosine (finite, >= 0) */
    float sigma_depth;           /* relative depth difference (finite, > 0) */
                                 /* defaults 64, 0.10: DESIGN.md "Render scale" */
} pt_upsample_params;
void pt_upsample_defaults(pt_upsample_params* out);
int pt_camera_scaled(const pt_camera* cam, int scale, pt_camera* out);
int pt_upsample(int w, int h, int scale, const float* rgba_sum_lo, const float* sq_sum_lo, int spp, int batches, const float* albedo_lo,
                const float* normal_depth_lo, const float* albedo, const float* normal_depth, const pt_upsample_params* params,
                float* out_cur);                                                                                 /* host, blocking */
int pt_upsample_device(int w, int h, int scale, const void* d_rgba_sum_lo, const void* d_sq_sum_lo, int spp, int batches,
                       const void* d_albedo_lo, const void* d_normal_depth_lo, const void* d_albedo, const void* d_normal_depth,
                       const pt_upsample_params* params, void* d_out_cur, void* stream);                         /* async */

/* The low-res guide of CENTRE feature buffers (pt_render_aovs_centre) without a second trace: out_lo[Y][X] = in[sY][sX], all four
 * floats, for both buffers; in is w x h float4, out (w / s) x (h / s). For a centre ray (float)(sX) / (float)(sW) and
 * (float)X / (float)W round the same rational and the aspect is the same number, so the result equals
 * pt_render_aovs_centre(pt_camera_scaled(camera, s)) bit for bit. It is NOT the low-res guide of jittered buffers. Arguments are
 * checked before any HIP call: image size, 2 <= scale <= 8 dividing w and h, NULL pointers, and no output may overlap an input or
 * the other output. Host and device form are bit-identical; the device form is asynchronous on `stream`. */
int pt_guide_subsample(int w, int h, int scale, const float* albedo, const float* normal_depth, float* out_albedo_lo,
                       float* out_normal_depth_lo);                                                              /* host, blocking */
int pt_guide_subsample_device(int w, int h, int scale, const void* d_albedo, const void* d_normal_depth, void* d_out_albedo_lo,
                              void* d_out_normal_depth_lo, void* stream);                                        /* async */

/* pt_temporal_accumulate with step 1 replaced: this frame's working pixel (e_cur, V_cur) is read from cur (w*h float4, as
 * pt_upsample writes it) instead of derived from S, Q, spp, batches and albedo. A pixel with !(cur.w >= 0) passes through: it
 * writes (cur.rgb, -1) and length 0. Steps 2-5, the identity path, the aliasing rule and the checks of the size, the cameras,
 * the history pointers and params are pt_temporal_accumulate's. Frames of any render scale blend into one history this way. */
int pt_temporal_accumulate_cur(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* cur, const float* normal_depth,
                               const float* prev_normal_depth, const float* hist, const float* hist_len, const pt_temporal_params* params,
                               float* out_hist, float* out_hist_len);                                            /* host, blocking */
int pt_temporal_accumulate_cur_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_cur,
                                      const void* d_normal_depth, const void* d_prev_normal_depth, const void* d_hist,
                                      const void* d_hist_len, const pt_temporal_params* params, void* d_out_hist, void* d_out_hist_len,
                                      void* stream);                                                             /* async */

/* ---- preview: display bytes on the device, and a session that owns a viewer's buffers ------------------------------
 * pt_resolve: a stateless post-process like pt_denoise*: radiance in, what a viewer shows out. Per pixel p, in f32 with IEEE
 * rounding and no contraction, left to right:
 *   1. n = (float)tile_spp[tile of p] with a tile map (one int32 per 8x8 tile, row-major over the ceil(w/8) x ceil(h/8) grid, as
 *      pt_render_adaptive writes it; the map overrides spp), else n = (float)spp.
 *   2. m.rgb = rgba_p.rgb / n (IEEE division: novum_finalise's, or the per-pixel mean of an adaptive frame); m.w = rgba_p.w.
 *   3. The paint of novum_finalise, in its order: any of m.rgb NaN -> m = (1, 0, 1, 0); then any of m.rgb Inf -> m = (0, 1, 0, 0).
 *   4. mean_p = m (if mean is given): bit for bit novum_finalise(rgba, spp).
 *   5. c = m.rgb * exposure;  with tonemap: c = powf(aces(c), 1.0f / 2.2f), aces(c) = clamp01((c (2.51f c + 0.03f)) /
 *      (c (2.43f c + 0.59f) + 0.14f)): novum_save_bmp's toneMap + gammaCorrect. (The device's powf may differ from the host
 *      libm's in the last bits, so a byte may differ by one code from novum_save_bmp's; without the tone map they are equal.)
 *   6. byte = (unsigned char)(clamp01(c) * 255.0f + 0.5f), 0 for a NaN: novum_save_bmp's.
 *   7. rgba8_p = (r, g, b, 255), four bytes per pixel. Rows and pixels keep the input's order (y = 0 is the bottom row).
 * Arguments are checked before any HIP call: image size, NULL rgba / rgba8, spp >= 1 unless a tile map is given, tonemap 0 or 1,
 * exposure finite and > 0, and no output may overlap an input or the other output. The host form also refuses a tile count
 * <= 0 (-1); the device form trusts the map it is given. Host and device form are bit-identical. params NULL = the defaults. */
typedef struct pt_resolve_params {
    int32_t tonemap;             /* 1: ACES + gamma 2.2 as novum_save_bmp(post_process = 1); 0: clamp and convert only */
    float exposure;              /* linear scale before the tone map (> 0, finite) */
                                 /* defaults 1, 1.0 */
} pt_resolve_params;
void pt_resolve_defaults(pt_resolve_params* out);
int pt_resolve_device(int w, int h, const void* d_rgba, int spp, const void* d_tile_spp /* or NULL */, const pt_resolve_params* params,
                      void* d_rgba8, void* d_mean /* w*h float4, or NULL */, void* stream);                         /* async */
int pt_resolve(int w, int h, const float* rgba, int spp, const int32_t* tile_spp, const pt_resolve_params* params, uint8_t* rgba8,
               float* mean);                                                                                       /* host, blocking */

/* pt_preview: the buffers of one w x h viewer on the current HIP device, and one call per frame that leaves a displayable image
 * there. A frame runs, on the session's own stream and through the public entry points above:
 *   pt_render_moments_device (spp samples in `batches` batches) -> pt_render_aovs_device (aov_spp rays, the beauty's seed) ->
 *   temporal 1: pt_temporal_accumulate_device from the previous good frame's camera, guide and history into the other half of a
 *               ping-pong pair (the guide ping-pongs too; the first frame after create / reset has no history), then
 *               pt_denoise_hist_device on the new history (filter 0: with 0 iterations, i.e. the history's mean a e), then
 *               pt_resolve_device(spp = 1) on that mean;
 *   temporal 0: pt_denoise_var_device on this frame alone, then pt_resolve_device(spp) (filter 0: on the raw sums).
 * So mean, hist and hist_len equal that chain through the host forms bit for bit. A camera whose 112 bytes equal the previous
 * frame's takes pt_temporal_accumulate's identity path. pt_preview_frame blocks until the frame is done (as
 * pt_render_moments_device does); nothing is copied to or from the host. A stage that fails ends the frame with its error and
 * its message: history, guide and previous camera stay those of the last good frame (the ping-pong flips only after every stage
 * was enqueued without error and the stream has synchronised). pt_preview_create checks its arguments before any HIP call
 * (NULL scene, image size, spp, batches >= 2 dividing spp, integrator, aov_spp, temporal / filter 0 or 1, resolve_params) and
 * allocates everything the session owns; temporal_params and filter_params are checked by their stages. The scene must outlive
 * the session and is not to be rendered from another thread during a frame. pt_preview_read copies the last good frame's
 * outputs to the host (any pointer may be NULL; hist / hist_len need temporal 1; -1 before the first frame after create / reset).
 * The device pointers stay valid until destroy; their contents are the last good frame's.
 *
 * RENDER SCALE. pt_preview_set_scale(p, s): s = 1 (the default) is the frame above, bit for bit. s = 2..8 must divide the
 * session's w and h (-1 otherwise, the scale unchanged); the first such call allocates four low-res float4 buffers and one
 * w*h float4 `cur`, a later one grows the low-res buffers if its low-res frame is larger (-2 if that fails, the scale and the
 * buffers unchanged). A scaled frame runs, on the same stream and through the public entry points: pt_camera_scaled ->
 * pt_render_moments_device with the low-res camera -> pt_render_aovs_device with the low-res camera and the beauty's seed ->
 * pt_render_aovs_device with the display camera and the same seed (into the guide half of the ping-pong) -> pt_upsample_device ->
 *   temporal 1: pt_temporal_accumulate_cur_device from the previous good frame's camera, guide and history, then
 *               pt_denoise_hist_device on the new history, then pt_resolve_device(spp = 1);
 *   temporal 0: pt_denoise_hist_device on cur itself (filter 0: with 0 iterations), then pt_resolve_device(spp = 1).
 * History, its lengths, the guide and the previous camera are display-size at every scale, so the scale may change from frame
 * to frame without a reset. A failed scaled frame leaves the session as a failed frame does above. Stats of a scaled frame:
 * render_ms is the low-res moments render, aov_ms both feature passes, accumulate_ms the upsample and the accumulation.
 *
 * GUIDE CHAIN. pt_preview_set_guide_chain(p, max_links): 0 (the default) is the frames above, bit for bit. With 1..16 EVERY
 * feature pass of a frame (the display-size guide, at a render scale above 1 the low-res one too, and a converging frame's) is
 * pt_render_aovs_chain_device(max_links, links NULL) with the same camera, aov_spp and seed in place of pt_render_aovs_device, so
 * the frames equal that chain of host calls. The value may change between frames; a call that CHANGES it resets the session as
 * pt_preview_reset does, because guides from before and after the change do not validate against each other (a call with the
 * current value changes nothing). -1 on a NULL session or a value outside 0..16, the session unchanged.
 *
 * CENTRE GUIDES. pt_preview_set_guide_centre(p, on): 0 (the default) is the frames above, bit for bit. With 1:
 *   - every feature pass is pt_render_aovs_centre_device(display camera, max_links = the guide chain's value, links NULL); aov_spp
 *     and the seed play no part in the guide;
 *   - at a render scale above 1 the low-res guide is pt_guide_subsample_device of the display guide: no low-res trace is launched;
 *   - a frame whose camera's 112 bytes equal the previous good frame's, while a history exists, launches NO feature pass
 *     (converging frames included): the previous good frame's guide is this frame's guide and its previous guide at once. The
 *     stages only read it, and the guide half of the ping-pong does not flip (the history half does). At a scale above 1 the
 *     subsample still runs. If a frame failed in between, the display guide is traced again: same camera, same bits.
 * So a frame equals, bit for bit, the chain of host calls above with pt_render_aovs_centre as the feature pass, pt_guide_subsample
 * for the low-res guide, and the previous guide passed as both guides on such a resting frame. A call that CHANGES the value
 * resets the session as pt_preview_reset does (a call with the current value changes nothing); -1 on a NULL session or a value
 * other than 0 or 1, the session unchanged. The failed-frame rule is unchanged. aov_ms covers the trace and the subsample and is
 * about 0 on a frame that reuses its guide. pt_preview_guide_passes: the feature-pass launches of all good frames since create
 * (with or without centre guides; a failed frame's are not counted, a subsample is none).
 *
 * CHANGED SCENE. pt_preview_scene_changed(p, keep_history) tells the session that the scene was updated (pt_scene_update_*)
 * since its last good frame. The next frame is then treated like a moved camera, whatever the camera's bytes say: it renders
 * every tile (no converging frame; pt_preview_last_live reports live == total) and traces its guide again (centre guides do
 * not reuse the previous guide; pt_preview_guide_passes counts the pass). keep_history 0 additionally resets the session as
 * pt_preview_reset does: the frame equals the first frame of a fresh session on a fresh scene of the new arrays, bit for bit.
 * keep_history 1 accumulates through the public entry points as usual: the previous guide is the old geometry's, a camera
 * whose 112 bytes are unchanged takes pt_temporal_accumulate's identity path, whose tap is still validated by depth and
 * normal, and the frame equals that chain of host calls bit for bit. Without motion vectors (MOTION below, off by default) a
 * surface that moved keeps its history only where depth and normal still agree at the same pixel. With respond on (RESPOND
 * below, off by default) keep_history 1 is also right when a light moved: a static surface whose lighting changed shortens its
 * own history. A session also remembers
 * pt_scene_generation from its last good frame (from create before the first): if the generation differs at pt_preview_frame
 * and this call was not made since that frame, the session behaves as if it had been made with keep_history 0. The
 * announcement holds until the next good frame. -1 on a NULL session or a keep_history other than 0 or 1.
 *
 * MOTION. pt_preview_set_motion(p, on): 0 (the default) is the frames above, bit for bit. The first call that turns it on allocates
 * one w*h float4 buffer M (-2 if that fails, the state unchanged); -1 on a NULL session or a value other than 0 or 1. Changing the
 * value does not reset the session: the guides do not depend on it. With 1, a frame is a MOTION FRAME if the session is temporal, a
 * history exists, pt_preview_scene_changed(p, 1) was called since the last good frame, pt_scene_generation equals the last good
 * frame's + 1 and pt_scene_has_motion(scene) is 1. Such a frame runs as above, and
 *   - after the display-size guide pass it runs pt_render_motion_device(display camera, NULL, NULL, M); with centre guides and guide
 *     chain 0 ONE pt_render_motion_device(display camera, A, N, M) replaces the display-size guide pass;
 *   - its accumulation is pt_temporal_accumulate_motion_device (scale 1) or pt_temporal_accumulate_cur_motion_device (scale > 1)
 *     with M;
 * so it equals that chain of host calls bit for bit. aov_ms includes the motion pass and pt_preview_guide_passes counts it as one
 * pass. Every other frame is unchanged: a generation that jumped by more than one, keep_history 0, an unannounced change, a
 * converging frame. The failed-frame rule holds. pt_render_motion is first hit only; MOTION CHAIN follows mirrors and glass.
 *
 * MOTION CHAIN. pt_preview_set_motion_chain(p, on): 0 (the default) is the frames above, bit for bit; -1 on a NULL session or a value
 * other than 0 or 1. Changing the value does not reset the session and allocates nothing. With 1, a MOTION FRAME (as defined above:
 * it needs pt_preview_set_motion(p, 1) as before) of a session whose guide chain is > 0 runs
 * pt_render_motion_chain_device(display camera, max_links = the guide chain) where it ran pt_render_motion_device: after the
 * display-size guide pass with the guide outputs NULL; with centre guides ONE pt_render_motion_chain_device(display camera,
 * max_links, A, N, NULL, M) replaces the display-size guide pass (its guide outputs are pt_render_aovs_centre_device's, bit for
 * bit). A session with guide chain 0 is unaffected by the switch. aov_ms, pt_preview_guide_passes (the fused pass counts as one),
 * the failed-frame rule, converging frames and respond compose as for motion frames above. */
typedef struct pt_preview pt_preview;
typedef struct pt_preview_params {
    int32_t spp, batches, max_depth, integrator, use_mis, aov_spp;
    int32_t temporal;            /* 1: accumulate + pt_denoise_hist; 0: pt_denoise_var on this frame alone */
    int32_t filter;              /* 0: no spatial filter (temporal 1: the history's mean a e; temporal 0: the raw mean) */
    pt_temporal_params temporal_params;
    pt_denoise_var_params filter_params;
    pt_resolve_params resolve_params;
                                 /* defaults 4, 2, 8, 0, 1, 1, 1, 1 and the three libraries' defaults */
} pt_preview_params;
typedef struct pt_preview_stats {
    int32_t frames;              /* good frames since create */
    float render_ms, aov_ms, accumulate_ms, filter_ms, resolve_ms, total_ms;   /* the last good frame: HIP events on the session's
                                    stream around each stage (render_ms includes pt_render_moments_device's per-batch waits) */
} pt_preview_stats;
void pt_preview_defaults(pt_preview_params* out);
pt_preview* pt_preview_create(pt_scene* scene, int w, int h, const pt_preview_params* params);   /* NULL on error: pt_last_error() */
int  pt_preview_frame(pt_preview* p, const pt_camera* camera, uint64_t seed);
int  pt_preview_reset(pt_preview* p);                                      /* the next frame is a first frame */
int  pt_preview_scene_changed(pt_preview* p, int keep_history);            /* the scene was updated: see CHANGED SCENE */
int  pt_preview_set_scale(pt_preview* p, int scale);                       /* 1..8: the render scale of the frames that follow */
int  pt_preview_scale(pt_preview* p);                                      /* the current scale; -1 on a NULL session */
int  pt_preview_set_guide_chain(pt_preview* p, int max_links);             /* 0..16: the feature passes of the frames that follow */
int  pt_preview_guide_chain(pt_preview* p);                                /* the current value; -1 on a NULL session */
int  pt_preview_set_guide_centre(pt_preview* p, int on);                   /* 0 or 1: centre guides for the frames that follow */
int  pt_preview_guide_centre(pt_preview* p);                               /* the current value; -1 on a NULL session */
int  pt_preview_set_motion(pt_preview* p, int on);                         /* 0 or 1: motion frames, see MOTION */
int  pt_preview_motion(pt_preview* p);                                     /* the current value; -1 on a NULL session */
int  pt_preview_set_motion_chain(pt_preview* p, int on);                   /* 0 or 1: motion frames follow the guide chain, see MOTION CHAIN */
int  pt_preview_motion_chain(pt_preview* p);                               /* the current value; -1 on a NULL session */
int  pt_preview_guide_passes(pt_preview* p);                               /* feature-pass launches of the good frames; -1 on NULL */
int  pt_preview_read(pt_preview* p, uint8_t* rgba8, float* mean, float* hist, float* hist_len);
const void* pt_preview_device_rgba8(pt_preview* p);                        /* w*h*4 bytes */
const void* pt_preview_device_mean(pt_preview* p);                         /* w*h float4 */
int  pt_preview_last_stats(pt_preview* p, pt_preview_stats* out);
void pt_preview_destroy(pt_preview* p);

/* ---- converge: a resting viewer stops sampling the 8x8 tiles whose history has converged ---------------------------------------
 * Three stateless stages and the session's switch for them. Tiles are the 8x8 tiles of pt_tile_range, row-major over the
 * ceil(w/8) x ceil(h/8) grid; T is their number. All arithmetic is f32 with IEEE rounding (division and sqrtf included) and no
 * contraction, left to right.
 *
 * pt_temporal_select: which tiles of a history (pt_temporal_accumulate's hist and hist_len) still need samples. Per in-image
 * pixel p of tile t:
 *   p is EXEMPT if hist_p.w < 0 or any of hist_p's four values is NaN / Inf (pt_denoise_hist's pass-through rule): r_p = 0 and
 *   p is never young, so it never holds its tile back (as a non-finite pixel never holds a tile of pt_render_adaptive back).
 *   Otherwise lum = 0.2126f e.r + 0.7152f e.g + 0.0722f e.b (pt_denoise's constants on hist_p.rgb) and
 *     r_p = sqrtf(V) / (1e-4f + sqrtf(lum))     with V = hist_p.w: the standard error of the mean over the root of the mean, the
 *   shape of pt_render_adaptive's estimator; a NaN r_p (lum < 0) counts as 0. p is YOUNG if hist_len_p < (float)min_history.
 *   E_t = max(0, r_p over the tile's in-image pixels). The tile is LIVE unless E_t < threshold and none of its pixels is young.
 * Outputs: out_tile_err[t] = E_t (T floats), out_tile_live[t] = 1 or 0 (T int32), out_list = the live tiles in ascending order
 * (room for T int32; the device form leaves the entries past the count as they were, the host form returns them as 0) and
 * *out_count = their number. threshold 0 keeps every tile live. Host and device form are bit-identical, and a float maximum does
 * not depend on its order, so the numpy restatement (tests/converge_ref.py) is exact as well. Arguments are checked before any
 * HIP call: image size, NULL pointers, params, and no output may overlap an input or another output. The device form is
 * asynchronous on `stream`; it needs no workspace from the caller (the library keeps one constant tile list per device and
 * process, and waits for `stream` once when that list has to grow). params NULL = pt_converge_defaults. */
typedef struct pt_converge_params {
    float threshold;             /* a tile stops when E_t < threshold; 0 = never (every tile live); NaN / < 0 / Inf rejected */
    int32_t min_history;         /* no tile stops while one of its filtered pixels has fewer frames (>= 1) */
                                 /* defaults 0.5, 8: DESIGN.md "Converged tiles" */
} pt_converge_params;
void pt_converge_defaults(pt_converge_params* out);
int pt_temporal_select(int w, int h, const float* hist, const float* hist_len, const pt_converge_params* params, float* out_tile_err,
                       int32_t* out_tile_live, int32_t* out_list, int32_t* out_count);                             /* host, blocking */
int pt_temporal_select_device(int w, int h, const void* d_hist, const void* d_hist_len, const pt_converge_params* params, void* d_tile_err,
                              void* d_tile_live, void* d_list, void* d_count, void* stream);                       /* async */

/* pt_render_moments_tiles: pt_render_moments on a list of tiles. A pixel's stream is keyed by the pixel alone, so the pixels
 * of the listed tiles get S and Q equal to pt_render_moments' bit for bit; every other pixel gets S = 0 and Q.rgb = 0; Q.w =
 * (float)B everywhere. count 0 launches no render and writes that zero frame. The host form takes a host list and refuses one
 * that is not strictly ascending within 0..T-1 (-1); the device form takes a device list and the host-known count and trusts
 * the list's contents (as pt_resolve_device trusts its map). count outside 0..T: -1. The megakernel only: with the wavefront
 * variant selected the call fails with -1 and leaves the outputs untouched (list mode needs the tile queue, as
 * pt_render_adaptive does); every launch uses the tile queue whatever the "persistent" option says. After every batch the host
 * waits and checks the queue's words as pt_render_moments does: an unfinished listed tile fails the call with -4 and no further
 * batch is launched. The scene's work buffers stay sized for the whole frame. Checks before any HIP call: image size, count and
 * list, then pt_render_moments', then the variant. */
int pt_render_moments_tiles(pt_scene* scene, const pt_camera* camera, int w, int h, int spp, int batch_spp, int max_depth, int integrator,
                            int use_mis, uint64_t seed, const int32_t* tile_list, int count, float* out_rgba_sum,
                            float* out_sq_sum);                                                                    /* host buffers */
int pt_render_moments_tiles_device(pt_scene* scene, const pt_camera* camera, int w, int h, int spp, int batch_spp, int max_depth,
                                   int integrator, int use_mis, uint64_t seed, const void* d_tile_list, int count, void* d_rgba_sum,
                                   void* d_sq_sum, void* stream);                                                  /* device buffers */

/* pt_temporal_accumulate_live: pt_temporal_accumulate with a map of live tiles (T int32, as pt_temporal_select writes it). A NULL
 * map means every tile live: pt_temporal_accumulate bit for bit. A map is accepted only on the identity path with a history
 * (cam_prev NULL or its 112 bytes equal to cam's, and the three history pointers set), -1 otherwise: a carried pixel has no
 * sample of its own, so it can only keep what it had at the same place. In a tile whose entry is 0, out_hist_p = hist_p and
 * out_hist_len_p = hist_len_p bit for bit, and S, Q and albedo are not read there: the length counts frames BLENDED, so a
 * carried pixel does not age. In every other tile: pt_temporal_accumulate's result bit for bit. The outputs must not overlap the
 * map. Everything else (checks, aliasing rule, params) is pt_temporal_accumulate's. */
int pt_temporal_accumulate_live(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* rgba_sum, const float* sq_sum,
                                int spp, int batches, const float* albedo, const float* normal_depth, const float* prev_normal_depth,
                                const float* hist, const float* hist_len, const int32_t* tile_live, const pt_temporal_params* params,
                                float* out_hist, float* out_hist_len);                                             /* host, blocking */
int pt_temporal_accumulate_live_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_rgba_sum,
                                       const void* d_sq_sum, int spp, int batches, const void* d_albedo, const void* d_normal_depth,
                                       const void* d_prev_normal_depth, const void* d_hist, const void* d_hist_len, const void* d_tile_live,
                                       const pt_temporal_params* params, void* d_out_hist, void* d_out_hist_len, void* stream);  /* async */

/* The session's switch. pt_preview_set_converge(p, params): NULL or threshold 0 turns it off; off is the default, and an off
 * session is the session above bit for bit. The first call that turns it on allocates the session's tile buffers (-2, with the
 * state unchanged, if that fails); params are checked as pt_temporal_select checks them (-1, the state unchanged).
 * A frame CONVERGES only if converge is on, the session is temporal, the scale is 1, a history exists and the camera's 112 bytes
 * equal the previous good frame's. Every other frame (a moved camera, a scale above 1, the first frame after create or reset,
 * temporal 0) renders every tile exactly as above and reports live == total. A converging frame runs, on the session's stream
 * and through the public entry points:
 *   pt_temporal_select_device on the current history -> one 4-byte read-back of the count -> pt_render_moments_tiles_device
 *   (skipped if the count is 0) -> pt_render_aovs_device on the full frame (the guide stays whole) ->
 *   pt_temporal_accumulate_live_device -> pt_denoise_hist_device -> pt_resolve_device(spp = 1),
 * so its results equal that chain of host calls bit for bit. The failed-frame rule holds unchanged: history, guide, camera, the
 * tile map and the live count flip only after every stage was enqueued without error and the stream has synchronised.
 * pt_preview_stats keeps its layout: render_ms of a converging frame includes the select stage and the read-back.
 * pt_preview_last_live: the live and total tile counts of the last good frame (-1 before the first). pt_preview_read_tiles: E_t
 * and the live map of the last converging frame (either pointer may be NULL; T entries each; -1 before the first converging
 * frame since create / reset). */
int  pt_preview_set_converge(pt_preview* p, const pt_converge_params* params);
int  pt_preview_last_live(pt_preview* p, int* live, int* total);
int  pt_preview_read_tiles(pt_preview* p, float* tile_err, int32_t* tile_live);

/* ---- adaptive frames with their variance; the variance-guided denoiser on a tile map ------------------
 * pt_render_adaptive_moments: pt_render_adaptive plus the second moment that pt_render_moments keeps. The schedule, the
 * estimator, the live lists, the checks, the -4 / stall handling and the megakernel-only rule are pt_render_adaptive's, and
 * out_rgba_sum, out_tile_spp, out_tile_err and stats are bit-identical to pt_render_adaptive's for the same arguments.
 * One more argument check, after pt_render_adaptive's checks of params and before any HIP call: max_spp must be a multiple of
 * 2 * chunk_spp (-1), so that every half-round renders exactly c = chunk_spp samples: a half-round is a batch of
 * pt_render_moments, and batches of unequal size would make pt_denoise_var's variance formula wrong. A NULL out_sq_sum: -1.
 * Q. All arithmetic is f32 with IEEE rounding and no contraction, the product rounded before the add. After each of a round's
 * two launches, per pixel of a live tile and per rgb channel: d = S - P, Q = Q + d d, P = S (P and Q start at 0). A tile that
 * stops with tile_spp = n therefore holds, over its in-image pixels, S and Q.rgb bit-identical to
 * pt_render_moments(spp = n, batch_spp = c), and Q.w = (float)(n / c): the batches of that tile. NaN / Inf propagate into Q.
 * out_sq_sum: w*h float4 scan-line like out_rgba_sum. This call WRITES both; it never touches the counters, and a later
 * pt_render of the same scene is unaffected. pt_render_adaptive itself launches exactly what it launched before. */
int pt_render_adaptive_moments(pt_scene* scene, const pt_camera* camera, int w, int h, int max_depth, int integrator, int use_mis,
                               uint64_t seed, const pt_adaptive_params* params, float* out_rgba_sum, float* out_sq_sum,
                               int32_t* out_tile_spp, float* out_tile_err, pt_adaptive_stats* stats);           /* host buffers */
int pt_render_adaptive_moments_device(pt_scene* scene, const pt_camera* camera, int w, int h, int max_depth, int integrator,
                                      int use_mis, uint64_t seed, const pt_adaptive_params* params, void* d_rgba_sum,
                                      void* d_sq_sum, void* d_tile_spp, void* d_tile_err, pt_adaptive_stats* stats,
                                      void* stream);                                                             /* device buffers */

/* pt_denoise_var_tiles: pt_denoise_var on such a frame. The contract is pt_denoise_var's except that the sample count and the
 * batch count are per pixel, from the frame's tile map (one int32 per tile, as pt_render_adaptive* writes it and pt_resolve
 * reads it):
 *   spp_p = tile_spp[(y / 8) * ceil(w / 8) + x / 8],   B_p = spp_p / batch_spp   (integer; Q.w is not read)
 *   m_p = S_p / spp_p; var_c and V_p as in pt_denoise_var with B_p and spp_p in place of B and spp.
 * L, the pass-through rule, the 3x3 prefilter, the weights and the iterations are pt_denoise_var's (the same iteration kernel).
 * Output: rgb = spp_p a_p e_p, w = S_p.w, in the units of the input, so pt_resolve(tile_spp = the map) applies unchanged; out
 * may alias rgba_sum. With a map whose entries all equal spp the result is bit-identical to pt_denoise_var(spp, batches = spp /
 * batch_spp), in the host and the device form, which are bit-identical to each other.
 * Checks before any HIP call: pt_denoise_var's (image size, NULL buffers, params), batch_spp >= 1, a NULL map. The host form
 * also refuses (-1) a map entry that is <= 0, no multiple of batch_spp, or smaller than 2 * batch_spp (B_p >= 2); the device
 * form trusts the map, as pt_resolve_device does. Workspace: pt_denoise_var_device's size and layout. */
size_t pt_denoise_var_tiles_workspace_bytes(int w, int h);
int pt_denoise_var_tiles(int w, int h, const float* rgba_sum, const float* sq_sum, const int32_t* tile_spp, int batch_spp,
                         const float* albedo, const float* normal_depth, const pt_denoise_var_params* params,
                         float* out_rgba_sum);                                                                     /* host, blocking */
int pt_denoise_var_tiles_device(int w, int h, const void* d_rgba_sum, const void* d_sq_sum, const void* d_tile_spp, int batch_spp,
                                const void* d_albedo, const void* d_normal_depth, const pt_denoise_var_params* params,
                                void* d_workspace, void* d_out, void* stream);                                     /* async */

/* ---- probes: single stages of the path on the GPU, for known-answer tests -------------- */
int pt_probe_rng(uint64_t seed, int n, const uint32_t* subsequences, int n_draws, uint32_t* out_state6, uint32_t* out_u32, float* out_uniform);
/* The bookkeeping pass of pt_render_adaptive_moments alone: on the first `live` tiles (1..T) of a w x h frame's buffers, one
 * warm-up launch, then `reps` launches between two HIP events; *out_ms = their mean time in milliseconds. For tools. */
int pt_probe_adaptive_moments(int w, int h, int live, int reps, float* out_ms);
int pt_probe_math(int n, const float* x, float* out_sin, float* out_cos, float* out_exp, float* out_rsqrt, float* out_pow5);
/* All 2^32 binary32 inputs through the kernels' exact fast reciprocal (v_rcp_f32 + one Newton step inside 1e-12 <= |a| <= 1e30,
 * the IEEE division outside) against the IEEE division it stands for (`f = 1.0 / a`, integratorUtilities.cuh:22; 1 / dir, :50-55;
 * rsqrtf, util.cuh:129). out3[0] = inputs whose results differ (the arithmetic contract needs 0 on the device at hand),
 * out3[1] = inputs inside the fast range, out3[2] = inputs outside it where the bare fast sequence would be wrong (the reason
 * for the range guard). first_bad (may be NULL): the lowest differing bit pattern, 0xffffffff if none. ~0.1 s. */
int pt_probe_rcp_exhaustive(unsigned long long* out3, uint32_t* first_bad);
int pt_probe_camera_rays(const pt_camera* camera, uint64_t seed, int n, const int32_t* xy, float* out_rays6);
/* The centre rays of pt_render_aovs_centre for n pixels xy = (x0, y0, x1, y1, ...): o.xyz, d.xyz per ray. No seed: none is read. */
int pt_probe_centre_rays(const pt_camera* camera, int n, const int32_t* xy, float* out_rays6);
/* rays: n x 6 floats. out_i: n x 4 (valid, triIDX, materialID, backface);
 * out_f: n x 12 (t,u,v, point xyz, normal xyz, uv xy, 0); counters: summed over the n rays. */
int pt_probe_trace_closest(pt_scene* scene, int n, const float* rays6, int32_t* out_i, float* out_f, pt_counters* counters);
int pt_probe_trace_shadow(pt_scene* scene, int n, const float* rays6, const float* max_t, float* out_throughput3, pt_counters* counters);
/* sample_f_eval on stream (seed, subseq): out 8 floats (wo xyz, f xyz, pdf, draws) */
int pt_probe_bsdf_sample(pt_scene* scene, int n, const int32_t* material, const float* wi3, const int32_t* backface,
                         float etaI, float etaT, uint64_t seed, const uint32_t* subseq, float* out8);
/* f_eval + pdf_eval: out 4 floats (f xyz, pdf) */
int pt_probe_bsdf_eval(pt_scene* scene, int n, const int32_t* material, const float* wi3, const float* wo3,
                       float etaI, float etaT, float* out4);

/* ---- f-4: BVH build on the device --------------------------------------------------------
 * Replaces computeInfoForBVH + buildBVH (main.cu:20-233; call site main.cu:524-530: host vectors
 * `bvhvec` / `indvec` out of `points` / `mesh`). PT_BVH_REFERENCE_TREE: the nodes (pre-order, as
 * nodes.size() numbers them, main.cu:137) and the BVHindices permutation are byte-identical to the
 * host builder's. Host pointers in and out; nodes_out needs room for 2*n_triangles-1 nodes.
 * Returns the node count (> 0) or a negative error (pt_last_error()). No CPU fallback: without a
 * HIP device it fails; novum_bvh_build_host is the kept host builder on the same arrays. */
#define PT_BVH_REFERENCE_TREE 0
typedef struct pt_bvh_build_stats {
    int32_t n_nodes, largest_leaf, backups, depth;   /* what main.cu:537-538 prints */
    int32_t sort_fallbacks, levels;
    float device_ms;                                 /* HIP events around the build kernels */
    float total_ms;                                  /* wall clock incl. allocation, upload, download */
} pt_bvh_build_stats;
int pt_bvh_build_device(const pt_float4* positions, int n_positions, const pt_triangle* triangles, int n_triangles,
                        int max_leaf_size, int mode, pt_bvh_node* nodes_out, int nodes_capacity,
                        int32_t* indices_out, pt_bvh_build_stats* stats);
/* The same, without leaving the device: builds the reference tree from desc->positions / triangles (desc->bvh and
 * desc->bvh_indices are ignored and may be NULL) and lays out the traversal records there — what main.cu:524-557
 * (buildBVH + uploads) becomes when the geometry is large. The scene renders exactly like one made by
 * pt_scene_create from the host-built tree. */
pt_scene* pt_scene_create_from_mesh(const pt_scene_desc* desc, int max_leaf_size, pt_bvh_build_stats* stats);
/* Test hook: copy the packed traversal records back (what: 0 nodes 64 B, 1 triangles 48 B, 2 attributes 80 B,
 * 3 lights 64 B,
 * 4 materials 96 B); returns the record count. */
int pt_debug_packed(pt_scene* scene, int what, void* dst, size_t capacity_bytes);

/* ---- dynamic geometry: in-place updates of a scene, the reference's tree rebuilt on the device -------------------
 * pt_scene_update_mesh: replace the scene's mesh, materials, lights and textures by desc's and rebuild the reference tree on
 * the device (desc->bvh / bvh_indices are not read), as pt_scene_create_from_mesh(desc, max_leaf_size) would. It accepts any
 * scene, one made by pt_scene_create from a caller's BVH included, which becomes a device-built scene.
 * pt_scene_update_vertices: topology, materials, the lights' triangles and textures unchanged; new vertex positions and,
 * optionally, new normals (normals NULL = keep the scene's; n_normals is then ignored). n_positions / n_normals must equal the
 * scene's. Host arrays; the _device form takes device arrays of the same layout on the scene's device and uploads nothing.
 * Both need a scene that went through the device builder — made by pt_scene_create_from_mesh, or updated once by
 * pt_scene_update_mesh — because only such a scene knows its leaf size and keeps device copies of its triangles, normals,
 * uvs, material types and light triangles: -1 with a message otherwise. This is the per-frame path: the builder's pool
 * belongs to the scene (grown on demand, freed by pt_scene_destroy), the light records are recomputed on the device, and
 * only the renumbering of the internal nodes by area for scenes in HBM still passes through the host, as at creation.
 * stats (may be NULL): the builder's, as pt_scene_create_from_mesh fills them; total_ms is the whole call's wall clock.
 *
 * EQUIVALENCE. After a successful update every entry point that takes the scene — the renders, _counted, both variants,
 * adaptive, moments (fused and batched), the feature passes, the probes, pt_scene_flags — gives results bit-identical to a
 * fresh pt_scene_create_from_mesh of the new arrays with the same options, variant and culling applied. The packed
 * triangles, attributes and lights are byte-identical and the packed tree is the same tree; what creation derives from them
 * (which kernels the scene qualifies for, the leaf table, the lights' triangles, the LDS cache split, the stack need and
 * the spill sizes that follow from it) is derived again by the same code.
 * KEPT: option values (pt_get_option), variant and culling; the sums of pt_get_counters; pt_queue_stalls; the work buffers.
 * ATOMICITY. Arguments are checked on the host before any HIP call (NULL pointers, counts, for the vertex forms the counts
 * against the scene's). The build goes into spare node / triangle / attribute / light buffers that are swapped in on
 * success. A failed update returns the builder's error (a non-finite position, an index out of range, a tree deeper than
 * 128) and leaves the scene rendering bit for bit what it rendered before.
 * ORDERING. An update is a frame boundary: it waits for the device's outstanding work on entry and is complete on return;
 * no launch on the scene may be in flight on another thread, and device arrays passed to the _device form must not be
 * written until the call returns. pt_scene_generation: 0 after create, +1 per successful update; -1 on NULL.
 * Multi-GPU replicas (pt_multi_*) are not updated: out of scope. */
int pt_scene_update_mesh(pt_scene* scene, const pt_scene_desc* desc, int max_leaf_size, pt_bvh_build_stats* stats);
int pt_scene_update_vertices(pt_scene* scene, const pt_float4* positions, int n_positions,
                             const pt_float4* normals, int n_normals, pt_bvh_build_stats* stats);
int pt_scene_update_vertices_device(pt_scene* scene, const void* d_positions, int n_positions,
                                    const void* d_normals, int n_normals, pt_bvh_build_stats* stats);
int pt_scene_generation(pt_scene* scene);

/* ---- material and emission edits: the look of a live scene changed in place, nothing rebuilt ------------------------------------
 * pt_scene_update_materials: the scene's description with its material table replaced by `materials`. n_materials must equal the
 * scene's (-1 otherwise: the number of materials does not change). Texture windows are checked against the scene's texel count
 * exactly as creation checks them. The triangles' materialIDs, the textures and everything else stay.
 * pt_scene_update_emission: for each k < n, with li = light_indices[k] in 0..n_lights-1, the description has lights[li].emission =
 * emission[k] and every triangle whose lightInd == li has that emission; a repeated index takes its last entry. The set of lights
 * does not change: a light set to (0, 0, 0) stays in the light list, as it would in a fresh scene of that description, and turning a
 * triangle that is no light into one stays pt_scene_update_mesh's job. n = 0 edits nothing and still counts as an edit.
 * Both are host, blocking calls on ANY scene, one made by pt_scene_create from a caller's BVH included: the edit runs on the packed
 * records, on the device, one thread per triangle. A device-built scene additionally refreshes what its next
 * pt_scene_update_vertices packs from (the material types; the emission of its kept triangles and light triangles).
 *
 * EQUIVALENCE, as for the updates above: after a successful call every entry point that takes the scene gives results bit-identical
 * to a fresh scene of the edited description — pt_scene_create_from_mesh for a device-built scene, pt_scene_create for one made from
 * a caller's BVH — with the same options, variant and culling. The packed triangles, attributes, lights and materials are
 * byte-identical to the fresh scene's, and so are pt_scene_flags before and after a launch and the choice of kernel: which kernel
 * family the scene qualifies for (SIMPLE, LEAN, the pair form's "no leaf triangle", a material type without a dispatch arm) is
 * decided again from scratch, so a diffuse box turned into a mirror leaves the SIMPLE kernels and comes back with the edit undone.
 * KEPT: everything the updates above keep, and the tree, the leaf table, the lights' triangles and the LDS cache split, which no
 * material or emission decides and which are neither read nor rebuilt.
 * GENERATION AND MOTION. A successful call adds 1 to pt_scene_generation and makes pt_scene_has_motion 0 until the next vertex
 * update: the previous positions describe a step the viewer has already seen, and a session must not reproject through them again.
 * The position buffers are kept; only the flag drops. So a frame preceded by a vertex update AND THEN an edit is no motion frame.
 * ATOMICITY. All arguments are checked on the host before any HIP call (NULL pointers, counts, light indices, texture windows); a
 * refused call returns -1 with a message that names the function and leaves the scene rendering bit for bit what it rendered. After
 * the checks nothing can fail but HIP itself. ORDERING: a frame boundary, exactly as for the updates above. */
int pt_scene_update_materials(pt_scene* scene, const pt_material* materials, int n_materials);
int pt_scene_update_emission(pt_scene* scene, int n, const int32_t* light_indices, const pt_float4* emission);

/* ---- motion: where a moved surface was, and a history stage that looks there ---------------------------------------------------
 * PREVIOUS POSITIONS. A device-built scene keeps two device arrays of n_positions pt_float4 (32 B per vertex): the current positions
 * and the positions before the most recent successful pt_scene_update_vertices[_device]. pt_scene_create_from_mesh uploads the
 * positions once: there are no previous ones yet. A successful vertex update copies its positions into the spare array and the pair
 * rotates, so a steady animation allocates nothing; a failed update touches neither. pt_scene_update_mesh keeps the new positions
 * and drops the previous ones (the topology may have changed). A pt_scene_create scene keeps none.
 * pt_scene_has_motion: 1 if previous positions exist (the last successful update was a vertex update), 0 otherwise, -1 on NULL.
 *
 * pt_render_motion: per pixel (x, y) the ray is pt_render_aovs_centre's centre ray (antiAliasJitterDist and aperture ignored, no
 * seed, no RNG stream) and the hit its closest hit (max_t 999999). out_motion is w*h float4, scan-line, y = 0 the bottom row. In
 * f32, every operation rounded once, left to right, nothing fused:
 *   no hit: (0, 0, 0, 0).
 *   STATIC, (0, 0, 0, 0): the scene has no previous positions; or, with tri the hit's original triangle index, (ia, ib, ic) its
 *     aInd, bInd, cInd in the scene's kept triangles, A, B, C the current and A', B', C' the previous positions at those indices,
 *     all nine floats of A, B, C compare equal (==) to those of A', B', C' (positions are finite: the builder refuses others).
 *   MOVED otherwise: bz = 1 - u - v (the hit's barycentrics, as the attribute interpolation forms it);
 *     P'.c = A'.c bz + B'.c u + C'.c v per component; the pixel is (P'.x, P'.y, P'.z, 1): where the point the ray hits was before
 *     the update.
 * out_albedo and out_normal_depth must be both NULL or both set (-1 otherwise); when set they are bit-identical, in all eight
 * floats, to pt_render_aovs_centre(max_links = 0): one trace serves the guide and the motion. The pass is FIRST HIT ONLY: a moved
 * object seen through a mirror or through glass reports the static mirror or pane in front of it, and so takes the path without
 * motion; pt_render_motion_chain (below) is the pass that follows the ray to the object. Like the other feature passes this one touches no RNG state, accumulator or counter of the scene. Arguments are checked
 * before any HIP call: those of pt_render_aovs_centre, the guide outputs both or neither, and out_motion not NULL. */
int pt_scene_has_motion(pt_scene* scene);
int pt_render_motion(pt_scene* scene, const pt_camera* camera, int w, int h, float* out_albedo /* NULL ok */,
                     float* out_normal_depth /* NULL ok */, float* out_motion);                                   /* host, blocking */
int pt_render_motion_device(pt_scene* scene, const pt_camera* camera, int w, int h, void* d_albedo /* NULL ok */,
                            void* d_normal_depth /* NULL ok */, void* d_motion, void* stream);                    /* async */

/* pt_render_motion_chain: motion through mirrors and glass, for sessions whose guides follow them (pt_render_aovs_centre with
 * max_links > 0). The ray is pt_render_aovs_centre's centre ray and the chain pt_render_aovs_chain's: its link rule, direction
 * arithmetic and fallback, max_links 0..16. out_albedo, out_normal_depth and out_links, when set, are bit-identical to
 * pt_render_aovs_centre(max_links) in all eight floats and in links; albedo and normal_depth must be both set or both NULL, and
 * out_links needs them set (-1 otherwise). max_links = 0 is pt_render_motion bit for bit in every output.
 * out_motion, w*h float4, in f32, every operation rounded once, left to right, nothing fused:
 *   no hit, or the scene has no previous positions: (0, 0, 0, 0).
 *   A ray whose result is its FIRST HIT (a non-specular first hit; the fallback where the chain leaves the scene or reaches the
 *     cap, links = 0): pt_render_motion's pixel for that hit, bit for bit.
 *   A ray whose chain ended on a non-specular surface after L >= 1 links:
 *     (0, 0, 0, 0) if the triangle of ANY of the L specular hits on the way MOVED (pt_render_motion's nine-float test on that
 *       triangle): a moving mirror changes the whole reflection, and the pixel stays on the path without motion;
 *     (0, 0, 0, 0) if the final triangle is STATIC by the same test;
 *     otherwise, with P' pt_render_motion's barycentric sum of the final triangle's previous positions at the final hit's u, v and
 *       bz = 1 - u - v, and P the final hit's point as pt_probe_trace_closest reports it: D.c = P'.c - P.c.
 *       UNFOLDING. A 3x3 M starts as the identity. At each link that REFLECTED (a mirror, or a dielectric's total internal
 *       reflection), in link order, with n the hit's normal at that link as pt_probe_trace_closest reports it, every row r becomes
 *         s = 2 * (M[r].x n.x + M[r].y n.y + M[r].z n.z);  M[r].c = M[r].c - s * n.c
 *       and a link that REFRACTED leaves M unchanged (a deliberate simplification: a pane shifts the image, it does not mirror it).
 *       Du.r = M[r].x D.x + M[r].y D.y + M[r].z D.z: the displacement reflected through the last mirror first.
 *       V.c = o.c + d.c * depth, (o, d) the centre ray and depth the chain's summed path length (the guide's w): for planar
 *       mirrors the virtual image of P. The pixel is (V.x + Du.x, V.y + Du.y, V.z + Du.z, 1): the virtual image of P'.
 * pt_temporal_accumulate[_cur]_motion and pt_temporal_accumulate_respond take this buffer as they take pt_render_motion's: they
 * reproject any point whose w is 1. Still out of scope: moving mirrors (zero, above), the image shift of a refraction, a
 * previous-normal transform, pt_multi_* replicas. Like every feature pass this one touches no RNG state, accumulator or counter
 * of the scene; it needs a device-built scene exactly where pt_render_motion does (any other scene is static). All arguments are
 * checked before any HIP call, -1 with a message that names pt_render_motion_chain: max_links, the guide outputs, out_links,
 * out_motion, the size, the camera and its size, then the scene. */
int pt_render_motion_chain(pt_scene* scene, const pt_camera* camera, int w, int h, int max_links, float* out_albedo /* NULL ok */,
                           float* out_normal_depth /* NULL ok */, float* out_links /* NULL ok */, float* out_motion);   /* host, blocking */
int pt_render_motion_chain_device(pt_scene* scene, const pt_camera* camera, int w, int h, int max_links, void* d_albedo /* NULL ok */,
                                  void* d_normal_depth /* NULL ok */, void* d_links /* NULL ok */, void* d_motion, void* stream); /* async */

/* pt_temporal_accumulate / pt_temporal_accumulate_cur with a motion buffer (w*h float4, as pt_render_motion writes it for the
 * current camera). The contract is the base function's except in step 3: a pixel p with motion_p.w == 1.0f takes P = motion_p.xyz
 * in place of origin + d z_p. The rest of step 3 is unchanged and uses the previous camera's fields (cam_prev NULL = the current
 * camera): q = P - origin'; z_c, x', y' as written; the expected previous depth is z' = sqrtf(q . q). The identity path does not
 * apply to such a pixel even when the cameras' 112 bytes are equal. Steps 4 and 5 are unchanged: the taps are validated against
 * prev_normal_depth with z' and the CURRENT normal, so a surface that rotates beyond normal_tol between the frames still loses
 * its history (a previous-normal transform is out of scope). Every other pixel is the base function bit for bit, the identity
 * path included. motion NULL is the base function bit for bit; without a history (the first frame) motion is not read. The outputs
 * must not overlap motion (-1); all other checks are the base function's. Host and device form are bit-identical. */
int pt_temporal_accumulate_motion(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* rgba_sum,
                                  const float* sq_sum, int spp, int batches, const float* albedo, const float* normal_depth,
                                  const float* prev_normal_depth, const float* hist, const float* hist_len, const float* motion,
                                  const pt_temporal_params* params, float* out_hist, float* out_hist_len);       /* host, blocking */
int pt_temporal_accumulate_motion_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_rgba_sum,
                                         const void* d_sq_sum, int spp, int batches, const void* d_albedo, const void* d_normal_depth,
                                         const void* d_prev_normal_depth, const void* d_hist, const void* d_hist_len,
                                         const void* d_motion, const pt_temporal_params* params, void* d_out_hist,
                                         void* d_out_hist_len, void* stream);                                    /* async */
int pt_temporal_accumulate_cur_motion(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* cur,
                                      const float* normal_depth, const float* prev_normal_depth, const float* hist,
                                      const float* hist_len, const float* motion, const pt_temporal_params* params, float* out_hist,
                                      float* out_hist_len);                                                      /* host, blocking */
int pt_temporal_accumulate_cur_motion_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_cur,
                                             const void* d_normal_depth, const void* d_prev_normal_depth, const void* d_hist,
                                             const void* d_hist_len, const void* d_motion, const pt_temporal_params* params,
                                             void* d_out_hist, void* d_out_hist_len, void* stream);              /* async */
/* ---- RESPOND: a responsive history: detect stale lighting and shorten the history per pixel -------------------------------------
 * pt_temporal_accumulate validates a tap by depth and normal only, so a static surface whose lighting changed (a light or an
 * occluder moved) keeps blending with alpha = 1 / N into a history that is no longer its own. Every frame carries its own variance
 * V and the history the variance of its mean V_h; pt_temporal_accumulate_respond compares the difference of the two means with the
 * sum of the two variances over a small window and scales the history length N_h by a factor lambda in [0, 1] per pixel.
 *
 * One host / device pair covers the four base forms: the frame as sums (rgba_sum, sq_sum, spp, batches, albedo; cur NULL) or as
 * working pixels (cur, as pt_upsample writes them; rgba_sum, sq_sum and albedo NULL, spp and batches ignored) - exactly one of the
 * two, -1 otherwise - and motion NULL or pt_render_motion's buffer.
 *
 * Steps 1-4 are the base function's (pt_temporal_accumulate, _cur, _motion, _cur_motion by the arguments given), bit for bit. They
 * give pixel p its working value (e, V), or mark it pass-through, and the gathered history (e_h, V_h, N_h) when the valid tap
 * weight W >= 0.01. A WITNESS is a pixel that is not pass-through and has a gathered history. It carries
 *     d = e - e_h (three f32 subtractions)   and   v = V + V_h.
 * A witness p whose own d and v are finite walks the window of (2 radius + 1)^2 pixels around it in raster order (dy from -radius
 * outermost, dx from -radius inner; p itself at its place in that order). A pixel q COUNTS if it is inside the image, is a witness,
 * its d and v are finite, and it passes a tap's two guide comparisons against p on the CURRENT guide: |z_q - z_p| <= depth_tol z_p,
 * both unit normals non-zero, and their dot product (x, y, z left to right) >= normal_tol. A pixel that does not count is skipped,
 * never multiplied by zero. Then in f32, one rounding per operation, no fma:
 *     D_c = sum of d_q,c and Vs = sum of v_q over the counted pixels, in walk order from 0;
 *     T = D_x D_x + D_y D_y + D_z D_z, left to right;   lim = (threshold threshold) Vs;
 *     lambda = 1 unless T > lim; otherwise rho = lim / T and lambda = rho, rho rho or (rho rho) (rho rho) for power 1, 2, 4.
 * Step 5 is the base blend with lambda N_h in place of N_h: len = min(lambda N_h + 1, max_history), alpha = 1 / len, and the same
 * e and V formulas. Every other pixel runs no test and has lambda = 1: a pass-through pixel, a pixel without a gathered history,
 * a witness whose own d or v is not finite. Since 1 N_h == N_h exactly, a pixel with lambda = 1 is the base function's bit for
 * bit, and so is every pixel with threshold +inf (lim is +inf or NaN and T > lim is false). Without a history (the first frame)
 * the call is the base function. Under unchanged lighting E[T] = Vs (V is the sum of the three channels' variances, hence T sums
 * the three squared channel sums), so threshold is a z-score.
 *
 * out_scale (NULL, or w*h floats) receives lambda of every pixel, 1 where no test ran; the other outputs do not depend on it.
 * The device form needs a workspace of pt_temporal_respond_workspace_bytes(w, h) = 36 w h bytes (two launches: the gather, then the
 * walk and the blend); the host form stages its own. -1 before any HIP call: everything the base functions check, a radius outside
 * 1..3, a power other than 1, 2 or 4, a threshold that is not > 0 (+inf is allowed), not exactly one frame form, a NULL workspace,
 * a workspace or out_scale that overlaps any other buffer of the call or each other. params or respond NULL: the defaults. Host
 * and device form are bit-identical. tests/respond_ref.py restates the function in numpy. */
typedef struct pt_respond_params {
    int32_t radius;     /* 1..3: the window is (2 radius + 1)^2 pixels */
    int32_t power;      /* 1, 2 or 4 */
    float   threshold;  /* k > 0; +inf is allowed and makes every pixel the base function's */
} pt_respond_params;
void   pt_respond_defaults(pt_respond_params* out);                                      /* radius 3, power 4, threshold 2 */
size_t pt_temporal_respond_workspace_bytes(int w, int h);                                /* 36 w h; 0 for a size that is not positive */
int pt_temporal_accumulate_respond(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const float* rgba_sum,
                                   const float* sq_sum, int spp, int batches, const float* albedo, const float* cur,
                                   const float* normal_depth, const float* prev_normal_depth, const float* hist, const float* hist_len,
                                   const float* motion /* NULL ok */, const pt_temporal_params* params, const pt_respond_params* respond,
                                   float* out_hist, float* out_hist_len, float* out_scale /* NULL ok */);        /* host, blocking */
int pt_temporal_accumulate_respond_device(int w, int h, const pt_camera* cam, const pt_camera* cam_prev, const void* d_rgba_sum,
                                          const void* d_sq_sum, int spp, int batches, const void* d_albedo, const void* d_cur,
                                          const void* d_normal_depth, const void* d_prev_normal_depth, const void* d_hist,
                                          const void* d_hist_len, const void* d_motion /* NULL ok */, const pt_temporal_params* params,
                                          const pt_respond_params* respond, void* d_workspace, void* d_out_hist, void* d_out_hist_len,
                                          void* d_out_scale /* NULL ok */, void* stream);                         /* async */
/* The session's option. pt_preview_set_respond(p, params): NULL turns it off (the default: the frames of "preview", bit for bit),
 * a parameter set turns it on. The first call that turns it on allocates the workspace (-2 if that fails, the state unchanged); -1
 * on a NULL session or parameters out of range, the session unchanged. A change of value does not reset the session: the guides
 * and the history's format do not depend on it. With the option on, every temporal frame that has a history and is not a
 * converging frame accumulates through pt_temporal_accumulate_respond_device with exactly the arguments it would have given the
 * base, _cur, _motion or _cur_motion form, so the frame equals that chain of host calls bit for bit. Converging frames (the camera
 * rests and the scene is unchanged: nothing to detect, and pt_temporal_accumulate_live carries tiles forward as before), first
 * frames, non-temporal sessions, pt_preview_stats (accumulate_ms covers both launches) and the failed-frame rule are unchanged.
 * A shortened history makes its tile live again in the next pt_temporal_select: that is intended, the tile needs samples.
 * pt_preview_respond(p, out): 1 and *out (NULL ok) = the parameters if the option is on, 0 if off, -1 on a NULL session. */
int  pt_preview_set_respond(pt_preview* p, const pt_respond_params* params);
int  pt_preview_respond(pt_preview* p, pt_respond_params* out);

/* ---- picking: per-pixel IDs, pick queries and a selection overlay ------- */
/* pt_render_ids: WHICH surface the centre guides show at each pixel, as the indices the edit calls take. Per pixel the pass follows
 * the one unjittered pinhole ray of pt_render_aovs_centre (no RNG, no seed) and writes one int32x4:
 *   [0] tri       index into the description's triangle array
 *   [1] material  the row pt_scene_update_materials replaces
 *   [2] light     the index pt_scene_update_emission takes, or -1 for a triangle that is no light
 *   [3] info      bit 0: the surface is seen from its back; bits 8 and up: the number of links followed to reach it
 * A miss writes (-1, -1, -1, 0). max_links 0 reports the first hit; max_links 1..16 follows the ray through delta mirrors and smooth
 * dielectrics exactly as pt_render_aovs_centre(max_links) does and reports THE SURFACE WHOSE RECORD THE GUIDES HOLD: the first
 * non-specular surface, or, where the chain leaves the scene after the first hit or reaches max_links on a specular surface, the
 * first hit, whose albedo the guide shows there (info then counts 0 links). What the guide shows is what is picked.
 * Like the other feature passes this one touches no RNG state, accumulator or counter of the scene and may run between the chunks
 * of a render. Arguments are checked before any HIP call, -1 with a message that names pt_render_ids: max_links, the size, the
 * camera (its w, h must be the image's), the output, the scene; the device check comes last. */
int pt_render_ids(pt_scene* scene, const pt_camera* camera, int w, int h, int max_links, int32_t* out_ids /* w*h*4 */);       /* host, blocking */
int pt_render_ids_device(pt_scene* scene, const pt_camera* camera, int w, int h, int max_links, void* d_ids, void* stream);   /* async */
/* pt_pick: the same kernels on a list of n >= 1 pixels xy[k] = (x, y), one lane per pixel. out_ids[k] is pt_render_ids's pixel bit
 * for bit. out_hit[k] = (point.xyz, depth): the reported surface's point (ray origin + t * direction of the ray that reached it) and
 * the chain's summed path length, which is normal_depth.w of pt_render_aovs_centre(max_links) at that pixel bit for bit: what a
 * viewer sets focal_dist to on click-to-focus. A miss writes four zeros. Blocking. The checks of pt_render_ids under pt_pick's name,
 * and: n, the list, both outputs, and every pixel inside [0, w) x [0, h): -1 before any HIP call, nothing written. */
int pt_pick(pt_scene* scene, const pt_camera* camera, int w, int h, int n, const int32_t* xy /* n*2 */, int max_links,
            int32_t* out_ids /* n*4 */, float* out_hit /* n*4 */);
/* pt_select_overlay: up to four selections drawn onto display bytes (pt_resolve's rgba8) from an ID buffer, in place. Integer
 * arithmetic only: the host form, the device form and tests/ids_ref.py agree in every byte. Entries apply in order. For entry e a
 * pixel p is SELECTED if lo <= ids_p[component] <= hi. A selected pixel is an OUTLINE pixel if some pixel INSIDE THE IMAGE in the
 * (2 radius + 1)^2 window around it is not selected, else a FILL pixel; the outline lies inside the selection, and there is none
 * along the frame. Per colour byte out = (in * (255 - a) + colour * a + 127) / 255 with a = colour[3] on the outline and fill_alpha
 * on the fill; the fourth byte and every unselected pixel stay as they are; n = 0 writes nothing (entries may be NULL).
 * Checked before any HIP call (-1): the size, NULL buffers, n 0..4, NULL entries, component 0..2, 0 <= lo <= hi, radius 1..4,
 * fill_alpha 0..255, and ids overlapping rgba8. */
typedef struct pt_select_entry {
    int32_t component;      /* 0 tri, 1 material, 2 light */
    int32_t lo, hi;         /* inclusive id range, 0 <= lo <= hi (a triangle range is an object) */
    uint8_t colour[4];      /* r, g, b, outline alpha */
    int32_t radius;         /* 1..4 */
    int32_t fill_alpha;     /* 0..255, 0 = no tint */
} pt_select_entry;
int pt_select_overlay(int w, int h, const int32_t* ids, int n /* 0..4 */, const pt_select_entry* e, uint8_t* rgba8 /* in place */);   /* host, blocking */
int pt_select_overlay_device(int w, int h, const void* d_ids, int n, const pt_select_entry* e, void* d_rgba8, void* stream);          /* async */
/* The session. pt_preview_set_selection(p, n, e, max_links): n = 0 (the default) turns the selection off and gives the frames of
 * "preview" bit for bit; n = 1..4 entries (checked as pt_select_overlay checks them) make every frame end with
 * pt_select_overlay_device on its rgba8, after pt_resolve_device. The ID buffer the overlay reads is the session's own, w*h int32x4
 * at display size at any render scale, allocated by the first call with n > 0 (-2 if that fails, the state unchanged) and traced by
 * pt_render_ids_device(the frame's camera, max_links) on the session's stream ONLY WHEN IT IS STALE: there is none yet, the camera's
 * bytes, pt_scene_generation or max_links differ from those it was traced with, the session was reset, pt_preview_scene_changed was
 * called, or a frame failed after tracing it. A resting camera on an unchanged scene traces it once; pt_preview_id_passes counts
 * the launches of all good frames (-1 on NULL). Nothing but rgba8 depends on the selection: mean, the history, the tile outputs,
 * pt_preview_guide_passes and the layout of pt_preview_stats (resolve_ms covers the ID pass and the overlay) are unchanged, and no
 * call here resets the session.
 * pt_preview_pick: pt_pick of one pixel with the last good frame's camera at display size; -1 before the first good frame (and
 * after a reset), or with the pixel outside the session's size. pt_preview_read_ids copies the ID buffer to the host (-1 while
 * there is no valid one); pt_preview_device_ids is the buffer itself, valid until the session is destroyed (NULL before the first
 * selection). */
int  pt_preview_set_selection(pt_preview* p, int n, const pt_select_entry* e, int max_links);
int  pt_preview_pick(pt_preview* p, int x, int y, int max_links, int32_t out_ids[4], float out_hit[4]);
int  pt_preview_read_ids(pt_preview* p, int32_t* out /* w*h*4 */);
const void* pt_preview_device_ids(pt_preview* p);
int  pt_preview_id_passes(pt_preview* p);

/* ---- ray queries: closest-hit and shadow rays for a caller's own rays ---- */
/* A buffer of n rays traced against the scene, on the device and on a stream. Ray i is (o, d, max_t) exactly as given: the direction
 * is NOT normalised by the library (t is in units of |d|), and pad is not read.
 * pt_query_closest: the non-counting closest-hit traversal of the feature passes with the ray's own max_t: a hit is accepted if
 *   t < max_t and it is smaller than the best so far. For max_t <= 999999 the result is therefore pt_probe_trace_closest's hit if that
 *   hit's t < max_t, and a miss otherwise, bit for bit. A hit writes (t, u, v, tri), tri the index into the description's triangle
 *   array (as pt_render_ids reports it); a miss writes (0, 0, 0, -1).
 *   surfaces (NULL: none is written, and nothing of such a buffer is touched): the resolved record of the same hit: its point
 *   (o + t d, one fma per component), its normal (interpolated, normalised, turned to face the ray), the interpolated uv, the
 *   material row pt_scene_update_materials replaces, the light index pt_scene_update_emission takes or -1 for a triangle that is no
 *   light, and backface = 1 if the triangle is seen from its back. A miss writes zeros, with material = light = -1.
 * pt_query_shadow: throughput[i] = (the shadow traversal's throughput, 0) as a float4: exactly (0, 0, 0) if anything opaque lies
 *   below max_t, else the product of the transmissions of the leaf-material triangles on the way (the reference's BVHShadowRay);
 *   pt_probe_trace_shadow's three floats bit for bit.
 * flags: 0, or PT_QUERY_REORDER: before tracing, every ray gets a 32-bit key (its direction's octant, then a Morton code of its
 *   origin quantised to 9 bits per axis in the scene's bounds, the union of the root's two child boxes, read on the device; a ray
 *   with a non-finite origin gets key 0), (key, index) pairs are sorted, and lane i of the trace kernels takes ray perm[i] and writes
 *   its outputs at perm[i]. Every output is bit-identical to the unordered call for every input: only the order of the work changes.
 *   A scene whose root is a leaf, and n <= 64, take the unordered path. Opt-in, and so far NOT a gain: on 2 M rays at 1080p the key
 *   kernel and the sort cost 0.17 ms, and the flag lost on every input measured (1.01 to 1.7 times the unordered call).
 * The calls touch no RNG state, accumulator or counter of the scene and may run between the chunks of a render. They use the scene's
 * feature spill area, a reordered call also scene-owned key, index and sort buffers (grown on demand, freed by pt_scene_destroy),
 * and the host forms a scene-owned staging buffer: like the scene's other work buffers these make the calls ORDERED with other
 * launches on the same scene (issue them on one stream, or synchronise between streams). After any pt_scene_update_* a query sees
 * the edited scene, bit for bit as a fresh scene of the edited arrays does.
 * The device forms are asynchronous on `stream`; d_rays (n pt_ray), d_hits (n pt_ray_hit), d_surfaces (n pt_ray_surface) and
 * d_throughput (n float4) are device buffers aligned to 16 bytes. The host forms copy in, run on the null stream and copy out.
 * Arguments are checked before any HIP call, -1 with a message that names the function: a NULL scene, rays or output, n < 0 or
 * n > 1 << 28, unknown flag bits; n == 0 returns 0 and launches nothing; the device check comes last. */
typedef struct pt_ray         { float ox, oy, oz, max_t;  float dx, dy, dz;  uint32_t pad; } pt_ray;           /* 32 bytes */
typedef struct pt_ray_hit     { float t, u, v;  int32_t tri; } pt_ray_hit;                                     /* 16 bytes */
typedef struct pt_ray_surface { float px, py, pz, uvx;  float nx, ny, nz, uvy;
                                int32_t material, light, backface, pad; } pt_ray_surface;                      /* 48 bytes */
#define PT_QUERY_REORDER 1u
int pt_query_closest_device(pt_scene* scene, int n, const void* d_rays, void* d_hits, void* d_surfaces /* NULL ok */, uint32_t flags,
                            void* stream);                                                                                    /* async */
int pt_query_shadow_device(pt_scene* scene, int n, const void* d_rays, void* d_throughput /* n float4 */, uint32_t flags, void* stream);   /* async */
int pt_query_closest(pt_scene* scene, int n, const pt_ray* rays, pt_ray_hit* hits, pt_ray_surface* surfaces /* NULL ok */,
                     uint32_t flags);                                                                                         /* host, blocking */
int pt_query_shadow(pt_scene* scene, int n, const pt_ray* rays, float* throughput4 /* n*4 */, uint32_t flags);                /* host, blocking */
/* Ray y*w + x = the centre ray of pixel (x, y) as pt_render_aovs_centre and pt_render_ids trace it (pt_probe_centre_rays's o and d
 * bit for bit), with the given max_t and pad = 0: coherent rays for a tool without an upload, and the tie between a query and those
 * passes. One thread per pixel, asynchronous on `stream`; needs no scene. Checked before any HIP call (-1, the message names the
 * function): the camera, a positive size of at most 1 << 28 pixels that is the camera's, the buffer. */
int pt_query_camera_rays_device(const pt_camera* camera, int w, int h, float max_t, void* d_rays /* w*h pt_ray */, void* stream);         /* async */
/* pt_query_radiance: the path tracer on the caller's rays: the light that arrives along each ray, summed over spp
 * samples. This is what a panorama, a fisheye or orthographic sensor, a stereo pair in one launch, lightmap texels and light probes
 * are rendered with. It is NOT a replacement for pt_render: a per-lane walk, far slower than the megakernels on a scene they hold
 * in LDS (the measured ratios are in §24).
 * Stream. Ray i owns one XORWOW stream: the stream rng_init_kernel gives subsequence k_i of `seed`, k_i = first_stream + i, or, with
 *   PT_QUERY_STREAM_PAD, first_stream + (the ray's pad word read as uint32), in uint32 arithmetic (it wraps). Without the flag
 *   first_stream + n must not pass 2^31. The stream runs on through the ray's spp samples, as a pixel's does.
 * Sample. Every sample uses the same ray. It first draws two uniforms and drops them (the two jitter draws the reference's camera
 *   spends) and draws no lens numbers. Then it runs the reference's Li_unidirectional (integrator 0, use_mis as given) or
 *   Li_naive_unidirectional (integrator 2) from path_begin's state at (o, d) as given: beta 1, Li 0, prevPoint 0, pdf = etaI = etaT =
 *   EPS, depth 0, the medium stack holding air. The direction is used as given, NOT normalised: the path's arithmetic assumes
 *   |d| = 1, and a caller whose d is not unit gets what that arithmetic makes of it. The first segment's closest hit uses the ray's own
 *   max_t, accepted as pt_query_closest accepts it (t < max_t); every later segment uses 999999, as the path does. The iteration
 *   guard of DESIGN.md §4 applies. max_depth: any value, as pt_render takes it.
 * Output. out[i].xyz = ((0 + Li_0) + Li_1) + ... in sample order, in f32; out[i].w = 0. The call writes; it does not add.
 * Identity. For a camera cam0 with antiAliasJitterDist = 0 and aperture = 0, the rays pt_query_camera_rays_device(cam0, w, h, 999999)
 *   gives, first_stream = 0 and flags = 0, `out` viewed as w*h float4 equals pt_render(scene, cam0, w, h, spp, max_depth, integrator,
 *   use_mis, seed, NULL, zeroed) bit for bit, and so the oracle's render.
 * Independence. A ray's result depends only on the scene, its 32 bytes, k_i, seed, spp, max_depth, integrator and use_mis: not on n,
 *   on its place in the buffer or on what the other lanes of its wave hold.
 * What a call touches: the scene's feature spill area and, the host form, its query staging buffer (so it is ORDERED with other
 *   launches on the scene, as the queries above). No per-pixel RNG state, tile accumulator, counter or tile queue. pt_set_variant
 *   does not reach it. Of the pt_set_option values the two that decide the material class of the kernel are honoured: "simple" 0
 *   and "lean" 0 turn the SIMPLE and the LEAN bounce off (same bits, the generic kernel). Scheduling options are not read, nor is
 *   "culling": there is no CULL form. After any pt_scene_update_* a call sees the edited scene. PT_QUERY_REORDER is refused (-1): it
 *   lost every measurement of §23, and a path leaves its first ray's order at once.
 * Checked before any HIP call, -1 with a message under pt_query_radiance: n < 0 or n > 1 << 28 (n == 0 then returns 0 before the
 *   scene or anything else is looked at); a NULL scene, rays or output; spp < 1 or spp > 1 << 22; an integrator other than 0 and 2;
 *   PT_QUERY_REORDER and unknown flag bits; without PT_QUERY_STREAM_PAD, first_stream + n > 2^31. The device check comes last.
 * d_rays (n pt_ray) and d_rgba_sum (n float4) are device buffers aligned to 16 bytes; the device form is asynchronous on `stream`. */
#define PT_QUERY_STREAM_PAD 2u
int pt_query_radiance_device(pt_scene* scene, int n, const void* d_rays /* n pt_ray */, int spp, int max_depth, int integrator, int use_mis,
                             uint64_t seed, uint32_t first_stream, void* d_rgba_sum /* n float4 */, unsigned flags, void* stream);   /* async */
int pt_query_radiance(pt_scene* scene, int n, const pt_ray* rays, int spp, int max_depth, int integrator, int use_mis, uint64_t seed,
                      uint32_t first_stream, float* out_rgba_sum /* n*4 */, unsigned flags);                                  /* host, blocking */
/* pt_query_radiance_moments: pt_query_radiance that keeps each ray's variance: the sample sum S and the sum of squared
 * batch sums Q per ray, pt_render_moments' pair, from one launch, so that pt_denoise_var can filter an image made of the caller's rays.
 * Everything pt_query_radiance states holds unchanged: stream, sample, max_t on the first segment only, independence, what a call
 *   touches, PT_QUERY_STREAM_PAD, the options "simple" and "lean", and the refusal of PT_QUERY_REORDER.
 * Batches. The ray's spp samples are B = spp / batch_spp batches of c = batch_spp samples. With S_j the ray's f32 running sum after
 *   j c samples (((0 + Li_0) + Li_1) + ..., S_0 = 0): out_rgba_sum[i] = (S_B, 0), pt_query_radiance's output bit for bit.
 * Q. Per rgb channel Q_j = Q_(j-1) + d d with d = S_j - S_(j-1), Q_0 = 0, the product rounded before the sum, no contraction, no
 *   special case for NaN or Inf: pt_render_moments' definition. out_sq_sum[i] = (Q_B, (float)B).
 * The call writes both buffers; it does not add to them.
 * Identity. With cam0's rays from pt_query_camera_rays_device(cam0, w, h, 999999), first_stream = 0 and flags = 0, both outputs equal
 *   pt_render_moments(scene, cam0, w, h, spp, batch_spp, ...) bit for bit.
 * Checked before any HIP call, -1 with a message under pt_query_radiance_moments: pt_query_radiance's checks in its order (n == 0
 *   returns 0 before the scene or anything else is looked at); batch_spp < 1; spp not a multiple of batch_spp; spp / batch_spp < 2;
 *   a NULL sq_sum. The device check comes last.
 * d_rays (n pt_ray), d_rgba_sum and d_sq_sum (n float4 each) are device buffers aligned to 16 bytes; the device form is asynchronous
 * on `stream`. */
int pt_query_radiance_moments_device(pt_scene* scene, int n, const void* d_rays /* n pt_ray */, int spp, int batch_spp, int max_depth, int integrator,
                                     int use_mis, uint64_t seed, uint32_t first_stream, void* d_rgba_sum /* n float4 */,
                                     void* d_sq_sum /* n float4 */, unsigned flags, void* stream);                                 /* async */
int pt_query_radiance_moments(pt_scene* scene, int n, const pt_ray* rays, int spp, int batch_spp, int max_depth, int integrator, int use_mis,
                              uint64_t seed, uint32_t first_stream, float* out_rgba_sum /* n*4 */, float* out_sq_sum /* n*4 */,
                              unsigned flags);                                                                                  /* host, blocking */
/* pt_query_guides: the denoisers' guides for the caller's rays: what pt_render_aovs_centre gives for the centre ray of
 * a pixel, for ray i = (o, d, max_t) as given. d is assumed to be unit length and is NOT normalised; pad is not read.
 * The first segment's closest hit is accepted as pt_query_closest accepts it (t < max_t); every link after it uses 999999. The hit,
 *   the link rule (mirrors and smooth dielectrics, deterministically, at most max_links links), the direction arithmetic and the
 *   fallback (the first hit's record stands when the chain ends in a miss or at the cap) are pt_render_aovs_centre's.
 * Output. albedo[i] = (a, 1), normal_depth[i] = (n, summed path length), links[i] (NULL: not written) = the number of links followed.
 *   A ray that hits nothing below its max_t: eight zeros and links 0. The call writes; lanes past n store nothing.
 * max_links 0 runs a first-hit kernel, 1..16 the chain kernel.
 * Identity. On cam0's centre-ray records at max_t = 999999 the three outputs are pt_render_aovs_centre(scene, cam, w, h, max_links, ...)
 *   bit for bit.
 * What a call touches: the scene's feature spill area and, the host form, its query staging buffer. No RNG state, accumulator or
 *   counter. After any pt_scene_update_* a call sees the edited scene.
 * flags is reserved and must be 0.
 * Checked before any HIP call, -1 with a message under pt_query_guides: n < 0 or n > 1 << 28; a NULL scene, rays, albedo or
 *   normal_depth; max_links outside 0..16; any flag bit. Then n == 0 returns 0 and launches nothing. The device check comes last.
 * d_rays (n pt_ray), d_albedo and d_normal_depth (n float4 each, aligned to 16 bytes) and d_links (n floats or NULL) are device
 * buffers; the device form is asynchronous on `stream`. */
int pt_query_guides_device(pt_scene* scene, int n, const void* d_rays /* n pt_ray */, int max_links, void* d_albedo /* n float4 */,
                           void* d_normal_depth /* n float4 */, void* d_links /* n floats, NULL ok */, unsigned flags, void* stream);   /* async */
int pt_query_guides(pt_scene* scene, int n, const pt_ray* rays, int max_links, float* out_albedo /* n*4 */, float* out_normal_depth /* n*4 */,
                    float* out_links /* n, NULL ok */, unsigned flags);                                                         /* host, blocking */
/* pt_query_irradiance: cosine-sampled light at surface points: what a lightmap texel or a light probe needs. The
 * library draws the directions itself, and a record's samples may be spread over several lanes of a wave.
 * Record. A pt_ray: (ox, oy, oz) is the surface point p, (dx, dy, dz) the unit normal nrm, used as given and NOT normalised, max_t
 *   bounds the first segment of every sample as in pt_query_radiance, pad is read only with PT_QUERY_STREAM_PAD. A pt_ray_surface of
 *   pt_query_closest (point, facing normal) becomes a record by copying those fields.
 * Lanes and streams. lanes = L, one of 1, 2, 4, 8, 16, 32, 64. Record i owns L lanes; lane l owns the XORWOW stream
 *   k = first_stream + i*L + l, or with PT_QUERY_STREAM_PAD first_stream + pad_i*L + l, in uint32 arithmetic (it wraps), seeded as
 *   pt_query_radiance seeds a ray's. Without the flag first_stream + n*L must not pass 2^31. A 64-lane tile holds 64 / L records;
 *   lanes of records past n take no work and store nothing. A lane runs spp_lane samples on its stream, one after the other.
 * Sample. A sample draws u1, then u2: the two draws a pt_query_radiance sample spends and drops. From them:
 *   DIRECTION ARITHMETIC, every operation rounded once to f32 in the order written, nothing fused but the fma() named here
 *   (fma(a, b, c) = a*b + c rounded once). EPS = 1e-5f, PI = 3.141592f, RAY_EPS = 1e-3f.
 *     u1 = min(u1, 1 - EPS);  r = sqrtf(u1);  phi = (2*PI)*u2;  (sn, cs) = the library's sincos of phi (pt_device.h: sincos_);
 *     local = (r*cs, r*sn, sqrtf(1 - u1))                                            (cosine_sample_f's direction)
 *     tangent: |nrm.x| > |nrm.z| ?  v = (-nrm.y, nrm.x, 0)  :  v = (0, -nrm.z, nrm.y);
 *              t = v * (1 / sqrtf(fma(v.z, v.z, fma(v.y, v.y, v.x*v.x))))            (sqrt, then the reciprocal, both correctly
 *              rounded, then three products; on the tie |nrm.x| = |nrm.z| the second arm)
 *     b = (fma(nrm.y, t.z, -(nrm.z*t.y)), fma(nrm.z, t.x, -(nrm.x*t.z)), fma(nrm.x, t.y, -(nrm.y*t.x)))          (cross(nrm, t))
 *     d = (local.x*t + local.y*b) + local.z*nrm    per component: (t.c*local.x + b.c*local.y) + nrm.c*local.z
 *     o = p + nrm*RAY_EPS                          per component: p.c + nrm.c*RAY_EPS
 *   the plain basis of the naive bounce and the offset the bounce gives a reflected ray. From (o, d) the sample runs exactly what a
 *   pt_query_radiance sample runs after its two draws: path_begin's state, the record's max_t on the first segment and 999999 on
 *   every later one, Li_unidirectional (integrator 0, use_mis as given) or Li_naive_unidirectional (integrator 2), the same kernel
 *   class for the scene's materials and the same honouring of the options "simple" and "lean".
 * Sums. A lane's sum is a_l = ((0 + Li_0) + Li_1) + ... in f32. The record's sum is the adjacent-pair tree over its lanes:
 *   T_0[l] = a_l, T_(k+1)[l] = T_k[2l] + T_k[2l+1], S = T_(log2 L)[0] per rgb channel; out_rgba_sum[i] = (S, 0).
 *   sq_sum (NULL: not written; needs L >= 2, a lane's sum being one batch): Q = the same tree over a_l*a_l per channel, the product
 *   rounded before any sum, no contraction; out_sq_sum[i] = (Q, (float)L). (S, Q) is pt_render_moments' pair for spp = L*spp_lane in
 *   batches = L, so pt_denoise_var with pt_query_guides' guides filters a baked lightmap as it filters a panorama.
 *   Irradiance is PI*S / (L*spp_lane); the library does not scale the sums. The call writes its outputs; it does not add to them.
 * Independence. A record's result depends only on the scene, its 32 bytes, its stream base, L, spp_lane, seed, max_depth, integrator
 *   and use_mis: not on n, on its place in the buffer or on what the other records of its tile hold.
 * What a call touches: what pt_query_radiance touches, the scene's feature spill area and, the host form, its query staging
 *   buffer. No RNG state, accumulator, counter or tile queue of the scene. After any pt_scene_update_* a call sees the edited scene.
 * pt_query_irradiance_rays_device: the tie to pt_query_radiance, as pt_query_camera_rays_device is the centre passes'. Ray i*L + l is
 *   the (o, d) a sample of lane l of record i starts from when draws draw_offset[i*L + l] and draw_offset[i*L + l] + 1 of the lane's
 *   stream play u1 and u2 (NULL: all 0, the lane's first sample). It carries the record's max_t, and pad = i*L + l, or pad_i*L + l
 *   with PT_QUERY_STREAM_PAD: what the lane adds to first_stream. One thread per ray; of the scene it reads the seeding tables only.
 * Identity. With spp_lane = 1, a_l equals, bit for bit, the .xyz of pt_query_radiance on that emitted ray with spp = 1,
 *   PT_QUERY_STREAM_PAD and the same seed, first_stream, max_depth, integrator and use_mis. With more samples the stream runs on:
 *   sample j of a lane starts at the draw after the last one sample j - 1 spent.
 * Checked before any HIP call, -1 with a message under the function's name, in this order: n < 0 or n*L > 1 << 28 (n == 0 then
 *   returns 0 before the scene or anything else is looked at); a NULL scene, records or sum (rays) buffer; lanes not a power of two
 *   in 1..64; spp_lane < 1 or L*spp_lane > 1 << 22; an integrator other than 0 and 2; sq_sum given with lanes == 1;
 *   PT_QUERY_REORDER and unknown flag bits; without PT_QUERY_STREAM_PAD, first_stream + n*L > 2^31. (The rays call has no samples,
 *   integrator or sq_sum to check.) The device check comes last.
 * d_records (n pt_ray), d_rgba_sum and d_sq_sum (n float4 each), d_rays (n*L pt_ray) and d_draw_offset (n*L uint32) are device
 * buffers, the first four aligned to 16 bytes; the device forms are asynchronous on `stream`. */
int pt_query_irradiance_device(pt_scene* scene, int n, const void* d_records /* n pt_ray */, int lanes, int spp_lane, int max_depth, int integrator,
                               int use_mis, uint64_t seed, uint32_t first_stream, void* d_rgba_sum /* n float4 */,
                               void* d_sq_sum /* n float4, NULL ok */, unsigned flags, void* stream);                              /* async */
int pt_query_irradiance(pt_scene* scene, int n, const pt_ray* records, int lanes, int spp_lane, int max_depth, int integrator, int use_mis,
                        uint64_t seed, uint32_t first_stream, float* out_rgba_sum /* n*4 */, float* out_sq_sum /* n*4, NULL ok */,
                        unsigned flags);                                                                                        /* host, blocking */
int pt_query_irradiance_rays_device(pt_scene* scene, int n, const void* d_records /* n pt_ray */, int lanes, uint64_t seed, uint32_t first_stream,
                                    const void* d_draw_offset /* n*lanes uint32, NULL = all 0 */, void* d_rays /* n*lanes pt_ray */,
                                    unsigned flags, void* stream);                                                              /* async */
/* pt_query_sh: a light probe's nine spherical-harmonic coefficients. The library draws uniform directions on the
 * sphere about a point in free space, walks the paths, and projects every sample's light onto the real spherical harmonics of bands
 * 0..2. A record's samples may be spread over up to 4096 lanes, that is 64 waves.
 * Record. A pt_ray: (ox, oy, oz) is the probe position p; max_t bounds the first segment of every sample as in pt_query_radiance;
 *   the three direction words are NOT read; pad is read only with PT_QUERY_STREAM_PAD.
 * Lanes and streams. lanes = L, a power of two in 1..4096. Record i owns lanes i*L .. i*L + L-1 of the launch; lane l owns the XORWOW
 *   stream k = first_stream + i*L + l, or with PT_QUERY_STREAM_PAD first_stream + pad_i*L + l, in uint32 arithmetic (it wraps), seeded
 *   as pt_query_radiance seeds a ray's. Without the flag first_stream + n*L must not pass 2^31. A lane runs spp_lane samples on its
 *   stream, one after the other. For L <= 64 a 64-lane tile holds 64 / L records; for L > 64 a record is L / 64 whole tiles, which any
 *   waves of the launch may take.
 * Sample. A sample draws u1, then u2: the two draws a pt_query_radiance sample spends and drops. From them
 *   DIRECTION ARITHMETIC, every operation rounded once to f32 in the order written, nothing fused. EPS = 1e-5f, PI = 3.141592f.
 *     u1 = min(u1, 1 - EPS);  r = sqrtf(u1);  phi = (2*PI)*u2;  (sn, cs) = the library's sincos of phi (pt_device.h: sincos_);
 *     w = (r*cs, r*sn, sqrtf(1 - u1))                                                (cosine_sample_f's direction, as above)
 *     s = 2*w.z;   d = (s*w.x, s*w.y, s*w.z - 1);   o = p
 *   Archimedes' map of the hemisphere onto the sphere: d.z = 2(1 - u1) - 1 is uniform in [-1, 1], the azimuth is w's, so d is
 *   uniform on the sphere. The clamp of u1 leaves out a cap of 1e-5 of the sphere's area around -z. d is used as formed, in world
 *   axes: no basis, no offset, no normalise (|d| is 1 to a few ulp). From (o, d) the sample runs exactly what a pt_query_radiance
 *   sample runs after its two draws: path_begin's state, the record's max_t on the first segment and 999999 on every later one,
 *   Li_unidirectional (integrator 0, use_mis as given) or Li_naive_unidirectional (integrator 2), the same kernel class for the
 *   scene's materials and the same honouring of the options "simple" and "lean".
 * Projection. With (x, y, z) = d, every product and difference rounded once, nothing contracted:
 *     C0 = 0.2820948f  C1 = 0.4886025f  C2 = 1.0925484f  C3 = 0.3153916f  C4 = 0.5462742f
 *     Y0 = C0          Y1 = C1*y        Y2 = C1*z        Y3 = C1*x
 *     Y4 = C2*(x*y)    Y5 = C2*(y*z)    Y6 = C3*(3*(z*z) - 1)    Y7 = C2*(x*z)    Y8 = C4*(x*x - y*y)
 *   The term of sample j is t_j[k][c] = Li_j.c * Y_k(d_j) for the three channels c, Li_j being the sample's own light.
 * Sums. A lane's sums are a_l[k][c] = ((0 + t_0) + t_1) + ... in f32. The record's sums are the adjacent-pair tree over its L lanes,
 *   T_0[l] = a_l, T_(m+1)[l] = T_m[2l] + T_m[2l+1], run first within each wave and then over the waves' partial sums in tile order:
 *   L being a power of two, one tree of depth log2 L. coeffs[9*i + k] = (R, G, B, 0). The radiance coefficient is
 *   4*pi*sum / (L*spp_lane); the library does not scale. The call writes its outputs; it does not add to them.
 * Workspace. For L > 64 the waves leave their partial sums in a workspace of pt_query_sh_workspace_bytes(n, L) = n * (L/64) * 9 * 16
 *   bytes (0 for L <= 64), aligned to 16 bytes, which the device form's caller brings (NULL is fine for L <= 64) and a second small
 *   kernel on the same stream reads. Its contents after the call are unspecified. The host form allocates its own.
 * pt_query_sh_rays_device: the tie to pt_query_radiance. Ray i*L + l is the (o, d) a sample of lane l of record i starts from when
 *   draws draw_offset[i*L + l] and draw_offset[i*L + l] + 1 of the lane's stream play u1 and u2 (NULL: all 0, the lane's first
 *   sample). It carries the record's max_t, and pad = i*L + l, or pad_i*L + l with PT_QUERY_STREAM_PAD: what the lane adds to
 *   first_stream, exactly as pt_query_irradiance_rays_device does it. One thread per ray; of the scene it reads the seeding tables only.
 * Identity. With spp_lane = 1, a_l[k][c] = 0 + Li.c * Y_k(d) bit for bit (a product of -0 sums to +0), Li being the .xyz of pt_query_radiance on that emitted ray
 *   with spp = 1, PT_QUERY_STREAM_PAD and the same seed, first_stream, max_depth, integrator and use_mis, and d the emitted
 *   direction. With more samples the stream runs on: sample j of a lane starts at the draw after the last one sample j - 1 spent.
 * Independence. A record's nine coefficients depend only on the scene, p, max_t, its stream base, L, spp_lane, seed, max_depth,
 *   integrator and use_mis: not on n, on its place in the buffer, on which waves took its tiles or on what other records hold.
 * What a call touches: what pt_query_radiance touches, the scene's feature spill area and, the host form, its query staging
 *   buffer. No RNG state, accumulator, counter or tile queue of the scene. After any pt_scene_update_* a call sees the edited scene.
 * Occupancy. The 27 sums and the direction of a lane live in LDS, 30 KB a workgroup: the kernels run at 3 waves per SIMD where the
 *   radiance kernels have 4 to 6 (the price is measured in §27).
 * Checked before any HIP call, -1 with a message under the function's name, in this order: n < 0 or n*L > 1 << 28 (n == 0 then
 *   returns 0 before the scene or anything else is looked at); a NULL scene, records or coefficient (rays) buffer; lanes not a power
 *   of two in 1..4096; spp_lane < 1 or L*spp_lane > 1 << 22; an integrator other than 0 and 2; PT_QUERY_REORDER and unknown flag
 *   bits; without PT_QUERY_STREAM_PAD, first_stream + n*L > 2^31; the device form, lanes > 64 with a NULL workspace. (The rays call
 *   has no samples, integrator or workspace to check.) The device check comes last.
 * d_records (n pt_ray), d_coeffs (n*9 float4), d_workspace, d_rays (n*L pt_ray) and d_draw_offset (n*L uint32) are device buffers,
 * the first four aligned to 16 bytes; the device forms are asynchronous on `stream`. */
size_t pt_query_sh_workspace_bytes(int n, int lanes);
int pt_query_sh_device(pt_scene* scene, int n, const void* d_records /* n pt_ray */, int lanes, int spp_lane, int max_depth, int integrator,
                       int use_mis, uint64_t seed, uint32_t first_stream, void* d_coeffs /* n*9 float4 */,
                       void* d_workspace /* NULL ok when lanes <= 64 */, unsigned flags, void* stream);                            /* async */
int pt_query_sh(pt_scene* scene, int n, const pt_ray* records, int lanes, int spp_lane, int max_depth, int integrator, int use_mis,
                uint64_t seed, uint32_t first_stream, float* out_coeffs /* n*9*4 */, unsigned flags);                            /* host, blocking */
int pt_query_sh_rays_device(pt_scene* scene, int n, const void* d_records /* n pt_ray */, int lanes, uint64_t seed, uint32_t first_stream,
                            const void* d_draw_offset /* n*lanes uint32, NULL = all 0 */, void* d_rays /* n*lanes pt_ray */, unsigned flags,
                            void* stream);                                                                                      /* async */
/* pt_query_distance: a probe's octahedral map of hit-distance moments: what a probe volume's visibility (Chebyshev)
 * test reads. About a point in free space the library makes directions texel by texel of an R x R octahedral map, finds the nearest
 * surface in each, and sums per texel the distance and its square.
 * Record. A pt_ray as pt_query_sh reads it: (ox, oy, oz) is the probe position p; max_t bounds every sample's ray, and is the distance
 *   a miss counts with; the three direction words are NOT read; pad is read only with PT_QUERY_STREAM_PAD.
 * Lanes and streams. res = R, one of 4, 8, 16, 32. Record i owns lanes i*R*R .. i*R*R + R*R-1 of the launch; lane l = ty*R + tx is
 *   texel (tx, ty) and owns the XORWOW stream k = first_stream + i*R*R + l, or with PT_QUERY_STREAM_PAD first_stream + pad_i*R*R + l,
 *   in uint32 arithmetic (it wraps), seeded as pt_query_radiance seeds a ray's: pt_query_irradiance's streams at L = R*R. Without the
 *   flag first_stream + n*R*R must not pass 2^31. A lane runs spp_lane samples on its stream, one after the other. A 64-lane tile
 *   holds four records at R = 4, one at R = 8, and a part of one at R >= 16.
 * Sample. A sample draws u1, then u2 (the two draws cosine_sample_f would spend); the trace draws nothing, so sample j of a lane uses
 *   draws 2j and 2j + 1 of its stream. With PT_QUERY_TEXEL_CENTRE u1 = u2 = 0.5 exactly, spp_lane must be 1, no stream is seeded,
 *   and seed, first_stream and PT_QUERY_STREAM_PAD are not read.
 *   DIRECTION ARITHMETIC, every operation rounded once to f32 in the order written, nothing fused but the two fmas of the dot. 1/R is exact.
 *     px = ((float)tx + u1) * (1/R);   py = ((float)ty + u2) * (1/R)
 *     fx = 2*px - 1;   fy = 2*py - 1;   ax = |fx|;   ay = |fy|;   z = (1 - ax) - ay
 *     z < 0:  x = copysign(1 - ay, fx),  y = copysign(1 - ax, fy);   else  x = fx,  y = fy
 *     dot = fma(z, z, fma(y, y, x*x));   il = 1 / sqrtf(dot) (both correctly rounded);   d = (x*il, y*il, z*il);   o = p
 *   The octahedron |x| + |y| + |z| = 1 in world axes with z as its fold axis (the pole pt_query_sh's map has): the square's centre is
 *   +z, its corners are -z, the middle of the edge u = 1 is +x and of v = 1 is +y.
 * Trace. trace_closest with the record's max_t, exactly what pt_query_closest runs on the ray (o, d, max_t). r = the hit's t, or max_t
 *   for a miss. `back` is the backface word pt_query_closest's surface record has for that hit, bit for bit.
 * Output. maps[i*R*R + l] = (A, B, H, K) as a float4: A = ((0 + r_0) + r_1) + ..., B = ((0 + r_0*r_0) + r_1*r_1) + ... with each product
 *   rounded first, H the number of the lane's samples that hit, K the number of those hits seen from behind, both as floats. The
 *   call writes; it does not add and does not scale: the mean distance is A / spp_lane, the mean square B / spp_lane. K / H near 1
 *   says the probe lies inside an object.
 * pt_query_distance_rays_device: the tie to pt_query_closest, shaped as pt_query_sh_rays_device. Ray g = i*R*R + l is the (o, d) of the
 *   sample of lane l of record i that draws draw_offset[g] and draw_offset[g] + 1 of the lane's stream (NULL: all 0, the lane's first
 *   sample). It carries the record's max_t and, in its pad word, what the lane adds to first_stream: g, or pad_i*R*R + l with
 *   PT_QUERY_STREAM_PAD. With PT_QUERY_TEXEL_CENTRE draw_offset is not read and the pad word is g. One thread per ray; of the scene it
 *   reads the seeding tables only.
 * Identity. With spp_lane = 1 a texel is (0 + r, 0 + r*r, hit, back) of pt_query_closest (with surfaces) on the ray
 *   pt_query_distance_rays_device emits for that lane with the same seed, first_stream and flags. With more samples the stream runs
 *   on: sample j is the ray emitted with draw_offset 2j.
 * Independence. A record's map depends only on the scene, p, max_t, its stream base, R, spp_lane and seed: not on n, on its place in the
 *   buffer, on which waves took its tiles or on what other records hold.
 * What a call touches: the scene's feature spill area and, the host form, its query staging buffer. No RNG state, accumulator,
 *   counter or tile queue of the scene. After any pt_scene_update_* a call sees the edited scene. The options "simple" and "lean" are
 *   not read: there is one kernel per mode.
 * Checked before any HIP call, -1 with a message under the function's name, in this order: n < 0 or n*R*R > 1 << 28 (n == 0 then
 *   returns 0 before the scene or anything else is looked at); a NULL scene, records or maps (rays) buffer; res not one of 4, 8, 16,
 *   32; spp_lane < 1 or R*R*spp_lane > 1 << 22; PT_QUERY_REORDER and unknown flag bits; PT_QUERY_TEXEL_CENTRE with spp_lane != 1;
 *   without PT_QUERY_STREAM_PAD and without PT_QUERY_TEXEL_CENTRE, first_stream + n*R*R > 2^31. (The rays call has no samples to
 *   check.) The device check comes last.
 * d_records (n pt_ray), d_maps (n*R*R float4), d_rays (n*R*R pt_ray) and d_draw_offset (n*R*R uint32) are device buffers, the first
 * three aligned to 16 bytes; the device forms are asynchronous on `stream`. */
#define PT_QUERY_TEXEL_CENTRE 4u
int pt_query_distance_device(pt_scene* scene, int n, const void* d_records /* n pt_ray */, int res, int spp_lane, uint64_t seed,
                             uint32_t first_stream, void* d_maps /* n*res*res float4 */, uint32_t flags, void* stream);        /* async */
int pt_query_distance(pt_scene* scene, int n, const pt_ray* records, int res, int spp_lane, uint64_t seed, uint32_t first_stream,
                      float* maps4 /* n*res*res*4 */, uint32_t flags);                                                          /* host, blocking */
int pt_query_distance_rays_device(pt_scene* scene, int n, const void* d_records /* n pt_ray */, int res, uint64_t seed, uint32_t first_stream,
                                  const void* d_draw_offset /* n*res*res uint32, NULL = all 0 */, void* d_rays /* n*res*res pt_ray */,
                                  uint32_t flags, void* stream);                                                                /* async */
/* pt_grid_*: the lookup side of a probe volume: irradiance at surface points from the SH probes of pt_query_sh and
 * the distance maps of pt_query_distance on one regular grid, what cudapathtracer_amd/rays.py's grid_irradiance computes in numpy or
 * torch. Two scene-free calls shaped as the post-process calls: pt_grid_pack turns the two queries' sums into the form a lookup
 * reads, pt_grid_irradiance looks m points up. No pt_scene is involved and nothing of one is touched.
 * Grid. pt_grid_desc names the grid of rays.sh_grid(lo, hi, counts): probe (ix, iy, iz) is record (iz*ny + iy)*nx + ix, n = nx*ny*nz;
 *   an axis with one probe has it at lo's coordinate, and its hi is not read. sh_samples is lanes*spp_lane of the pt_query_sh call,
 *   map_samples spp_lane of the pt_query_distance call, map_res its res R, or 0 for a grid without maps; power the exponent of the
 *   Chebyshev test. pt_grid_irradiance must be given the desc its packed buffer was made with.
 * Packed buffer, pt_grid_packed_bytes(desc) = n*9*16 + n*(R+2)*(R+2)*8 bytes (R = 0: n*144), aligned to 16 bytes: first n*9 float4
 *   (E_r, E_g, E_b, 0), probe j's convolved coefficient k at j*9 + k; then n*(R+2)*(R+2) float2 (mean, mean square), probe j's
 *   bordered map at j*(R+2)*(R+2), texel (gx, gy) of it at gy*(R+2) + gx: interior texel (tx, ty) is (tx+1, ty+1), and the gutter is
 *   rays.oct_border's: gutter texel (tx, ty), tx or ty one of -1 and R, copies interior texel (sx, sy) from
 *     sx = tx, sy = ty;  tx < 0: sx = -1 - tx, sy = R-1 - ty;   tx > R-1: sx = 2R-1 - tx, sy = R-1 - ty;   then on the result
 *     sy < 0: sy = -1 - sy, sx = R-1 - sx;   sy > R-1: sy = 2R-1 - sy, sx = R-1 - sx.
 * ARITHMETIC, f32, every operation rounded once in the order written, nothing fused but the fmas named; / and sqrt are IEEE; min and
 *   max ignore a NaN operand (v_min_f32, v_max_f32), so no index leaves its range whatever the data.
 *   Pack. scale = (float)(4 pi / sh_samples) (the quotient in double); lobe = (float)pi for k = 0, (float)(2 pi / 3) for k = 1..3,
 *     (float)(pi / 4) for k = 4..8; E_kc = (c_kc * scale) * lobe_k from coeff_sums[j*9 + k]'s channel c. mean = A / (float)map_samples,
 *     mean square = B / (float)map_samples from maps[j*R*R + ty*R + tx] = (A, B, ., .).
 *   Lookup of record (p, n) = (ox, oy, oz), (dx, dy, dz); max_t and pad are NOT read.
 *   1. Any of the six components not finite: out = (0, 0, 0, 0), nothing is indexed.
 *   2. Per axis a with counts_a > 1: inv_a = (float)((counts_a - 1) / ((double)hi_a - lo_a));  g = (p_a - lo_a) * inv_a;
 *      low = min(max(floor(g), 0), counts_a - 2) in float, then converted to int;  f_a = min(max(g - low, 0), 1). The corners of the
 *      axis are probes low and low + 1. An axis with one probe: low = 0, f_a = 0, both corners are probe 0.
 *   3. y_0 = C0;  y_1 = C1*ny;  y_2 = C1*nz;  y_3 = C1*nx;  y_4 = C2*(nx*ny);  y_5 = C2*(ny*nz);  y_6 = C3*(3*(nz*nz) - 1);
 *      y_7 = C2*(nx*nz);  y_8 = C4*(nx*nx - ny*ny), with pt_query_sh's constants 0.2820948, 0.4886025, 1.0925484, 0.3153916, 0.5462742.
 *   4. The eight corners in the order cz, cy, cx with cx fastest, w_a = c_a ? f_a : 1 - f_a:  tri = (w_x * w_y) * w_z;  probe j =
 *      (i_z*ny + i_y)*nx + i_x;  e_c = E_0c * y_0, then e_c = fma(E_kc, y_k, e_c) for k = 1..8;  plain_c = fma(tri, e_c, plain_c)
 *      from plain_c = 0. Without maps W = W + tri from 0, and out = (plain, W).
 *   5. With maps, per corner: step_a = (float)(((double)hi_a - lo_a) / (counts_a - 1)), 0 on an axis with one probe;
 *      at_a = fma((float)i_a, step_a, lo_a);  v = p - at;  dist = sqrt(fma(v_z, v_z, fma(v_y, v_y, v_x*v_x)));  d = dist > 0 ? v :
 *      (0, 0, 1);  s = (|d_x| + |d_y|) + |d_z|;  px = d_x / s;  py = d_y / s;  for d_z < 0:  qx = (1 - |py|) * copysign(1, d_x),
 *      qy = (1 - |px|) * copysign(1, d_y), else qx = px, qy = py;  u = (qx + 1) * 0.5;  v likewise;  gx = u*R + 0.5;
 *      ix = min(max(floor(gx), 0), R);  wx = gx - ix;  gy, iy, wy likewise. On the bordered map, per component of (mean, mean square):
 *      top = t(ix, iy) + wx*(t(ix+1, iy) - t(ix, iy));  bot likewise in row iy + 1;  m = top + wy*(bot - top).
 *      var = m2 - mean*mean;  var > 0 or else var = 0;  t = dist - mean;  den = var + t*t;  ratio = den > 0 ? var / den : 0;
 *      vis = dist <= mean ? 1 : ((ratio*ratio)*ratio)... with `power` factors;  w = tri * vis;  num_c = fma(w, e_c, num_c);  W = W + w.
 *   6. With maps out = W >= 1e-6f ? (num_r / W, num_g / W, num_b / W, W) : (plain_r, plain_g, plain_b, W).
 *   E is in rays.grid_irradiance's units (those of pi * S / N of pt_query_irradiance); W is the weight sum the result was divided by
 *   or, in the fallback and without maps, the sum that was found. A record's output depends on the record, the desc and the packed
 *   buffer only.
 * Checked before any HIP call, -1 with a message under the function's name (pt_grid_packed_bytes: 0), in this order: a NULL desc; a
 *   count below 1 or counts whose product passes 1 << 22; a corner that is not finite, or hi <= lo on an axis with more than one
 *   probe; sh_samples < 1; map_res not one of 0, 4, 8, 16, 32; map_samples < 1 with maps; power outside 1..8; m < 0 (m == 0 then
 *   returns 0); a NULL buffer, maps given although map_res == 0 or missing although it is not; in the device forms the output
 *   overlapping an input.
 * d_coeff_sums (n*9 float4, pt_query_sh's), d_maps (n*R*R float4, pt_query_distance's), d_packed, d_records (m pt_ray) and d_out
 * (m float4) are device buffers aligned to 16 bytes; the device forms are asynchronous on `stream`. */
typedef struct pt_grid_desc {
    float lo[3], hi[3];        /* sh_grid's corners, both included                       */
    int32_t counts[3];         /* nx, ny, nz; probe (ix,iy,iz) is (iz*ny+iy)*nx+ix       */
    int32_t sh_samples;        /* lanes * spp_lane of the pt_query_sh call               */
    int32_t map_res;           /* 0: no maps (plain trilinear); else 4, 8, 16, 32        */
    int32_t map_samples;       /* spp_lane of the pt_query_distance call                 */
    int32_t power;             /* Chebyshev exponent, 1..8 (rays.py's default is 3)      */
} pt_grid_desc;                                                                                                                  /* 52 bytes */
size_t pt_grid_packed_bytes(const pt_grid_desc* desc);                                                                           /* 0 on a bad desc */
int pt_grid_pack_device(const pt_grid_desc* desc, const void* d_coeff_sums /* n*9 float4 */, const void* d_maps /* n*R*R float4, NULL iff map_res == 0 */,
                        void* d_packed, void* stream);                                                                           /* async */
int pt_grid_pack(const pt_grid_desc* desc, const float* coeff_sums /* n*9*4 */, const float* maps4 /* n*R*R*4, NULL iff map_res == 0 */,
                 void* packed);                                                                                                  /* host, blocking */
int pt_grid_irradiance_device(const pt_grid_desc* desc, const void* d_packed, int m, const void* d_records /* m pt_ray */, void* d_out /* m float4 */,
                              void* stream);                                                                                     /* async */
int pt_grid_irradiance(const pt_grid_desc* desc, const void* packed, int m, const pt_ray* records, float* out4 /* m*4 */);       /* host, blocking */

/* pt_grid_classify, pt_grid_update, pt_grid_irradiance_states: a probe volume that stays current. Three scene-free
 * calls beside the five above, shaped as they are: a state word per probe from its distance map's hit counts, a lookup that leaves out
 * the probes found inside an object, and fresh query sums blended into a packed buffer in place. Nothing above changes.
 * States. n uint32, one per probe in the grid's order. PT_PROBE_INSIDE: the probe lies inside an object, lookups skip it.
 *   PT_PROBE_IDLE: no surface within the maps' max_t, so nothing the probe can light is near; lookups still read it, a caller may
 *   spare its re-bake. A lookup reads bit 0 only: junk in the other 31 bits changes nothing.
 * The probe list. k rows of fresh query output, row i that of probe indices[i] (int32). indices == NULL requires k == n and means
 *   the identity. An index outside [0, n) is skipped: that row touches nothing, in the host and the device form alike. A list that
 *   names a probe twice is the caller's error: that probe's result is then one of the rows', and nothing outside it is touched. A
 *   subset re-bake gets the full bake's streams through PT_QUERY_STREAM_PAD with the pad word set to the probe number; by the
 *   queries' independence clause its rows then equal the full bake's bit for bit.
 * ARITHMETIC as above: f32, every operation rounded once in the order written, nothing fused but the fmas named, / is IEEE.
 *   Classify. Per listed probe Hs = sum of H and Ks = sum of K over the R*R texels (C, D of maps[i*R*R + ty*R + tx] = (., ., C, D):
 *     the hits and the hits seen from behind). The values are whole numbers and the totals at most 2^22, so every order of summation
 *     gives the same sum.  state = (Ks > back_fraction * Hs ? PT_PROBE_INSIDE : 0) | (Hs == 0 ? PT_PROBE_IDLE : 0), the product
 *     rounded once. The map's contents are not checked: every comparison with a NaN is false, so a map with a NaN count gives 0.
 *     Only the listed probes' words are written.
 *   Update. Per word of a listed probe's coefficient rows and bordered map, fresh = what pt_grid_pack computes for that word from the
 *     row's sums and map, the gutter's source rule included (desc.sh_samples and desc.map_samples are the FRESH sums' and may differ
 *     from the bake's; counts, lo, hi and map_res must be the buffer's own);  new = hysteresis == 0 ? fresh :
 *     fma(hysteresis, old - fresh, fresh) on E_r, E_g, E_b, on the mean and on the mean square; the fourth word of a coefficient row
 *     is written as 0. A gutter texel blends its own old value with its source's fresh value, so a buffer whose gutter was consistent
 *     stays so. hysteresis 0 over all probes writes pt_grid_pack's buffer.
 *   Lookup with states. Steps 1 to 3 as pt_grid_irradiance. In step 4 a corner whose states[j] & 1 is set loads nothing else and
 *     adds nothing; a live corner does what it does above and also T = T + tri, from T = 0. The output, in this order:
 *       with maps and W >= 1e-6f:       (num_r / W, num_g / W, num_b / W, W), as above;
 *       else if no corner was skipped:  (plain_r, plain_g, plain_b, W), pt_grid_irradiance's result bit for bit;
 *       else if T > 0:                  (plain_r / T, plain_g / T, plain_b / T, W), W the sum that was found; without maps W = T;
 *       else (all corners dead, or the live ones have no weight): exact zeros in all four words.
 *     With every state's bit 0 clear the output is pt_grid_irradiance's bit for bit.
 * Checked before any HIP call, -1 with a message under the function's name, in this order: the desc as above; pt_grid_classify:
 *   map_res == 0; k (or m) < 0 (0 then returns 0); k > n, or NULL indices with k != n; back_fraction not in [0, 1] or hysteresis not
 *   in [0, 1) (a NaN is in neither); a NULL buffer, and maps against map_res as pt_grid_pack checks them; in the device forms a
 *   written buffer overlapping a read one.
 * d_indices (k int32), d_states (n uint32), d_coeff_sums (k*9 float4), d_maps (k*R*R float4), d_packed, d_records and d_out are
 * device buffers, the float4 ones aligned to 16 bytes; the device forms are asynchronous on `stream`. */
#define PT_PROBE_INSIDE 1u   /* the probe lies inside an object: lookups skip it */
#define PT_PROBE_IDLE   2u   /* no surface within the maps' max_t: nothing it can light is near; lookups still read it */
int pt_grid_classify_device(const pt_grid_desc* desc, int k, const void* d_indices /* k int32, or NULL: k == n, probe i */,
                            const void* d_maps /* k*R*R float4, pt_query_distance's */, float back_fraction,
                            void* d_states /* n uint32, entry indices[i] written */, void* stream);                              /* async */
int pt_grid_classify(const pt_grid_desc* desc, int k, const int32_t* indices, const float* maps4 /* k*R*R*4 */, float back_fraction,
                     uint32_t* states /* n */);                                                                                  /* host, blocking */
int pt_grid_update_device(const pt_grid_desc* desc, int k, const void* d_indices, const void* d_coeff_sums /* k*9 float4 */,
                          const void* d_maps /* k*R*R float4; NULL iff map_res == 0 */, float hysteresis,
                          void* d_packed /* read and written in place */, void* stream);                                         /* async */
int pt_grid_update(const pt_grid_desc* desc, int k, const int32_t* indices, const float* coeff_sums /* k*9*4 */,
                   const float* maps4 /* k*R*R*4, NULL iff map_res == 0 */, float hysteresis, void* packed);                      /* host, blocking */
int pt_grid_irradiance_states_device(const pt_grid_desc* desc, const void* d_packed, const void* d_states /* n uint32 */,
                                     int m, const void* d_records /* m pt_ray */, void* d_out /* m float4 */, void* stream);      /* async */
int pt_grid_irradiance_states(const pt_grid_desc* desc, const void* packed, const uint32_t* states /* n */, int m, const pt_ray* records,
                              float* out4 /* m*4 */);                                                                            /* host, blocking */

/* pt_grid_relocate, pt_grid_irradiance_offsets: probes that move out of the way. Two scene-free calls beside the
 * eight above, shaped as they are: an offset per probe from its distance map, so that a probe found inside an object moves out
 * through the nearest back face instead of going dark and a probe just in front of a wall steps back from it; and the lookup that
 * reads a probe's position as grid position + offset. Nothing above changes.
 * Offsets. n float4, one per probe in the grid's order: (dx, dy, dz) the probe's displacement from its grid position in world units;
 *   word 3 what the last relocation did to the probe, as a float: 0 kept, 1 pushed out through a back face, 2 pushed off a front
 *   face. A lookup reads words 0 to 2 only. The caller bakes a moved probe at grid position + offset (rays.sh_grid(offsets=...)).
 * The probe list (k, indices, maps) is pt_grid_classify's: row i is probe indices[i], NULL indices need k == n, an index outside
 *   [0, n) is skipped. Only the listed probes' offsets are written. The indices must be distinct: a listed probe's offset is read
 *   and then written, so for a probe named twice the result is unspecified (one row's move, or one applied after the other);
 *   nothing outside that probe's entry is touched.
 * ARITHMETIC as above: f32, every operation rounded once in the order written, nothing fused but the fmas named, / and sqrt IEEE, min
 *   and max ignore a NaN operand (v_min_f32, v_max_f32).
 *   Relocate. Per texel l = ty*R + tx of a listed probe's map, (A, ., H, K) = maps[i*R*R + l]:  m = A / (float)map_samples, the
 *     pack's mean bit for bit;  back = (K + K > H);  front = (H > 0) && !back;  the texel is a candidate only if m >= 0 is true (a
 *     NaN or a negative mean is none).  Hs = sum of H, Ks = sum of K, inside = Ks > back_fraction * Hs: pt_grid_classify's bits.
 *     The chosen texel: among the candidates with `back` if inside, else among those with `front`, the one with the smallest m by
 *     f32 comparison (+0 and -0 are equal), ties to the smaller l. The key (m, l) is total, so the order of the reduction is free.
 *     c = the direction of the chosen texel's centre: pt_query_distance's DIRECTION ARITHMETIC with u1 = u2 = 0.5, operation for
 *     operation. With old = the offset read:
 *       inside and a texel was chosen:                     t = m + 0.5f*min_dist;  new_a = fma(c_a, t, old_a);   code 1
 *       not inside, a texel was chosen and m < min_dist:   t = min_dist - m;       new_a = fma(-c_a, t, old_a);  code 2
 *       otherwise:                                         new = old;                                            code 0
 *     then in every case new_a = min(max(new_a, -max_offset_a), max_offset_a): a written offset lies in the box whatever was read,
 *     a NaN included. The sign of a zero that the clamp produces is not part of the contract. max_offset should stay under half a
 *     cell, since the lookup's cell and trilinear weights stay the regular grid's.
 *   Lookup with offsets. pt_grid_irradiance_states' lookup with one change in step 5: the probe stands at
 *     at_a = fma((float)i_a, step_a, lo_a) + off_a, one rounded add per axis. The cell, tri and the corner order are unchanged.
 *     states == NULL means that no probe is dead: no state word is read and the end is pt_grid_irradiance's step 6 (plain_c and W).
 *     With every offset +0 or -0 the output is pt_grid_irradiance's (states NULL) and pt_grid_irradiance_states' (states given) bit
 *     for bit: fma(i, step, lo) with i >= 0 and step >= 0 is never -0 (the product is +0 or positive, and a sum that cancels rounds
 *     to +0), and x + (+-0) = x for every x but -0.
 * Checked before any HIP call, -1 with a message under the function's name, in this order: the desc as above; map_res == 0 (a grid
 *   without maps has no positions to read); k (or m) < 0 (0 then returns 0); pt_grid_relocate: k > n, or NULL indices with k != n;
 *   back_fraction not in [0, 1]; min_dist not finite or < 0; a max_offset component not finite or < 0; a NULL buffer (max_offset
 *   among them; states may be NULL in the lookup only); in the device forms a written buffer overlapping a read one.
 * max_offset is three floats in host memory in both forms. d_offsets (n float4) is a device buffer aligned to 16 bytes, read and
 * written by pt_grid_relocate_device; the other buffers are as above; the device forms are asynchronous on `stream`. */
int pt_grid_relocate_device(const pt_grid_desc* desc, int k, const void* d_indices /* k int32, or NULL: k == n, probe i */,
                            const void* d_maps /* k*R*R float4, pt_query_distance's */, float back_fraction, float min_dist,
                            const float* max_offset /* 3, host */, void* d_offsets /* n float4, entry indices[i] read and written */,
                            void* stream);                                                                                       /* async */
int pt_grid_relocate(const pt_grid_desc* desc, int k, const int32_t* indices, const float* maps4 /* k*R*R*4 */, float back_fraction,
                     float min_dist, const float* max_offset /* 3 */, float* offsets4 /* n*4, read and written */);             /* host, blocking */
int pt_grid_irradiance_offsets_device(const pt_grid_desc* desc, const void* d_packed, const void* d_states /* n uint32, or NULL */,
                                      const void* d_offsets /* n float4 */, int m, const void* d_records /* m pt_ray */,
                                      void* d_out /* m float4 */, void* stream);                                                 /* async */
int pt_grid_irradiance_offsets(const pt_grid_desc* desc, const void* packed, const uint32_t* states /* n, or NULL */,
                               const float* offsets4 /* n*4 */, int m, const pt_ray* records, float* out4 /* m*4 */);            /* host, blocking */

/* For tools (tools/update_time.py): host wall clock, in ms, of parts of the scene's last build. out3[0]: the renumbering of the
 * internal nodes by area through the host, in the last successful update or, before any, at creation (0 for a scene of at most
 * 128 internal nodes, which is not renumbered); out3[1]: the whole last successful update (0 before any); out3[2]: 0. */
int pt_debug_update_ms(pt_scene* scene, float* out3);
/* Test hook, host only (needs no device): out[i], for each of desc->n_lights lights, is the position in leaf order
 * (desc->bvh_indices) of the scene triangle the light was made from — the triangle whose lightInd is i and whose packed
 * v0, e1 = b - a, e2 = c - a equal the light's bit for bit — or -1. Only positions below 63 are reported: the table serves
 * the kernels for scenes of at most 64 triangles, which do not test a shadow ray against the light it was aimed at. */
int pt_light_triangles(const pt_scene_desc* desc, int32_t* out);
int novum_bvh_build_host(const pt_float4* positions, int n_positions, const pt_triangle* triangles, int n_triangles,
                         int max_leaf_size, pt_bvh_node* nodes_out, int nodes_capacity,
                         int32_t* indices_out, pt_bvh_build_stats* stats);

/* ---- novum_*: the kept host side (scene loader / initRender) --------------------------- */
typedef struct novum_scene novum_scene;    /* host arrays + RenderConfig + Camera */

/* loadConfig (objects.cuh:844-943) + material table (main.cu:397-467) + readObjSimple per mesh
 * (main.cu:474-482, 936-1068) + computeInfoForBVH/buildBVH (main.cu:524-530) + camera
 * (main.cu:268-273). Mesh paths are resolved against base_dir (NULL = directory of the config). */
novum_scene* novum_scene_load(const char* config_path, const char* base_dir, int render_number);
/* Same, choosing who runs buildBVH: the host (as the reference does) or pt_bvh_build_device (f-4).
 * Both give the same arrays. */
#define NOVUM_BVH_HOST 0
#define NOVUM_BVH_DEVICE 1
novum_scene* novum_scene_load_ex(const char* config_path, const char* base_dir, int render_number, int bvh_builder);
void novum_scene_free(novum_scene* s);
/* info[16]: width,height,spp,maxDepth,integrator,leafSize,nTris,nLights,nNodes,nPoints,nNormals,
 * nUvs,nMats,largestLeaf,backupCount,treeDepth */
void novum_scene_info(const novum_scene* s, int32_t* info16);
void novum_scene_desc(const novum_scene* s, pt_scene_desc* out);     /* pointers stay owned by s */
void novum_scene_camera(const novum_scene* s, pt_camera* out);
/* Camera::Pinhole / Camera::NotPinhole (objects.cuh:221-264) */
void novum_make_camera(int pinhole, const float* pos3, const float* rot3, float fov, float aperture, float focal_dist, int w, int h, pt_camera* out);
/* main.cu:860-870: colors /= spp; NaN -> (1,0,1); Inf -> (0,1,0). n = pixel count. */
void novum_finalise(float* rgba, int n, int sample_count);
/* initRender (main.cu:235-923) for the two unidirectional integrators: load, upload, launch,
 * read back, finalise into out_rgba (w*h float4, may be NULL) and, if bmp_path != NULL, write the
 * tonemapped 24-bit BMP (imageUtil.cu:69-100, 202-232). Returns 0, or < 0 on error. */
int novum_init_render(const char* config_path, const char* base_dir, int render_number, float* out_rgba, const char* bmp_path);
/* Image::saveImageBMP (imageUtil.cu:69-100): rgba is w*h float4 linear radiance, y = 0 bottom. */
int novum_save_bmp(const char* path, const float* rgba, int w, int h, int post_process);
/* Image::saveImageCSV_MONO(channel) (imageUtil.cu:123-142): one channel, scientific, 3 digits. */
int novum_save_csv_mono(const char* path, const float* rgba, int w, int h, int channel);
/* initRender with the reference's progressive preview (deviceCode.cu:574-604): renders in chunks of
 * chunk_spp samples and, whenever at least interval_seconds have passed since the last preview,
 * writes the running average to preview_bmp (and preview_csv if not NULL), as the reference does with
 * render.bmp / renderCSV.csv every 5 s. Final image as novum_init_render. */
int novum_init_render_progressive(const char* config_path, const char* base_dir, int render_number, float* out_rgba,
                                  const char* bmp_path, const char* preview_bmp, const char* preview_csv,
                                  double interval_seconds, int chunk_spp);

#ifdef __cplusplus
}
#endif
#endif /* PT_API_H */
