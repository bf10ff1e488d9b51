// pt_feature_host.h — the host's view of the feature passes (pt_aov.hip, pt_motion.hip, pt_motion_chain.hip, pt_ids.hip) and of the ray
// queries (pt_query.hip, pt_query_guides.hip, pt_radiance.hip, pt_radiance_moments.hip, pt_irradiance.hip, pt_sh.hip, pt_distance.hip): the tiling and block count every one of them is
// launched with, each kernel's waves per SIMD, and the launchers pt_feature_api.hip calls. The kernels' shared pieces are in
// pt_feature.h, the radiance kernels' walk in pt_radiance.h.
#pragma once
#include <algorithm>
#include "pt_params.h"

namespace pt {

// One wave per 8x8 tile, tiles in row-major order.
struct FeatureTiles { int tilesX, nTiles; };
inline FeatureTiles feature_tiles(int w, int h) {
    const int tilesX = (w + 7) / 8;
    return {tilesX, tilesX * ((h + 7) / 8)};
}

// Workgroups of a feature pass: four waves each, persistent over the tiles, as many as are resident at once at the kernel's waves per
// SIMD (= workgroups per CU). Each kernel's count comes from its own resources (the table in DESIGN.md §9):
constexpr int kAovWavesPerSimd = 6;          // aov_kernel: 76 VGPRs (the stream seeding), 16 KB of LDS per workgroup
constexpr int kAovChainWavesPerSimd = 6;     // aov_chain_kernel: 80 VGPRs, 23 KB of LDS: 6 workgroups are 138 of the CU's 160 KB. Also
                                             // aov_centre_chain_kernel (69 VGPRs, 23 KB): 7 workgroups would need 161 KB
constexpr int kAovCentreWavesPerSimd = 8;    // aov_centre_kernel: without the seeding 63 VGPRs, 8 x 16 KB of LDS
constexpr int kMotionWavesPerSimd = 8;       // motion_kernel: 63 VGPRs, 8 x 16 KB of LDS, as the centre pass
constexpr int kMotionChainWavesPerSimd = 5;  // motion_chain_kernel: 93 VGPRs (the unfolding matrix stays in registers), 26 KB of LDS: 6 workgroups
                                             // would fit the LDS, 5 waves fit the registers
constexpr int kIdsWavesPerSimd = 8;          // ids_kernel: 63 VGPRs, 8 x 16 KB of LDS, as the centre pass
constexpr int kIdsChainWavesPerSimd = 6;     // ids_chain_kernel: 76 VGPRs, 18 KB of LDS (the compiler drops follow_chain's record, which the
                                             // kernel never reads): register-bound at aov_centre_chain_kernel's 6
constexpr int kQueryClosestWavesPerSimd = 8; // query_closest_kernel<false>: 59 VGPRs, 8 x 16 KB of LDS, as the centre pass
constexpr int kQuerySurfaceWavesPerSimd = 8; // query_closest_kernel<true>: 55 VGPRs, 8 x 16 KB of LDS
constexpr int kQueryShadowWavesPerSimd = 8;  // query_shadow_kernel: 56 VGPRs, 8 x 16 KB of LDS
// radiance_kernel<INTEG, SIMPLE, LEAN> (pt_radiance.hip): the waves per SIMD each instantiation is launched at and compiled for
// (amdgpu_waves_per_eu), from the compile and, where one step more costs scratch, from the measurement. VGPRs /
// scratch bytes per lane at the setting, and at the one not taken:
//   naive, SIMPLE    6: 79 / 0     (8: 64 / 52, +13 % on the blob)      MIS, SIMPLE    6: 80 / 28    (5: 91 / 0, 4-6 % slower)
//   naive, LEAN      5: 94 / 0     (6: 80 / 72, level)                  MIS, LEAN      5: 96 / 84    (4: 118 / 0, 11 % slower)
//   naive, generic   4: 96 / 0     (5: 96 / 20)                         MIS, generic   4: 128 / 12   (5: 96 / 148; 3: 131 / 0)
// LDS: 16 KB of stacks, and 4 KB of medium stacks in the kernels that are not SIMPLE: 8 workgroups fit a CU either way.
constexpr int radiance_waves_per_simd(int integrator, bool simple, bool lean) { return simple ? 6 : lean ? 5 : 4; }
// radiance_moments_kernel<INTEG, SIMPLE, LEAN> (pt_radiance_moments.hip): radiance_kernel's settings, unmeasured against their
// neighbours. With the batch bookkeeping in LDS (7 KB more per workgroup), VGPRs / scratch bytes per lane, and with
// it in registers:
//   naive, SIMPLE    6: 80 / 0     (registers: 80 / 16)                 MIS, SIMPLE    6: 80 / 36    (registers: 80 / 64)
//   naive, LEAN      5: 95 / 0     (registers: 96 / 20)                 MIS, LEAN      5: 96 / 88    (registers: 96 / 112)
//   naive, generic   4: 97 / 0     (registers: 103 / 0)                 MIS, generic   4: 128 / 12   (registers: 128 / 28)
// LDS: 23 KB in the SIMPLE kernels (6 workgroups: 138 KB), 27 KB in the others (5: 135 KB).
constexpr int radiance_moments_waves_per_simd(int integrator, bool simple, bool lean) { return simple ? 6 : lean ? 5 : 4; }
// irradiance_kernel<INTEG, SIMPLE, LEAN> (pt_irradiance.hip): radiance_kernel's settings and LDS; the lanes' tree is wave shuffles
// after the walk. VGPRs / scratch bytes per lane at the setting, and radiance_kernel's beside them: the sample's start, which there
// is two loads, is here a square root, a sincos and a basis, and four of the six kernels pay for it in 12 to 20 bytes of scratch
// (tests/test_query_irradiance_api.py pins the table):
//   naive, SIMPLE    6: 80 / 16    (79 / 0)                                 MIS, SIMPLE    6: 80 / 40    (80 / 28)
//   naive, LEAN      5: 95 / 20    (94 / 0)                                 MIS, LEAN      5: 96 / 100   (96 / 84)
//   naive, generic   4: 100 / 0    (96 / 0)                                 MIS, generic   4: 128 / 8    (128 / 12)
constexpr int irradiance_waves_per_simd(int integrator, bool simple, bool lean) { return radiance_waves_per_simd(integrator, simple, lean); }
// Its tiles: n records of 1 << log2L lanes each, 64 lanes a tile (n << log2L is at most 1 << 28).
constexpr int irradiance_tiles(int n, int log2L) { return ((n << log2L) + 63) / 64; }
// sh_kernel<INTEG, SIMPLE, LEAN> (pt_sh.hip): the lanes' 27 sums and the sample's direction are 30 LDS words a lane, 30 720 bytes a
// workgroup on top of the class's 16 or 20 KB: three workgroups fit a CU's 160 KB, so the kernels are compiled for and launched at
// min(radiance_kernel's waves, 3). At 3 waves a SIMD has 168 VGPRs a lane to give, and no kernel needs scratch. VGPRs / scratch
// bytes per lane / LDS bytes (tests/test_query_sh_api.py pins the table):
//   naive, SIMPLE    3: 79 / 0 / 47104                                    MIS, SIMPLE    3: 91 / 0 / 47104
//   naive, LEAN      3: 96 / 0 / 51200                                    MIS, LEAN      3: 119 / 0 / 51200
//   naive, generic   3: 96 / 0 / 51200                                    MIS, generic   3: 131 / 0 / 51200
constexpr int sh_waves_per_simd(int integrator, bool simple, bool lean) { return std::min(radiance_waves_per_simd(integrator, simple, lean), 3); }
constexpr int kDistanceWavesPerSimd = 7;         // distance_kernel<false> (pt_distance.hip): 66 VGPRs (the stream and the four sums stay live across
                                                 // the trace), 16 KB of LDS, no scratch (tests/test_query_distance_api.py pins both)
constexpr int kDistanceCentreWavesPerSimd = 8;   // distance_kernel<true>: without the stream 54 VGPRs, 8 x 16 KB of LDS
constexpr int kQueryGuidesWavesPerSimd = 8;      // query_guides_kernel: 55 VGPRs, 8 x 16 KB of LDS, as the centre pass
constexpr int kQueryGuidesChainWavesPerSimd = 6;  // query_guides_chain_kernel: 60 VGPRs, 23 KB of LDS: 7 workgroups would need 161 KB
inline int feature_blocks(int nTiles, int numCU, int wavesPerSimd) { return std::max(1, std::min((nTiles + 3) / 4, numCU * wavesPerSimd)); }

// spill (every launcher): blocks * 4 waves x S.stackSpill entries x 64 lanes, or NULL for a scene whose stack never leaves the LDS.
// pt_aov.hip
hipError_t launch_aov(const DeviceScene& S, const CamK& cam, const uint32_t* jump, unsigned long long seed, int w, int h, int aovSpp,
                      int blocks, float4* albedo, float4* normalDepth, int32_t* spill, hipStream_t stream);
hipError_t launch_aov_chain(const DeviceScene& S, const CamK& cam, const uint32_t* jump, unsigned long long seed, int w, int h, int aovSpp,
                            int maxLinks, int blocks, float4* albedo, float4* normalDepth, float* links, int32_t* spill, hipStream_t stream);
hipError_t launch_aov_centre(const DeviceScene& S, const CamK& cam, int w, int h, int blocks, float4* albedo, float4* normalDepth, int32_t* spill,
                             hipStream_t stream);
hipError_t launch_aov_centre_chain(const DeviceScene& S, const CamK& cam, int w, int h, int maxLinks, int blocks, float4* albedo, float4* normalDepth,
                                   float* links, int32_t* spill, hipStream_t stream);
hipError_t launch_probe_centre(const CamK& cam, int n, const int* xy, float* out, hipStream_t stream);
// pt_motion.hip
hipError_t launch_motion(const DeviceScene& S, const void* tris, const void* posCur, const void* posPrev, int nPos, const CamK& cam, int w, int h,
                         int blocks, float4* albedo, float4* normalDepth, float4* motion, int32_t* spill, hipStream_t stream);
// pt_motion_chain.hip
hipError_t launch_motion_chain(const DeviceScene& S, const void* tris, const void* posCur, const void* posPrev, int nPos, const CamK& cam, int w,
                               int h, int maxLinks, int blocks, float4* albedo, float4* normalDepth, float* links, float4* motion, int32_t* spill,
                               hipStream_t stream);
// pt_ids.hip: the first-hit kernel for maxLinks 0, else the chain kernel. xy NULL: the w x h tile map, hit NULL. xy set: nPick pixels,
// one lane each, ids and hit indexed by entry.
hipError_t launch_ids(const DeviceScene& S, const CamK& cam, int w, int h, int maxLinks, const int32_t* xy, int nPick, int blocks, int4* ids,
                      float4* hit, int32_t* spill, hipStream_t stream);
// pt_query.hip: n rays (pt_ray), "tile" t being rays 64 t .. 64 t + 63. perm NULL: lane i takes ray i; else ray perm[i], outputs at perm[i].
// surfaces NULL: the hits-only kernel. launch_query_keys: every ray's sort key and its index; query_sort: rocprim's radix sort of
// those pairs (temp NULL: only *tempBytes, the workspace it needs for n pairs, is set). The keys read the root's record: rootRef >= 0.
hipError_t launch_query_closest(const DeviceScene& S, int n, const void* rays, const uint32_t* perm, int blocks, void* hits, void* surfaces,
                                int32_t* spill, hipStream_t stream);
hipError_t launch_query_shadow(const DeviceScene& S, int n, const void* rays, const uint32_t* perm, int blocks, void* throughput, int32_t* spill,
                               hipStream_t stream);
hipError_t launch_query_camera_rays(const CamK& cam, int w, int h, float maxT, void* rays, hipStream_t stream);
hipError_t launch_query_keys(const DeviceScene& S, int n, const void* rays, uint32_t* keys, uint32_t* idx, hipStream_t stream);
hipError_t query_sort(void* temp, size_t* tempBytes, const uint32_t* keysIn, uint32_t* keysOut, const uint32_t* idxIn, uint32_t* idxOut, int n,
                      hipStream_t stream);
// pt_radiance.hip: radiance_kernel<integrator, simple, lean> on n rays, ray i on stream firstStream + i of `seed` (streamPad: + its pad
// word instead of i), spp samples each, out[i] = (the sum of its samples' Li, 0). blocks: feature_blocks at radiance_waves_per_simd.
hipError_t launch_radiance(const DeviceScene& S, int integrator, bool simple, bool lean, int n, const void* rays, const uint32_t* jump,
                           unsigned long long seed, uint32_t firstStream, bool streamPad, int spp, int maxDepth, int useMIS, int blocks, void* out,
                           int32_t* spill, hipStream_t stream);
// pt_radiance_moments.hip: radiance_moments_kernel likewise, the spp samples in batches of batchSpp (spp a multiple of it): out[i] as
// launch_radiance writes it, sq[i] = (the sum of the ray's squared batch sums, spp / batchSpp). blocks: feature_blocks at
// radiance_moments_waves_per_simd.
hipError_t launch_radiance_moments(const DeviceScene& S, int integrator, bool simple, bool lean, int n, const void* rays, const uint32_t* jump,
                                   unsigned long long seed, uint32_t firstStream, bool streamPad, int spp, int batchSpp, int maxDepth, int useMIS,
                                   int blocks, void* out, void* sq, int32_t* spill, hipStream_t stream);
// pt_irradiance.hip: irradiance_kernel<integrator, simple, lean> on n records (pt_ray: point, max_t, unit normal, pad) of 1 << log2L
// lanes each, lane l of record i on stream firstStream + (i << log2L) + l of `seed` (streamPad: the record's pad word for i), sppLane
// samples per lane: out[i] = (the adjacent-pair tree over the lanes' sums, 0), sq[i] (NULL ok) = (the tree over their squares, lanes).
// blocks: feature_blocks of irradiance_tiles at irradiance_waves_per_simd. launch_irradiance_rays: rays[(i << log2L) + l] = the ray
// such a lane's sample starts from, after skip[...] draws of its stream (skip NULL: none); one thread per ray, no scene.
hipError_t launch_irradiance(const DeviceScene& S, int integrator, bool simple, bool lean, int n, const void* recs, int log2L, const uint32_t* jump,
                             unsigned long long seed, uint32_t firstStream, bool streamPad, int sppLane, int maxDepth, int useMIS, int blocks, void* out,
                             void* sq, int32_t* spill, hipStream_t stream);
hipError_t launch_irradiance_rays(int n, const void* recs, int log2L, const uint32_t* jump, unsigned long long seed, uint32_t firstStream,
                                  bool streamPad, const void* skip, void* rays, hipStream_t stream);
// pt_sh.hip: sh_kernel<integrator, simple, lean> on n records (pt_ray: point, max_t; the direction words are not read) of 1 << log2L
// lanes each, log2L 0..12, lanes and streams as launch_irradiance has them. log2L <= 6: out[9 i + k] = (the tree over the lanes' sums
// of Li * Y_k, 0), work is not read. log2L > 6: work[9 t + k] = tile t's tree, and launch_sh_reduce, on the same stream behind it,
// writes out[9 i + k] = the tree over record i's (1 << log2L) / 64 tiles. blocks: feature_blocks of irradiance_tiles at
// sh_waves_per_simd. launch_sh_rays: launch_irradiance_rays for these records.
hipError_t launch_sh(const DeviceScene& S, int integrator, bool simple, bool lean, int n, const void* recs, int log2L, const uint32_t* jump,
                     unsigned long long seed, uint32_t firstStream, bool streamPad, int sppLane, int maxDepth, int useMIS, int blocks, void* out,
                     void* work, int32_t* spill, hipStream_t stream);
hipError_t launch_sh_reduce(int n, int log2L, const void* work, void* out, hipStream_t stream);
hipError_t launch_sh_rays(int n, const void* recs, int log2L, const uint32_t* jump, unsigned long long seed, uint32_t firstStream, bool streamPad,
                          const void* skip, void* rays, hipStream_t stream);
// pt_distance.hip: distance_kernel<centre> on n records (pt_ray: point, max_t; the direction words are not read) of R * R lanes each,
// R = 1 << log2R in 4..32, lane l = ty * R + tx being texel (tx, ty) of the record's octahedral map, on launch_irradiance's streams
// with log2L = 2 log2R; sppLane samples per lane: out[i * R * R + l] = (the sum of the samples' distances, of their squares, the hits,
// the hits seen from behind). centre: one sample at the texel's centre; jump, seed, firstStream, streamPad and sppLane are not read.
// blocks: feature_blocks of irradiance_tiles at kDistanceWavesPerSimd / kDistanceCentreWavesPerSimd. launch_distance_rays:
// launch_irradiance_rays for these lanes (centre: skip is not read, the pad word is the lane's index in the launch).
hipError_t launch_distance(const DeviceScene& S, int n, const void* recs, int log2R, const uint32_t* jump, unsigned long long seed, uint32_t firstStream,
                           bool streamPad, bool centre, int sppLane, int blocks, void* out, int32_t* spill, hipStream_t stream);
hipError_t launch_distance_rays(int n, const void* recs, int log2R, const uint32_t* jump, unsigned long long seed, uint32_t firstStream, bool streamPad,
                                bool centre, const void* skip, void* rays, hipStream_t stream);
// pt_query_guides.hip: n rays, lane i of tile t takes ray 64 t + i. maxLinks 0: the first-hit kernel (links, if set, gets zeros); else
// the chain kernel. albedo[i] = (a, 1), normalDepth[i] = (n, summed path length), links[i] (NULL ok) the links followed; a miss: zeros.
hipError_t launch_query_guides(const DeviceScene& S, int n, const void* rays, int maxLinks, int blocks, void* albedo, void* normalDepth, float* links,
                               int32_t* spill, hipStream_t stream);

}  // namespace pt
