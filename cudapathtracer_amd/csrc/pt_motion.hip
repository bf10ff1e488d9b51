// pt_motion.hip — the motion pass (pt_render_motion, include/pt_api.h): for the centre ray of each pixel, where the surface point it
// hits WAS before the scene's most recent vertex update. pt_temporal_accumulate_motion reprojects that point in place of the one on
// the ray, so a surface that moved finds the history it left behind.
//
// pt_feature.h's FeatureWave and tile loop around the centre ray, as aov_centre_kernel (pt_aov.hip). After the traversal the hit's
// original triangle index names three vertex indices in the scene's kept pt_triangle array, and those name three current and three
// previous positions: three int32 loads, then six float4 loads, all dependent on the hit, none live across the traversal. The previous
// point is the barycentric sum of the previous positions with resolve_hit's weights, every operation rounded once (no fma).
// With albedo / normalDepth set the kernel also writes first_hit_record of the same hit: aov_centre_kernel's output.
// MotionSrc, what the pass reads beside the packed scene, is in pt_feature.h: pt_motion_chain.hip's pass through mirrors and glass
// reads the same.
#include "pt_feature.h"
#include "../../include/pt_api.h"

namespace pt {

__global__ void __launch_bounds__(256) motion_kernel(DeviceScene S, MotionSrc M, CamK cam, int w, int h, int tilesX, int nTiles,
                                                     float4* __restrict__ albedo, float4* __restrict__ normalDepth, float4* __restrict__ motion,
                                                     int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    FeatureWave W(ldsStack, S, spill);
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        const TilePixel p = tile_pixel(tile, tilesX, W.lane, w, h);
        if (!p.inside) continue;
        const size_t idx = (size_t)p.y * w + p.x;
        V3 o, d;
        camera_ray_centre(cam, p.x, p.y, o, d);
        Hit hit;
        trace_closest<false, kStackLds>(S, W.C, o, d, 999999.0f, W.st, hit, W.c);
        float4 om = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (hit.tri >= 0 && M.prev != nullptr) {
            const pt_triangle& T = M.tris[hit.tri];
            const int ia = T.aInd, ib = T.bInd, ic = T.cInd;
            // (the builder refused the mesh if an index were out of range: the test only keeps a corrupt array from a wild read)
            if ((unsigned)ia < (unsigned)M.nPos && (unsigned)ib < (unsigned)M.nPos && (unsigned)ic < (unsigned)M.nPos) {
                const float4 a = M.cur[ia], b = M.cur[ib], cc = M.cur[ic];
                const float4 pa = M.prev[ia], pb = M.prev[ib], pc = M.prev[ic];
                const bool still = a.x == pa.x && a.y == pa.y && a.z == pa.z && b.x == pb.x && b.y == pb.y && b.z == pb.z &&
                                   cc.x == pc.x && cc.y == pc.y && cc.z == pc.z;
                if (!still) {
                    const float bz = 1.0f - hit.u - hit.v;         // as resolve_hit forms it
                    om = make_float4(pa.x * bz + pb.x * hit.u + pc.x * hit.v, pa.y * bz + pb.y * hit.u + pc.y * hit.v,
                                     pa.z * bz + pb.z * hit.u + pc.z * hit.v, 1.0f);
                }
            }
        }
        motion[idx] = om;
        if (albedo != nullptr) {                                   // (uniform: a kernel argument)
            float4 oa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), on = oa;
            if (hit.tri >= 0) { HitInfo hi; resolve_hit(S, hit, o, d, hi); first_hit_record(S, hi, hit.t, oa, on); }
            albedo[idx] = oa;
            normalDepth[idx] = on;
        }
    }
}

hipError_t launch_motion(const DeviceScene& S, const void* tris, const void* posCur, const void* posPrev, int nPos, const CamK& cam, int w, int h,
                         int blocks, float4* albedo, float4* normalDepth, float4* motion, int32_t* spill, hipStream_t stream) {
    const FeatureTiles T = feature_tiles(w, h);
    MotionSrc M;
    M.tris = (const pt_triangle*)tris; M.cur = (const float4*)posCur; M.prev = (const float4*)posPrev; M.nPos = nPos;
    hipLaunchKernelGGL(motion_kernel, dim3(blocks), dim3(256), 0, stream, S, M, cam, w, h, T.tilesX, T.nTiles, albedo, normalDepth, motion, spill);
    return hipGetLastError();
}

}  // namespace pt
