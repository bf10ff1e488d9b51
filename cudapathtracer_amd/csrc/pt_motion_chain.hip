// pt_motion_chain.hip — the motion pass through mirrors and glass (pt_render_motion_chain, include/pt_api.h): the centre ray of each
// pixel followed as aov_centre_chain_kernel follows it (pt_feature.h's follow_chain), and for the surface the chain ends on, where its
// VIRTUAL IMAGE was before the scene's most recent vertex update. For planar mirrors `ray origin + ray direction * summed path length`
// is the virtual image of the surface point, and the image of where that point was is it plus the point's displacement reflected
// through the mirrors, last mirror first. pt_temporal_accumulate_motion reprojects that point as it does pt_render_motion's.
//
// MotionChain is the kernel's ChainHook. Per lane it keeps, across the traversals, the nine floats of the unfolding matrix (identity;
// at a link that reflected at normal n every row r becomes r - 2 (r . n) n) and one bit "a link's triangle moved". The normals of
// up to 16 links are never kept. The motion pixel is not kept either: the first hit's (pt_render_motion's pixel) is stored when the
// first hit is seen, and the store is repeated where the chain ends on a surface behind at least one link, so the pixel of a chain
// that leaves the scene or reaches the cap stays the first hit's, as follow_chain's record does. The centre ray is formed again
// where the chain ends. At every hit whose outcome needs it: triangle_moved's nine dependent loads.
#include "pt_feature.h"

namespace pt {

// Whether triangle `tri` (a Hit::tri) MOVED in the last update: some of the nine floats of its current positions differs from the
// previous ones. pa, pb, pc are its previous positions when it did. Three int32 loads, then six float4 loads, all dependent on the
// hit: motion_kernel's test. Call it only where M.prev is set.
// (the builder refused the mesh if an index were out of range: the test only keeps a corrupt array from a wild read)
PT_DEV bool triangle_moved(const MotionSrc& M, int tri, float4& pa, float4& pb, float4& pc) {
    const pt_triangle& T = M.tris[tri];
    const int ia = T.aInd, ib = T.bInd, ic = T.cInd;
    if (!((unsigned)ia < (unsigned)M.nPos && (unsigned)ib < (unsigned)M.nPos && (unsigned)ic < (unsigned)M.nPos)) return false;
    const float4 a = M.cur[ia], b = M.cur[ib], cc = M.cur[ic];
    pa = M.prev[ia]; pb = M.prev[ib]; pc = M.prev[ic];
    return !(a.x == pa.x && a.y == pa.y && a.z == pa.z && b.x == pb.x && b.y == pb.y && b.z == pb.z && cc.x == pc.x && cc.y == pc.y &&
             cc.z == pc.z);
}

// Where the point with barycentrics (u, v) of a triangle was, given its previous positions: (P', 1), every operation rounded once.
PT_DEV float4 previous_point(const float4& pa, const float4& pb, const float4& pc, float u, float v) {
    const float bz = 1.0f - u - v;                                 // as resolve_hit forms it
    return make_float4(pa.x * bz + pb.x * u + pc.x * v, pa.y * bz + pb.y * u + pc.y * v, pa.z * bz + pb.z * u + pc.z * v, 1.0f);
}

struct MotionChain {
    const MotionSrc& src;
    const CamK& cam;
    int maxLinks;
    float4* out;                // the lane's motion pixel
    const float* ray;           // ray[0], ray[64], ray[128]: the centre ray's direction, in the lane's LDS words
    V3 m0, m1, m2;              // the rows of the unfolding matrix
    bool linkMoved;
    PT_DEV MotionChain(const MotionSrc& src_, const CamK& cam_, int maxLinks_, float4* out_, const float* ray_)
        : src(src_), cam(cam_), maxLinks(maxLinks_), out(out_), ray(ray_), m0(v3(1.0f, 0.0f, 0.0f)), m1(v3(0.0f, 1.0f, 0.0f)), m2(v3(0.0f, 0.0f, 1.0f)),
          linkMoved(false) {}

    PT_DEV void surface(int i, const Hit& hit, const HitInfo& hi, bool spec, float depth) {
        const bool ends = i == 0 || !spec, follows = spec && i < maxLinks;
        if (!ends && !follows) return;                             // (specular at the cap: the first hit's pixel stands)
        float4 pa, pb, pc;
        const bool moved = src.prev != nullptr && triangle_moved(src, hit.tri, pa, pb, pc);
        if (ends) {
            float4 om = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (moved && i == 0) {
                om = previous_point(pa, pb, pc, hit.u, hit.v);
            } else if (moved && !linkMoved) {
                const float4 pp = previous_point(pa, pb, pc, hit.u, hit.v);
                const V3 dl = v3(pp.x - hi.point.x, pp.y - hi.point.y, pp.z - hi.point.z);
                const V3 du = v3(m0.x * dl.x + m0.y * dl.y + m0.z * dl.z, m1.x * dl.x + m1.y * dl.y + m1.z * dl.z, m2.x * dl.x + m2.y * dl.y + m2.z * dl.z);
                const V3 o = cam.origin + v3(0.0f);                // (camera_ray_centre's origin)
                const V3 vi = v3(o.x + ray[0] * depth, o.y + ray[64] * depth, o.z + ray[128] * depth);
                om = make_float4(vi.x + du.x, vi.y + du.y, vi.z + du.z, 1.0f);
            }
            *out = om;
        }
        if (follows && moved) linkMoved = true;
    }

    PT_DEV static V3 unfold(const V3& r, const V3& n) {
        const float s = 2.0f * (r.x * n.x + r.y * n.y + r.z * n.z);
        return v3(r.x - s * n.x, r.y - s * n.y, r.z - s * n.z);
    }
    PT_DEV void link(bool reflect, const V3& n) {
        if (!reflect) return;                                      // (a pane shifts the image, it does not mirror it)
        m0 = unfold(m0, n); m1 = unfold(m1, n); m2 = unfold(m2, n);
    }
};

// (pt_render_motion_chain; include/pt_api.h states the contract.) aov_centre_chain_kernel with the hook; the guide outputs are its.
__global__ void __launch_bounds__(256) motion_chain_kernel(DeviceScene S, MotionSrc M, CamK cam, int w, int h, int tilesX, int nTiles, int maxLinks,
                                                           float4* __restrict__ albedo, float4* __restrict__ normalDepth,
                                                           float* __restrict__ linksOut, float4* __restrict__ motion, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ float ldsRec[4][10][64];          // follow_chain's record and the centre ray's direction, lane-interleaved
    FeatureWave W(ldsStack, S, spill);
    float* rec = &ldsRec[W.wave][0][W.lane];
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        const TilePixel p = tile_pixel(tile, tilesX, W.lane, w, h);
        const size_t idx = p.inside ? (size_t)p.y * w + p.x : 0;    // (a lane outside has no ray: its hook is never called)
        V3 o = v3(0.0f), d = v3(0.0f);
        if (p.inside) camera_ray_centre(cam, p.x, p.y, o, d);
        rec[448] = d.x; rec[512] = d.y; rec[576] = d.z;
        const int links = follow_chain(S, W.C, W.st, W.c, o, d, p.inside, maxLinks, rec, MotionChain(M, cam, maxLinks, motion + idx, rec + 448));
        if (!p.inside) continue;
        if (links < 0) motion[idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // a miss: the hook saw no surface
        if (albedo == nullptr) continue;
        float4 oa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), on = oa;
        float ol = 0.0f;
        if (links >= 0) {
            oa = make_float4(rec[0], rec[64], rec[128], 1.0f);
            on = make_float4(rec[192], rec[256], rec[320], rec[384]);
            ol = (float)links;
        }
        albedo[idx] = oa;
        normalDepth[idx] = on;
        if (linksOut) linksOut[idx] = ol;
    }
}

hipError_t launch_motion_chain(const DeviceScene& S, const void* tris, const void* posCur, const void* posPrev, int nPos, const CamK& cam, int w,
                               int h, int maxLinks, int blocks, float4* albedo, float4* normalDepth, float* links, float4* motion, int32_t* spill,
                               hipStream_t stream) {
    const FeatureTiles T = feature_tiles(w, h);
    MotionSrc M;
    M.tris = (const pt_triangle*)tris; M.cur = (const float4*)posCur; M.prev = (const float4*)posPrev; M.nPos = nPos;
    hipLaunchKernelGGL(motion_chain_kernel, dim3(blocks), dim3(256), 0, stream, S, M, cam, w, h, T.tilesX, T.nTiles, maxLinks, albedo, normalDepth, links,
                       motion, spill);
    return hipGetLastError();
}

}  // namespace pt
