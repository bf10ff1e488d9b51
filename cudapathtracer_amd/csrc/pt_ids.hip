// pt_ids.hip — the ID pass (pt_render_ids, pt_pick; include/pt_api.h): for the centre ray of each pixel, WHICH surface the guides show
// there, as the indices the scene's edit calls take: the triangle (Hit::tri, the description's order), its material row
// (pt_scene_update_materials), its light index (pt_scene_update_emission, -1 for a triangle that is no light) and an info word
// (bit 0: seen from the back; bits 8 and up: the links followed to reach it). A miss is (-1, -1, -1, 0).
//
// Two kernels, pt_feature.h's FeatureWave and tile loop around the centre ray:
//   ids_kernel        the first hit                aov_centre_kernel's organisation
//   ids_chain_kernel  follow_chain with IdsChain   the surface whose record the chain's guides hold: the last one seen with
//                                                  i == 0 || !spec, so a chain that leaves the scene after a mirror, or reaches the
//                                                  cap, reports the surface the albedo guide shows there
// IdsChain keeps the end surface's triangle and backface bit in two LDS words beside follow_chain's record (nothing of it is live
// across the traversals in registers); the material and the light index are read from the triangle's attributes once the chain has
// ended. No RNG, no seed.
//
// Both kernels also serve a LIST of pixels (pt_pick): with PickList::xy set, "tile" t is queries 64 t .. 64 t + 63, one lane each,
// outputs are indexed by query, and `hit` receives (the surface's point, the summed path length). The chain kernel stores that record
// where the hook sees an end surface, as motion_chain_kernel stores its pixel, so the point is not kept either.
#include "pt_feature.h"

namespace pt {

struct PickList { const int32_t* xy; int n; };     // xy NULL: the tile map of a w x h image

// The pixel of `lane` in tile `tile` and the index of its outputs: the image's pixel, or the list's entry.
PT_DEV TilePixel ids_pixel(const PickList& L, int tile, int tilesX, int lane, int w, int h, int& idx) {
    if (L.xy == nullptr) {
        const TilePixel p = tile_pixel(tile, tilesX, lane, w, h);
        idx = p.y * w + p.x;
        return p;
    }
    TilePixel p;
    idx = tile * 64 + lane;
    p.inside = idx < L.n;
    p.x = p.inside ? L.xy[2 * idx] : 0; p.y = p.inside ? L.xy[2 * idx + 1] : 0;      // (the host refused a pixel outside the image)
    return p;
}

// The four words of a surface: PAttr's lightInd is -51 for a triangle that is no light.
PT_DEV int4 id_words(int tri, int material, int lightInd, bool backface, int links) {
    return make_int4(tri, material, lightInd < 0 ? -1 : lightInd, (backface ? 1 : 0) | (links << 8));
}

__global__ void __launch_bounds__(256) ids_kernel(DeviceScene S, CamK cam, PickList L, int w, int h, int tilesX, int nTiles, int4* __restrict__ ids,
                                                  float4* __restrict__ hitOut, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    FeatureWave W(ldsStack, S, spill);
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        int idx;
        const TilePixel p = ids_pixel(L, tile, tilesX, W.lane, w, h, idx);
        if (!p.inside) continue;
        V3 o, d;
        camera_ray_centre(cam, p.x, p.y, o, d);
        Hit hit;
        trace_closest<false, kStackLds>(S, W.C, o, d, 999999.0f, W.st, hit, W.c);
        int4 oi = make_int4(-1, -1, -1, 0);
        float4 oh = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (hit.tri >= 0) {
            HitInfo hi; resolve_hit(S, hit, o, d, hi);
            oi = id_words(hit.tri, hi.material, hi.lightInd, hi.backface, 0);
            oh = make_float4(hi.point.x, hi.point.y, hi.point.z, hit.t);
        }
        ids[(size_t)idx] = oi;
        if (hitOut != nullptr) hitOut[(size_t)idx] = oh;           // (uniform: a kernel argument)
    }
}

// ids_chain_kernel's ChainHook. kept[0], kept[64]: the lane's two LDS words.
struct IdsChain {
    int32_t* kept;
    float4* hitOut;             // pt_pick's records, or NULL
    int idx;
    PT_DEV IdsChain(int32_t* kept_, float4* hitOut_, int idx_) : kept(kept_), hitOut(hitOut_), idx(idx_) {}
    PT_DEV void surface(int i, const Hit& hit, const HitInfo& hi, bool spec, float depth) {
        if (!(i == 0 || !spec)) return;                            // follow_chain's own condition for its record
        kept[0] = hit.tri; kept[64] = hi.backface ? 1 : 0;
        if (hitOut != nullptr) hitOut[(size_t)idx] = make_float4(hi.point.x, hi.point.y, hi.point.z, depth);
    }
    PT_DEV void link(bool reflect, const V3& n) {}
};

__global__ void __launch_bounds__(256) ids_chain_kernel(DeviceScene S, CamK cam, PickList L, int w, int h, int tilesX, int nTiles, int maxLinks,
                                                        int4* __restrict__ ids, float4* hitOut, int32_t* spill) {
    __shared__ int32_t ldsStack[4][kStackLds][64];
    __shared__ float ldsRec[4][7][64];           // follow_chain's record, lane-interleaved
    __shared__ int32_t ldsKept[4][2][64];        // IdsChain's words
    FeatureWave W(ldsStack, S, spill);
    float* rec = &ldsRec[W.wave][0][W.lane];
    int32_t* kept = &ldsKept[W.wave][0][W.lane];
    for (int tile = W.gw; tile < nTiles; tile += gridDim.x * 4) {
        int idx;
        const TilePixel p = ids_pixel(L, tile, tilesX, W.lane, w, h, idx);
        V3 o = v3(0.0f), d = v3(0.0f);
        if (p.inside) camera_ray_centre(cam, p.x, p.y, o, d);
        const int links = follow_chain(S, W.C, W.st, W.c, o, d, p.inside, maxLinks, rec, IdsChain(kept, hitOut, idx));
        if (!p.inside) continue;                                   // (a lane outside has no ray: its hook is never called)
        int4 oi = make_int4(-1, -1, -1, 0);
        if (links >= 0) {
            const int tri = kept[0];
            const PAttr& at = S.attrs[tri];
            oi = id_words(tri, at.material, at.lightInd, kept[64] != 0, links);
        } else if (hitOut != nullptr) {
            hitOut[(size_t)idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);        // a miss: the hook saw no surface
        }
        ids[(size_t)idx] = oi;
    }
}

hipError_t launch_ids(const DeviceScene& S, const CamK& cam, int w, int h, int maxLinks, const int32_t* xy, int nPick, int blocks, int4* ids,
                      float4* hit, int32_t* spill, hipStream_t stream) {
    const FeatureTiles T = xy ? FeatureTiles{0, (nPick + 63) / 64} : feature_tiles(w, h);
    const PickList L = {xy, nPick};
    if (maxLinks > 0)
        hipLaunchKernelGGL(ids_chain_kernel, dim3(blocks), dim3(256), 0, stream, S, cam, L, w, h, T.tilesX, T.nTiles, maxLinks, ids, hit, spill);
    else
        hipLaunchKernelGGL(ids_kernel, dim3(blocks), dim3(256), 0, stream, S, cam, L, w, h, T.tilesX, T.nTiles, ids, hit, spill);
    return hipGetLastError();
}

}  // namespace pt
