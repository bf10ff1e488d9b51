// pt_pack.h — where a packed record (pt_device.h: PTri, PAttr, PLight, PNode, PMat) is made. The makers are __host__ __device__, so
// the host re-pack (pt_scene.hip), the device pack and the edits (pt_bvh_build.hip, pt_scene.hip) write the same bytes because they
// run the same lines. Index checking stays with the callers: the host names the triangle and the index in a message, the device
// sets a flag bit. Below the makers: the host re-pack of a caller's own tree, which touches no device (tools/repack_check.hip runs
// it as a plain program). Internal: not part of the C ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/pt_api.h"
#include "pt_device.h"

// What a triangle takes from its material's TYPE: pt_tri_flags_ is the PTri.flags word (kTriLeaf: a MAT_LEAF triangle), and a type
// without a dispatch arm (pt_path.h) carries kTriArmless in its class.
constexpr uint32_t kTriLeaf = 1u, kTriArmless = 0x100u;
__host__ __device__ inline uint32_t pt_tri_flags_(int ty) { return ty == PT_MAT_LEAF ? kTriLeaf : 0u; }
__host__ __device__ inline bool pt_type_has_arm_(int ty) {
    return ty == PT_MAT_DIFFUSE || ty == PT_MAT_METAL || ty == PT_MAT_SMOOTHDIELECTRIC || ty == PT_MAT_LEAF || ty == PT_MAT_DELTAMIRROR;
}
__host__ __device__ inline uint32_t pt_tri_class_(int ty) { return pt_tri_flags_(ty) | (pt_type_has_arm_(ty) ? 0u : kTriArmless); }
// The class word of a material ROW: pt_tri_class_ of its type, kRowTextured if a triangle of it samples a texture or a transmission
// map, kRowNotSimple unless it is an untextured PT_MAT_DIFFUSE that is neither boundary nor specular (pt_path.h: SIMPLE). OR-ed over
// the triangles' rows this word decides noLeafTris, armless, leanOk and (with material 0's absorption) simpleOk.
constexpr uint32_t kRowTextured = 2u, kRowNotSimple = 4u;
inline uint32_t pt_material_class_(const pt_material& m) {
    const bool tex = m.hasTexture || m.hasTransMap;
    return pt_tri_class_(m.type) | (tex ? kRowTextured : 0u) | ((m.type == PT_MAT_DIFFUSE && !tex && !m.boundary && !m.isSpecular) ? 0u : kRowNotSimple);
}

namespace pt {

// ---- the makers ---------------------------------------------------------------------------------------------------------------
// idx: the triangle's original index; leafEnd: it is the last of its leaf; type: its material's.
__host__ __device__ inline PTri make_tri(const pt_float4& a, const pt_float4& b, const pt_float4& c, int idx, bool leafEnd, int material, int type) {
    PTri p;
    p.v0[0] = a.x; p.v0[1] = a.y; p.v0[2] = a.z;
    p.e1[0] = b.x - a.x; p.e1[1] = b.y - a.y; p.e1[2] = b.z - a.z;      // trib - tria, integratorUtilities.cuh:13
    p.e2[0] = c.x - a.x; p.e2[1] = c.y - a.y; p.e2[2] = c.z - a.z;      // tric - tria, :14
    p.idx = (uint32_t)idx | (leafEnd ? 0x80000000u : 0u);
    p.material = material;
    p.flags = pt_tri_flags_(type);
    return p;
}
// n, uv: the triangle's three normals and uvs; a lightInd outside the light list becomes the reference's -51.
__host__ __device__ inline PAttr make_attr(const pt_triangle& t, const pt_float4 n[3], const pt_float2 uv[3], int nLights) {
    PAttr a;
    float* nd[3] = {a.n0, a.n1, a.n2}; float* ud[3] = {a.uv0, a.uv1, a.uv2};
    for (int k = 0; k < 3; k++) { nd[k][0] = n[k].x; nd[k][1] = n[k].y; nd[k][2] = n[k].z; ud[k][0] = uv[k].x; ud[k][1] = uv[k].y; }
    a.emission[0] = t.emission.x; a.emission[1] = t.emission.y; a.emission[2] = t.emission.z;
    a.material = t.materialID;
    a.lightInd = (t.lightInd >= 0 && t.lightInd < nLights) ? t.lightInd : -51;
    return a;
}
// area = 0.5f * length(cross3(b - a, c - a)) exactly as the kernels used to evaluate it per NEE sample: IEEE subtractions,
// cross = fma(p, q, -(r * s)), dot = fma(z, z', fma(y, y', x * x')), correctly rounded sqrt.
__host__ __device__ inline PLight make_light(const pt_float4& a, const pt_float4& b, const pt_float4& c, const pt_float4& n, const pt_float4& emission) {
    PLight L;
    L.a[0] = a.x; L.a[1] = a.y; L.a[2] = a.z; L.b[0] = b.x; L.b[1] = b.y; L.b[2] = b.z; L.c[0] = c.x; L.c[1] = c.y; L.c[2] = c.z;
    L.na[0] = n.x; L.na[1] = n.y; L.na[2] = n.z;
    L.emission[0] = emission.x; L.emission[1] = emission.y; L.emission[2] = emission.z;
    const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
    const float cx = fmaf(uy, vz, -(uz * vy)), cy = fmaf(uz, vx, -(ux * vz)), cz = fmaf(ux, vy, -(uy * vx));
    L.area = 0.5f * sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
    return L;
}
// An internal node from its children's boxes (three floats each) and references.
__host__ __device__ inline PNode make_node(const float* lmin, const float* lmax, const float* rmin, const float* rmax, int32_t left, int32_t right) {
    PNode p;
    for (int k = 0; k < 3; k++) { p.lmin[k] = lmin[k]; p.lmax[k] = lmax[k]; p.rmin[k] = rmin[k]; p.rmax[k] = rmax[k]; }
    p.left = left; p.right = right; p.pad0 = p.pad1 = 0;
    return p;
}

// ---- the host re-pack of a caller's own tree: reads the caller's arrays, returns 0 or what it failed with -----------------------
int fail(int code, const char* fmt, ...);      // (pt_api.hip: the message pt_last_error returns)

// Scenes in HBM: the kernels keep PNodes [0, K) in LDS, so the internal nodes are numbered by how often rays visit them rather
// than by level — a ray enters a box with a probability proportional to its surface area (the SAH's own estimate), and a
// child's box lies inside its parent's, so descending area (ties: breadth-first order) still numbers parents first.
// (Against plain breadth-first numbering: 82 k triangles 765 -> 729 ms at 128 spp, 263 k 387 -> 379 ms at 16 spp, 7.5 % fewer
// node fetches from global memory; profiles/r03_ab_node_order_area.log)
inline float order_area(const float* mn, const float* mx) {
    const float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
    const float a = dx * dy + dy * dz + dz * dx;
    return std::isfinite(a) ? a : 0.0f;
}
// area[k]: of the k-th node in breadth-first order -> its new number; the root stays node 0.
inline std::vector<int> rank_by_area(const std::vector<float>& area) {
    std::vector<int> order(area.size()), rank(area.size());
    for (size_t k = 0; k < order.size(); k++) order[k] = (int)k;
    if (!order.empty()) std::stable_sort(order.begin() + 1, order.end(), [&](int a, int b) { return area[a] > area[b]; });
    for (size_t k = 0; k < order.size(); k++) rank[order[k]] = (int)k;
    return rank;
}

struct Box3 { float lo[3], hi[3]; };
inline Box3 box3(const pt_bvh_node& n) { return Box3{{n.aabbMIN.x, n.aabbMIN.y, n.aabbMIN.z}, {n.aabbMAX.x, n.aabbMAX.y, n.aabbMAX.z}}; }

// Validates the nodes and numbers the internal ones; packs them into `nodes`. leafEnd[i]: packed triangle i is the last of its leaf.
inline int number_nodes(const pt_bvh_node* bvh, int nN, int nT, std::vector<PNode>& nodes, std::vector<uint8_t>& leafEnd, int& nInternal, int& rootRef) {
    // --- internal nodes renumbered BREADTH-FIRST from the root, so PNodes [0, K) are the top of the
    //     tree (the part every ray visits) and can be staged in LDS as one contiguous block ---
    std::vector<int> internalId(nN, -1);
    for (int i = 0; i < nN; i++) {
        const pt_bvh_node& n = bvh[i];
        if (n.primCount > 0) {
            if (n.first < 0 || n.first + n.primCount > nT) return fail(-1, "pt_scene_create: leaf %d range [%d,+%d) out of bounds", i, n.first, n.primCount);
        } else {
            if (n.left < 0 || n.right < 0 || n.left >= nN || n.right >= nN) return fail(-1, "pt_scene_create: internal node %d has child out of range", i);
        }
    }
    {
        std::vector<int> queue;
        if (bvh[0].primCount <= 0) { queue.push_back(0); internalId[0] = nInternal++; }
        for (size_t q = 0; q < queue.size(); q++) {
            const pt_bvh_node& n = bvh[queue[q]];
            for (int c : {n.left, n.right}) {
                if (bvh[c].primCount > 0) continue;
                if (internalId[c] >= 0 || (int)queue.size() >= nN) return fail(-1, "pt_scene_create: BVH is not a tree");
                internalId[c] = nInternal++;
                queue.push_back(c);
            }
        }
    }
    if (nInternal > 128) {                                     // scenes in HBM: by area (above)
        std::vector<float> area((size_t)nInternal, 0.0f);
        for (int i = 0; i < nN; i++)
            if (internalId[i] >= 0) { const Box3 b = box3(bvh[i]); area[internalId[i]] = order_area(b.lo, b.hi); }
        const std::vector<int> rank = rank_by_area(area);
        for (int i = 0; i < nN; i++) if (internalId[i] >= 0) internalId[i] = rank[internalId[i]];
    }
    auto childRef = [&](int c) -> int32_t { return bvh[c].primCount > 0 ? ~bvh[c].first : internalId[c]; };
    nodes.assign(std::max(nInternal, 1), PNode{});
    leafEnd.assign(nT, 0);
    for (int i = 0; i < nN; i++) {
        const pt_bvh_node& n = bvh[i];
        if (n.primCount > 0) { leafEnd[n.first + n.primCount - 1] = 1; continue; }
        if (internalId[i] < 0) continue;                       // unreachable from the root
        const Box3 L = box3(bvh[n.left]), R = box3(bvh[n.right]);
        nodes[internalId[i]] = make_node(L.lo, L.hi, R.lo, R.hi, childRef(n.left), childRef(n.right));
    }
    rootRef = childRef(0);
    return 0;
}

// stack need = the largest number of internal nodes on a root-to-leaf path (each can leave one
// far child pending); also rejects cycles.
inline int stack_need(const pt_bvh_node* bvh, int nN, int& stackNeed) {
    std::vector<std::pair<int, int>> st; st.push_back({0, 1});
    size_t visited = 0;
    while (!st.empty()) {
        auto [i, depth] = st.back(); st.pop_back();
        if (++visited > (size_t)nN) return fail(-1, "pt_scene_create: BVH is not a tree");
        if (bvh[i].primCount > 0) continue;
        stackNeed = std::max(stackNeed, depth);
        st.push_back({bvh[i].left, depth + 1});
        st.push_back({bvh[i].right, depth + 1});
    }
    if (stackNeed > 128) return fail(-1, "pt_scene_create: BVH depth %d exceeds the reference's nodeStack[128] (integratorUtilities.cuh:89)", stackNeed);
    return 0;
}

// Position i of the description, for vertex `what` of triangle (or light) `tri`; out of range: the message is set and ok cleared.
inline pt_float4 pos(const pt_scene_desc* d, int i, const char* what, int tri, bool& ok) {
    if (i < 0 || i >= d->n_positions) { ok = false; fail(-1, "pt_scene_create: triangle %d %s index %d out of range", tri, what, i); return pt_float4{0, 0, 0, 0}; }
    return d->positions[i];
}

// The triangles in leaf order and the hit attributes by original index, from the description's arrays.
inline int pack_triangles(const pt_scene_desc* d, const std::vector<uint8_t>& leafEnd, std::vector<PTri>& tris, std::vector<PAttr>& attrs) {
    const int nT = d->n_triangles;
    tris.resize(nT);
    for (int i = 0; i < nT; i++) {
        int idx = d->bvh_indices[i];
        if (idx < 0 || idx >= nT) return fail(-1, "pt_scene_create: BVHindices[%d] = %d out of range", i, idx);
        const pt_triangle& t = d->triangles[idx];
        bool ok = true;
        pt_float4 a = pos(d, t.aInd, "a", idx, ok), b = pos(d, t.bInd, "b", idx, ok), c = pos(d, t.cInd, "c", idx, ok);
        if (!ok) return -1;
        if (t.materialID < 0 || t.materialID >= d->n_materials) return fail(-1, "pt_scene_create: triangle %d material %d out of range", idx, t.materialID);
        tris[i] = make_tri(a, b, c, idx, leafEnd[i] != 0, t.materialID, d->materials[t.materialID].type);
    }
    attrs.resize(nT);
    for (int i = 0; i < nT; i++) {
        const pt_triangle& t = d->triangles[i];
        const int ni[3] = {t.naInd, t.nbInd, t.ncInd}, ui[3] = {t.uvaInd, t.uvbInd, t.uvcInd};
        pt_float4 n[3]; pt_float2 uv[3];
        for (int k = 0; k < 3; k++) {
            if (ni[k] < 0 || ni[k] >= d->n_normals || !d->normals) return fail(-1, "pt_scene_create: triangle %d normal index %d out of range (faces without vn must be given a normal by the loader)", i, ni[k]);
            if (ui[k] < 0 || ui[k] >= d->n_uvs || !d->uvs) return fail(-1, "pt_scene_create: triangle %d uv index %d out of range", i, ui[k]);
            n[k] = d->normals[ni[k]]; uv[k] = d->uvs[ui[k]];
        }
        attrs[i] = make_attr(t, n, uv, d->n_lights);
    }
    return 0;
}

// The light records, one zero record for a scene without lights.
inline int pack_lights(const pt_scene_desc* d, std::vector<PLight>& lights) {
    lights.resize(std::max(d->n_lights, 1));
    std::memset(lights.data(), 0, lights.size() * sizeof(PLight));
    for (int i = 0; i < d->n_lights; i++) {
        const pt_triangle& t = d->lights[i];
        bool ok = true;
        pt_float4 a = pos(d, t.aInd, "a", i, ok), b = pos(d, t.bInd, "b", i, ok), c = pos(d, t.cInd, "c", i, ok);
        if (!ok) return -1;
        if (t.naInd < 0 || t.naInd >= d->n_normals) return fail(-1, "pt_scene_create: light %d normal index out of range", i);
        lights[i] = make_light(a, b, c, d->normals[t.naInd], t.emission);
    }
    return 0;
}

// The material table as the kernels read it, and the class word of every row (pt_material_class_). Creation and
// pt_scene_update_materials both pack through here; fn names the caller in the message of a refused texture window.
inline int pack_materials(const pt_material* materials, int nMats, int nTexels, const char* fn, std::vector<PMat>& mats, std::vector<uint32_t>& matClass) {
    mats.resize((size_t)nMats); matClass.resize((size_t)nMats);
    std::memset(mats.data(), 0, mats.size() * sizeof(PMat));
    for (int i = 0; i < nMats; i++) {
        const pt_material& m = materials[i];
        PMat& p = mats[i];
        p.type = m.type;
        p.flags = (m.hasTexture ? kMatHasTexture : 0) | (m.hasTransMap ? kMatHasTransMap : 0) | (m.isSpecular ? kMatSpecular : 0) | (m.boundary ? kMatBoundary : 0);
        p.priority = m.priority;
        p.texStart = m.startInd; p.texW = m.width; p.texH = m.height;
        if ((m.hasTexture || m.hasTransMap) && m.width > 0 && m.height > 0 &&
            (m.startInd < 0 || (long long)m.startInd + (long long)m.width * m.height > nTexels))
            return fail(-1, "%s: material %d texture window exceeds the texel array", fn, i);
        p.roughness = m.roughness; p.ior = m.ior; p.transmission = m.transmission;
        p.albedo[0] = m.albedo.x; p.albedo[1] = m.albedo.y; p.albedo[2] = m.albedo.z;
        p.eta[0] = m.eta.x; p.eta[1] = m.eta.y; p.eta[2] = m.eta.z;
        p.k[0] = m.k.x; p.k[1] = m.k.y; p.k[2] = m.k.z;
        p.absorption[0] = m.absorption.x; p.absorption[1] = m.absorption.y; p.absorption[2] = m.absorption.z;
        p.albedoOverPi[0] = m.albedo.x / kPi; p.albedoOverPi[1] = m.albedo.y / kPi; p.albedoOverPi[2] = m.albedo.z / kPi;   // cosine_f, reflectors.cuh:10-13
        matClass[i] = pt_material_class_(m);
    }
    return 0;
}

}  // namespace pt
