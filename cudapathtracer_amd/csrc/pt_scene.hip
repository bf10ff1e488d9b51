// pt_scene.hip — a scene's making and editing behind include/pt_api.h: the re-pack of the reference's data model and its upload,
// the layout derived from the packed records, pt_scene_create* / pt_scene_destroy and the in-place updates. Host code only.
#include <chrono>
#include <cmath>

#include "pt_host.h"
#include "pt_bvh_build.h"
#include "pt_box_table.h"
#include "xorwow_host.h"

using namespace pt;

static_assert(sizeof(pt_bvh_node) == 48 && sizeof(pt_triangle) == 80 && sizeof(pt_material) == 176 && sizeof(pt_camera) == 112,
              "boundary structs must keep the reference's CUDA layouts (SURVEY.md Appendix A)");
static_assert(offsetof(pt_triangle, emission) == 48 && offsetof(pt_triangle, lightInd) == 64, "Triangle layout");
static_assert(offsetof(pt_material, type) == 32 && offsetof(pt_material, albedo) == 48 && offsetof(pt_material, eta) == 80 &&
              offsetof(pt_material, ior) == 112 && offsetof(pt_material, isSpecular) == 128 && offsetof(pt_material, absorption) == 144 &&
              offsetof(pt_material, priority) == 160, "Material layout");
static_assert(offsetof(pt_camera, forward) == 64 && offsetof(pt_camera, fovScale) == 44, "Camera layout");

static double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static int upload(DevBuf& b, const void* src, size_t bytes) {
    if (int r = b.ensure(std::max<size_t>(bytes, 16))) return r;
    if (bytes) HIP_OK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return 0;
}

// For each light: the packed triangle (position in leaf order, the FLAT kernels' numbering) it was made from, or -1. The pair pass
// leaves that triangle out of the tests of a shadow ray aimed at the light (pt_trace.h: trace_pair_flat), which is exact only if
// the bounce's own test of the ray against the light (PLight a, b - a, c - a) and the pass's test against the triangle (PTri v0, e1,
// e2) see the same operands: checked here bit for bit, on the records as the kernels read them. A light that is no triangle of
// the scene, or whose vertices are in another order, gets -1 and its shadow rays are tested against everything.
// The records are read as the kernels read them: PLight a, b, c ARE the positions' floats, and lightIndOf(idx) is the lightInd of
// original triangle idx (anything outside 0..nLights-1 matches no light), so the table can be made from a description's host
// arrays and from a scene's device records alike.
template <class LightIndOf>
static void light_triangles(const PTri* pt, int nT, const PLight* lights, int nLights, int nTriangles, LightIndOf lightIndOf, int32_t* out) {
    for (int i = 0; i < nLights; i++) {
        out[i] = -1;
        const PLight& L = lights[i];
        const float v0[3] = {L.a[0], L.a[1], L.a[2]}, e1[3] = {L.b[0] - L.a[0], L.b[1] - L.a[1], L.b[2] - L.a[2]},
                    e2[3] = {L.c[0] - L.a[0], L.c[1] - L.a[1], L.c[2] - L.a[2]};
        for (int p = 0; p < nT && p < 63; p++) {                 // (the pair pass holds a ray's triangles in one 64-bit mask, and clears bit p as (1 << (p + 1)) >> 1)
            const int idx = (int)(pt[p].idx & 0x7fffffffu);
            if (idx >= nTriangles || lightIndOf(idx) != i) continue;
            if (!memcmp(pt[p].v0, v0, 12) && !memcmp(pt[p].e1, e1, 12) && !memcmp(pt[p].e2, e2, 12)) { out[i] = p; break; }
        }
    }
}
// ... from a description: a light whose vertex indices are out of range gets -1.
static void light_triangles(const PTri* pt, int nT, const pt_scene_desc* d, int32_t* out) {
    std::vector<PLight> L((size_t)std::max(d->n_lights, 1));
    std::vector<uint8_t> bad((size_t)std::max(d->n_lights, 1), 0);
    for (int i = 0; i < d->n_lights; i++) {
        const pt_triangle& t = d->lights[i];
        L[i] = PLight{};
        if (t.aInd < 0 || t.aInd >= d->n_positions || t.bInd < 0 || t.bInd >= d->n_positions || t.cInd < 0 || t.cInd >= d->n_positions) { bad[i] = 1; continue; }
        const pt_float4 a = d->positions[t.aInd], b = d->positions[t.bInd], c = d->positions[t.cInd];
        L[i].a[0] = a.x; L[i].a[1] = a.y; L[i].a[2] = a.z; L[i].b[0] = b.x; L[i].b[1] = b.y; L[i].b[2] = b.z; L[i].c[0] = c.x; L[i].c[1] = c.y; L[i].c[2] = c.z;
    }
    light_triangles(pt, nT, L.data(), d->n_lights, d->n_triangles, [&](int idx) { const int li = d->triangles[idx].lightInd; return (li >= 0 && li < d->n_lights && bad[li]) ? -1 : li; }, out);
}

// The material table as the kernels read it, and the class word of every row (pt_bvh_build.h: pt_material_class_). Creation and
// pt_scene_update_materials both pack through here; fn names the caller in the message of a refused texture window.
static int pack_materials(const pt_material* materials, int nMats, int nTexels, const char* fn, std::vector<PMat>& mats, std::vector<uint32_t>& matClass) {
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

// What a scene decides from its triangles' materials alone, from `used` = the class words of the rows its triangles use, OR-ed:
// all four from scratch, since an edit can clear what another set.
// SIMPLE scenes (pt_path.h): every triangle's material an untextured MAT_DIFFUSE that is neither boundary nor specular, in air
// (material 0) that does not absorb — then the medium stack never changes and the dispatchers have one arm. noLeafTris: no triangle
// carries MAT_LEAF. LEAN (pt_shade.h): additionally no triangle's material samples a texture. armless: pt_bvh_build.h.
static void apply_material_class(pt_scene* s, uint32_t used, const pt_material& air) {
    s->facts.simpleOk = air.absorption.x == 0.0f && air.absorption.y == 0.0f && air.absorption.z == 0.0f && !(used & kRowNotSimple);
    s->facts.noLeafTris = !(used & kTriLeaf);
    s->facts.leanOk = s->facts.noLeafTris && !(used & kRowTextured);
    s->facts.armless = (used & kTriArmless) != 0;
}

// Scenes in HBM: the numbering the host re-pack gives the internal nodes (descending surface area of a node's own box — here
// read from its parent's record, the same floats — so that the LDS copy of PNodes [0, K) holds the most-visited ones), applied to
// the records the device builder packed into s->geo.nodes. Through the host: one download and one upload of the internal nodes.
static int renumber_by_area(pt_scene* s, int nInternal, int rootRef) {
    s->upd.renumberMs = 0.0f;
    const double t0 = wall_ms();
        if (nInternal > 128 && rootRef == 0) {
            std::vector<PNode> pn((size_t)nInternal);
            HIP_OK(hipMemcpy(pn.data(), s->geo.nodes.p, (size_t)nInternal * sizeof(PNode), hipMemcpyDeviceToHost));
            std::vector<float> area((size_t)nInternal, 0.0f);
            std::vector<int> bfs; bfs.reserve((size_t)nInternal); bfs.push_back(0);
            std::vector<uint8_t> seen((size_t)nInternal, 0); seen[0] = 1;
            bool tree = true;
            for (size_t q = 0; q < bfs.size() && tree; q++) {
                const PNode& p = pn[bfs[q]];
                const int32_t ref[2] = {p.left, p.right};
                for (int k = 0; k < 2; k++) {
                    if (ref[k] < 0) continue;
                    if (ref[k] >= nInternal || seen[ref[k]]) { tree = false; break; }
                    seen[ref[k]] = 1;
                    const float* mn = k == 0 ? p.lmin : p.rmin; const float* mx = k == 0 ? p.lmax : p.rmax;
                    const float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
                    const float a = dx * dy + dy * dz + dz * dx;
                    area[ref[k]] = std::isfinite(a) ? a : 0.0f;
                    bfs.push_back(ref[k]);
                }
            }
            if (tree && (int)bfs.size() == nInternal) {
                // bfs[k]: k-th node in breadth-first order; sort those positions by area (stable: ties keep breadth-first order)
                std::vector<int> order(bfs);
                std::stable_sort(order.begin() + 1, order.end(), [&](int a, int b) { return area[a] > area[b]; });
                std::vector<int> rank((size_t)nInternal);
                for (int k = 0; k < nInternal; k++) rank[order[k]] = k;
                std::vector<PNode> out((size_t)nInternal);
                for (int i = 0; i < nInternal; i++) {
                    PNode p = pn[i];
                    if (p.left >= 0) p.left = rank[p.left];
                    if (p.right >= 0) p.right = rank[p.right];
                    out[rank[i]] = p;
                }
                HIP_OK(hipMemcpy(s->geo.nodes.p, out.data(), (size_t)nInternal * sizeof(PNode), hipMemcpyHostToDevice));
            }
            s->upd.renumberMs = (float)(wall_ms() - t0);
        }
    return 0;
}

// What creation derives from the packed records in s->geo.nodes / tris / attrs / lights, and an update derives again: the device
// scene's pointers, the LDS cache split, the spill need, whether the FLAT kernels can run it (and then the leaf counts in the
// PNodes' spare words, the leaf table and the lights' triangles). hostLights: the PLight records as uploaded (haveLights: the
// scene has a light list at all); lightIndOf[i]: lightInd of original triangle i (nLightInd entries; read only for scenes of at
// most 128 triangles).
static int derive_layout(pt_scene* s, int nInternal, int stackNeed, int rootRef, int nT, int nLights, bool haveLights, int nMats, const PLight* hostLights,
                         const int32_t* lightIndOf, int nLightInd) {
    std::vector<int32_t> lightTri((size_t)std::max(nLights, 1), -1);      // filled in below for the scenes the pair kernels can run
    s->facts.lightTri8 = 0ull;
    s->facts.nInternal = nInternal;
    s->facts.stackNeed = stackNeed;
    s->facts.ds.nodes = (const PNode*)s->geo.nodes.p; s->facts.ds.tris = (const PTri*)s->geo.tris.p; s->facts.ds.attrs = (const PAttr*)s->geo.attrs.p;
    s->facts.ds.lights = (const PLight*)s->geo.lights.p; s->facts.ds.mats = (const PMat*)s->data.mats.p; s->facts.ds.textures = (const float4*)s->data.textures.p;
    s->facts.ds.rootRef = rootRef;
    s->facts.ds.nLights = nLights; s->facts.ds.nTris = nT;
    s->facts.nMats = nMats; s->facts.nLightsPacked = std::max(nLights, 1);
    s->facts.ds.stackSpill = std::max(0, stackNeed - kStackLds);
    // scene cache: everything if it fits the LDS budget, else only the top of the (breadth-first) tree
    s->facts.nTrisPacked = nT;
    if ((size_t)nInternal * 64 + (size_t)nT * 48 <= (size_t)kCacheBytes) { s->facts.cacheNodes = nInternal; s->facts.cacheTris = nT; }
    else { s->facts.cacheNodes = std::min(nInternal, kCacheBytes / 64); s->facts.cacheTris = 0; }
    // FLAT kernels (pt_trace.h): one forward pass over the internal nodes with 64- or 128-bit masks — needs at most 128 of
    // each, every child numbered after its parent (the breadth-first numbering gives that; checked on the packed records)
    // and the triangle count of every leaf child, which goes into the spare words of its PNode.
    s->facts.flatOk = false;
    if (nInternal <= 128 && nT >= 1 && nT <= 128 && scene_onchip_wg(s->facts, s->opt) > 0) {
        std::vector<PNode> pn((size_t)std::max(nInternal, 1));
        std::vector<PTri> pt((size_t)nT);
        if (nInternal > 0) HIP_OK(hipMemcpy(pn.data(), s->geo.nodes.p, (size_t)nInternal * sizeof(PNode), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(pt.data(), s->geo.tris.p, (size_t)nT * sizeof(PTri), hipMemcpyDeviceToHost));
        auto leafCount = [&](int first) {                      // triangles up to and including the one flagged last
            int k = first;
            while (k < nT) { uint32_t w; memcpy(&w, (const char*)&pt[k] + 36, 4); k++; if (w & 0x80000000u) return k - first; }
            return 0;                                          // runs off the end: not a well-formed leaf
        };
        bool ok = rootRef < 0 ? (~rootRef == 0 && leafCount(0) == nT) : (rootRef == 0);
        std::vector<int> first((size_t)std::max(nInternal, 1), 0);   // first triangle below node i
        for (int i = nInternal - 1; i >= 0 && ok; i--) {          // children come after their parent: bottom-up
            int32_t* ref = &pn[i].left;                         // left, right, pad0, pad1
            int firstOf[2] = {0, 0};
            for (int k = 0; k < 2 && ok; k++) {
                if (ref[k] >= 0) {
                    ok = ref[k] > i && ref[k] < nInternal;
                    if (ok) { ref[2 + k] = pn[ref[k]].pad0 + pn[ref[k]].pad1; firstOf[k] = first[ref[k]]; }
                } else {
                    const int f = ~ref[k]; const int cnt = (ref[k] != kRefNone && f < nT) ? leafCount(f) : 0;
                    ok = cnt >= 1; ref[2 + k] = cnt; firstOf[k] = f;
                }
            }
            // leaf order is left to right: the right subtree's triangles follow the left subtree's
            ok = ok && firstOf[1] == firstOf[0] + ref[2];
            first[i] = firstOf[0];
        }
        if (ok && nInternal > 0) ok = first[0] == 0 && pn[0].pad0 + pn[0].pad1 == nT;
        if (ok && nInternal > 0) HIP_OK(hipMemcpy(s->geo.nodes.p, pn.data(), (size_t)nInternal * sizeof(PNode), hipMemcpyHostToDevice));
        s->facts.flatOk = ok;
        s->facts.nLeaves = 0; s->facts.nBoxes = 0; s->facts.nBoxGroups = 0; s->facts.boxAxis = 0;
        if (ok && nLights > 0 && haveLights) {
            // the table travels as a kernel argument, a byte per light: the first 8 lights (a scene of at most 64 triangles rarely has
            // more; a light beyond them is simply tested like any other triangle)
            light_triangles(pt.data(), nT, hostLights, nLights, nLightInd, [&](int idx) { return lightIndOf[idx]; }, lightTri.data());
            for (int i = 0; i < nLights && i < 8; i++) s->facts.lightTri8 |= (uint64_t)(lightTri[i] + 1) << (8 * i);
        }
        if (ok && nInternal > 0 && boxes_nested_and_finite(pn, nInternal)) {     // the leaf table, and behind it in the same buffer the pair kernels' box table (pt_box_table.h)
            std::vector<PLeaf> lf = build_leaf_table(pn, nInternal);
            std::vector<PBox> bx = build_box_table(lf, nT);
            const int nBoxes = (int)bx.size();
            const BoxGroups G = group_box_table(bx);              // (sorted by group, the group headers behind the records)
            const size_t nLeaves = lf.size();
            lf.resize(nLeaves + bx.size());
            if (!bx.empty()) memcpy((void*)(lf.data() + nLeaves), bx.data(), bx.size() * sizeof(PBox));
            if (int r = upload(s->geo.leaves, lf.data(), lf.size() * sizeof(PLeaf))) return r;
            s->facts.nLeaves = (int)nLeaves; s->facts.nBoxes = nBoxes; s->facts.nBoxGroups = G.nGroups; s->facts.boxAxis = G.axis;
        }
    }
    return 0;
}

// Position i of the description, for vertex `what` of triangle (or light) `tri`; out of range: the message is set and ok cleared.
static pt_float4 pos(const pt_scene_desc* d, int i, const char* what, int tri, bool& ok) {
    if (i < 0 || i >= d->n_positions) { ok = false; fail(-1, "pt_scene_create: triangle %d %s index %d out of range", tri, what, i); return pt_float4{0, 0, 0, 0}; }
    return d->positions[i];
}

// The three host-only parts of repack for a caller's own tree; each reads the caller's arrays and returns 0 or what it failed with.
// Validates the nodes and numbers the internal ones; packs them into `nodes`. leafEnd[i]: packed triangle i is the last of its leaf.
static int number_nodes(const pt_bvh_node* bvh, int nN, int nT, std::vector<PNode>& nodes, std::vector<uint8_t>& leafEnd, int& nInternal, int& rootRef) {
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
    // Scenes in HBM: the kernels keep PNodes [0, K) in LDS, so number the internal nodes by how often rays visit them rather
    // than by level — a ray enters a box with a probability proportional to its surface area (the SAH's own estimate), and a
    // child's box lies inside its parent's, so descending area (ties: breadth-first order) still numbers parents first.
    // (Against plain breadth-first numbering: 82 k triangles 765 -> 729 ms at 128 spp, 263 k 387 -> 379 ms at 16 spp, 7.5 % fewer
    // node fetches from global memory; profiles/r03_ab_node_order_area.log)
    if (nInternal > 128) {
        std::vector<float> area((size_t)nInternal, 0.0f);
        for (int i = 0; i < nN; i++) {
            if (internalId[i] < 0) continue;
            const pt_bvh_node& n = bvh[i];
            const float dx = n.aabbMAX.x - n.aabbMIN.x, dy = n.aabbMAX.y - n.aabbMIN.y, dz = n.aabbMAX.z - n.aabbMIN.z;
            const float a = dx * dy + dy * dz + dz * dx;
            area[internalId[i]] = std::isfinite(a) ? a : 0.0f;
        }
        std::vector<int> order((size_t)nInternal);
        for (int i = 0; i < nInternal; i++) order[i] = i;
        std::stable_sort(order.begin() + 1, order.end(), [&](int a, int b) { return area[a] > area[b]; });     // the root stays node 0
        std::vector<int> rank((size_t)nInternal);
        for (int k = 0; k < nInternal; k++) rank[order[k]] = k;
        for (int i = 0; i < nN; i++) if (internalId[i] >= 0) internalId[i] = rank[internalId[i]];
    }
    auto childRef = [&](int c) -> int32_t { return bvh[c].primCount > 0 ? ~bvh[c].first : internalId[c]; };
    nodes.assign(std::max(nInternal, 1), PNode{});
    leafEnd.assign(nT, 0);
    for (int i = 0; i < nN; i++) {
        const pt_bvh_node& n = bvh[i];
        if (n.primCount > 0) { leafEnd[n.first + n.primCount - 1] = 1; continue; }
        if (internalId[i] < 0) continue;                       // unreachable from the root
        PNode& p = nodes[internalId[i]];
        const pt_bvh_node& L = bvh[n.left];
        const pt_bvh_node& R = bvh[n.right];
        p.lmin[0] = L.aabbMIN.x; p.lmin[1] = L.aabbMIN.y; p.lmin[2] = L.aabbMIN.z;
        p.lmax[0] = L.aabbMAX.x; p.lmax[1] = L.aabbMAX.y; p.lmax[2] = L.aabbMAX.z;
        p.rmin[0] = R.aabbMIN.x; p.rmin[1] = R.aabbMIN.y; p.rmin[2] = R.aabbMIN.z;
        p.rmax[0] = R.aabbMAX.x; p.rmax[1] = R.aabbMAX.y; p.rmax[2] = R.aabbMAX.z;
        p.left = childRef(n.left); p.right = childRef(n.right); p.pad0 = p.pad1 = 0;
    }
    rootRef = childRef(0);
    return 0;
}

// stack need = the largest number of internal nodes on a root-to-leaf path (each can leave one
// far child pending); also rejects cycles.
static int stack_need(const pt_bvh_node* bvh, int nN, int& stackNeed) {
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

// The triangles in leaf order and the hit attributes by original index, from the description's arrays.
static int pack_triangles(const pt_scene_desc* d, const std::vector<uint8_t>& leafEnd, std::vector<PTri>& tris, std::vector<PAttr>& attrs) {
    const int nT = d->n_triangles;
    // --- triangles in leaf order ---
    tris.resize(nT);
    for (int i = 0; i < nT; i++) {
        int idx = d->bvh_indices[i];
        if (idx < 0 || idx >= nT) return fail(-1, "pt_scene_create: BVHindices[%d] = %d out of range", i, idx);
        const pt_triangle& t = d->triangles[idx];
        bool ok = true;
        pt_float4 a = pos(d, t.aInd, "a", idx, ok), b = pos(d, t.bInd, "b", idx, ok), c = pos(d, t.cInd, "c", idx, ok);
        if (!ok) return -1;
        if (t.materialID < 0 || t.materialID >= d->n_materials) return fail(-1, "pt_scene_create: triangle %d material %d out of range", idx, t.materialID);
        PTri& p = tris[i];
        p.v0[0] = a.x; p.v0[1] = a.y; p.v0[2] = a.z;
        p.e1[0] = b.x - a.x; p.e1[1] = b.y - a.y; p.e1[2] = b.z - a.z;      // trib - tria, integratorUtilities.cuh:13
        p.e2[0] = c.x - a.x; p.e2[1] = c.y - a.y; p.e2[2] = c.z - a.z;      // tric - tria, :14
        p.idx = (uint32_t)idx | (leafEnd[i] ? 0x80000000u : 0u);
        p.material = t.materialID;
        p.flags = pt_tri_flags_(d->materials[t.materialID].type);
    }
    // --- hit attributes by original index ---
    attrs.resize(nT);
    for (int i = 0; i < nT; i++) {
        const pt_triangle& t = d->triangles[i];
        PAttr& a = attrs[i];
        const int ni[3] = {t.naInd, t.nbInd, t.ncInd}, ui[3] = {t.uvaInd, t.uvbInd, t.uvcInd};
        float* nd[3] = {a.n0, a.n1, a.n2}; float* ud[3] = {a.uv0, a.uv1, a.uv2};
        for (int k = 0; k < 3; k++) {
            if (ni[k] < 0 || ni[k] >= d->n_normals || !d->normals) return fail(-1, "pt_scene_create: triangle %d normal index %d out of range (faces without vn must be given a normal by the loader)", i, ni[k]);
            if (ui[k] < 0 || ui[k] >= d->n_uvs || !d->uvs) return fail(-1, "pt_scene_create: triangle %d uv index %d out of range", i, ui[k]);
            nd[k][0] = d->normals[ni[k]].x; nd[k][1] = d->normals[ni[k]].y; nd[k][2] = d->normals[ni[k]].z;
            ud[k][0] = d->uvs[ui[k]].x; ud[k][1] = d->uvs[ui[k]].y;
        }
        a.emission[0] = t.emission.x; a.emission[1] = t.emission.y; a.emission[2] = t.emission.z;
        a.material = t.materialID;
        a.lightInd = (t.lightInd >= 0 && t.lightInd < d->n_lights) ? t.lightInd : -51;
    }
    return 0;
}

// Re-pack the reference's data model for gfx950.
// deviceLeaf < 0: the caller's BVH, packed on the host. deviceLeaf >= 0 (pt_scene_create_from_mesh): the tree is built AND
// packed on the device (pt_bvh_build.hip) with that leaf size; d->bvh / d->bvh_indices are not read.
// update: the scene is being updated in place (pt_scene_update_mesh): `s` is the staging scene whose buffers are swapped in on
// success; the jump table and the counters stay the live scene's and are not touched here.
static int repack(pt_scene* s, const pt_scene_desc* d, int deviceLeaf = -1, pt_bvh_build_stats* buildStats = nullptr, bool update = false) {
    const bool onDevice = deviceLeaf >= 0;
    const int nT = d->n_triangles, nN = onDevice ? 1 : d->n_nodes;
    if (nT <= 0 || nN <= 0 || !d->triangles || (!onDevice && (!d->bvh || !d->bvh_indices)) || !d->positions || !d->materials)
        return fail(-1, "pt_scene_create: empty scene (the reference aborts with 'No triangles loaded', main.cu:505-508)");
    if (d->n_materials <= 0 || d->n_materials > 256) return fail(-1, "pt_scene_create: %d materials (1..256 supported)", d->n_materials);

    int nInternal = 0, stackNeed = 0, rootRef = 0;
    std::vector<PNode> nodes; std::vector<PTri> tris; std::vector<PAttr> attrs;
    if (!onDevice) {
        std::vector<uint8_t> leafEnd;
        if (int r = number_nodes(d->bvh, nN, nT, nodes, leafEnd, nInternal, rootRef)) return r;
        if (int r = stack_need(d->bvh, nN, stackNeed)) return r;
        if (int r = pack_triangles(d, leafEnd, tris, attrs)) return r;
    }
    // --- lights ---
    std::vector<PLight> lights(std::max(d->n_lights, 1));
    std::memset(lights.data(), 0, lights.size() * sizeof(PLight));
    for (int i = 0; i < d->n_lights; i++) {
        const pt_triangle& t = d->lights[i];
        bool ok = true;
        pt_float4 a = pos(d, t.aInd, "a", i, ok), b = pos(d, t.bInd, "b", i, ok), c = pos(d, t.cInd, "c", i, ok);
        if (!ok) return -1;
        if (t.naInd < 0 || t.naInd >= d->n_normals) return fail(-1, "pt_scene_create: light %d normal index out of range", i);
        PLight& L = lights[i];
        L.a[0] = a.x; L.a[1] = a.y; L.a[2] = a.z; L.b[0] = b.x; L.b[1] = b.y; L.b[2] = b.z; L.c[0] = c.x; L.c[1] = c.y; L.c[2] = c.z;
        L.na[0] = d->normals[t.naInd].x; L.na[1] = d->normals[t.naInd].y; L.na[2] = d->normals[t.naInd].z;
        L.emission[0] = t.emission.x; L.emission[1] = t.emission.y; L.emission[2] = t.emission.z;
        // area = 0.5f * length(cross3(b - a, c - a)) exactly as the kernels used to evaluate it per NEE sample: IEEE
        // subtractions, cross = fma(p, q, -(r * s)), dot = fma(z, z', fma(y, y', x * x')), correctly rounded sqrt
        const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
        const float cx = fmaf(uy, vz, -(uz * vy)), cy = fmaf(uz, vx, -(ux * vz)), cz = fmaf(ux, vy, -(uy * vx));
        L.area = 0.5f * sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
    }
    // --- materials ---
    std::vector<PMat> mats; std::vector<uint32_t> matClass;
    if (int r = pack_materials(d->materials, d->n_materials, d->n_texels, "pt_scene_create", mats, matClass)) return r;
    {
        uint32_t used = 0u;                       // the classes of the rows the triangles use (a device-built scene's builder refuses an index outside the table)
        for (int i = 0; i < nT; i++) {
            const int id = d->triangles[i].materialID;
            if (id >= 0 && id < d->n_materials) used |= matClass[id];
        }
        apply_material_class(s, used, d->materials[0]);
    }
    if (!onDevice) {
        if (int r = upload(s->geo.nodes, nodes.data(), nodes.size() * sizeof(PNode))) return r;
        if (int r = upload(s->geo.tris, tris.data(), tris.size() * sizeof(PTri))) return r;
        if (int r = upload(s->geo.attrs, attrs.data(), attrs.size() * sizeof(PAttr))) return r;
    } else {
        if (int r = s->geo.nodes.ensure((size_t)nT * sizeof(PNode))) return r;
        if (int r = s->geo.tris.ensure((size_t)nT * sizeof(PTri))) return r;
        if (int r = s->geo.attrs.ensure((size_t)nT * sizeof(PAttr))) return r;
        std::vector<int> types(d->n_materials);
        for (int i = 0; i < d->n_materials; i++) types[i] = d->materials[i].type;
        // what the builder packs from stays on the device with the scene: pt_scene_update_vertices rebuilds from it
        if (int r = upload(s->data.kTris, d->triangles, (size_t)nT * sizeof(pt_triangle))) return r;
        if (int r = upload(s->data.kNormals, d->normals, d->normals ? (size_t)std::max(d->n_normals, 0) * sizeof(pt_float4) : 0)) return r;
        if (int r = upload(s->data.kUvs, d->uvs, d->uvs ? (size_t)std::max(d->n_uvs, 0) * sizeof(pt_float2) : 0)) return r;
        if (int r = upload(s->data.kTypes, types.data(), types.size() * sizeof(int))) return r;
        if (int r = upload(s->data.kLightTris, d->lights, d->lights ? (size_t)std::max(d->n_lights, 0) * sizeof(pt_triangle) : 0)) return r;
        if (int r = upload(s->data.posCur, d->positions, (size_t)d->n_positions * sizeof(pt_float4))) return r;      // the motion pass reads them
        s->kept.deviceLeaf = deviceLeaf; s->kept.nPositions = d->n_positions; s->kept.nNormals = d->normals ? std::max(d->n_normals, 0) : 0; s->kept.nUvs = d->uvs ? std::max(d->n_uvs, 0) : 0;
        pt_build_src_ src{};
        src.positions = d->positions; src.n_positions = d->n_positions; src.positions_on_device = 0;
        src.d_triangles = (const pt_triangle*)s->data.kTris.p; src.n_triangles = nT;
        src.d_normals = (const pt_float4*)s->data.kNormals.p; src.n_normals = s->kept.nNormals;
        src.d_uvs = (const pt_float2*)s->data.kUvs.p; src.n_uvs = s->kept.nUvs;
        src.d_mat_types = (const int*)s->data.kTypes.p; src.n_materials = d->n_materials;
        src.d_light_tris = (const pt_triangle*)s->data.kLightTris.p; src.n_lights = d->n_lights;
        if (update) { src.pool = &s->spare.pool.p; src.pool_bytes = &s->spare.pool.bytes; }     // (creation allocates and frees its pool, as it always did)
        int out5[5] = {0, 0, 0, 0, 0};
        if (int r = pt_bvh_build_pack_(&src, deviceLeaf, s->geo.nodes.p, s->geo.tris.p, s->geo.attrs.p, nullptr, out5, buildStats)) return r;
        nInternal = out5[0]; stackNeed = out5[1]; rootRef = out5[2];
        if (out5[3]) s->facts.armless = true;
        if (stackNeed > 128) return fail(-1, "pt_scene_create_from_mesh: BVH depth %d exceeds the reference's nodeStack[128] (integratorUtilities.cuh:89)", stackNeed);
        if (int r = renumber_by_area(s, nInternal, rootRef)) return r;
    }
    if (int r = upload(s->geo.lights, lights.data(), lights.size() * sizeof(PLight))) return r;
    if (int r = upload(s->data.mats, mats.data(), mats.size() * sizeof(PMat))) return r;
    if (int r = upload(s->data.textures, d->textures, (size_t)std::max(d->n_texels, 0) * sizeof(float4))) return r;
    s->kept.nTexels = d->n_texels;                 // (what a later material edit checks its texture windows against, as above)
    if (!update) {
        const std::vector<uint32_t>& jt = xorwow_host::jump_table();
        if (int r = upload(s->data.jump, jt.data(), jt.size() * sizeof(uint32_t))) return r;
        if (int r = s->data.totals.ensure(16 * sizeof(unsigned long long))) return r;      // 8 counters + 6 diagnostic stamp sums
        HIP_OK(hipMemset(s->data.totals.p, 0, 16 * sizeof(unsigned long long)));
    }
    std::vector<int32_t> lightInd;                         // (only the scenes the pair kernels can run look at it)
    if (nT <= 128) { lightInd.resize((size_t)nT); for (int i = 0; i < nT; i++) lightInd[i] = d->triangles[i].lightInd; }
    return derive_layout(s, nInternal, stackNeed, rootRef, nT, d->n_lights, d->lights != nullptr, d->n_materials, lights.data(), lightInd.data(), (int)lightInd.size());
}

static pt_scene* create_scene(const pt_scene_desc* desc, int deviceLeaf, pt_bvh_build_stats* stats) {
    if (!desc) { fail(-1, "pt_scene_create: null desc"); return nullptr; }
    pt_scene* s = new pt_scene();
    if (hipError_t e = hipGetDevice(&s->dev.id); e != hipSuccess) {
        fail(-2, "pt_scene_create: no usable HIP device (%s); the path has no CPU fallback", hipGetErrorString(e));
        delete s;
        return nullptr;
    }
    if (repack(s, desc, deviceLeaf, stats) != 0) { pt_scene_destroy(s); return nullptr; }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, s->dev.id) == hipSuccess && prop.multiProcessorCount > 0) s->dev.numCU = prop.multiProcessorCount;
    }
    if (hipEventCreate(&s->dev.ev0) != hipSuccess || hipEventCreate(&s->dev.ev1) != hipSuccess) { fail(-2, "hipEventCreate failed"); pt_scene_destroy(s); return nullptr; }
    return s;
}

pt_scene* pt_scene_create(const pt_scene_desc* desc) { return create_scene(desc, -1, nullptr); }

pt_scene* pt_scene_create_from_mesh(const pt_scene_desc* desc, int max_leaf_size, pt_bvh_build_stats* stats) {
    if (max_leaf_size < 0) { fail(-1, "pt_scene_create_from_mesh: negative leaf size"); return nullptr; }
    return create_scene(desc, max_leaf_size, stats);
}

void pt_scene_destroy(pt_scene* s) {
    if (!s) return;
    DevBuf* all[] = {&s->geo.nodes, &s->geo.tris, &s->geo.attrs, &s->geo.lights, &s->geo.leaves, &s->data.mats, &s->data.textures, &s->data.jump, &s->data.totals,
                     &s->data.kTris, &s->data.kNormals, &s->data.kUvs, &s->data.kTypes, &s->data.kLightTris, &s->data.posCur, &s->data.posPrev,
                     &s->spare.geo.nodes, &s->spare.geo.tris, &s->spare.geo.attrs, &s->spare.geo.lights, &s->spare.geo.leaves, &s->spare.normals, &s->spare.pool,
                     &s->work.rng, &s->work.spill, &s->work.tilebuf, &s->work.colors, &s->work.pixcnt, &s->work.queue, &s->work.left, &s->wf.state, &s->wf.ctl, &s->wf.ctr,
                     &s->wf.spill, &s->ad.S, &s->ad.M, &s->ad.H, &s->ad.list, &s->ad.keep, &s->ad.count, &s->ad.P, &s->ad.Q, &s->ad.err, &s->ad.out,
                     &s->mo.S, &s->mo.P, &s->mo.Q, &s->mo.out, &s->mo.list, &s->feat.spill, &s->feat.aovOut, &s->feat.motionOut, &s->feat.idsOut, &s->feat.queryOut,
                     &s->feat.queryKeys, &s->feat.queryIdx, &s->feat.querySort, &s->upd.edit};
    for (DevBuf* b : all) b->release();
    if (s->dev.ev0) (void)hipEventDestroy(s->dev.ev0);
    if (s->dev.ev1) (void)hipEventDestroy(s->dev.ev1);
    delete s;
}

// ---- dynamic geometry: pt_scene_update_* ---------------------------------------------------------------------------------
// An update fills a STAGING scene — a default pt_scene on the caller's stack that borrows the live scene's spare buffers and the
// builder's pool — through the code creation runs (repack, or the builder + renumber_by_area + derive_layout), and only a
// complete one is swapped into the live scene. The buffers swapped out become the spares of the next update.
// What only an update of the whole mesh replaces: the tables and the builder's inputs (but the normals, which a vertex update can bring too).
static DevBuf Data::* const kMeshOnly[] = {&Data::mats, &Data::textures, &Data::kTris, &Data::kUvs, &Data::kTypes, &Data::kLightTris, &Data::posCur};
static void stage_begin(pt_scene* s, pt_scene& t) {
    auto take = [](auto& from) { auto b = from; from = {}; return b; };
    t.dev.id = s->dev.id; t.dev.numCU = s->dev.numCU;
    t.geo = take(s->spare.geo); t.data.kNormals = take(s->spare.normals); t.spare.pool = take(s->spare.pool);
}
static void stage_end(pt_scene* s, pt_scene& t) {
    s->spare.geo = t.geo; s->spare.normals = t.data.kNormals; s->spare.pool = t.spare.pool;
    for (DevBuf Data::*m : kMeshOnly) (t.data.*m).release();      // an update of the whole mesh: the old ones (or, failed, the new ones)
}
// mesh: materials, textures and the builder's inputs are the staging scene's too (pt_scene_update_mesh); otherwise only the
// geometry and, if the update brought normals, those.
static void adopt_geometry(pt_scene* s, pt_scene& t, bool mesh, bool normals) {
    std::swap(s->geo, t.geo);
    if (mesh || normals) std::swap(s->data.kNormals, t.data.kNormals);
    if (mesh) {
        for (DevBuf Data::*m : kMeshOnly) std::swap(s->data.*m, t.data.*m);
        s->upd.hasMotion = false;        // the topology may have changed: no previous positions, no motion
        s->kept = t.kept;
    }
    s->facts = t.facts;
    s->facts.ds.nodes = (const PNode*)s->geo.nodes.p; s->facts.ds.tris = (const PTri*)s->geo.tris.p; s->facts.ds.attrs = (const PAttr*)s->geo.attrs.p;
    s->facts.ds.lights = (const PLight*)s->geo.lights.p; s->facts.ds.mats = (const PMat*)s->data.mats.p; s->facts.ds.textures = (const float4*)s->data.textures.p;
    s->last.forget();
    s->upd.renumberMs = t.upd.renumberMs;
    s->upd.generation++;
}

// The per-frame path: everything but the positions (and the normals, if given) is the scene's own device copy.
static int update_vertices_staged(pt_scene* s, pt_scene& t, const void* pos, const void* nrm, bool onDevice, pt_bvh_build_stats* stats) {
    const int nT = s->facts.nTrisPacked, nL = s->facts.ds.nLights;
    if (int r = t.geo.nodes.ensure((size_t)nT * sizeof(PNode))) return r;
    if (int r = t.geo.tris.ensure((size_t)nT * sizeof(PTri))) return r;
    if (int r = t.geo.attrs.ensure((size_t)nT * sizeof(PAttr))) return r;
    if (int r = t.geo.lights.ensure((size_t)std::max(nL, 1) * sizeof(PLight))) return r;
    const void* normals = s->data.kNormals.p;
    if (nrm) {
        const size_t bytes = (size_t)s->kept.nNormals * sizeof(pt_float4);
        if (int r = t.data.kNormals.ensure(std::max<size_t>(bytes, 16))) return r;
        if (bytes) HIP_OK(hipMemcpy(t.data.kNormals.p, nrm, bytes, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        normals = t.data.kNormals.p;
    }
    pt_build_src_ src{};
    src.positions = (const pt_float4*)pos; src.n_positions = s->kept.nPositions; src.positions_on_device = onDevice ? 1 : 0;
    src.d_triangles = (const pt_triangle*)s->data.kTris.p; src.n_triangles = nT;
    src.d_normals = (const pt_float4*)normals; src.n_normals = s->kept.nNormals;
    src.d_uvs = (const pt_float2*)s->data.kUvs.p; src.n_uvs = s->kept.nUvs;
    src.d_mat_types = (const int*)s->data.kTypes.p; src.n_materials = s->facts.nMats;
    src.d_light_tris = (const pt_triangle*)s->data.kLightTris.p; src.n_lights = nL;
    src.pool = &t.spare.pool.p; src.pool_bytes = &t.spare.pool.bytes;
    int out5[5] = {0, 0, 0, 0, 0};
    if (int r = pt_bvh_build_pack_(&src, s->kept.deviceLeaf, t.geo.nodes.p, t.geo.tris.p, t.geo.attrs.p, t.geo.lights.p, out5, stats)) return r;
    const int nInternal = out5[0], stackNeed = out5[1], rootRef = out5[2];
    if (stackNeed > 128) return fail(-1, "pt_scene_update_vertices: BVH depth %d exceeds the reference's nodeStack[128] (integratorUtilities.cuh:89)", stackNeed);
    // what creation decides from the triangles' materials alone stands: neither changed
    t.facts.armless = s->facts.armless; t.facts.simpleOk = s->facts.simpleOk; t.facts.noLeafTris = s->facts.noLeafTris; t.facts.leanOk = s->facts.leanOk;
    if (int r = renumber_by_area(&t, nInternal, rootRef)) return r;
    std::vector<PLight> hostLights((size_t)std::max(nL, 1));
    std::vector<int32_t> lightInd;
    if (nT <= 128) {                       // the scenes whose lights' triangles derive_layout looks for: read the records the device made
        HIP_OK(hipMemcpy(hostLights.data(), t.geo.lights.p, hostLights.size() * sizeof(PLight), hipMemcpyDeviceToHost));
        std::vector<PAttr> at((size_t)nT);
        HIP_OK(hipMemcpy(at.data(), t.geo.attrs.p, at.size() * sizeof(PAttr), hipMemcpyDeviceToHost));
        lightInd.resize((size_t)nT);
        for (int i = 0; i < nT; i++) lightInd[i] = at[i].lightInd;
    }
    return derive_layout(&t, nInternal, stackNeed, rootRef, nT, nL, nL > 0, s->facts.nMats, hostLights.data(), lightInd.data(), (int)lightInd.size());
}

static int update_vertices(pt_scene* s, const void* pos, int nPos, const void* nrm, int nNrm, bool onDevice, pt_bvh_build_stats* stats, const char* fn) {
    if (!s) return fail(-1, "%s: null scene", fn);
    if (!pos) return fail(-1, "%s: null positions", fn);
    if (s->kept.deviceLeaf < 0)
        return fail(-1, "%s: the scene's tree was the caller's (pt_scene_create): only a scene that went through the device builder "
                        "(pt_scene_create_from_mesh, or one pt_scene_update_mesh) keeps what a vertex update rebuilds from", fn);
    if (nPos != s->kept.nPositions) return fail(-1, "%s: %d positions, the scene has %d", fn, nPos, s->kept.nPositions);
    if (nrm && nNrm != s->kept.nNormals) return fail(-1, "%s: %d normals, the scene has %d", fn, nNrm, s->kept.nNormals);
    const double t0 = wall_ms();
    HIP_OK(hipDeviceSynchronize());        // a frame boundary: nothing of the old geometry is in flight
    pt_scene t;
    stage_begin(s, t);
    int r = update_vertices_staged(s, t, pos, nrm, onDevice, stats);
    // the new positions go into the spare of the pair, and only once the build has taken them: a refused update touches neither
    const size_t posBytes = (size_t)nPos * sizeof(pt_float4);
    if (r == 0) r = s->data.posPrev.ensure(std::max<size_t>(posBytes, 16));
    if (r == 0) {
        const hipError_t e = hipMemcpy(s->data.posPrev.p, pos, posBytes, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
        if (e != hipSuccess) { s->upd.hasMotion = false; r = fail(-2, "%s: copying the positions failed: %s", fn, hipGetErrorString(e)); }
    }
    if (r == 0) {
        std::swap(s->data.posCur, s->data.posPrev); s->upd.hasMotion = true;
        adopt_geometry(s, t, false, nrm != nullptr);
    }
    stage_end(s, t);
    if (r == 0) s->upd.updateMs = (float)(wall_ms() - t0);
    if (r == 0 && stats) stats->total_ms = s->upd.updateMs;
    return r;
}

int pt_scene_update_vertices(pt_scene* s, const pt_float4* positions, int n_positions, const pt_float4* normals, int n_normals, pt_bvh_build_stats* stats) {
    return update_vertices(s, positions, n_positions, normals, n_normals, false, stats, "pt_scene_update_vertices");
}
int pt_scene_update_vertices_device(pt_scene* s, const void* d_positions, int n_positions, const void* d_normals, int n_normals, pt_bvh_build_stats* stats) {
    return update_vertices(s, d_positions, n_positions, d_normals, n_normals, true, stats, "pt_scene_update_vertices_device");
}

int pt_scene_update_mesh(pt_scene* s, const pt_scene_desc* d, int max_leaf_size, pt_bvh_build_stats* stats) {
    if (!s) return fail(-1, "pt_scene_update_mesh: null scene");
    if (!d) return fail(-1, "pt_scene_update_mesh: null desc");
    if (max_leaf_size < 0) return fail(-1, "pt_scene_update_mesh: negative leaf size");
    if (d->n_triangles <= 0 || d->n_positions <= 0 || !d->triangles || !d->positions || !d->materials)
        return fail(-1, "pt_scene_update_mesh: empty scene (triangles, positions and materials are needed)");
    if ((d->n_lights > 0 && !d->lights) || (d->n_normals > 0 && !d->normals) || (d->n_uvs > 0 && !d->uvs) || (d->n_texels > 0 && !d->textures))
        return fail(-1, "pt_scene_update_mesh: an array with a positive count is NULL");
    const double t0 = wall_ms();
    HIP_OK(hipDeviceSynchronize());        // a frame boundary: nothing of the old geometry is in flight
    pt_scene t;
    stage_begin(s, t);
    const int r = repack(&t, d, max_leaf_size, stats, true);
    if (r == 0) adopt_geometry(s, t, true, true);
    stage_end(s, t);
    if (r == 0) s->upd.updateMs = (float)(wall_ms() - t0);
    if (r == 0 && stats) stats->total_ms = s->upd.updateMs;
    return r;
}

// ---- material and emission edits: pt_scene_update_materials / pt_scene_update_emission --------------------------------------------
// Neither touches the tree, the geometry records' geometry, the leaf table, lightTri8 or the cache split: derive_layout reads a
// material only through scene_onchip_wg's per-wave area (a medium stack unless the scene is SIMPLE), and that cannot decide whether
// a scene small enough for the FLAT kernels is LDS-resident: at 16 waves the largest such scene fits with the medium stacks.
static_assert(kAttrCacheBytes > 0 && 128 * 64 + 128 * 48 + 4 * kAttrCacheBytes + 16 * (kStackFlat2Rows * 256 + kMediumMax * 64) <= 160 * 1024,
              "a material edit would have to derive flatOk again");

// The end of a successful edit: one generation on, and the previous positions describe a step the viewer has already seen.
static void edit_done(pt_scene* s, double t0) {
    s->upd.hasMotion = false;
    s->last.forget();
    s->upd.generation++;
    s->upd.updateMs = (float)(wall_ms() - t0);
}

int pt_scene_update_materials(pt_scene* s, const pt_material* materials, int n_materials) {
    const char* fn = "pt_scene_update_materials";
    if (!s) return fail(-1, "%s: null scene", fn);
    if (!materials) return fail(-1, "%s: null materials", fn);
    if (n_materials != s->facts.nMats) return fail(-1, "%s: %d materials, the scene has %d", fn, n_materials, s->facts.nMats);
    std::vector<PMat> mats; std::vector<uint32_t> matClass;
    if (int r = pack_materials(materials, n_materials, s->kept.nTexels, fn, mats, matClass)) return r;
    const double t0 = wall_ms();
    HIP_OK(hipDeviceSynchronize());        // a frame boundary: nothing that reads the old table is in flight
    // the edit buffer: the kernel's result word, then the class of every row
    const size_t classOff = 256, classBytes = matClass.size() * sizeof(uint32_t);
    if (int r = s->upd.edit.ensure(classOff + classBytes)) return r;
    uint32_t* dUsed = (uint32_t*)s->upd.edit.p;
    uint32_t* dClass = (uint32_t*)((char*)s->upd.edit.p + classOff);
    HIP_OK(hipMemset(dUsed, 0, sizeof(uint32_t)));
    HIP_OK(hipMemcpy(dClass, matClass.data(), classBytes, hipMemcpyHostToDevice));
    if (int r = pt_edit_materials_(s->geo.tris.p, s->facts.nTrisPacked, dClass, n_materials, dUsed)) return r;
    uint32_t used = 0u;
    HIP_OK(hipMemcpy(&used, dUsed, sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(s->data.mats.p, mats.data(), mats.size() * sizeof(PMat), hipMemcpyHostToDevice));
    if (s->kept.deviceLeaf >= 0) {              // what the next vertex update packs the triangles' flags from
        std::vector<int> types((size_t)n_materials);
        for (int i = 0; i < n_materials; i++) types[i] = materials[i].type;
        HIP_OK(hipMemcpy(s->data.kTypes.p, types.data(), types.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    apply_material_class(s, used, materials[0]);
    edit_done(s, t0);
    return 0;
}

int pt_scene_update_emission(pt_scene* s, int n, const int32_t* light_indices, const pt_float4* emission) {
    const char* fn = "pt_scene_update_emission";
    if (!s) return fail(-1, "%s: null scene", fn);
    if (n < 0) return fail(-1, "%s: negative count", fn);
    if (n > 0 && (!light_indices || !emission)) return fail(-1, "%s: null %s", fn, !light_indices ? "light_indices" : "emission");
    const int nL = s->facts.ds.nLights, nT = s->facts.nTrisPacked;
    for (int k = 0; k < n; k++)
        if (light_indices[k] < 0 || light_indices[k] >= nL) return fail(-1, "%s: light index %d (entry %d) out of range, the scene has %d lights", fn, light_indices[k], k, nL);
    // the edit as a table by light: the new emission and whether the light is edited at all (a repeated index: the last entry stands)
    std::vector<pt_float4> table((size_t)std::max(nL, 1));
    std::vector<int32_t> on((size_t)std::max(nL, 1), 0);
    std::memset(table.data(), 0, table.size() * sizeof(pt_float4));
    for (int k = 0; k < n; k++) { table[light_indices[k]] = emission[k]; on[light_indices[k]] = 1; }
    const double t0 = wall_ms();
    HIP_OK(hipDeviceSynchronize());        // a frame boundary
    if (n > 0) {
        const size_t tableBytes = table.size() * sizeof(pt_float4), onBytes = on.size() * sizeof(int32_t);
        if (int r = s->upd.edit.ensure(tableBytes + onBytes)) return r;
        pt_float4* dTable = (pt_float4*)s->upd.edit.p;
        int32_t* dOn = (int32_t*)((char*)s->upd.edit.p + tableBytes);
        HIP_OK(hipMemcpy(dTable, table.data(), tableBytes, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dOn, on.data(), onBytes, hipMemcpyHostToDevice));
        const bool kept = s->kept.deviceLeaf >= 0;       // ... and what the next vertex update packs attributes and lights from
        if (int r = pt_edit_emission_(s->geo.attrs.p, nT, s->geo.lights.p, nL, dTable, dOn, kept ? (pt_triangle*)s->data.kTris.p : nullptr,
                                      kept ? (pt_triangle*)s->data.kLightTris.p : nullptr))
            return r;
        HIP_OK(hipDeviceSynchronize());
    }
    edit_done(s, t0);
    return 0;
}

int pt_scene_generation(pt_scene* s) { return s ? s->upd.generation : fail(-1, "pt_scene_generation: null scene"); }

int pt_scene_has_motion(pt_scene* s) { return s ? (s->upd.hasMotion ? 1 : 0) : fail(-1, "pt_scene_has_motion: null scene"); }

int pt_debug_update_ms(pt_scene* s, float* out3) {
    if (!s || !out3) return fail(-1, "pt_debug_update_ms: null argument");
    out3[0] = s->upd.renumberMs; out3[1] = s->upd.updateMs; out3[2] = 0.0f;
    return 0;
}

// what: 0 PNodes (64 B each), 1 PTris (48 B), 2 PAttrs (80 B), 3 PLights (64 B), 4 PMats (96 B). Returns the record count (or < 0);
// copies min(count * size, capacity) bytes. For tests: the device re-layout must equal the host one.
int pt_debug_packed(pt_scene* s, int what, void* dst, size_t capacity) {
    if (!s) return fail(-1, "null scene");
    const void* src = what == 0 ? s->geo.nodes.p : what == 1 ? s->geo.tris.p : what == 2 ? s->geo.attrs.p : what == 3 ? s->geo.lights.p : what == 4 ? s->data.mats.p : nullptr;
    const size_t rec = what == 0 ? sizeof(PNode) : what == 1 ? sizeof(PTri) : what == 2 ? sizeof(PAttr) : what == 3 ? sizeof(PLight) : sizeof(PMat);
    const int count = what == 0 ? s->facts.nInternal : what == 3 ? s->facts.ds.nLights : what == 4 ? s->facts.nMats : s->facts.nTrisPacked;
    if (!src) return fail(-1, "pt_debug_packed: unknown array %d", what);
    const size_t bytes = std::min((size_t)count * rec, capacity);
    if (dst && bytes) HIP_OK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return count;
}

// Host only: light_triangles on the triangles in the leaf order desc->bvh_indices gives, packed as repack packs them.
int pt_light_triangles(const pt_scene_desc* d, int32_t* out) {
    if (!d || !out) return fail(-1, "null argument");
    if (d->n_triangles <= 0 || !d->triangles || !d->bvh_indices || !d->positions || (d->n_lights > 0 && !d->lights)) return fail(-1, "pt_light_triangles: empty scene");
    std::vector<PTri> pt((size_t)d->n_triangles);
    for (int i = 0; i < d->n_triangles; i++) {
        const int idx = d->bvh_indices[i];
        if (idx < 0 || idx >= d->n_triangles) return fail(-1, "pt_light_triangles: BVHindices[%d] = %d out of range", i, idx);
        const pt_triangle& t = d->triangles[idx];
        if (t.aInd < 0 || t.aInd >= d->n_positions || t.bInd < 0 || t.bInd >= d->n_positions || t.cInd < 0 || t.cInd >= d->n_positions)
            return fail(-1, "pt_light_triangles: triangle %d position index out of range", idx);
        const pt_float4 a = d->positions[t.aInd], b = d->positions[t.bInd], c = d->positions[t.cInd];
        PTri& p = pt[i];
        p.v0[0] = a.x; p.v0[1] = a.y; p.v0[2] = a.z;
        p.e1[0] = b.x - a.x; p.e1[1] = b.y - a.y; p.e1[2] = b.z - a.z;
        p.e2[0] = c.x - a.x; p.e2[1] = c.y - a.y; p.e2[2] = c.z - a.z;
        p.idx = (uint32_t)idx; p.material = t.materialID; p.flags = 0u;
    }
    light_triangles(pt.data(), d->n_triangles, d, out);
    return 0;
}
