// pt_scene.hip — a scene's making and editing behind include/pt_api.h: the re-pack of the reference's data model and its upload,
// the layout derived from the packed records, pt_scene_create* / pt_scene_destroy, the in-place updates and the two edit kernels. The
// records themselves, and the host re-pack of a caller's own tree, are made in pt_pack.h.
#include <chrono>

#include "pt_host.h"
#include "pt_pack.h"
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
        const PTri want = make_tri(pt_float4{L.a[0], L.a[1], L.a[2], 0}, pt_float4{L.b[0], L.b[1], L.b[2], 0}, pt_float4{L.c[0], L.c[1], L.c[2], 0}, 0, false, 0, 0);
        for (int p = 0; p < nT && p < 63; p++) {                 // (the pair pass holds a ray's triangles in one 64-bit mask, and clears bit p as (1 << (p + 1)) >> 1)
            const int idx = (int)(pt[p].idx & 0x7fffffffu);
            if (idx >= nTriangles || lightIndOf(idx) != i) continue;
            if (!memcmp(pt[p].v0, want.v0, 12) && !memcmp(pt[p].e1, want.e1, 12) && !memcmp(pt[p].e2, want.e2, 12)) { out[i] = p; break; }
        }
    }
}

// What a scene decides from its triangles' materials alone, from `used` = the class words of the rows its triangles use, OR-ed:
// all four from scratch, since an edit can clear what another set.
// SIMPLE scenes (pt_path.h): every triangle's material an untextured MAT_DIFFUSE that is neither boundary nor specular, in air
// (material 0) that does not absorb — then the medium stack never changes and the dispatchers have one arm. noLeafTris: no triangle
// carries MAT_LEAF. LEAN (pt_shade.h): additionally no triangle's material samples a texture. armless: pt_pack.h.
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
    if (nInternal <= 128 || rootRef != 0) return 0;
    const double t0 = wall_ms();
    std::vector<PNode> pn((size_t)nInternal);
    HIP_OK(hipMemcpy(pn.data(), s->geo.nodes.p, (size_t)nInternal * sizeof(PNode), hipMemcpyDeviceToHost));
    std::vector<int> bfs; bfs.reserve((size_t)nInternal); bfs.push_back(0);      // bfs[k]: k-th node in breadth-first order,
    std::vector<float> area; area.reserve((size_t)nInternal); area.push_back(0.0f);      // area[k]: of its box (the root's is not read)
    std::vector<uint8_t> seen((size_t)nInternal, 0); seen[0] = 1;
    bool tree = true;
    for (size_t q = 0; q < bfs.size() && tree; q++) {
        const PNode& p = pn[bfs[q]];
        const int32_t ref[2] = {p.left, p.right};
        for (int k = 0; k < 2; k++) {
            if (ref[k] < 0) continue;
            if (ref[k] >= nInternal || seen[ref[k]]) { tree = false; break; }
            seen[ref[k]] = 1;
            area.push_back(k == 0 ? order_area(p.lmin, p.lmax) : order_area(p.rmin, p.rmax));
            bfs.push_back(ref[k]);
        }
    }
    if (tree && (int)bfs.size() == nInternal) {
        const std::vector<int> byPlace = rank_by_area(area);
        std::vector<int> rank((size_t)nInternal);
        for (int k = 0; k < nInternal; k++) rank[bfs[k]] = byPlace[k];
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
    return 0;
}

// The device scene's six pointers, at the scene's own buffers.
static void point_ds(pt_scene* s) {
    s->facts.ds.nodes = (const PNode*)s->geo.nodes.p; s->facts.ds.tris = (const PTri*)s->geo.tris.p; s->facts.ds.attrs = (const PAttr*)s->geo.attrs.p;
    s->facts.ds.lights = (const PLight*)s->geo.lights.p; s->facts.ds.mats = (const PMat*)s->data.mats.p; s->facts.ds.textures = (const float4*)s->data.textures.p;
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
    point_ds(s);
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
            while (k < nT) if (pt[k++].idx & 0x80000000u) return k - first;
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

// What the device builder packs from: the scene's kept device arrays and the given positions (a host array unless onDevice).
static pt_build_src_ build_src(const pt_scene* s, const void* positions, bool onDevice, int nT, int nMats, int nLights) {
    pt_build_src_ src{};
    src.positions = (const pt_float4*)positions; src.n_positions = s->kept.nPositions; src.positions_on_device = onDevice ? 1 : 0;
    src.d_triangles = (const pt_triangle*)s->data.kTris.p; src.n_triangles = nT;
    src.d_normals = (const pt_float4*)s->data.kNormals.p; src.n_normals = s->kept.nNormals;
    src.d_uvs = (const pt_float2*)s->data.kUvs.p; src.n_uvs = s->kept.nUvs;
    src.d_mat_types = (const int*)s->data.kTypes.p; src.n_materials = nMats;
    src.d_light_tris = (const pt_triangle*)s->data.kLightTris.p; src.n_lights = nLights;
    return src;
}
// The tree and the records of t->geo from src, on the device (pt_bvh_build.hip), the internal nodes then numbered by area. dLights:
// t's PLight buffer, or NULL when the host packs the lights. fn names the caller when the tree is refused as too deep.
static int build_geometry(pt_scene* t, const pt_build_src_& src, int leaf, void* dLights, const char* fn, pt_bvh_build_stats* stats, pt_build_out_& built) {
    const size_t nT = (size_t)src.n_triangles;
    if (int r = t->geo.nodes.ensure(nT * sizeof(PNode))) return r;
    if (int r = t->geo.tris.ensure(nT * sizeof(PTri))) return r;
    if (int r = t->geo.attrs.ensure(nT * sizeof(PAttr))) return r;
    if (int r = pt_bvh_build_pack_(&src, leaf, t->geo.nodes.p, t->geo.tris.p, t->geo.attrs.p, dLights, &built, stats)) return r;
    if (built.stack_need > 128) return fail(-1, "%s: BVH depth %d exceeds the reference's nodeStack[128] (integratorUtilities.cuh:89)", fn, built.stack_need);
    return renumber_by_area(t, built.n_internal, built.root_ref);
}

// Re-pack the reference's data model for gfx950: pack, upload, derive_layout.
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
    std::vector<PLight> lights;
    if (int r = pack_lights(d, lights)) return r;
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
        pt_build_src_ src = build_src(s, d->positions, false, nT, d->n_materials, d->n_lights);
        if (update) { src.pool = &s->spare.pool.p; src.pool_bytes = &s->spare.pool.bytes; }     // (creation allocates and frees its pool, as it always did)
        pt_build_out_ built{};
        if (int r = build_geometry(s, src, deviceLeaf, nullptr, "pt_scene_create_from_mesh", buildStats, built)) return r;
        nInternal = built.n_internal; stackNeed = built.stack_need; rootRef = built.root_ref;
        if (built.armless) s->facts.armless = true;
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
// The end of an update that began at t0 and came to r: the staging scene's buffers go back; a successful one is timed. Returns r.
static int stage_end(pt_scene* s, pt_scene& t, int r, double t0, pt_bvh_build_stats* stats) {
    s->spare.geo = t.geo; s->spare.normals = t.data.kNormals; s->spare.pool = t.spare.pool;
    for (DevBuf Data::*m : kMeshOnly) (t.data.*m).release();      // an update of the whole mesh: the old ones (or, failed, the new ones)
    if (r == 0) s->upd.updateMs = (float)(wall_ms() - t0);
    if (r == 0 && stats) stats->total_ms = s->upd.updateMs;
    return r;
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
    point_ds(s);
    s->last.forget();
    s->upd.renumberMs = t.upd.renumberMs;
    s->upd.generation++;
}

// The per-frame path: everything but the positions (and the normals, if given) is the scene's own device copy.
static int update_vertices_staged(pt_scene* s, pt_scene& t, const void* pos, const void* nrm, bool onDevice, pt_bvh_build_stats* stats) {
    const int nT = s->facts.nTrisPacked, nL = s->facts.ds.nLights;
    if (int r = t.geo.lights.ensure((size_t)std::max(nL, 1) * sizeof(PLight))) return r;
    const void* normals = s->data.kNormals.p;
    if (nrm) {
        const size_t bytes = (size_t)s->kept.nNormals * sizeof(pt_float4);
        if (int r = t.data.kNormals.ensure(std::max<size_t>(bytes, 16))) return r;
        if (bytes) HIP_OK(hipMemcpy(t.data.kNormals.p, nrm, bytes, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        normals = t.data.kNormals.p;
    }
    pt_build_src_ src = build_src(s, pos, onDevice, nT, s->facts.nMats, nL);
    src.d_normals = (const pt_float4*)normals;
    src.pool = &t.spare.pool.p; src.pool_bytes = &t.spare.pool.bytes;
    pt_build_out_ built{};
    if (int r = build_geometry(&t, src, s->kept.deviceLeaf, t.geo.lights.p, "pt_scene_update_vertices", stats, built)) return r;
    // what creation decides from the triangles' materials alone stands: neither changed
    t.facts.armless = s->facts.armless; t.facts.simpleOk = s->facts.simpleOk; t.facts.noLeafTris = s->facts.noLeafTris; t.facts.leanOk = s->facts.leanOk;
    std::vector<PLight> hostLights((size_t)std::max(nL, 1));
    std::vector<int32_t> lightInd;
    if (nT <= 128) {                       // the scenes whose lights' triangles derive_layout looks for: read the records the device made
        HIP_OK(hipMemcpy(hostLights.data(), t.geo.lights.p, hostLights.size() * sizeof(PLight), hipMemcpyDeviceToHost));
        std::vector<PAttr> at((size_t)nT);
        HIP_OK(hipMemcpy(at.data(), t.geo.attrs.p, at.size() * sizeof(PAttr), hipMemcpyDeviceToHost));
        lightInd.resize((size_t)nT);
        for (int i = 0; i < nT; i++) lightInd[i] = at[i].lightInd;
    }
    return derive_layout(&t, built.n_internal, built.stack_need, built.root_ref, nT, nL, nL > 0, s->facts.nMats, hostLights.data(), lightInd.data(), (int)lightInd.size());
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
    return stage_end(s, t, r, t0, stats);
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
    return stage_end(s, t, r, t0, stats);
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

// ---- the edit kernels: what the pack kernels (pt_bvh_build.hip) would write for the edited description, without the tree, the
// positions or the builder's arrays. Both are launched on the null stream; every pointer is a device pointer.
// One thread per packed triangle: its flags word from its material row's class (pt_material_class_), the only word of the record a
// material decides; the classes are OR-ed over the wave with one ballot per class bit and leave it in one atomicOr into *orOut, which
// the caller zeroes. Lanes past the end carry class 0 and stay for the ballots.
constexpr int kEditBlock = 256;
constexpr uint32_t kClassBits[4] = {kTriLeaf, kRowTextured, kRowNotSimple, kTriArmless};
__global__ void k_edit_materials(PTri* tris, int n, const uint32_t* cls, int nMats, uint32_t* orOut) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = 0u;
    if (i < n) {
        const int mat = tris[i].material;                      // creation refused an index outside the table
        if (mat >= 0 && mat < nMats) c = cls[mat];
        tris[i].flags = c & kTriLeaf;
    }
    uint32_t w = 0u;
    for (int b = 0; b < 4; b++)
        if (__ballot((c & kClassBits[b]) != 0u)) w |= kClassBits[b];
    if ((threadIdx.x & 63) == 0 && w) atomicOr(orOut, w);
}
// Thread i < n: attribute i (original triangle index, as the kept triangles are) takes its light's emission if that light is edited;
// thread i < nLights: light i itself. emission / on: the edit as a table by light (on[li] != 0: light li is edited), so that a
// triangle does one lookup. keptTris / keptLightTris (both NULL for a scene without a device builder): the pt_triangle arrays the
// builder packs from, whose `emission` gets all four floats.
__global__ void k_edit_emission(PAttr* attrs, int n, PLight* lights, int nLights, const pt_float4* emission, const int32_t* on,
                                pt_triangle* keptTris, pt_triangle* keptLightTris) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int li = attrs[i].lightInd;
        if (li >= 0 && li < nLights && on[li]) {
            const pt_float4 e = emission[li];
            attrs[i].emission[0] = e.x; attrs[i].emission[1] = e.y; attrs[i].emission[2] = e.z;
            if (keptTris) keptTris[i].emission = e;
        }
    }
    if (i < nLights && on[i]) {
        const pt_float4 e = emission[i];
        lights[i].emission[0] = e.x; lights[i].emission[1] = e.y; lights[i].emission[2] = e.z;
        if (keptLightTris) keptLightTris[i].emission = e;
    }
}
static int edit_blocks(int n) { return std::max(1, (n + kEditBlock - 1) / kEditBlock); }
static int launched() { const hipError_t e = hipGetLastError(); return e == hipSuccess ? 0 : fail(-2, "%s", hipGetErrorString(e)); }

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
    hipLaunchKernelGGL(k_edit_materials, dim3(edit_blocks(s->facts.nTrisPacked)), dim3(kEditBlock), 0, nullptr, (PTri*)s->geo.tris.p, s->facts.nTrisPacked, dClass, n_materials, dUsed);
    if (int r = launched()) return r;
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
        hipLaunchKernelGGL(k_edit_emission, dim3(edit_blocks(std::max(nT, nL))), dim3(kEditBlock), 0, nullptr, (PAttr*)s->geo.attrs.p, nT, (PLight*)s->geo.lights.p, nL,
                           dTable, dOn, kept ? (pt_triangle*)s->data.kTris.p : nullptr, kept ? (pt_triangle*)s->data.kLightTris.p : nullptr);
        if (int r = launched()) return r;
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
        pt[i] = make_tri(d->positions[t.aInd], d->positions[t.bInd], d->positions[t.cInd], idx, false, t.materialID, PT_MAT_DIFFUSE);      // (no leaf ends, flags 0: only v0, e1, e2 are compared)
    }
    std::vector<PLight> L((size_t)std::max(d->n_lights, 1), PLight{});
    std::vector<uint8_t> bad((size_t)std::max(d->n_lights, 1), 0);      // a light whose vertex indices are out of range gets -1
    for (int i = 0; i < d->n_lights; i++) {
        const pt_triangle& t = d->lights[i];
        if (t.aInd < 0 || t.aInd >= d->n_positions || t.bInd < 0 || t.bInd >= d->n_positions || t.cInd < 0 || t.cInd >= d->n_positions) { bad[i] = 1; continue; }
        L[i] = make_light(d->positions[t.aInd], d->positions[t.bInd], d->positions[t.cInd], pt_float4{0, 0, 0, 0}, t.emission);
    }
    light_triangles(pt.data(), d->n_triangles, L.data(), d->n_lights, d->n_triangles,
                    [&](int idx) { const int li = d->triangles[idx].lightInd; return (li >= 0 && li < d->n_lights && bad[li]) ? -1 : li; }, out);
    return 0;
}
