// pt_bvh_build.h — what pt_scene.hip hands the device builder (pt_bvh_build.hip) when it builds AND packs a scene's tree
// (pt_scene_create_from_mesh, pt_scene_update_*). Internal: not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/pt_api.h"

// What a triangle takes from its material's TYPE: pt_tri_flags_ is the PTri.flags word (kTriLeaf: a MAT_LEAF triangle), and a type
// without a dispatch arm (pt_path.h) carries kTriArmless in its class. One pair of expressions for the device pack (k_pack_tris),
// the host re-pack (repack) and the material edit (k_edit_materials, through pt_material_class_), so the three cannot drift.
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

struct pt_build_src_ {
    const pt_float4* positions; int n_positions;     // a host array (uploaded into the pool), or,
    int positions_on_device;                         // if set, a device array that the builder reads in place: nothing is uploaded
    // device arrays that the scene keeps between builds (desc->triangles, normals, uvs, materials[].type, lights)
    const pt_triangle* d_triangles; int n_triangles;
    const pt_float4* d_normals; int n_normals;
    const pt_float2* d_uvs; int n_uvs;
    const int* d_mat_types; int n_materials;
    const pt_triangle* d_light_tris; int n_lights;
    // the builder's pool. Both NULL: allocated and freed by the call. Otherwise the caller's, grown here when it is too small and
    // never freed here, a failed build included
    void** pool; size_t* pool_bytes;
};
// d_nodes / d_tris / d_attrs: device buffers for n_triangles PNodes, PTris and PAttrs. d_lights (may be NULL): room for
// max(n_lights, 1) PLights, written by the device from d_light_tris and the positions, byte for byte what the host re-pack
// computes. out5 = internal nodes, stack need (internal nodes on the longest root-to-leaf path), root reference, 1 if a triangle
// uses a material type without a dispatch arm, total reference nodes.
extern "C" int pt_bvh_build_pack_(const pt_build_src_* src, int max_leaf_size, void* d_nodes, void* d_tris, void* d_attrs, void* d_lights,
                                  int* out5, pt_bvh_build_stats* stats);

// In-place edits of the packed records (pt_scene_update_materials / pt_scene_update_emission). Both launch on the null stream and
// return without waiting; every pointer is a device pointer.
// Materials: d_tris[i].flags = d_class[d_tris[i].material] & kTriLeaf for the n_triangles PTris, and *d_or |= the OR of the classes of
// the rows the triangles use (pt_material_class_ words, n_materials of them). The caller zeroes *d_or.
extern "C" int pt_edit_materials_(void* d_tris, int n_triangles, const uint32_t* d_class, int n_materials, uint32_t* d_or);
// Emission: d_on[li] != 0 marks light li as edited, d_emission[li] is its new emission (n_lights entries each). Every PAttr whose
// lightInd is an edited light gets the emission's x, y, z, and so does the PLight itself. d_kept_tris / d_kept_light_tris (both NULL
// for a scene without a device builder): the pt_triangle arrays the builder packs from, whose `emission` gets all four floats.
extern "C" int pt_edit_emission_(void* d_attrs, int n_triangles, void* d_lights, int n_lights, const pt_float4* d_emission, const int32_t* d_on,
                                 pt_triangle* d_kept_tris, pt_triangle* d_kept_light_tris);
