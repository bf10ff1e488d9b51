// pt_bvh_build.h — what pt_scene.hip hands the device builder (pt_bvh_build.hip) when it builds AND packs a scene's tree
// (pt_scene_create_from_mesh, pt_scene_update_*). Internal: not part of the C ABI.
#pragma once
#include <stddef.h>

#include "../../include/pt_api.h"

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
// What a build tells the scene: internal nodes, stack need (internal nodes on the longest root-to-leaf path), root reference, and
// whether a triangle uses a material type without a dispatch arm.
struct pt_build_out_ { int n_internal, stack_need, root_ref, armless; };
// d_nodes / d_tris / d_attrs: device buffers for n_triangles PNodes, PTris and PAttrs. d_lights (may be NULL): room for
// max(n_lights, 1) PLights, written by the device from d_light_tris and the positions through the host re-pack's own maker (pt_pack.h).
extern "C" int pt_bvh_build_pack_(const pt_build_src_* src, int max_leaf_size, void* d_nodes, void* d_tris, void* d_attrs, void* d_lights,
                                  pt_build_out_* out, pt_bvh_build_stats* stats);
