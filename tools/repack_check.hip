// repack_check.hip — a host-only check of the three functions repack (csrc/pt_scene.hip) runs on a caller's own tree: number_nodes,
// stack_need and pack_triangles. They are static in that unit, so this program includes it, and links libptamd.so for the rest of
// what the unit calls. No device is touched. Meant for a sanitizer build of the host side (from the repository root):
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -g -Xarch_host -fsanitize=address,undefined -o tools/_repack_check \
//         tools/repack_check.hip -Lcudapathtracer_amd/csrc -lptamd -Wl,-rpath,$PWD/cudapathtracer_amd/csrc
//   tools/_repack_check
// Prints one line per case and returns 0 iff every case came out as expected.
#include "../cudapathtracer_amd/csrc/pt_scene.hip"

#include <cstdio>

static int expect(const char* what, bool ok) {
    printf("%-60s %s\n", what, ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    const pt_float4 lo = {0, 0, 0, 0}, hi = {1, 1, 1, 0};
    // two triangles, one internal node
    const pt_bvh_node tree[3] = {{lo, hi, 1, 2, -1, 0}, {lo, hi, -1, -1, 0, 1}, {lo, hi, -1, -1, 1, 1}};
    // node 1 points back at the root
    const pt_bvh_node cyclic[3] = {{lo, hi, 1, 2, -1, 0}, {lo, hi, 0, 2, -1, 0}, {lo, hi, -1, -1, 0, 2}};
    {
        std::vector<PNode> nodes; std::vector<uint8_t> leafEnd; int nInternal = 0, rootRef = -7, need = 0;
        const int r = number_nodes(tree, 3, 2, nodes, leafEnd, nInternal, rootRef);
        bad += expect("number_nodes accepts the two-triangle tree", r == 0 && nInternal == 1 && rootRef == 0 && nodes.size() == 1 && nodes[0].left == ~0 &&
                                                                   nodes[0].right == ~1 && leafEnd.size() == 2 && leafEnd[0] == 1 && leafEnd[1] == 1);
        bad += expect("stack_need of the two-triangle tree is 1", stack_need(tree, 3, need) == 0 && need == 1);

        const pt_float4 positions[4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {0, 1, 0, 0}, {1, 1, 0, 0}};
        const pt_float4 normals[1] = {{0, 0, 1, 0}};
        const pt_float2 uvs[1] = {{0, 0}};
        pt_triangle tris[2] = {};
        tris[0].aInd = 0; tris[0].bInd = 1; tris[0].cInd = 2; tris[0].lightInd = -51;
        tris[1].aInd = 1; tris[1].bInd = 3; tris[1].cInd = 2; tris[1].lightInd = -51; tris[1].triInd = 1;
        const int32_t order[2] = {1, 0};
        pt_material mat = {};
        pt_scene_desc d = {};
        d.positions = positions; d.n_positions = 4; d.normals = normals; d.n_normals = 1; d.uvs = uvs; d.n_uvs = 1;
        d.triangles = tris; d.n_triangles = 2; d.bvh = tree; d.n_nodes = 3; d.bvh_indices = order; d.materials = &mat; d.n_materials = 1;
        std::vector<PTri> pt; std::vector<PAttr> at;
        const int rp = pack_triangles(&d, leafEnd, pt, at);
        bad += expect("pack_triangles packs it in leaf order", rp == 0 && pt.size() == 2 && at.size() == 2 && pt[0].idx == (1u | 0x80000000u) &&
                                                              pt[1].idx == (0u | 0x80000000u) && pt[0].v0[0] == 1.0f && pt[0].e1[1] == 1.0f && at[1].lightInd == -51);
        tris[1].cInd = 4;
        bad += expect("pack_triangles refuses a position index out of range", pack_triangles(&d, leafEnd, pt, at) == -1 && strstr(pt_last_error(), "index 4 out of range"));
    }
    {
        std::vector<PNode> nodes; std::vector<uint8_t> leafEnd; int nInternal = 0, rootRef = 0, need = 0;
        const int r = number_nodes(cyclic, 3, 2, nodes, leafEnd, nInternal, rootRef);
        bad += expect("number_nodes: the cyclic tree is not a tree", r == -1 && !strcmp(pt_last_error(), "pt_scene_create: BVH is not a tree"));
        fail(0, "none");
        bad += expect("stack_need: the cyclic tree is not a tree", stack_need(cyclic, 3, need) == -1 && !strcmp(pt_last_error(), "pt_scene_create: BVH is not a tree"));
    }
    return bad ? 1 : 0;
}
