// repack_check.hip — a host-only check of csrc/pt_pack.h: the makers of the packed records on exactly representable values, the
// area ranking, and the host re-pack of a caller's own tree (number_nodes, stack_need, pack_triangles). No device is touched and no
// library is linked: tests/test_repack_check.py builds it with --cuda-host-only, plain and with -fsanitize=address,undefined.
// Prints one line per case and returns 0 iff every case came out as expected.
#include "../cudapathtracer_amd/csrc/pt_pack.h"

#include <cstdarg>
#include <cstdio>

using namespace pt;

static char g_msg[512] = "";      // the unit's own error channel: what pt_last_error would return
int pt::fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof g_msg, fmt, ap); va_end(ap);
    return code;
}
static int expect(const char* what, bool ok) {
    printf("%-60s %s\n", what, ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}
template <class T, size_t N> static bool same(const T (&a)[N], std::initializer_list<T> b) { return std::equal(a, a + N, b.begin()); }

int main() {
    int bad = 0;
    const pt_float4 lo = {0, 0, 0, 0}, hi = {1, 1, 1, 0};
    {   // the makers
        const pt_float4 a = {0, 0, 0, 9}, b = {3, 0, 0, 9}, c = {0, 4, 0, 9}, n = {0, 0, 1, 9}, e = {2, 4, 8, 9};
        const PLight L = make_light(a, b, c, n, e);
        bad += expect("make_light: the 3-4-5 triangle has area 6", L.area == 6.0f && same(L.a, {0.f, 0.f, 0.f}) && same(L.b, {3.f, 0.f, 0.f}) && same(L.c, {0.f, 4.f, 0.f}) &&
                                                                  same(L.na, {0.f, 0.f, 1.f}) && same(L.emission, {2.f, 4.f, 8.f}));
        const PTri t = make_tri(b, c, a, 5, true, 7, PT_MAT_LEAF), u = make_tri(b, c, a, 5, false, 7, PT_MAT_DIFFUSE);
        bad += expect("make_tri: v0, e1 = b - a, e2 = c - a, leaf-end bit, flags", same(t.v0, {3.f, 0.f, 0.f}) && same(t.e1, {-3.f, 4.f, 0.f}) && same(t.e2, {-3.f, 0.f, 0.f}) &&
                                                                                  t.idx == (5u | 0x80000000u) && t.material == 7 && t.flags == kTriLeaf && u.idx == 5u && u.flags == 0u);
        pt_triangle tr = {}; tr.emission = e; tr.materialID = 3; tr.lightInd = 2;
        const pt_float4 nn[3] = {{1, 0, 0, 9}, {0, 1, 0, 9}, {0, 0, 1, 9}};
        const pt_float2 uv[3] = {{0.25f, 0.5f}, {0.75f, 1}, {2, 4}};
        const PAttr in = make_attr(tr, nn, uv, 3), out = make_attr(tr, nn, uv, 2);
        bad += expect("make_attr: a lightInd outside the light list becomes -51", in.lightInd == 2 && out.lightInd == -51 && in.material == 3 && same(in.n1, {0.f, 1.f, 0.f}) &&
                                                                                 same(in.uv0, {0.25f, 0.5f}) && same(in.uv2, {2.f, 4.f}) && same(in.emission, {2.f, 4.f, 8.f}));
        const float l0[3] = {0, 1, 2}, l1[3] = {3, 4, 5}, r0[3] = {-1, -2, -3}, r1[3] = {6, 7, 8};
        const PNode p = make_node(l0, l1, r0, r1, 4, ~9);
        bad += expect("make_node: two boxes, two refs, spare words zero", same(p.lmin, {0.f, 1.f, 2.f}) && same(p.lmax, {3.f, 4.f, 5.f}) && same(p.rmin, {-1.f, -2.f, -3.f}) &&
                                                                         same(p.rmax, {6.f, 7.f, 8.f}) && p.left == 4 && p.right == ~9 && p.pad0 == 0 && p.pad1 == 0);
        const float big[3] = {3e38f, 3e38f, 3e38f}, nb[3] = {-3e38f, -3e38f, -3e38f};
        bad += expect("order_area: dx*dy + dy*dz + dz*dx, non-finite -> 0", order_area(l0, l1) == 27.0f && order_area(nb, big) == 0.0f);
        // the root stays first whatever its area; then descending, the tie (nodes 1 and 4) and the zeros (3 and 5) in breadth-first order
        bad += expect("rank_by_area: stable, descending, root fixed", rank_by_area({0.0f, 2.0f, 8.0f, order_area(nb, big), 2.0f, 0.0f}) == std::vector<int>({0, 2, 1, 4, 3, 5}));
    }
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
        d.lights = tris; d.n_lights = 1;
        std::vector<PTri> pt; std::vector<PAttr> at; std::vector<PLight> li;
        const int rp = pack_triangles(&d, leafEnd, pt, at);
        bad += expect("pack_triangles packs it in leaf order", rp == 0 && pt.size() == 2 && at.size() == 2 && pt[0].idx == (1u | 0x80000000u) &&
                                                              pt[1].idx == (0u | 0x80000000u) && pt[0].v0[0] == 1.0f && pt[0].e1[1] == 1.0f && at[1].lightInd == -51);
        bad += expect("pack_lights: the half square has area 1/2", pack_lights(&d, li) == 0 && li.size() == 1 && li[0].area == 0.5f && li[0].na[2] == 1.0f);
        tris[1].cInd = 4;
        bad += expect("pack_triangles refuses a position index out of range", pack_triangles(&d, leafEnd, pt, at) == -1 && strstr(g_msg, "index 4 out of range"));
    }
    {
        std::vector<PNode> nodes; std::vector<uint8_t> leafEnd; int nInternal = 0, rootRef = 0, need = 0;
        const int r = number_nodes(cyclic, 3, 2, nodes, leafEnd, nInternal, rootRef);
        bad += expect("number_nodes: the cyclic tree is not a tree", r == -1 && !strcmp(g_msg, "pt_scene_create: BVH is not a tree"));
        fail(0, "none");
        bad += expect("stack_need: the cyclic tree is not a tree", stack_need(cyclic, 3, need) == -1 && !strcmp(g_msg, "pt_scene_create: BVH is not a tree"));
    }
    return bad ? 1 : 0;
}
