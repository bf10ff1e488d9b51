// pt_box_table.h — the tables the FLAT kernels test instead of walking the tree, as pure host functions of the packed internal
// nodes: no HIP call, no pt_scene, no allocation besides the vectors they return, so tests/box_table_driver.hip builds them without
// a GPU (in the manner of pt_plan.h). derive_layout (pt_scene.hip) is their one caller in the library: a scene's creation, every
// update and the spare set all come through there.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "pt_device.h"

namespace pt {

// The leaf table of the FLAT kernels replaces the reference's root-to-leaf box walk by a test of each leaf's OWN box.
// That equals the reference's visiting set only if every box contains the boxes
// below it and no box holds a NaN or an infinity (pt_trace.h: inv_is_regular and the monotonicity argument above it). The
// reference's builder nests exactly (a parent's box is the float-wise min / max of its children's, main.cu:20-233), but
// pt_scene_create also takes a caller's own BVH arrays — a refit, loose or corrupt tree must fall back to the walk that
// tests the boxes the caller gave. pn: packed internal nodes, children numbered after their parents.
inline bool boxes_nested_and_finite(const std::vector<PNode>& pn, int nInternal) {
    for (int i = 0; i < nInternal; i++) {
        const PNode& p = pn[i];
        for (int a = 0; a < 3; a++)
            if (!(std::isfinite(p.lmin[a]) && std::isfinite(p.lmax[a]) && std::isfinite(p.rmin[a]) && std::isfinite(p.rmax[a]))) return false;
        const int32_t ref[2] = {p.left, p.right};
        for (int k = 0; k < 2; k++) {
            if (ref[k] < 0) continue;                              // a leaf child: its box IS the one the table tests
            if (ref[k] <= i || ref[k] >= nInternal) return false;
            const PNode& c = pn[ref[k]];
            const float* mn = k == 0 ? p.lmin : p.rmin; const float* mx = k == 0 ? p.lmax : p.rmax;
            for (int a = 0; a < 3; a++)
                if (!(mn[a] <= c.lmin[a] && mn[a] <= c.rmin[a] && mx[a] >= c.lmax[a] && mx[a] >= c.rmax[a])) return false;
        }
    }
    return true;
}

// The leaf table: every leaf child's box and triangle range, in the order of the internal nodes, left before right. pn's spare
// words hold the triangle counts of the children (derive_layout). The caller has checked boxes_nested_and_finite.
inline std::vector<PLeaf> build_leaf_table(const std::vector<PNode>& pn, int nInternal) {
    std::vector<PLeaf> lf;
    for (int i = 0; i < nInternal; i++) {
        const int32_t* ref = &pn[i].left;                           // left, right, pad0, pad1
        for (int k = 0; k < 2; k++) {
            if (ref[k] >= 0) continue;
            PLeaf L;
            const float* mn = k == 0 ? pn[i].lmin : pn[i].rmin; const float* mx = k == 0 ? pn[i].lmax : pn[i].rmax;
            for (int a = 0; a < 3; a++) { L.mn[a] = mn[a]; L.mx[a] = mx[a]; }
            L.first = ~ref[k]; L.count = ref[2 + k];
            lf.push_back(L);
        }
    }
    return lf;
}

// The box table of the timed pair kernels (pt_trace.h: trace_pair_flat under ARMS): one record per DISTINCT leaf box — all six
// floats equal as bit patterns — with the 64-bit mask of the triangles of every leaf that carries it. Two leaves with the same box
// are hit by the same rays (the slab test reads nothing else of a leaf), so one test with the OR of their ranges gives the same
// triangle set; and the mask is a constant of the scene, which the leaf loop otherwise rebuilds from (first, count) in every pass.
// Records keep the order in which their box first appears in the leaf table. Built only for scenes of at most 64 triangles (the
// pair form's limit); an empty table otherwise, or if a leaf's range does not fit the mask.
struct __attribute__((aligned(16))) PBox {
    float mn[3], mx[3];
    uint32_t maskLo, maskHi;
};
static_assert(sizeof(PBox) == sizeof(PLeaf), "the box table follows the leaf table in one buffer, and the leaf loop reads either as eight dwords");

inline std::vector<PBox> build_box_table(const std::vector<PLeaf>& leaves, int nTris) {
    std::vector<PBox> bx;
    if (nTris > 64) return bx;
    for (const PLeaf& L : leaves) {
        if (L.first < 0 || L.count < 1 || L.count > 64 || L.first > 64 - L.count) return std::vector<PBox>();
        const uint64_t m = (L.count == 64 ? ~0ull : (1ull << L.count) - 1ull) << L.first;      // (count 64: first is 0; no shift by 64)
        size_t k = 0;
        while (k < bx.size() && (std::memcmp(bx[k].mn, L.mn, 12) || std::memcmp(bx[k].mx, L.mx, 12))) k++;
        if (k == bx.size()) {
            PBox B;
            for (int a = 0; a < 3; a++) { B.mn[a] = L.mn[a]; B.mx[a] = L.mx[a]; }
            B.maskLo = 0u; B.maskHi = 0u;
            bx.push_back(B);
        }
        bx[k].maskLo |= (uint32_t)m; bx[k].maskHi |= (uint32_t)(m >> 32);
    }
    return bx;
}

// Grouping by one axis. Many distinct boxes still share an INTERVAL on some axis (the headline Cornell box: 15 boxes, 5 distinct
// (min, max) pairs on y), and a slab test's work for that axis — two subtractions, two products, min, max and the two clamps per ray —
// has the same operands and the same result for every box of such a group. group_box_table picks the axis on which the boxes have
// the fewest distinct intervals (bit patterns; ties: x before y before z), sorts the records by that interval (stable: groups in the
// order their interval first appears, records in table order inside), rotates every record's floats so that the grouped axis
// comes first — mn = {g, u, v}, mx = {g, u, v} with (g, u, v) = (axis, axis + 1, axis + 2) mod 3 — and appends one header per group
// behind the records, in a record's 32 bytes: mn[0] = lo, mx[0] = hi, maskLo = the number of records in the group. A table with no
// sharing gets one group per record. Returns the axis and the number of groups; bx grows by the headers.
struct BoxGroups { int axis = 0, nGroups = 0; };
inline BoxGroups group_box_table(std::vector<PBox>& bx) {
    BoxGroups G;
    if (bx.empty()) return G;
    auto same = [&](const PBox& a, const PBox& b, int ax) { return !std::memcmp(&a.mn[ax], &b.mn[ax], 4) && !std::memcmp(&a.mx[ax], &b.mx[ax], 4); };
    std::vector<int> best;
    for (int ax = 0; ax < 3; ax++) {
        std::vector<int> grp(bx.size());
        std::vector<size_t> rep;
        for (size_t k = 0; k < bx.size(); k++) {
            size_t g = 0;
            while (g < rep.size() && !same(bx[rep[g]], bx[k], ax)) g++;
            if (g == rep.size()) rep.push_back(k);
            grp[k] = (int)g;
        }
        if (ax == 0 || (int)rep.size() < G.nGroups) { G.axis = ax; G.nGroups = (int)rep.size(); best = grp; }
    }
    std::vector<PBox> out, heads;
    for (int g = 0; g < G.nGroups; g++) {
        PBox H{};
        for (size_t k = 0; k < bx.size(); k++) {
            if (best[k] != g) continue;
            PBox B = bx[k];
            for (int a = 0; a < 3; a++) { B.mn[a] = bx[k].mn[(G.axis + a) % 3]; B.mx[a] = bx[k].mx[(G.axis + a) % 3]; }
            H.mn[0] = B.mn[0]; H.mx[0] = B.mx[0]; H.maskLo++;
            out.push_back(B);
        }
        heads.push_back(H);
    }
    out.insert(out.end(), heads.begin(), heads.end());
    bx.swap(out);
    return G;
}

}  // namespace pt
