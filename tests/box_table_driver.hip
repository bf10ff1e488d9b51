// Host-only driver of tests/test_box_table.py: builds the leaf table and the pair kernels' box table (pt_box_table.h) from packed
// internal nodes, as derive_layout (pt_scene.hip) does, and prints them. Built with --cuda-host-only: no device code, no GPU.
//
//   box_table_driver <file of PNode records> <number of triangles> [...]
//
// A file holds the 64-byte PNode records of a tree, the children's triangle counts in their spare words (what derive_layout writes
// there before it builds the tables). Per file, on stdout:
//   tree <file> nodes <n> nested <0|1> leaves <n> boxes <n>
//   L <first> <count> <six floats as hex bit patterns: mn x y z, mx x y z>          one line per leaf record
//   B <mask as 16 hex digits> <six floats as hex bit patterns>                      one line per box record, before grouping
//   groups axis <0|1|2> n <groups>                                                  then group_box_table's result:
//   R <mask> <six floats: mn g u v, mx g u v>                                       one line per record as the kernel reads it, sorted by group
//   G <count> <lo> <hi>                                                             one line per group header
// A tree that is not nested and finite gets no table: leaves 0 boxes 0, as derive_layout leaves it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "pt_box_table.h"

using namespace pt;

static void bits6(const float* mn, const float* mx) {
    for (int a = 0; a < 6; a++) { uint32_t w; memcpy(&w, a < 3 ? &mn[a] : &mx[a - 3], 4); printf(" %08x", w); }
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 3 || (argc - 1) % 2) { fprintf(stderr, "usage: %s <PNode file> <triangles> [...]\n", argv[0]); return 2; }
    for (int k = 1; k + 1 < argc; k += 2) {
        FILE* f = fopen(argv[k], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[k]); return 2; }
        std::vector<PNode> pn;
        PNode rec;
        while (fread((void*)&rec, sizeof rec, 1, f) == 1) pn.push_back(rec);
        fclose(f);
        const int nInternal = (int)pn.size(), nT = atoi(argv[k + 1]);
        const bool nested = nInternal > 0 && boxes_nested_and_finite(pn, nInternal);
        std::vector<PLeaf> lf;
        std::vector<PBox> bx;
        if (nested) { lf = build_leaf_table(pn, nInternal); bx = build_box_table(lf, nT); }
        printf("tree %s nodes %d nested %d leaves %d boxes %d\n", argv[k], nInternal, nested ? 1 : 0, (int)lf.size(), (int)bx.size());
        for (const PLeaf& L : lf) { printf("L %d %d", L.first, L.count); bits6(L.mn, L.mx); }
        for (const PBox& B : bx) { printf("B %08x%08x", B.maskHi, B.maskLo); bits6(B.mn, B.mx); }
        const size_t nB = bx.size();
        const BoxGroups G = group_box_table(bx);
        printf("groups axis %d n %d\n", G.axis, G.nGroups);
        if (bx.size() != nB + (size_t)G.nGroups) { fprintf(stderr, "group_box_table: %zu records and %d groups became %zu\n", nB, G.nGroups, bx.size()); return 1; }
        for (size_t r = 0; r < nB; r++) { printf("R %08x%08x", bx[r].maskHi, bx[r].maskLo); bits6(bx[r].mn, bx[r].mx); }
        for (size_t g = nB; g < bx.size(); g++) {
            uint32_t lo, hi; memcpy(&lo, &bx[g].mn[0], 4); memcpy(&hi, &bx[g].mx[0], 4);
            printf("G %u %08x %08x\n", bx[g].maskLo, lo, hi);
        }
    }
    return 0;
}
