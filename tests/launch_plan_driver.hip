// Host-only driver of tests/test_mk_choice.py, the sibling of mk_choice_driver.hip one step earlier on the launch path: walks
// plan_launch and size_launch (pt_plan.hip) with megakernel_choose and launch_megakernel (pt_kernels.hip) between and after them, as
// render_tiles (pt_render.hip) calls them, over scene shapes x fact flags x options x what a launch is asked for, at 256 CUs. Built
// with --cuda-host-only: no device code, no GPU; the same stubs as mk_choice_driver.hip, so a "launch" records its dynamic LDS.
//
// An input's outcome has four parts, each `-` where render_tiles does not get that far (it refuses a counting launch with a tile
// list before it plans; without a row nothing is sized):
//   plan   `wg <onchipWg> hbm <> cull <> refill <> flat <> simple <> lean <> simpleTimed <> timedHbm <>`
//   row    the name of the row megakernel_choose returned, or `none`
//   scene  `wgWaves <> wavesPerSimd <> cacheNodes <> cacheTris <> cacheAttrs <> cacheMats <> cacheLights <> nLeaves <> gnodeFrom <>
//           stackSpill <> refillKeep <> spillEntries <> lds <dynamic LDS bytes of the stubbed launch> attr <hipFuncSetAttribute calls>`
//   grid   `blocks <> queueCap <> queueMask <> gridBlocks <> tileCount <> useMIS <>`
// Output: on stdout a line `A <shapes, option sets and live counts as JSON>`, then one line per distinct part, `<P|R|S|G> <id> <text>`,
// ids in the order of first appearance; in the file argv[1]
// four int32 ids (plan, row, scene, grid) per input, the inputs in the order of the loops of main(): shape, flags, options, live,
// listed, integrator, count, useMIS.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "pt_plan.h"

static unsigned g_lds;
static int g_attr, g_launches;
extern "C" hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t lds, hipStream_t) { g_lds = (unsigned)lds; g_launches++; return hipSuccess; }
extern "C" hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { g_attr++; return hipSuccess; }
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }
extern "C" void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
extern "C" void __hipUnregisterFatBinary(void**) {}
extern "C" void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
extern "C" void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}

using namespace pt;

// ---- the axes (tests/golden/launch_plan_parent.json lists the same: test_mk_choice.py compares them) ----
struct Shape { int nInternal, nTris, nMats, nLights, stackNeed, nLeaves; };
static const Shape kShapes[] = {
    {11, 36, 24, 2, 5, 12},             // a Cornell box: resident in 4-wave workgroups, FLAT with 64-bit masks
    {11, 36, 24, 2, 20, 12},            // ... with a tree deeper than the LDS stack: stackSpill != 0, in HBM with its triangles cached
    {64, 64, 4, 1, 7, 65},              // 64 / 64: 1 KB over at 4 waves with medium stacks (8 then), fits with the SIMPLE per-wave area
    {65, 65, 4, 1, 8, 0},               // 128-bit masks; no leaf table
    {128, 128, 1, 1, 9, 129},           // 16-wave workgroups with medium stacks, 8 without
    {129, 129, 1, 1, 9, 0},
    {300, 2000, 8, 4, 14, 0},           // in HBM, cacheTris 0: nInternal below kCacheBytesHbm / 64 and kCacheBytesHbmSimple / 64,
    {600, 5000, 8, 4, 18, 0},           // between them,
    {100000, 263000, 40, 16, 30, 0},    // and above both
};
// what derive_layout (pt_scene.hip) derives from a shape; the five flags are crossed freely
static Facts facts_of(const Shape& sh, int flags) {
    Facts F;
    F.nInternal = sh.nInternal; F.nTrisPacked = sh.nTris; F.ds.nTris = sh.nTris; F.nMats = sh.nMats; F.nLightsPacked = sh.nLights; F.ds.nLights = sh.nLights;
    F.stackNeed = sh.stackNeed; F.ds.stackSpill = sh.stackNeed > kStackLds ? sh.stackNeed - kStackLds : 0; F.nLeaves = sh.nLeaves;
    if ((size_t)sh.nInternal * 64 + (size_t)sh.nTris * 48 <= (size_t)kCacheBytes) { F.cacheNodes = sh.nInternal; F.cacheTris = sh.nTris; }
    else { F.cacheNodes = sh.nInternal < kCacheBytes / 64 ? sh.nInternal : kCacheBytes / 64; F.cacheTris = 0; }
    F.flatOk = flags & 1; F.simpleOk = flags & 2; F.leanOk = flags & 4; F.armless = flags & 8; F.noLeafTris = flags & 16;
    return F;
}
// every option the plan or the sizing reads, at every value pt_set_option accepts for it besides its default
struct Setting { const char* name; int value; };
static const Setting kSettings[] = {{"onchip", 0}, {"waves_hbm", 0}, {"waves_hbm", 2}, {"refill", 0}, {"culling", 1}, {"flat", 0}, {"flat", 2}, {"flat2", 0},
                                    {"simple", 0}, {"lean", 0}, {"leaf_boxes", 0}, {"refill_keep", 3}, {"persistent", 0}};
static const int kNumSettings = sizeof kSettings / sizeof kSettings[0];
static void set_option(Options& O, const Setting& s) {          // as pt_set_option stores it (pt_api.hip: kOptions)
    const std::string n = s.name;
    if (n == "onchip") O.onchipOk = s.value;
    else if (n == "waves_hbm") { O.wavesHbmOk = s.value != 0; O.wavesHbmForce = s.value == 2; }
    else if (n == "refill") O.refill = s.value;
    else if (n == "culling") O.cull = s.value;
    else if (n == "flat") O.flatWanted = s.value;
    else if (n == "flat2") O.flat2Wanted = s.value;
    else if (n == "simple") O.simpleWanted = s.value;
    else if (n == "lean") O.leanWanted = s.value;
    else if (n == "leaf_boxes") O.leafBoxes = s.value;
    else if (n == "refill_keep") { O.refillKeep = s.value; O.refillKeepSet = true; }
    else if (n == "persistent") O.persistent = s.value;
    else abort();
}
static const int kLive[] = {1, 6143, 6144, 7679, 7680, 32400}, kFrameTiles = 32400, kNumCU = 256;

struct Outcome { std::string plan = "-", row = "-", scene = "-", grid = "-"; };

// ---- what render_tiles does between its argument checks and its launch ----
static Outcome evaluate(const Facts& F, const Options& O, int integrator, bool count, int useMIS, int live, bool listed) {
    Outcome o;
    char b[512];
    const TileSpan t = {0, 1, listed ? kFrameTiles : live, 240};
    if (listed && count) return o;                  // "render_tiles: bad tile list"
    const LaunchAsk ask = {integrator, count, useMIS, live};
    const LaunchPlan plan = plan_launch(F, O, kNumCU, ask);
    snprintf(b, sizeof b, "wg %d hbm %d cull %d refill %d flat %d simple %d lean %d simpleTimed %d timedHbm %d", plan.onchipWg, plan.hbm, plan.cull, plan.refill,
             plan.flat, plan.simple, plan.lean, plan.simpleTimed, plan.timedHbm);
    o.plan = b;
    KParams P = plan_selectors(plan);
    const MkRow* row = megakernel_choose(integrator, count, true, P, false);
    o.row = row ? row->name : "none";
    if (!row) return o;
    const LaunchSizes z = size_launch(F, O, kNumCU, ask, t, listed, plan, *row, P);
    g_attr = g_launches = 0; g_lds = 0;
    // (no queue and no list: their pointers are render_tiles' to set, and the launch's LDS does not depend on them)
    if (launch_megakernel(*row, P, live, nullptr, nullptr, nullptr) != hipSuccess || g_launches != 1) abort();
    snprintf(b, sizeof b, "wgWaves %d wavesPerSimd %d cacheNodes %d cacheTris %d cacheAttrs %d cacheMats %d cacheLights %d nLeaves %d gnodeFrom %d stackSpill %d refillKeep %d spillEntries %d lds %u attr %d",
             P.wgWaves, P.wavesPerSimd, P.cacheNodes, P.cacheTris, P.cacheAttrs, P.cacheMats, P.cacheLights, P.nLeaves, P.gnodeFrom, P.S.stackSpill, P.refillKeep,
             z.spillEntries, g_lds, g_attr);
    o.scene = b;
    snprintf(b, sizeof b, "blocks %d queueCap %d queueMask %d gridBlocks %d tileCount %d useMIS %d", z.blocks, z.queueCap, P.queueMask, P.gridBlocks, P.tileCount, P.useMIS);
    o.grid = b;
    return o;
}

static int id_of(std::map<std::string, int>& ids, const std::string& text, char tag) {
    auto it = ids.find(text);
    if (it != ids.end()) return it->second;
    const int id = (int)ids.size();
    printf("%c %d %s\n", tag, id, text.c_str());
    return ids[text] = id;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    // the defaults, every setting alone, every pair of settings of two different options
    std::vector<std::vector<int>> optionSets = {{}};
    for (int a = 0; a < kNumSettings; a++) optionSets.push_back({a});
    for (int a = 0; a < kNumSettings; a++)
        for (int c = a + 1; c < kNumSettings; c++)
            if (strcmp(kSettings[a].name, kSettings[c].name)) optionSets.push_back({a, c});
    // the axes that are tables here, as JSON, for the test to hold against the record's
    printf("A {\"shape\":[");
    for (const Shape& sh : kShapes) printf("%s[%d,%d,%d,%d,%d,%d]", &sh == kShapes ? "" : ",", sh.nInternal, sh.nTris, sh.nMats, sh.nLights, sh.stackNeed, sh.nLeaves);
    printf("],\"options\":[");
    for (size_t i = 0; i < optionSets.size(); i++) {
        printf("%s[", i ? "," : "");
        for (size_t k = 0; k < optionSets[i].size(); k++) printf("%s[\"%s\",%d]", k ? "," : "", kSettings[optionSets[i][k]].name, kSettings[optionSets[i][k]].value);
        printf("]");
    }
    printf("],\"live\":[");
    for (int live : kLive) printf("%s%d", live == kLive[0] ? "" : ",", live);
    printf("]}\n");
    std::map<std::string, int> ids[4];
    std::vector<int32_t> index;
    for (const Shape& sh : kShapes) for (int flags = 0; flags < 32; flags++) for (const std::vector<int>& set : optionSets) {
        const Facts F = facts_of(sh, flags);
        Options O;
        for (int k : set) set_option(O, kSettings[k]);
        for (int live : kLive) for (int listed = 0; listed < 2; listed++) for (int integ : {0, 2}) for (int count = 0; count < 2; count++) for (int mis = 0; mis < 2; mis++) {
            const Outcome o = evaluate(F, O, integ, count != 0, mis, live, listed != 0);
            index.push_back(id_of(ids[0], o.plan, 'P')); index.push_back(id_of(ids[1], o.row, 'R'));
            index.push_back(id_of(ids[2], o.scene, 'S')); index.push_back(id_of(ids[3], o.grid, 'G'));
        }
    }
    FILE* f = fopen(argv[1], "wb");
    if (!f || fwrite(index.data(), sizeof(int32_t), index.size(), f) != index.size() || fclose(f)) return 1;
    return 0;
}
