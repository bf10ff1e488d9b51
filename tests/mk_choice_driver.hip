// Host-only driver of tests/test_mk_choice.py: walks megakernel_choose and launch_megakernel (pt_kernels.hip) over the cross product
// of everything a launch is chosen by, against the tables of pt_mk_lds.hip and pt_mk_hbm.hip, and prints what would be launched. Built
// with --cuda-host-only: no device code, no GPU. The HIP entry points the launch path reaches are defined HERE (the executable's
// definitions win over the runtime library's), so a "launch" records the kernel's address, its dynamic LDS and whether the LDS
// attribute was raised for it, and the registration calls of the translation units end in stubs.
//
// One line per input, the inputs in the order of the loops below:
//   <outcome at parameter set 0> | <outcome at set 1> | <megakernel_has_moments_twin> | <the row megakernel_choose returned>
// outcome: `<kernel, demangled from the launched address> ; <lds bytes> ; <attribute calls>` or `refused`;
// row: `<its name> ; <stack entries> ; <medium stacks> ; <attribute cache> ; <waves per workgroup> ; <waves per SIMD>` or `none`.
#include <hip/hip_runtime.h>
#include <cxxabi.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "pt_params.h"

static const void* g_fn;
static unsigned g_lds;
static int g_attr, g_launches;
extern "C" hipError_t hipLaunchKernel(const void* f, dim3, dim3, void**, size_t lds, hipStream_t) { g_fn = f; g_lds = (unsigned)lds; g_launches++; return hipSuccess; }
extern "C" hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { g_attr++; return hipSuccess; }
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }
extern "C" void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
extern "C" void __hipUnregisterFatBinary(void**) {}
extern "C" void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
extern "C" void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}

// "void pt::megakernel<0, true>(pt::KParams)" -> "megakernel<0, true>"
static std::string kernel_name(const void* f) {
    Dl_info di;
    if (!dladdr(f, &di) || !di.dli_sname) return "?";
    int st = 0;
    char* d = abi::__cxa_demangle(di.dli_sname, nullptr, nullptr, &st);
    std::string s = d ? d : di.dli_sname;
    free(d);
    const size_t a = s.find("pt::"), b = s.rfind("(pt::KParams");
    return (a == std::string::npos || b == std::string::npos) ? s : s.substr(a + 4, b - a - 4);
}

int main() {
    using namespace pt;
    // cacheNodes, cacheTris, wgWaves, cacheAttrs, cacheMats, cacheLights: every family stays below 64 KB at set 0 and crosses it at set 1
    const int sets[2][6] = {{63, 64, 4, 64, 10, 2}, {700, 100, 12, 100, 20, 4}};
    for (int integ : {0, 2}) for (int count = 0; count < 2; count++) for (int sync = 1; sync >= 0; sync--) for (int hbm = 0; hbm < 2; hbm++) for (int onchip = 0; onchip < 2; onchip++)
    for (int flat = 0; flat < 4; flat++) for (int simple = 0; simple < 2; simple++) for (int lean = 0; lean < 2; lean++) for (int refill = 0; refill < 2; refill++) for (int cull = 0; cull < 2; cull++)
    for (int mo = 0; mo < 2; mo++) {
        KParams P;
        memset(&P, 0, sizeof P);
        P.hbm = hbm; P.onchip = onchip; P.flat = flat; P.simple = simple; P.lean = lean; P.refill = refill; P.cull = cull;
        P.tileCount = 1;
        const MomentsK M = {nullptr, nullptr, 2, 0.5f};
        const MkRow* row = megakernel_choose(integ, count != 0, sync != 0, P, mo != 0);
        for (int k = 0; k < 2; k++) {
            P.cacheNodes = sets[k][0]; P.cacheTris = sets[k][1]; P.wgWaves = sets[k][2]; P.cacheAttrs = sets[k][3]; P.cacheMats = sets[k][4]; P.cacheLights = sets[k][5];
            g_fn = nullptr; g_attr = 0; g_launches = 0;
            const hipError_t e = row ? launch_megakernel(*row, P, 1, nullptr, nullptr, mo ? &M : nullptr) : hipErrorInvalidValue;
            if (e != hipSuccess || g_launches != 1) printf("refused | ");
            else printf("%s ; %u ; %d | ", kernel_name(g_fn).c_str(), g_lds, g_attr);
        }
        printf("%d | ", megakernel_has_moments_twin(integ, count != 0, sync != 0, P) ? 1 : 0);
        if (row) printf("%s ; %d ; %d ; %d ; %d ; %d\n", row->name, row->f.stackEntries, row->f.mediumStacks ? 1 : 0, row->f.attrCache ? 1 : 0, row->f.wgWaves, row->f.wavesPerSimd);
        else printf("none\n");
    }
    return 0;
}
