// pt_mk_hbm.hip — megakernel instantiations for scenes in HBM: megakernel_hbm (6 waves per SIMD, 12-wave workgroups
// sharing a 44 KB copy of the top of the tree; loop exits, REFILL, opt-in culling) and the general 4-wave kernel
// (launches with too few tiles to fill its waves).
// Built without the SLP vectorizer since round 3 (Makefile: at 64 VGPRs its packed pairs cost spills, -3.4 / -3.8 %), and with the
// per-lane range test in rcp_exact: the wave-uniform form that pays for the issue-bound LDS-resident kernels measures 0.7-1.0 %
// slower here (profiles/r03_ab_rcp_uniform_hbm.log).
#ifndef PT_RCP_UNIFORM
#define PT_RCP_UNIFORM 0
#endif
#include "pt_megakernel.h"

namespace pt {

// The kernels this file builds, and the launch each serves (pt_params.h: MkRow; pt_kernels.hip: megakernel_choose). A row is what
// instantiates its kernel. PT_MK_ROW2: the row for integrator 0 and the one for integrator 2.
const MkRow kMkRowsHbm[] = {
    // megakernel_hbm: counting and timed, the plain loops, REFILL, culling; timed REFILL launches with the LEAN and the SIMPLE bounce
    PT_MK_ROW2(kMkHbm | kMkCount, megakernel_hbm, true, false, false, false, false),
    PT_MK_ROW2(kMkHbm, megakernel_hbm, false, false, false, false, false),
    PT_MK_ROW2(kMkHbm | kMkCount | kMkRefill, megakernel_hbm, true, false, true, false, false),
    PT_MK_ROW2(kMkHbm | kMkRefill, megakernel_hbm, false, false, true, false, false),
    PT_MK_ROW2(kMkHbm | kMkCount | kMkCull, megakernel_hbm, true, true, false, false, false),
    PT_MK_ROW2(kMkHbm | kMkCull, megakernel_hbm, false, true, false, false, false),
    PT_MK_ROW2(kMkHbm | kMkRefill | kMkLean, megakernel_hbm, false, false, true, false, true),
    PT_MK_ROW2(kMkHbm | kMkRefill | kMkSimple, megakernel_hbm_simple),
    // the general 4-wave kernel, the same forms but culling
    PT_MK_ROW2(kMkCount, megakernel, true, false, false, false, false, false, 1, false),
    PT_MK_ROW2(0u, megakernel, false, false, false, false, false, false, 1, false),
    PT_MK_ROW2(kMkCount | kMkRefill, megakernel, true, false, false, true, false, false, 1, false),
    PT_MK_ROW2(kMkRefill, megakernel, false, false, false, true, false, false, 1, false),
    PT_MK_ROW2(kMkRefill | kMkLean, megakernel, false, false, false, true, false, false, 1, true),
    PT_MK_ROW2(kMkRefill | kMkSimple, megakernel, false, false, false, true, false, true, 1, false),
    // The fused moments twins: the REFILL forms with their 4-wave forms. Not built: culling and the plain loops ("refill" 0).
    PT_MK_ROW2(kMkMoments | kMkHbm | kMkRefill, megakernel_hbm_moments, false),
    PT_MK_ROW2(kMkMoments | kMkHbm | kMkRefill | kMkLean, megakernel_hbm_moments, true),
    PT_MK_ROW2(kMkMoments | kMkHbm | kMkRefill | kMkSimple, megakernel_hbm_simple_moments),
    PT_MK_ROW2(kMkMoments | kMkRefill, megakernel_moments, false, true, false, false, 1, false),
    PT_MK_ROW2(kMkMoments | kMkRefill | kMkLean, megakernel_moments, false, true, false, false, 1, true),
    PT_MK_ROW2(kMkMoments | kMkRefill | kMkSimple, megakernel_moments, false, true, false, true, 1, false),
};
const int kMkRowsHbmCount = sizeof(kMkRowsHbm) / sizeof(kMkRowsHbm[0]);

}  // namespace pt
