// pt_mk_lds.hip — megakernel instantiations for scenes that live in LDS (ONCHIP: every PNode / PTri / PAttr / PMat /
// PLight of the scene staged per workgroup; Cornell-class, BASELINE C1 / C2). These kernels are VALU-bound; this file is
// built with -fno-slp-vectorize (Makefile): the SLP vectorizer's v_pk_mul_f32 / v_pk_add_f32 pairs do not issue at twice
// the scalar rate on gfx950 and cost register-pair moves (+2.3 % on C2 without them, profiles/r02_ab_noslp.log).
#include "pt_megakernel.h"

namespace pt {

// The kernels this file builds, and the launch each serves (pt_params.h: MkRow; pt_kernels.hip: megakernel_choose). A row is what
// instantiates its kernel. PT_MK_ROW2: the row for integrator 0 and the one for integrator 2.
const MkRow kMkRowsLds[] = {
    PT_MK_ROW2(kMkLds | kMkCount, megakernel, true, false, true, false, false, false, 1, false),
    PT_MK_ROW2(kMkLds, megakernel, false, false, true, false, false, false, 1, false),
    PT_MK_ROW2(kMkLds | kMkFlat * 1, megakernel, false, false, true, false, true, false, 1, false),
    PT_MK_ROW2(kMkLds | kMkFlat * 1 | kMkSimple, megakernel, false, false, true, false, true, true, 1, false),
    PT_MK_ROW2(kMkLds | kMkFlat * 2, megakernel, false, false, true, false, true, false, 2, false),
    PT_MK_ROW2(kMkLds | kMkFlat * 2 | kMkSimple, megakernel, false, false, true, false, true, true, 2, false),
    // both rays of a lane in one FLAT pass (SIMPLE scenes, MIS)
    PT_MK_ROW(kMkLds | kMkFlat * 3 | kMkSimple, megakernel_flat2, 0, true, false),
    PT_MK_ROW(kMkLds | kMkFlat * 3 | kMkLean, megakernel_flat2, 0, false, true),
    PT_MK_ROW(kMkLds | kMkFlat * 3, megakernel_flat2, 0, false, false),
    // the fused moments twins of the timed kernels above
    PT_MK_ROW2(kMkMoments | kMkLds, megakernel_moments, true, false, false, false, 1, false),
    PT_MK_ROW2(kMkMoments | kMkLds | kMkFlat * 1, megakernel_moments, true, false, true, false, 1, false),
    PT_MK_ROW2(kMkMoments | kMkLds | kMkFlat * 1 | kMkSimple, megakernel_moments, true, false, true, true, 1, false),
    PT_MK_ROW2(kMkMoments | kMkLds | kMkFlat * 2, megakernel_moments, true, false, true, false, 2, false),
    PT_MK_ROW2(kMkMoments | kMkLds | kMkFlat * 2 | kMkSimple, megakernel_moments, true, false, true, true, 2, false),
    // The SIMPLE pair kernel's twin is built and bit-exact but out of the dispatch: on the 1080p Cornell frame at 4 spp in 2 batches it
    // measured 13.01 ms a preview frame against 12.71 ms in two launches.
    PT_MK_ROW(kMkMoments | kMkLds | kMkFlat * 3 | kMkSimple | kMkBuiltOnly, megakernel_flat2_moments, 0, true, false),
    PT_MK_ROW(kMkMoments | kMkLds | kMkFlat * 3 | kMkLean, megakernel_flat2_moments, 0, false, true),
    PT_MK_ROW(kMkMoments | kMkLds | kMkFlat * 3, megakernel_flat2_moments, 0, false, false),
};
const int kMkRowsLdsCount = sizeof(kMkRowsLds) / sizeof(kMkRowsLds[0]);

}  // namespace pt
