// pt_probe.hip — the probe entry points of include/pt_api.h: single device functions run on the caller's inputs, for the tests.
#include "pt_host.h"
#include "pt_feature_host.h"
#include "xorwow_host.h"

using namespace pt;

// ---- probes -------------------------------------------------------------------------------------
struct Scratch {      // RAII device scratch for the probe entry points
    std::vector<void*> ptrs;
    ~Scratch() { for (void* p : ptrs) (void)hipFree(p); }
    void* get(size_t bytes, const void* init = nullptr) {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        if (init && bytes) { if (hipMemcpy(p, init, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr; }
        return p;
    }
};
#define SCRATCH(var, type, bytes, init)                              \
    type* var = (type*)sc.get(bytes, init);                          \
    if (!var) return fail(-2, "probe: device scratch allocation failed")

static int jump_device(Scratch& sc, const uint32_t*& dj) {
    const std::vector<uint32_t>& jt = xorwow_host::jump_table();
    dj = (const uint32_t*)sc.get(jt.size() * 4, jt.data());
    return dj ? 0 : fail(-2, "probe: device scratch allocation failed");
}

int pt_probe_rng(uint64_t seed, int n, const uint32_t* subseq, int nDraws, uint32_t* outState6, uint32_t* outU32, float* outUni) {
    if (n <= 0 || nDraws < 0) return fail(-1, "bad sizes");
    Scratch sc;
    const uint32_t* dj; if (int r = jump_device(sc, dj)) return r;
    SCRATCH(dsub, uint32_t, (size_t)n * 4, subseq);
    SCRATCH(dst, uint32_t, (size_t)n * 24, nullptr);
    SCRATCH(du, uint32_t, (size_t)n * nDraws * 4, nullptr);
    SCRATCH(df, float, (size_t)n * nDraws * 4, nullptr);
    HIP_OK(launch_probe_rng(dj, seed, n, dsub, nDraws, dst, du, df, nullptr));
    HIP_OK(hipDeviceSynchronize());
    if (outState6) HIP_OK(hipMemcpy(outState6, dst, (size_t)n * 24, hipMemcpyDeviceToHost));
    if (outU32 && nDraws) HIP_OK(hipMemcpy(outU32, du, (size_t)n * nDraws * 4, hipMemcpyDeviceToHost));
    if (outUni && nDraws) HIP_OK(hipMemcpy(outUni, df, (size_t)n * nDraws * 4, hipMemcpyDeviceToHost));
    return 0;
}

// The moments pass of pt_render_adaptive_moments alone, as a round runs it: `live` tiles (the first of the frame, ascending) of a
// w x h frame's tile-major S, P and Q, one warm-up launch and then `reps` launches between two HIP events. *out_ms: their mean.
int pt_probe_adaptive_moments(int w, int h, int live, int reps, float* out_ms) {
    if (w <= 0 || h <= 0) return fail(-1, "pt_probe_adaptive_moments: image size %d x %d must be positive", w, h);
    const long long T = (long long)((w + 7) / 8) * ((h + 7) / 8);
    if (T * 64 > 0x7fffffffll) return fail(-1, "pt_probe_adaptive_moments: image of %d x %d pixels is too large", w, h);
    if (live < 1 || live > T) return fail(-1, "pt_probe_adaptive_moments: live %d must lie in 1..%lld, the frame's tiles", live, T);
    if (reps < 1) return fail(-1, "pt_probe_adaptive_moments: reps %d must be positive", reps);
    if (!out_ms) return fail(-1, "pt_probe_adaptive_moments: null output");
    Scratch sc;
    const size_t tileBytes = (size_t)T * 64 * sizeof(float4);
    SCRATCH(S, float4, tileBytes, nullptr);
    SCRATCH(P, float4, tileBytes, nullptr);
    SCRATCH(Q, float4, tileBytes, nullptr);
    SCRATCH(list, int, (size_t)live * sizeof(int), nullptr);
    HIP_OK(hipMemset(S, 0, tileBytes));
    HIP_OK(launch_adaptive_iota(live, list, nullptr));
    HIP_OK(launch_adaptive_moments(list, live, S, P, Q, true, 1, nullptr));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_OK(hipEventCreate(&e0));
    hipError_t e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
    for (int k = 0; k < reps && e == hipSuccess; k++) e = launch_adaptive_moments(list, live, S, P, Q, false, k + 2, nullptr);
    if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(-2, "pt_probe_adaptive_moments: %s", hipGetErrorString(e));
    *out_ms = ms / (float)reps;
    return 0;
}

int pt_probe_math(int n, const float* x, float* oSin, float* oCos, float* oExp, float* oRsqrt, float* oPow5) {
    if (n <= 0) return fail(-1, "bad sizes");
    Scratch sc;
    SCRATCH(dx, float, (size_t)n * 4, x);
    float* d[5]; float* outs[5] = {oSin, oCos, oExp, oRsqrt, oPow5};
    for (int k = 0; k < 5; k++) { d[k] = (float*)sc.get((size_t)n * 4); if (!d[k]) return fail(-2, "probe: device scratch allocation failed"); }
    HIP_OK(launch_probe_math(n, dx, d[0], d[1], d[2], d[3], d[4], nullptr));
    HIP_OK(hipDeviceSynchronize());
    for (int k = 0; k < 5; k++) if (outs[k]) HIP_OK(hipMemcpy(outs[k], d[k], (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int pt_probe_rcp_exhaustive(unsigned long long* out3, uint32_t* first_bad) {
    if (!out3) return fail(-1, "bad arguments");
    Scratch sc;
    SCRATCH(dout, unsigned long long, 32, nullptr);
    SCRATCH(dfb, uint32_t, 16, nullptr);
    HIP_OK(hipMemset(dout, 0, 32));
    HIP_OK(hipMemset(dfb, 0xff, 16));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(launch_probe_rcp_exhaustive(dout, dfb, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out3, dout, 24, hipMemcpyDeviceToHost));
    if (first_bad) HIP_OK(hipMemcpy(first_bad, dfb, 4, hipMemcpyDeviceToHost));
    return 0;
}

int pt_probe_camera_rays(const pt_camera* cam, uint64_t seed, int n, const int32_t* xy, float* outRays6) {
    if (!cam || n <= 0) return fail(-1, "bad arguments");
    Scratch sc;
    const uint32_t* dj; if (int r = jump_device(sc, dj)) return r;
    std::vector<uint32_t> sub(n);
    for (int i = 0; i < n; i++) sub[i] = (uint32_t)(xy[2 * i + 1] * cam->w + xy[2 * i]);
    SCRATCH(dsub, uint32_t, (size_t)n * 4, sub.data());
    SCRATCH(dst, uint32_t, (size_t)n * 24, nullptr);
    SCRATCH(du, uint32_t, 16, nullptr);
    SCRATCH(df, float, 16, nullptr);
    SCRATCH(dxy, int, (size_t)n * 8, xy);
    SCRATCH(dout, float, (size_t)n * 24, nullptr);
    HIP_OK(launch_probe_rng(dj, seed, n, dsub, 0, dst, du, df, nullptr));
    HIP_OK(launch_probe_camera(dst, cam_to_kernel(*cam), n, dxy, dout, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(outRays6, dout, (size_t)n * 24, hipMemcpyDeviceToHost));
    return 0;
}

int pt_probe_centre_rays(const pt_camera* cam, int n, const int32_t* xy, float* outRays6) {
    if (!cam || n <= 0 || !xy || !outRays6) return fail(-1, "pt_probe_centre_rays: bad arguments");
    Scratch sc;
    SCRATCH(dxy, int, (size_t)n * 8, xy);
    SCRATCH(dout, float, (size_t)n * 24, nullptr);
    HIP_OK(launch_probe_centre(cam_to_kernel(*cam), n, dxy, dout, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(outRays6, dout, (size_t)n * 24, hipMemcpyDeviceToHost));
    return 0;
}

static int probe_spill(pt_scene* s, int n, int32_t*& spill) {
    spill = nullptr;
    if (s->facts.ds.stackSpill > 0) {
        if (int r = s->work.spill.ensure((size_t)probe_trace_blocks(n) * s->facts.ds.stackSpill * 64 * sizeof(int32_t))) return r;
        spill = (int32_t*)s->work.spill.p;
    }
    return 0;
}

int pt_probe_trace_closest(pt_scene* s, int n, const float* rays6, int32_t* outI, float* outF, pt_counters* counters) {
    if (!s || n <= 0) return fail(-1, "bad arguments");
    Scratch sc;
    SCRATCH(dr, float, (size_t)n * 24, rays6);
    SCRATCH(di, int32_t, (size_t)n * 16, nullptr);
    SCRATCH(df, float, (size_t)n * 48, nullptr);
    SCRATCH(dt, unsigned long long, 64, nullptr);
    HIP_OK(hipMemset(dt, 0, 64));
    int32_t* spill; if (int r = probe_spill(s, n, spill)) return r;
    HIP_OK(launch_probe_closest(s->facts.ds, n, dr, di, df, dt, spill, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(outI, di, (size_t)n * 16, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(outF, df, (size_t)n * 48, hipMemcpyDeviceToHost));
    if (counters) HIP_OK(hipMemcpy(counters, dt, 64, hipMemcpyDeviceToHost));
    return 0;
}

int pt_probe_trace_shadow(pt_scene* s, int n, const float* rays6, const float* maxT, float* outThr3, pt_counters* counters) {
    if (!s || n <= 0) return fail(-1, "bad arguments");
    Scratch sc;
    SCRATCH(dr, float, (size_t)n * 24, rays6);
    SCRATCH(dm, float, (size_t)n * 4, maxT);
    SCRATCH(df, float, (size_t)n * 12, nullptr);
    SCRATCH(dt, unsigned long long, 64, nullptr);
    HIP_OK(hipMemset(dt, 0, 64));
    int32_t* spill; if (int r = probe_spill(s, n, spill)) return r;
    HIP_OK(launch_probe_shadow(s->facts.ds, n, dr, dm, df, dt, spill, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(outThr3, df, (size_t)n * 12, hipMemcpyDeviceToHost));
    if (counters) HIP_OK(hipMemcpy(counters, dt, 64, hipMemcpyDeviceToHost));
    return 0;
}

int pt_probe_bsdf_sample(pt_scene* s, int n, const int32_t* material, const float* wi3, const int32_t* backface, float etaI, float etaT,
                         uint64_t seed, const uint32_t* subseq, float* out8) {
    (void)etaT;      // the reference's sample_f_eval never reads etaT (reflectors.cuh:588-629)
    if (!s || n <= 0) return fail(-1, "bad arguments");
    Scratch sc;
    const uint32_t* dj; if (int r = jump_device(sc, dj)) return r;
    SCRATCH(dsub, uint32_t, (size_t)n * 4, subseq);
    SCRATCH(dst, uint32_t, (size_t)n * 24, nullptr);
    SCRATCH(du, uint32_t, 16, nullptr);
    SCRATCH(dfu, float, 16, nullptr);
    SCRATCH(dm, int, (size_t)n * 4, material);
    SCRATCH(dw, float, (size_t)n * 12, wi3);
    SCRATCH(db, int, (size_t)n * 4, backface);
    SCRATCH(dout, float, (size_t)n * 32, nullptr);
    HIP_OK(launch_probe_rng(dj, seed, n, dsub, 0, dst, du, dfu, nullptr));
    HIP_OK(launch_probe_bsdf_sample(s->facts.ds, n, dm, dw, db, etaI, dst, dout, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out8, dout, (size_t)n * 32, hipMemcpyDeviceToHost));
    return 0;
}

int pt_probe_bsdf_eval(pt_scene* s, int n, const int32_t* material, const float* wi3, const float* wo3, float etaI, float etaT, float* out4) {
    (void)etaT;
    if (!s || n <= 0) return fail(-1, "bad arguments");
    Scratch sc;
    SCRATCH(dm, int, (size_t)n * 4, material);
    SCRATCH(dwi, float, (size_t)n * 12, wi3);
    SCRATCH(dwo, float, (size_t)n * 12, wo3);
    SCRATCH(dout, float, (size_t)n * 16, nullptr);
    HIP_OK(launch_probe_bsdf_eval(s->facts.ds, n, dm, dwi, dwo, etaI, dout, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out4, dout, (size_t)n * 16, hipMemcpyDeviceToHost));
    return 0;
}
