// pt_postfx_host.h — what the host side of the post-process files (pt_temporal, pt_denoise, pt_upsample, pt_converge, pt_preview)
// writes once: the error helpers, the alias test, the size check and the staging of a host form. Host code only.
#pragma once
#include <cstdarg>
#include <cstdio>

#include <hip/hip_runtime.h>

extern "C" int pt_fail_(int code, const char* msg);

namespace pt {

static inline int postfx_vfail(int code, const char* fn, const char* fmt, va_list ap) {
    char buf[256];
    const int n = fn ? snprintf(buf, sizeof(buf), "%s: ", fn) : 0;
    vsnprintf(buf + n, sizeof(buf) - n, fmt, ap);
    return pt_fail_(code, buf);
}
// pt_fail_ with a printf-style message; postfx_fail_fn puts "<fn>: " in front of it.
__attribute__((format(printf, 2, 3))) static inline int postfx_fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    const int r = postfx_vfail(code, nullptr, fmt, ap);
    va_end(ap);
    return r;
}
__attribute__((format(printf, 3, 4))) static inline int postfx_fail_fn(int code, const char* fn, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    const int r = postfx_vfail(code, fn, fmt, ap);
    va_end(ap);
    return r;
}
#define POSTFX_HIP_OK(expr)                                                                                        \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess) return pt::postfx_fail(-2, "%s failed: %s", #expr, hipGetErrorString(e_));           \
    } while (0)

static inline bool overlaps(const void* a, size_t aBytes, const void* b, size_t bBytes) {
    const char* pa = (const char*)a; const char* pb = (const char*)b;
    return pa < pb + bBytes && pb < pa + aBytes;
}

static inline int postfx_check_size(const char* fn, int w, int h) {
    if (w <= 0 || h <= 0) return postfx_fail_fn(-1, fn, "image size %d x %d must be positive", w, h);
    if ((long long)w * h > 0x7fffffffll) return postfx_fail_fn(-1, fn, "image of %d x %d pixels is too large", w, h);
    return 0;
}

// A host form's buffers. An input with a NULL host pointer, or an output with one, has no slice: its device pointer is NULL.
struct HostIn { const void* host; size_t bytes; };
struct HostOut { void* host; size_t bytes; int in = -1; };        // in >= 0: the output is read back from that input's slice

// One host form: one allocation of [workspace | inputs | outputs], every slice at a multiple of 16 bytes; the uploads in order;
// launch(ws, dIn, dOut), which runs on the null stream and returns 0 or what it failed with; the downloads in order; the free.
template <size_t NI, size_t NO, class Launch>
static int postfx_host_form(const char* fn, size_t wsBytes, const HostIn (&in)[NI], const HostOut (&out)[NO], Launch launch) {
    const auto pad = [](size_t b) { return (b + 15) & ~(size_t)15; };
    size_t offIn[NI], offOut[NO], total = pad(wsBytes);
    for (size_t i = 0; i < NI; i++) { offIn[i] = total; total += in[i].host ? pad(in[i].bytes) : 0; }
    for (size_t i = 0; i < NO; i++) { offOut[i] = out[i].in >= 0 ? offIn[out[i].in] : total; total += out[i].host && out[i].in < 0 ? pad(out[i].bytes) : 0; }
    char* d = nullptr;
    POSTFX_HIP_OK(hipMalloc(&d, total));
    char *dIn[NI], *dOut[NO];
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < NI; i++) {
        dIn[i] = in[i].host ? d + offIn[i] : nullptr;
        if (e == hipSuccess && in[i].host) e = hipMemcpy(dIn[i], in[i].host, in[i].bytes, hipMemcpyHostToDevice);
    }
    for (size_t i = 0; i < NO; i++) dOut[i] = out[i].host ? d + offOut[i] : nullptr;
    int r = 0;
    if (e != hipSuccess) {
        r = postfx_fail_fn(-2, fn, "upload failed");
    } else if ((r = launch(d, dIn, dOut)) == 0) {
        for (size_t i = 0; i < NO && e == hipSuccess; i++)
            if (out[i].host) e = hipMemcpy(out[i].host, dOut[i], out[i].bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) r = postfx_fail_fn(-2, fn, "download failed");
    }
    (void)hipFree(d);
    return r;
}

}  // namespace pt
