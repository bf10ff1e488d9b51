// pt_denoise_shared.h — the per-pixel arithmetic that pt_denoise.hip's prepare kernels and pt_temporal.hip share: one statement of
// pt_denoise_var's m, a, e, V and pass-through rule (include/pt_api.h), and of the guide's normalisation.
#pragma once
#include <hip/hip_runtime.h>

namespace pt {

__device__ inline bool finite3(float4 v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z); }
__device__ inline float demod_albedo(float a) { return a >= 0.01f ? a : 1.0f; }

// pt_denoise_var's working pixel from S, Q and the albedo: rgb = e = m / a, w = V (the variance of that mean) or -1 for a
// pass-through pixel. m = S / spp comes back as well (a pass-through pixel keeps it).
__device__ inline float4 dn_var_pixel(float4 s, float4 q, float4 a, float spp, float batches, float4& m) {
    m = make_float4(s.x / spp, s.y / spp, s.z / spp, s.w / spp);
    const float ax = demod_albedo(a.x), ay = demod_albedo(a.y), az = demod_albedo(a.z);
    // var_c = max(0, Q_c - S_c^2 / B) / (B - 1) * B / spp^2, left to right; max(0, x) keeps a NaN
    const float spp2 = spp * spp;
    float vx = q.x - s.x * s.x / batches, vy = q.y - s.y * s.y / batches, vz = q.z - s.z * s.z / batches;
    vx = (vx < 0.0f ? 0.0f : vx) / (batches - 1.0f) * batches / spp2;
    vy = (vy < 0.0f ? 0.0f : vy) / (batches - 1.0f) * batches / spp2;
    vz = (vz < 0.0f ? 0.0f : vz) / (batches - 1.0f) * batches / spp2;
    const float V = vx / (ax * ax) + vy / (ay * ay) + vz / (az * az);
    const bool filtered = a.w > 0.0f && finite3(m) && __builtin_isfinite(V);
    return make_float4(m.x / ax, m.y / ay, m.z / az, filtered ? V : -1.0f);
}

// The guide of the filters: the unit mean normal (0 where the mean normal is 0) and the depth.
__device__ inline float4 dn_unit_guide(float4 g) {
    const float len = sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
    return len > 0.0f ? make_float4(g.x / len, g.y / len, g.z / len, g.w) : make_float4(0.0f, 0.0f, 0.0f, g.w);
}

}  // namespace pt
