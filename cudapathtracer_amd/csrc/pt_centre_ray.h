// pt_centre_ray.h — the centre ray of a pixel, shared by the centre feature passes (pt_aov.hip) and the motion pass (pt_motion.hip).
#pragma once
#include "pt_device.h"

namespace pt {

// The centre ray of pixel (x, y): camera_ray with antiAliasJitterDist = 0 and aperture = 0, operation for operation. With those two
// zeros camera_ray's draws reach nothing: (u01 - 0.5) * 0 is +-0 and (float)x + +-0 is (float)x; the lens sample is skipped and lens
// stays (0, 0, 0). So no Rng is needed, and the ray has no seed. `origin + 0` is kept: it turns a -0 component of the origin into +0,
// as camera_ray does.
PT_DEV void camera_ray_centre(const CamK& cam, int x, int y, V3& o, V3& d) {
    const float aspect = (float)cam.w / (float)cam.h;
    const float u = (2.0f * ((float)x / (float)cam.w) - 1.0f) * aspect * cam.fovScale;
    const float v = (2.0f * ((float)y / (float)cam.h) - 1.0f) * cam.fovScale;
    const V3 focal = cam.origin + (cam.right * (u * cam.focalDist)) + (cam.up * (v * cam.focalDist)) + (cam.forward * cam.focalDist);
    o = cam.origin + v3(0.0f);
    d = normalize(focal - o);
}

}  // namespace pt
