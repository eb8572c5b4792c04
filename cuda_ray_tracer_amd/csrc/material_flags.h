// The three facts of a material that the call plan reads (render_plan.h, SceneFacts: any_trans, any_rough, colors_finite), as
// bits.  ONE copy of the rule: mirt_scene_create and the light / plane setters call it on the host, the material kernels
// (update_shading.hip) on the device, and tests/material_flags_probe.cpp with a plain host compiler -- no HIP needed here.
#ifndef MIRT_MATERIAL_FLAGS_H
#define MIRT_MATERIAL_FLAGS_H

#include <math.h>

#if defined(__HIPCC__)
#define MIRT_HOST_DEVICE __host__ __device__
#else
#define MIRT_HOST_DEVICE
#endif

namespace mirt {

constexpr unsigned MAT_TRANS = 1u;       // transparency is not zero: the scene needs a pending-children list
constexpr unsigned MAT_ROUGH = 2u;       // roughness > 0: shading draws random numbers
constexpr unsigned MAT_NONFINITE = 4u;   // a colour channel is inf or NaN: colour * 0 terms may not be dropped

// |x| <= FLT_MAX: false for an infinity and for a NaN (std::isfinite's answer, without a host-only call)
MIRT_HOST_DEVICE inline bool finite_f32(float x) { return fabsf(x) <= 3.402823466e+38f; }
MIRT_HOST_DEVICE inline bool finite_rgb(float r, float g, float b) { return finite_f32(r) && finite_f32(g) && finite_f32(b); }

// m: colour rgb, shininess rgb, trans rgb, ior, roughness (MirtMaterials' field order).
//   trans: "not all three below 1e-6 in magnitude" -- a NaN channel counts as transparent, -0.0f does not
//   roughness: > 0.0f -- a NaN or a negative one does not count
MIRT_HOST_DEVICE inline unsigned material_flags(const float m[11])
{
  unsigned f = 0u;
  if (!(fabsf(m[6]) < 1e-6f && fabsf(m[7]) < 1e-6f && fabsf(m[8]) < 1e-6f)) f |= MAT_TRANS;
  if (m[10] > 0.0f) f |= MAT_ROUGH;
  if (!finite_rgb(m[0], m[1], m[2])) f |= MAT_NONFINITE;
  return f;
}

} // namespace mirt
#endif
