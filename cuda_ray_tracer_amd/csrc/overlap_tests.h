// Device code the box-overlap kernels share (overlap.hip, overlap_list.hip, through overlap_walk.h; DESIGN.md sections 6w, 6x): a
// sphere's and a triangle's overlap test against a box, by the operations include_ext/mirt_overlap.h fixes.  Everything here is
// inlined into its caller, so the results' bits do not depend on who calls it.
#ifndef MIRT_OVERLAP_TESTS_H
#define MIRT_OVERLAP_TESTS_H

#include "device_common.h"

namespace mirt {

MIRT_DEV float min3(float x, float y, float z) { return fminf(fminf(x, y), z); }
MIRT_DEV float max3(float x, float y, float z) { return fmaxf(fmaxf(x, y), z); }

// the header's sphere test: the box reaches the surface and is not wholly inside it
MIRT_DEV bool sphere_overlaps(const f3& lo, const f3& hi, const f3& c, float rs)
{
  const f3 dn = mk3(fmaxf(fmaxf(lo.x - c.x, c.x - hi.x), 0.0f), fmaxf(fmaxf(lo.y - c.y, c.y - hi.y), 0.0f), fmaxf(fmaxf(lo.z - c.z, c.z - hi.z), 0.0f));
  const f3 df = mk3(fmaxf(fabsf(c.x - lo.x), fabsf(hi.x - c.x)), fmaxf(fabsf(c.y - lo.y), fabsf(hi.y - c.y)), fmaxf(fabsf(c.z - lo.z), fabsf(hi.z - c.z)));
  const float rr = rs * rs;
  return dot(dn, dn) <= rr && dot(df, df) >= rr;
}

// One edge axis of the header, for the components k1 (the `a` arguments) and k2 (the `b` arguments) of the three vertices, the edge
// f and the half extent: p_i = v_i[k2] * f[k1] - v_i[k1] * f[k2] against rr = h[k1] * |f[k2]| + h[k2] * |f[k1]|.
MIRT_DEV bool edge_axis(float v0a, float v0b, float v1a, float v1b, float v2a, float v2b, float fa, float fb, float ha, float hb)
{
  const float p0 = v0b * fa - v0a * fb;
  const float p1 = v1b * fa - v1a * fb;
  const float p2 = v2b * fa - v2a * fb;
  const float rr = ha * fabsf(fb) + hb * fabsf(fa);
  return min3(p0, p1, p2) <= rr && max3(p0, p1, p2) >= -rr;
}

// ... and the three of an edge f: k = 0 (k1 = y, k2 = z), k = 1 (z, x), k = 2 (x, y)
MIRT_DEV bool edge_axes(const f3& v0, const f3& v1, const f3& v2, const f3& f, const f3& h)
{
  bool ok = edge_axis(v0.y, v0.z, v1.y, v1.z, v2.y, v2.z, f.y, f.z, h.y, h.z);
  ok = ok & edge_axis(v0.z, v0.x, v1.z, v1.x, v2.z, v2.x, f.z, f.x, h.z, h.x);
  ok = ok & edge_axis(v0.x, v0.y, v1.x, v1.y, v2.x, v2.y, f.x, f.y, h.x, h.y);
  return ok;
}

// the header's triangle test: thirteen axes in one running boolean, the box axes first
MIRT_DEV bool triangle_overlaps(const f3& m, const f3& h, const f3& a, const f3& b, const f3& c)
{
  const f3 v0 = a - m, v1 = b - m, v2 = c - m;
  bool ok = min3(v0.x, v1.x, v2.x) <= h.x && max3(v0.x, v1.x, v2.x) >= -h.x;
  ok = ok & (min3(v0.y, v1.y, v2.y) <= h.y && max3(v0.y, v1.y, v2.y) >= -h.y);
  ok = ok & (min3(v0.z, v1.z, v2.z) <= h.z && max3(v0.z, v1.z, v2.z) >= -h.z);
  if (!ok) return false;           // (most leaves a walk reaches end here)
  // The face and one edge's axes at a time, a branch between the groups: what is live is the vertices, h and one edge.  Folded
  // into one expression the compiler keeps all 27 projections in flight and the kernel needs 110 VGPRs (section 6w).
  const f3 f0 = v1 - v0, f1 = v2 - v1;
  const f3 nn = mk3(f0.y * f1.z - f0.z * f1.y, f0.z * f1.x - f0.x * f1.z, f0.x * f1.y - f0.y * f1.x);
  ok = fabsf(dot(nn, v0)) <= (h.x * fabsf(nn.x) + h.y * fabsf(nn.y)) + h.z * fabsf(nn.z);
  ok = ok & edge_axes(v0, v1, v2, f0, h);
  if (!ok) return false;
  if (!edge_axes(v0, v1, v2, f1, h)) return false;
  return edge_axes(v0, v1, v2, v0 - v2, h);
}

} // namespace mirt

#endif
