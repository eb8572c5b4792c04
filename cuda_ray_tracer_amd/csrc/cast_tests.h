// Device code of the sphere-cast kernels (spherecast.hip, cast_lists.hip; DESIGN.md sections 6v, 6ab): a candidate's contact
// parameter t -- sphere, plane, triangle in seven pieces -- and the centre ray's interval in a grown box, by the operations
// include_ext/mirt_spherecast.h fixes.  Everything here is inlined into its caller, so the results' bits do not depend on who
// calls it.
#ifndef MIRT_CAST_TESTS_H
#define MIRT_CAST_TESTS_H

#include "device_common.h"
#include "point_query.h"

#include <cmath>

namespace mirt {

constexpr float TAU = 9.5367431640625e-07f;          // 2^-20 (mirt_spherecast.h, "Pruning"; SLACK: point_query.h)

// the moving ball: the centre's ray (o, d normalised) and the radius
struct Ball { f3 o, d; float r; };

// ---- the header's operations, candidate by candidate: each returns t, or a NaN (or +inf) for no contact ----------------------------
// the centre ray against the ball (p, R), closest-approach form: a the parameter of the closest approach, h2 = R^2 - |w|^2
MIRT_DEV void approach(const f3& p, float R, const Ball& k, float& a, float& h2)
{
  const f3 m = p - k.o;
  a = dot(m, k.d);
  const f3 w = m - k.d * a;
  h2 = R * R - dot(w, w);
}
MIRT_DEV float ball_entry(const f3& p, float R, const Ball& k)
{
  float a, h2;
  approach(p, R, k, a, h2);
  return h2 >= 0.0f ? a - sqrtf(h2) : NAN;
}
MIRT_DEV float ball_exit(const f3& p, float R, const Ball& k)
{
  float a, h2;
  approach(p, R, k, a, h2);
  return a + sqrtf(h2 < 0.0f ? 0.0f : h2);
}

MIRT_DEV float sphere_cast(const float4& s, const Ball& k)
{
  const f3 c = mk3(s.x, s.y, s.z);
  const float g = length(k.o - c) - s.w;
  if (fabsf(g) <= k.r) return 0.0f;
  return g > 0.0f ? ball_entry(c, s.w + k.r, k) : ball_exit(c, s.w - k.r, k);
}

// the plane rule for a unit normal N: a plane's normalize(nor), a triangle's nor
MIRT_DEV float plane_cast(const f3& N, const f3& point, const Ball& k)
{
  const float s = dot(N, k.o - point);
  if (fabsf(s) <= k.r) return 0.0f;
  const float dn = dot(N, k.d);
  if (s > 0.0f && dn < 0.0f) return (k.r - s) / dn;
  if (s < 0.0f && dn > 0.0f) return (-k.r - s) / dn;
  return NAN;
}

// mirt_closest.h's region walk for q falls through to its last case (closest_on_triangle's tests, in its order)
MIRT_DEV bool in_face_region(const f3& a, const f3& b, const f3& c, const f3& q)
{
  const f3 ab = b - a, ac = c - a, ap = q - a;
  const float d1 = dot(ab, ap), d2 = dot(ac, ap);
  if (d1 <= 0.0f && d2 <= 0.0f) return false;
  const f3 bp = q - b;
  const float d3 = dot(ab, bp), d4 = dot(ac, bp);
  if (d3 >= 0.0f && d4 <= d3) return false;
  const float vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) return false;
  const f3 cp = q - c;
  const float d5 = dot(ab, cp), d6 = dot(ac, cp);
  if (d6 >= 0.0f && d5 <= d6) return false;
  const float vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) return false;
  const float va = d3 * d6 - d5 * d4;
  const float e = d4 - d3, f = d5 - d6;
  return !(va <= 0.0f && e >= 0.0f && f >= 0.0f);
}

// the edge (p, q): the centre ray against the cylinder of radius r about its line, valid between its end points
MIRT_DEV float edge_cast(const f3& p, const f3& q, const Ball& k)
{
  const f3 e = q - p;
  const float ee = dot(e, e);
  const f3 m = k.o - p;
  const float u = dot(m, e) / ee, kk = dot(k.d, e) / ee;
  const f3 mp = m - e * u, dp = k.d - e * kk;
  const float A = dot(dp, dp);
  const float t0 = -dot(mp, dp) / A;
  const f3 wv = mp + dp * t0;
  const float h2 = k.r * k.r - dot(wv, wv);
  const float t = t0 - sqrtf(h2 / A);
  const float at = u + t * kk;
  return (ee != 0.0f && A != 0.0f && h2 >= 0.0f && at >= 0.0f && at <= 1.0f) ? t : NAN;
}

// (the smallest piece with t >= 0: a NaN never counts)
MIRT_DEV void take_piece(float& t, float piece) { t = (piece >= 0.0f && piece < t) ? piece : t; }

MIRT_DEV float triangle_cast(const f3& a, const f3& b, const f3& c, const f3& nor, const Ball& k)
{
  if (length(k.o - closest_on_triangle(a, b, c, k.o)) <= k.r) return 0.0f;
  float t = INFINITY;
  const float tf = plane_cast(nor, a, k);
  // (a record normal of (0, 0, 0) -- a cross product shorter than 1e-6 -- names no plane: such a triangle has no face piece)
  if (dot(nor, nor) > 0.0f && in_face_region(a, b, c, k.o + k.d * tf)) take_piece(t, tf);
  take_piece(t, ball_entry(a, k.r, k));
  take_piece(t, ball_entry(b, k.r, k));
  take_piece(t, ball_entry(c, k.r, k));
  take_piece(t, edge_cast(a, b, k));
  take_piece(t, edge_cast(a, c, k));
  take_piece(t, edge_cast(b, c, k));
  return t;
}

// the centre ray's interval in the box [x0, x1] x [y0, y1] x [z0, z1] grown by `grow`, from parameter 0 on: fminf / fmaxf drop a
// NaN (0 * inf: the centre on a face of a slab it runs along), so such an axis does not decide
MIRT_DEV void box_interval(float x0, float x1, float y0, float y1, float z0, float z1, const f3& o, const f3& inv, float grow, float& enter, float& leave)
{
  const float ax = ((x0 - grow) - o.x) * inv.x, bx = ((x1 + grow) - o.x) * inv.x;
  const float ay = ((y0 - grow) - o.y) * inv.y, by = ((y1 + grow) - o.y) * inv.y;
  const float az = ((z0 - grow) - o.z) * inv.z, bz = ((z1 + grow) - o.z) * inv.z;
  enter = fmaxf(fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz)), 0.0f);
  leave = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
}

} // namespace mirt

#endif
