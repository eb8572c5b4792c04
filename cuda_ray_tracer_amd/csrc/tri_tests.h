// Device code of the triangle-overlap kernels (overlap_tris.hip): a row's decode and the narrow phase --
// triangle against plane, against sphere surface and against triangle -- by the operations include_ext2/mirt_overlap_tris.h fixes.
// Everything here is inlined into its caller, so the results' bits do not depend on who calls it.
#ifndef MIRT_TRI_TESTS_H
#define MIRT_TRI_TESTS_H

#include "device_common.h"
#include "point_query.h"
#include "overlap_tests.h"      // (min3, max3)

namespace mirt {

// A row's vertices as given, its bounds [lo, hi] (the componentwise min3 and max3: exact) and the header's live rule: nine finite
// coordinates, and dot(n1, n1) finite and above 0 for n1 = cross(b - a, c - a).
struct TriRow { f3 a, b, c, lo, hi; bool live; };
MIRT_DEV TriRow tri_row(const float* tris, long long i)
{
  const float* r = tris + 9 * i;
  TriRow t;
  t.a = mk3(r[0], r[1], r[2]); t.b = mk3(r[3], r[4], r[5]); t.c = mk3(r[6], r[7], r[8]);
  const f3 a = t.a, b = t.b, c = t.c;
  t.lo = mk3(min3(a.x, b.x, c.x), min3(a.y, b.y, c.y), min3(a.z, b.z, c.z));
  t.hi = mk3(max3(a.x, b.x, c.x), max3(a.y, b.y, c.y), max3(a.z, b.z, c.z));
  const f3 n1 = cross(b - a, c - a);
  const float m1 = dot(n1, n1);
  // (x - x is 0 for a finite x and NaN for an infinity or a NaN)
  t.live = (a.x - a.x) == 0.0f && (a.y - a.y) == 0.0f && (a.z - a.z) == 0.0f && (b.x - b.x) == 0.0f && (b.y - b.y) == 0.0f &&
           (b.z - b.z) == 0.0f && (c.x - c.x) == 0.0f && (c.y - c.y) == 0.0f && (c.z - c.z) == 0.0f && (m1 - m1) == 0.0f && m1 > 0.0f;
  return t;
}

// the header's plane test: the three signed distances lie on both sides of 0 (or one is 0), and none is a NaN
MIRT_DEV bool tri_meets_plane(const f3& N, const f3& p, const f3& a, const f3& b, const f3& c)
{
  const float sa = dot(N, a - p), sb = dot(N, b - p), sc = dot(N, c - p);
  return min3(sa, sb, sc) <= 0.0f && max3(sa, sb, sc) >= 0.0f && sa == sa && sb == sb && sc == sc;
}

// The header's sphere test for the row (a, a + ub, a + uc) with bounds [lo, hi]: (0) the builder's box of the sphere meets the
// bounds, (1) the surface is reached, (2) some vertex is not inside.
MIRT_DEV bool tri_meets_sphere(const f3& lo, const f3& hi, const f3& a, const f3& ub, const f3& uc, const f3& ctr, float rs)
{
  // (prim_box of lbvh_build.hip, operation for operation)
  const float ax = ctr.x - rs, bx = ctr.x + rs, ay = ctr.y - rs, by = ctr.y + rs, az = ctr.z - rs, bz = ctr.z + rs;
  const bool ox = ax <= bx, oy = ay <= by, oz = az <= bz;
  const bool near = (ox ? ax : bx) <= hi.x && (ox ? bx : ax) >= lo.x && (oy ? ay : by) <= hi.y && (oy ? by : ay) >= lo.y &&
                    (oz ? az : bz) <= hi.z && (oz ? bz : az) >= lo.z;
  if (!near) return false;         // (most leaves a walk reaches end here)
  const f3 zero = mk3(0.0f, 0.0f, 0.0f);
  const f3 C = ctr - a;
  const float dn = length(C - closest_on_triangle(zero, ub, uc, C));
  const float df = max3(length(zero - C), length(ub - C), length(uc - C));
  return dn <= rs && df >= rs;
}

// does the axis L separate the row (0, ub, uc) from the scene triangle (P, Q, R)
MIRT_DEV bool axis_separates(const f3& L, const f3& ub, const f3& uc, const f3& P, const f3& Q, const f3& R)
{
  const float r1 = dot(L, ub), r2 = dot(L, uc);
  const float s0 = dot(L, P), s1 = dot(L, Q), s2 = dot(L, R);
  return max3(0.0f, r1, r2) < min3(s0, s1, s2) || max3(s0, s1, s2) < min3(0.0f, r1, r2);
}

// A point of the triangle test's code the compiler may not move values across or share them over: it emits nothing.  What the next
// group needs of the edges and normals it makes again from the five vectors, a few operations, rather than hold it in registers
// over the groups before (DESIGN.md section 6aa has the compiler's figures with and without).
MIRT_DEV void group_fence(f3& ub, f3& uc, f3& P, f3& Q, f3& R)
{
  asm volatile("" : "+v"(ub.x), "+v"(ub.y), "+v"(ub.z), "+v"(uc.x), "+v"(uc.y), "+v"(uc.z), "+v"(P.x), "+v"(P.y), "+v"(P.z), "+v"(Q.x), "+v"(Q.y),
               "+v"(Q.z), "+v"(R.x), "+v"(R.y), "+v"(R.z));
}

// the three axes cross(e, f_j) of a row edge e
MIRT_DEV bool edge_separates(const f3& e, const f3& ub, const f3& uc, const f3& P, const f3& Q, const f3& R)
{
  bool s = axis_separates(cross(e, Q - P), ub, uc, P, Q, R);
  s = s | axis_separates(cross(e, R - Q), ub, uc, P, Q, R);
  s = s | axis_separates(cross(e, R - P), ub, uc, P, Q, R);
  return s;
}

// The header's triangle test against the scene triangle (p, q, r): (i) the bounds, (ii) its area, (iii) the seventeen axes in the
// header's order, a branch and a fence between the groups: what is live across a group is the five vectors ub, uc, P, Q, R and one
// edge or normal, not the 102 projections.  The fence before the first group also keeps what depends on the row alone -- n1, the
// in-plane axes, their projections of the row -- from being made once per row and held across the whole walk.
MIRT_DEV bool tri_meets_triangle(const f3& lo, const f3& hi, const f3& a, const f3& row_ub, const f3& row_uc, const f3& p, const f3& q, const f3& r)
{
  const bool near = min3(p.x, q.x, r.x) <= hi.x && max3(p.x, q.x, r.x) >= lo.x && min3(p.y, q.y, r.y) <= hi.y && max3(p.y, q.y, r.y) >= lo.y &&
                    min3(p.z, q.z, r.z) <= hi.z && max3(p.z, q.z, r.z) >= lo.z;
  if (!near) return false;         // (most leaves a walk reaches end here)
  f3 ub = row_ub, uc = row_uc;
  f3 P = p - a, Q = q - a, R = r - a;
  group_fence(ub, uc, P, Q, R);
  {
    const f3 n2 = cross(Q - P, R - P);
    const float m2 = dot(n2, n2);
    if (!((m2 - m2) == 0.0f && m2 > 0.0f)) return false;
    bool s = axis_separates(cross(ub, uc), ub, uc, P, Q, R);
    s = s | axis_separates(n2, ub, uc, P, Q, R);
    if (s) return false;
  }
  group_fence(ub, uc, P, Q, R);
  if (edge_separates(ub, ub, uc, P, Q, R)) return false;
  group_fence(ub, uc, P, Q, R);
  if (edge_separates(uc - ub, ub, uc, P, Q, R)) return false;
  group_fence(ub, uc, P, Q, R);
  if (edge_separates(uc, ub, uc, P, Q, R)) return false;
  group_fence(ub, uc, P, Q, R);
  {
    // the in-plane axes: they decide the coplanar case
    const f3 n1 = cross(ub, uc);
    bool s = axis_separates(cross(n1, ub), ub, uc, P, Q, R);
    s = s | axis_separates(cross(n1, uc - ub), ub, uc, P, Q, R);
    s = s | axis_separates(cross(n1, uc), ub, uc, P, Q, R);
    if (s) return false;
  }
  group_fence(ub, uc, P, Q, R);
  const f3 n2 = cross(Q - P, R - P);
  bool s = axis_separates(cross(n2, Q - P), ub, uc, P, Q, R);
  s = s | axis_separates(cross(n2, R - Q), ub, uc, P, Q, R);
  s = s | axis_separates(cross(n2, R - P), ub, uc, P, Q, R);
  return !s;
}

} // namespace mirt

#endif
