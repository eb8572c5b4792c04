// Device code the point, cast and box queries share (closest.hip, closest_multi.hip, spherecast.hip, overlap.hip, overlap_list.hip, query_lists.hip;
// DESIGN.md sections 6o, 6s, 6v, 6w, 6y): the walks' slack, a point's squared distance to a box, its closest point on a triangle and
// the tie rule of the single-winner walks, by the operations include/mirt_closest.h fixes.  Everything here is inlined into its
// caller, so the results' bits do not depend on who calls it.
#ifndef MIRT_POINT_QUERY_H
#define MIRT_POINT_QUERY_H

#include "device_common.h"

namespace mirt {

constexpr float SLACK = 3.814697265625e-06f;         // 2^-18 ("Pruning" in mirt_closest.h, mirt_spherecast.h and mirt_overlap.h)

MIRT_DEV float largest_abs(const f3& p) { return fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)); }
// the headers' sigma, once per row: (the largest coordinate magnitude of the row + coord_max [+ r]) * SLACK
MIRT_DEV float row_sigma(float largest, float coord_max) { return (largest + coord_max) * SLACK; }
MIRT_DEV float row_sigma(float largest, float coord_max, float r) { return ((largest + coord_max) + r) * SLACK; }

// squared distance of q to the box [x0, x1] x [y0, y1] x [z0, z1]
MIRT_DEV float box_dist2(float x0, float x1, float y0, float y1, float z0, float z1, const f3& q)
{
  const float ex = fmaxf(fmaxf(x0 - q.x, q.x - x1), 0.0f);
  const float ey = fmaxf(fmaxf(y0 - q.y, q.y - y1), 0.0f);
  const float ez = fmaxf(fmaxf(z0 - q.z, q.z - z1), 0.0f);
  return ex * ex + ey * ey + ez * ez;
}

// the closest point of the triangle (a, b, c) to q: mirt_closest.h, region by region
MIRT_DEV f3 closest_on_triangle(const f3& a, const f3& b, const f3& c, const f3& q)
{
  const f3 ab = b - a, ac = c - a, ap = q - a;
  const float d1 = dot(ab, ap), d2 = dot(ac, ap);
  if (d1 <= 0.0f && d2 <= 0.0f) return a;
  const f3 bp = q - b;
  const float d3 = dot(ab, bp), d4 = dot(ac, bp);
  if (d3 >= 0.0f && d4 <= d3) return b;
  const float vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) return a + ab * (d1 / (d1 - d3));
  const f3 cp = q - c;
  const float d5 = dot(ab, cp), d6 = dot(ac, cp);
  if (d6 >= 0.0f && d5 <= d6) return c;
  const float vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) return a + ac * (d2 / (d2 - d6));
  const float va = d3 * d6 - d5 * d4;
  const float e = d4 - d3, f = d5 - d6;
  if (va <= 0.0f && e >= 0.0f && f >= 0.0f) return b + (c - b) * (e / (e + f));
  const float den = 1.0f / ((va + vb) + vc);
  return (a + ab * (vb * den)) + ac * (vc * den);
}

// ... of triangle `id` of the file-order vertex array (p0, p1, p2 of every triangle)
MIRT_DEV f3 triangle_point(const float4* tri_verts, uint32_t id, const f3& q)
{
  const float4* v = tri_verts + 3 * (size_t)id;
  const float4 a = v[0], b = v[1], c = v[2];
  return closest_on_triangle(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), q);
}

// A candidate at the winner's distance (closest.hip, spherecast.hip): (kind, id) decides -- a primitive before a plane, a sphere
// before a triangle, the lower index.  cur is the candidate's record and id its file-order id if it is a triangle (a sphere's is
// loaded here); the winner is a plane (plane_id >= 0) or the record refbest.
MIRT_DEV bool wins_tie(uint32_t cur, uint32_t id, int plane_id, uint32_t refbest, const uint32_t* unit_prim, uint32_t prim_base16)
{
  if (plane_id >= 0 || (cur & REF_TRI) != (refbest & REF_TRI)) return plane_id >= 0 || !(cur & REF_TRI);
  if (!(cur & REF_TRI)) id = unit_prim[(cur & REF_OFFMASK) - prim_base16] & 0x7fffffffu;
  return id < (unit_prim[(refbest & REF_OFFMASK) - prim_base16] & 0x7fffffffu);
}

} // namespace mirt

#endif
