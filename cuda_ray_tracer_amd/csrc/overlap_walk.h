// The box-overlap walk as a function (DESIGN.md sections 6w, 6x, 6y): a row's decode, the planes and the stack walk over the exact
// 64-byte records, by the operations include_ext/mirt_overlap.h fixes, parametrised by what an admitted candidate does.
// overlap_list.hip uses it.  overlap.hip keeps the same walk written out, because its count-only and record instances measured
// 0.8 to 1.8 % slower through this function (section 6y): a change to the pruning or to the degenerate-triangle rule goes into
// both.  Everything here is inlined into its caller, and the walk takes its pointers and the row by value: taken through a
// reference to the kernel's argument struct it spills registers in the list kernel (section 6y).
#ifndef MIRT_OVERLAP_WALK_H
#define MIRT_OVERLAP_WALK_H

#include "query_walk.h"
#include "point_query.h"
#include "overlap_tests.h"

namespace mirt {

// A row's box [lo, hi], its centre m and half extent h; live: every coordinate finite and lo <= hi on every axis.
struct BoxRow { f3 lo, hi, m, h; bool live; };
MIRT_DEV BoxRow box_row(const float4* boxes, long long i)
{
  const float4 r0 = boxes[2 * i], r1 = boxes[2 * i + 1];
  BoxRow b;
  b.lo = mk3(r0.x, r0.y, r0.z); b.hi = mk3(r1.x, r1.y, r1.z);
  const f3 lo = b.lo, hi = b.hi;
  // (x - x is 0 for a finite x and NaN for an infinity or a NaN)
  b.live = (lo.x - lo.x) == 0.0f && (lo.y - lo.y) == 0.0f && (lo.z - lo.z) == 0.0f && (hi.x - hi.x) == 0.0f && (hi.y - hi.y) == 0.0f &&
           (hi.z - hi.z) == 0.0f && lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z;
  b.m = (lo + hi) * 0.5f; b.h = (hi - lo) * 0.5f;
  return b;
}

// What an admitted candidate does is the caller's action, a struct held by value (the walks return it): act.plane(dist, j) for plane
// j, act.leaf(dist, cur, id) for a sphere or triangle.
// the planes the box meets, in index order
template <class Act>
MIRT_DEV Act overlap_planes(ConstPlanes planes, int num_planes, f3 m, f3 h, Act act)
{
  for (int j = 0; j < num_planes; ++j) {
    const f3 N = normalize(mk3(planes[j].nx, planes[j].ny, planes[j].nz));
    const float s = dot(N, m - mk3(planes[j].px, planes[j].py, planes[j].pz));
    const float e = (h.x * fabsf(N.x) + h.y * fabsf(N.y)) + h.z * fabsf(N.z);
    if (fabsf(s) <= e) act.plane(fabsf(s), (uint32_t)j);       // (s is then no NaN, and dist = fabsf(s) is none)
  }
  return act;
}

// The spheres and triangles the box meets, in the scene's leaf order (left child first): a child is visited when its box meets the
// row's grown by sigma on every axis (negated compares: a NaN visits); a leaf is the header's test and, for a candidate that
// passes, mirt_closest.h's dist at m -- a NaN dist (a triangle without area) is not admitted.  act.leaf(dist, cur, id), cur the leaf's
// reference and id a triangle's file-order id (a sphere's is a unit_prim load the caller makes if it wants it), returns whether the
// walk ends there.  root_ref is no REF_NONE.
template <class Act>
MIRT_DEV Act overlap_walk(const unsigned char* heap, const uint32_t* unit_prim, const float4* tri_verts, uint32_t prim_base16, uint32_t root_ref,
                           float coord_max, int lds_depth, uint32_t* lds_stack, uint32_t* spill, int tid, f3 lo, f3 hi, f3 m, f3 h, Act act)
{
  const float sigma = row_sigma(fmaxf(largest_abs(lo), largest_abs(hi)), coord_max);
  uint32_t cur = root_ref;
  int sp = 0;
  for (;;) {
    const float4* rec = reinterpret_cast<const float4*>(heap + (cur << 4));
    bool pop;
    if (cur & REF_LEAF) {
      float dist = 0.0f;
      uint32_t id = 0u;
      bool pass;
      if (cur & REF_TRI) {
        id = unit_prim[(cur & REF_OFFMASK) - prim_base16] & 0x7fffffffu;
        const float4* v = tri_verts + 3 * (size_t)id;
        const float4 pa = v[0], pb = v[1], pc = v[2];
        const f3 ta = mk3(pa.x, pa.y, pa.z), tb = mk3(pb.x, pb.y, pb.z), tc = mk3(pc.x, pc.y, pc.z);
        pass = triangle_overlaps(m, h, ta, tb, tc);
        if (pass) {
          // (the vertices are loaded again, through an id the compiler cannot see through: kept from the test above they are
          // nine registers more at the kernel's peak, section 6w)
          asm volatile("" : "+v"(id));
          dist = length(m - triangle_point(tri_verts, id, m));
        }
      } else {
        const float4 s = rec[0];
        const f3 c = mk3(s.x, s.y, s.z);
        pass = sphere_overlaps(lo, hi, c, s.w);
        if (pass) dist = fabsf(length(m - c) - s.w);
      }
      if (pass && dist == dist) {          // (a NaN dist is not admitted)
        if (act.leaf(dist, cur, id)) break;
      }
      pop = true;
    } else {
      const float4 b0 = rec[0], b1 = rec[1], b2 = rec[2];
      const uint2 ch = *reinterpret_cast<const uint2*>(rec + 3);
      // hi + sigma and lo - sigma are made here, from a copy of sigma the compiler cannot see through: hoisted out of the walk
      // they are six registers held across every leaf's test (section 6w)
      float sg = sigma;
      asm volatile("" : "+v"(sg));
      const f3 los = mk3(lo.x - sg, lo.y - sg, lo.z - sg), his = mk3(hi.x + sg, hi.y + sg, hi.z + sg);
      const bool hl = !(b0.x > his.x) && !(b0.y < los.x) && !(b0.z > his.y) && !(b0.w < los.y) && !(b1.x > his.z) && !(b1.y < los.z);
      const bool hr = !(b1.z > his.x) && !(b1.w < los.x) && !(b2.x > his.y) && !(b2.y < los.y) && !(b2.z > his.z) && !(b2.w < los.z);
      if (hl && hr) stack_push(lds_stack, spill, lds_depth, tid, sp, ch.y);
      cur = hl ? ch.x : ch.y;
      pop = !(hl || hr);
    }
    if (pop) {
      if (sp == 0) break;
      cur = stack_pop(lds_stack, spill, lds_depth, tid, sp);
    }
    // One latch for every path (an empty statement the compiler may not duplicate; it emits nothing).  Without it this function's
    // loop is split in two -- lanes that have to pop wait until no lane descends any more -- and the walk is 10 to 25 % slower
    // (section 6y).
    asm volatile("");
  }
  return act;
}

} // namespace mirt

#endif
