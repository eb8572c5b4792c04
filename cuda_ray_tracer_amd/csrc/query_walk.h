// Device code that query kernels share (DESIGN.md sections 6n, 6q): the walk over the exact 64-byte records (light.hip,
// indirect.hip), the pieces every walk is made of -- the lane's stack, the live-ray rule, the planes' scalar loads, a MirtHit's
// stores (also query.hip, multihit.hip, query_lists.hip, closest.hip, closest_multi.hip, spherecast.hip and overlap_walk.h, which write their own
// loops) --, hitNearest's choice between the tree's hit
// and the planes' and the winner's normal (query.hip, indirect.hip), a light's shadow ray and a row's field of the wave's ballot
// (light.hip).  Which file uses which piece was decided by measurement, kernel by kernel: sections 6n, 6q.  Everything here is
// inlined into its caller, and every helper keeps the operation order the headers under include/ fix, so the results' bits do
// not depend on who calls it.  The render's walks (render.hip, wavefront.hip) are quantised, batched and another loop: they do
// not use this file.
#ifndef MIRT_QUERY_WALK_H
#define MIRT_QUERY_WALK_H

#include "scene_dev.h"
#include "shade_common.h"
#include "query_launch.h"

#include <cmath>

namespace mirt {

// A lane's stack of node references: entry sp lives in the block's LDS (lds_stack[QUERY_STACK_LDS * QUERY_BLOCK], [entry][lane],
// tid the lane's index in the block) while sp < lds_depth, deeper entries in the lane's private array spill[STACK_TOTAL]
// (scratch: the rarely taken path).  The tree is at most 58 levels deep, so sp stays below STACK_TOTAL;
// the mask only bounds the index.
__device__ __forceinline__ void stack_push(uint32_t* lds_stack, uint32_t* spill, int lds_depth, int tid, int& sp, uint32_t ref)
{
  if (sp < lds_depth) lds_stack[sp * QUERY_BLOCK + tid] = ref;
  else spill[(sp - lds_depth) & (STACK_TOTAL - 1)] = ref;
  ++sp;
}
__device__ __forceinline__ uint32_t stack_pop(const uint32_t* lds_stack, const uint32_t* spill, int lds_depth, int tid, int& sp)
{
  --sp;
  return sp < lds_depth ? lds_stack[sp * QUERY_BLOCK + tid] : spill[(sp - lds_depth) & (STACK_TOTAL - 1)];
}

// mirt_trace_rays' rule, d normalised: a ray with nothing to look for (tmax <= 0 or NaN) or no direction (shorter than
// normalize's 1e-6, or NaN) is a miss.
__device__ __forceinline__ bool ray_is_live(float tmax, const f3& d)
{
  return tmax > 0.0f && (fabsf(d.x) + fabsf(d.y) + fabsf(d.z)) > 0.0f;
}

// The planes are the same for every lane and never written by a kernel: scalar loads through the constant address space.
typedef const PlaneDev __attribute__((address_space(4))) * ConstPlanes;
__device__ __forceinline__ ConstPlanes const_planes(const PlaneDev* planes)
{
  return (ConstPlanes)(unsigned long long)planes;
}

// One MirtHit record (6 words at h).  Word by word: three 8-byte stores for an 8-byte aligned buffer were measured and took 20
// to 58 % longer.
__device__ __forceinline__ void store_hit(uint32_t* h, float t, uint32_t kind, uint32_t id, const f3& n)
{
  h[0] = __float_as_uint(t);
  h[1] = kind;
  h[2] = id;
  h[3] = __float_as_uint(n.x);
  h[4] = __float_as_uint(n.y);
  h[5] = __float_as_uint(n.z);
}

// The reference's hitNearest without the final choice, for the ray (o, tmax, d), d normalised: the planes (checkPlane,
// draw.cu:581-615), then the walk of traverse_lbvh (bvh_traversal.cu:92-183) over the exact 64-byte node records, left child
// first -- the reference's own walk, so no vetting and no second walk is ever needed.  ANY: an occlusion query, which ends at the
// first occluder nearer than tmax.  Leaves tbest / refbest (the tree's answer) and tplane / plane_id (the planes').
// A lane carries the ray, 1/d, the best distance and record and a stack pointer; the stack is stack_push's.
template <bool ANY>
__device__ __forceinline__ void walk(const unsigned char* heap, uint32_t root_ref, const PlaneDev* planes, int num_planes, const f3& o, const f3& d, float tmax,
                                     uint32_t* lds_stack, uint32_t* spill, int lds_depth, int tid, float& tbest, uint32_t& refbest, float& tplane,
                                     int& plane_id)
{
  const float tmin = 0.0001f;
  const bool live = ray_is_live(tmax, d);
  tplane = INFINITY; tbest = INFINITY;
  plane_id = -1;
  refbest = REF_NONE;
  if (live) nearest_plane(planes, num_planes, o, d, tplane, plane_id);
  // an occlusion query that a plane already answers needs no walk
  if (live && root_ref != REF_NONE && !(ANY && plane_id >= 0 && tplane < tmax)) {
    const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    uint32_t cur = root_ref;
    int sp = 0;
    for (;;) {
      const float4* rec = reinterpret_cast<const float4*>(heap + (cur << 4));
      bool pop;
      if (cur & REF_LEAF) {
        // intersect_leaf_primitives, bvh_traversal.cu:47-89
        float t = 0.0f;
        bool hit;
        if (cur & REF_TRI) {
          hit = triangle_hit(rec[0], rec[1], rec[2], o, d, t);
        } else {
          float tc, t_far;
          hit = sphere_hit(rec[0], o, d, t, tc, t_far);
        }
        const bool closer = closer_hit(hit, t, tbest, cur & REF_OFFMASK, refbest);
        tbest = closer ? t : tbest;
        refbest = closer ? cur : refbest;
        if (ANY && closer && t < tmax) break;           // the first occluder ends an occlusion query
        pop = true;
      } else {
        // hit_aabb_adapted on both children, left first (bvh_traversal.cu:11-44, 149-157)
        const float4 b0 = rec[0], b1 = rec[1], b2 = rec[2];
        const uint2 ch = *reinterpret_cast<const uint2*>(rec + 3);
        bool hl, hr;
        float tel, ter;
        box_pair(b0, b1, b2, o.x, o.y, o.z, inv.x, inv.y, inv.z, tbest, tmin, hl, hr, tel, ter);
        if (hl && hr) stack_push(lds_stack, spill, lds_depth, tid, sp, ch.y);
        cur = hl ? ch.x : ch.y;
        pop = !(hl || hr);
      }
      if (pop) {
        if (sp == 0) break;
        cur = stack_pop(lds_stack, spill, lds_depth, tid, sp);
      }
    }
  }
}

// hitNearest's choice (draw.cu:292-318): the nearer of the tree's hit and the planes', the plane winning a tie; an occlusion query
// (ANY) reports the occluder it found.  Then the caller's bound (draw.cu:365-370).
struct Nearest { bool report, use_bvh; float t; };
template <bool ANY>
__device__ __forceinline__ Nearest nearest_of(float tbest, uint32_t refbest, float tplane, int plane_id, float tmax)
{
  Nearest w;
  const bool bvh_hit = refbest != REF_NONE;
  w.use_bvh = bvh_hit && (ANY ? tbest < tmax : (plane_id < 0 || tbest < tplane));
  w.t = w.use_bvh ? tbest : tplane;
  w.report = (w.use_bvh || plane_id >= 0) && w.t < tmax;
  return w;
}

// ObjectInfo.normal of a hit as mirt_trace_rays reports it, from p = t d + o (struct.cu:64-163, draw.cu:581-615): of the
// primitive record `refbest` names, and of a plane.
__device__ __forceinline__ f3 prim_normal(const float4* nodes, uint32_t refbest, float t, const f3& o, const f3& d)
{
  const float4* rec = nodes + (refbest & REF_OFFMASK);
  if (refbest & REF_TRI) {
    const float4 q0 = rec[0], q1 = rec[1];
    const f3 nor = mk3(q0.w, q1.x, q1.y);
    return (dot(d, nor) < 0.0f) ? nor : -nor;
  }
  const float4 s = rec[0];
  const f3 c = mk3(s.x, s.y, s.z);
  const f3 p = t * d + o;
  const f3 cr0 = c - o;
  const bool inside = (dot(cr0, cr0) < s.w * s.w);
  return normalize(inside ? (c - p) : (p - c));
}
__device__ __forceinline__ f3 plane_normal(const PlaneDev* planes_generic, int plane_id, const f3& d)
{
  const ConstPlanes planes = const_planes(planes_generic);
  const f3 pnor = mk3(planes[plane_id].nx, planes[plane_id].ny, planes[plane_id].nz);
  return (dot(pnor, d) < 0.0f) ? pnor : -pnor;
}

// diffuseLight's shadow ray from the point P to a light (draw.cu:346 / 362-363): L, the unit vector the facing test takes; d, the
// ray's direction; tmax, the distance of a bulb (a sun: +inf).
__device__ __forceinline__ void light_ray(const LightDev* lt, bool is_sun, const f3& P, f3& L, f3& d, float& tmax)
{
  if (is_sun) {
    L = mk3(lt->nx, lt->ny, lt->nz);
    d = normalize(mk3(lt->x, lt->y, lt->z));            // Ray(eye, dir, bounce), object.cuh:69 -- as mirt_trace_rays does it
    tmax = INFINITY;
  } else {
    const f3 bd = mk3(lt->x, lt->y, lt->z) - P;
    tmax = length(bd);
    L = normalize(bd);
    d = L;
  }
}

// One ballot of `flag` is the wave's 64-bit word, of which a row's mask is the G-bit field of its lanes (G = 1 << gshift; lane:
// the lane's index in the wave).  Every lane of the wave must get here.
__device__ __forceinline__ unsigned long long group_field(bool flag, int lane, int gshift)
{
  const int G = 1 << gshift;
  const unsigned long long word = __ballot(flag);
  const int group = lane >> gshift;
  return ((word >> (group << gshift)) << (64 - G)) >> (64 - G);
}

} // namespace mirt

#endif
