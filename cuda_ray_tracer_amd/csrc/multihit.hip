// Multi-hit ray queries on a built scene (include/mirt_multihit.h: mirt_trace_rays_multi): for each ray the
// k nearest of ALL the hits the reference's walk admits with its bound held at tmax, in (t, class, index) order, and their number.
//
// multihit_kernel<CAP>  one lane = one ray (grid-stride over the batch), the loop of trace_rays_kernel (query.hip) with a bound
//                       that never shrinks: the planes, one by one (checkPlane, draw.cu:581-615), through scalar loads, then the
//                       walk over the exact 64-byte records with box_pair at tbest = tmax.  No bound changes, so the admitted set
//                       does not depend on the visiting order; the walk goes left first like its sibling.
//                       What a lane carries beside the ray and the stack pointer is the count and the list of its CAP best as
//                       64-bit keys, ascending, in registers: high word t's bits (every admitted t is positive: they order as
//                       unsigned integers), low word the plane's index, or bit 31 | the leaf record's offset << 1 | triangle.  One
//                       unsigned compare is the header's whole order -- t, planes before primitives, lower plane index, earlier
//                       sorted leaf (records are stored in sorted order, scene_dev.h).  A new key goes in by a compare-exchange
//                       chain over compile-time indices (a runtime index would move the list to scratch); a key not below the
//                       list's last is counted and dropped.  The loop keeps keys only: the winners' ids and normals are made
//                       after the walk, by mirt_trace_rays' operations (unit_prim, prim_normal, plane_normal: query_walk.h).
//                       CAP = 0 is the count-only instance: no list at all.
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "query_walk.h"
#include "key_list.h"
#include "../../include/mirt_multihit.h"

#include <cmath>
#include <string>

namespace mirt {
namespace {

// Waves per SIMD an instance is compiled for.  8 is what the LDS stack allows (20 KiB per block, 8 blocks per CU) and what the
// count-only instance reaches, like trace_rays_kernel (64 VGPRs).  The list and the records' code need more registers: capacity 1
// fits the 72 of 7 waves, capacities 4 and 8 the 80 of 6; asked for more waves they spill registers.
constexpr int multihit_waves(int cap) { return cap == 0 ? 8 : cap == 1 ? 7 : 6; }
constexpr uint32_t KEY_PRIM = 0x80000000u;

struct MultiArgs {
  const float4* rays;             // MirtRay: (o, tmax), (d, pad)
  uint32_t* hits;                 // MirtHit: 6 words, k per ray
  uint32_t* counts;               // (may be null)
  long long num_rays;
  int k;
  const float4* nodes;            // record heap (scene_dev.h)
  const uint32_t* unit_prim;
  const PlaneDev* planes; int num_planes;
  uint32_t root_ref;              // the exact records' root (REF_NONE: no primitive)
  uint32_t prim_base16;
  int lds_depth;                  // stack entries kept in LDS (<= QUERY_STACK_LDS)
};

template <int CAP>
__global__ void __launch_bounds__(QUERY_BLOCK, multihit_waves(CAP)) multihit_kernel(const MultiArgs q)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];                     // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * QUERY_BLOCK;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(q.nodes);
  const ConstPlanes planes = const_planes(q.planes);
  const float tmin = 0.0001f;
  for (long long i = (long long)blockIdx.x * QUERY_BLOCK + tid; i < q.num_rays; i += stride) {
    const float4 r0 = q.rays[2 * i], r1 = q.rays[2 * i + 1];
    const f3 o = mk3(r0.x, r0.y, r0.z);
    const float tmax = r0.w;
    const f3 d = normalize(mk3(r1.x, r1.y, r1.z));      // Ray(eye, dir, bounce), object.cuh:69
    const bool live = ray_is_live(tmax, d);
    KeyList<CAP> best;
    best.clear();
    uint32_t count = 0u;
    if (live) {
      // checkPlane as nearest_plane tests each plane, the bound being tmax
      for (int j = 0; j < q.num_planes; ++j) {
        const f3 pnor = mk3(planes[j].nx, planes[j].ny, planes[j].nz);
        const float t = dot(mk3(planes[j].px, planes[j].py, planes[j].pz) - o, pnor) / dot(d, pnor);
        if (!(t <= 1e-6f) && t > EPSILON && t < (float)(INT_MAX - 10) && t < tmax) {
          ++count;
          best.insert(((unsigned long long)__float_as_uint(t) << 32) | (uint32_t)j);
        }
      }
    }
    if (live && q.root_ref != REF_NONE) {
      const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
      uint32_t cur = q.root_ref;
      int sp = 0;
      for (;;) {
        const float4* rec = reinterpret_cast<const float4*>(heap + (cur << 4));
        bool pop;
        if (cur & REF_LEAF) {
          // intersect_leaf_primitives, bvh_traversal.cu:47-89, with the bound left at tmax
          float t = 0.0f;
          bool hit;
          if (cur & REF_TRI) {
            hit = triangle_hit(rec[0], rec[1], rec[2], o, d, t);
          } else {
            float tc, t_far;
            hit = sphere_hit(rec[0], o, d, t, tc, t_far);
          }
          if (hit && t > 1e-6f && t < tmax) {
            ++count;
            best.insert(((unsigned long long)__float_as_uint(t) << 32) | KEY_PRIM | ((cur & REF_OFFMASK) << 1) | ((cur & REF_TRI) ? 1u : 0u));
          }
          pop = true;
        } else {
          // hit_aabb_adapted on both children (bvh_traversal.cu:11-44, 149-157), the bound tmax for every box
          const float4 b0 = rec[0], b1 = rec[1], b2 = rec[2];
          const uint2 ch = *reinterpret_cast<const uint2*>(rec + 3);
          bool hl, hr;
          float tel, ter;
          box_pair(b0, b1, b2, o.x, o.y, o.z, inv.x, inv.y, inv.z, tmax, tmin, hl, hr, tel, ter);
          if (hl && hr) stack_push(lds_stack, spill, q.lds_depth, tid, sp, ch.y);
          cur = hl ? ch.x : ch.y;
          pop = !(hl || hr);
        }
        if (pop) {
          if (sp == 0) break;
          cur = stack_pop(lds_stack, spill, q.lds_depth, tid, sp);
        }
      }
    }
    if (q.counts) q.counts[i] = count;
    if (CAP > 0) {
      // the k records, nearest first: a winner's file-order id, its normal and MirtHit's kind, as trace_rays_kernel makes them
      uint32_t* h = q.hits + 6 * (i * q.k);
      for (int j = 0; j < q.k; ++j, h += 6) {
        const unsigned long long key = best.pop_front();
        const uint32_t low = (uint32_t)key;
        float t = -1.0f;
        uint32_t kind = 0u, id = 0u;
        f3 n = mk3(0.0f, 0.0f, 0.0f);
        if (key != KEY_NONE) {
          t = __uint_as_float((uint32_t)(key >> 32));
          if (low & KEY_PRIM) {
            const uint32_t ref = REF_LEAF | ((low & 1u) ? REF_TRI : 0u) | ((low >> 1) & REF_OFFMASK);
            id = q.unit_prim[(ref & REF_OFFMASK) - q.prim_base16] & 0x7fffffffu;
            n = prim_normal(q.nodes, ref, t, o, d);
            kind = (ref & REF_TRI) ? MIRT_HIT_TRIANGLE : MIRT_HIT_SPHERE;
          } else {
            n = plane_normal(q.planes, (int)low, d);
            id = low;
            kind = MIRT_HIT_PLANE;
          }
        }
        // (store_hit of query_walk.h, written out: as a call it renames this loop's registers)
        h[0] = __float_as_uint(t);
        h[1] = kind;
        h[2] = id;
        h[3] = __float_as_uint(n.x);
        h[4] = __float_as_uint(n.y);
        h[5] = __float_as_uint(n.z);
      }
    }
  }
}

} // namespace

int trace_rays_multi(MirtScene* sc, const void* d_rays, int64_t num_rays, int k, void* d_hits, uint32_t* d_counts, uint32_t flags, hipStream_t stream)
{
  bool go = false;
  const int rc = check_trace_rays_multi(d_rays, num_rays, k, d_hits, d_counts, flags, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  MultiArgs q;
  q.rays = reinterpret_cast<const float4*>(d_rays);
  q.hits = reinterpret_cast<uint32_t*>(d_hits);
  q.counts = d_counts;
  q.num_rays = num_rays;
  q.k = k;
  fill_walk_args(q, sc);
  // the smallest instance that holds k
  return with_capacity(k, [&](auto cap, int slot) {
    constexpr int CAP = decltype(cap)::value;
    return launch_rows(sc, multihit_kernel<CAP>, multihit_waves(CAP), &sc->multihit_blocks[slot], num_rays, q, stream);
  });
}

} // namespace mirt
