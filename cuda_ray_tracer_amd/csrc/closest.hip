// Closest-point queries on a built scene (include/mirt_closest.h: mirt_closest_points): for each point the
// nearest plane, sphere or triangle within the row's radius -- the admitted candidate with the smallest (dist, kind, id), which the
// header defines over the scene's arrays, so the order of the visits is free.  Like the ray queries it reads the scene only and
// touches no render context, counter, hand-out table or RNG table.
//
// closest_points_kernel  one lane = one row (grid-stride over the batch).  The planes from scalar loads, then a best-first stack walk
//                        over the exact 64-byte node records: the squared point-box distance of both children against
//                        (best + sigma)^2, the nearer child first, the other pushed.  best starts at the row's radius and shrinks
//                        with every admitted candidate; sigma is the header's slack, once per row.  The loop computes distances
//                        only; the winner's point and normal are made after it, by the same operations.  The stack is the query
//                        kernels': [entry][lane] in LDS, deeper entries in the lane's private array.
//                        Left-first order, stack entries that carry their box distance (so that a pop is dropped without a visit
//                        once best has shrunk: two words per entry, half the waves) and unsquared box distances were measured and
//                        lost: section 6o.
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "query_walk.h"
#include "point_query.h"
#include "../../include/mirt_closest.h"

#include <cmath>

namespace mirt {
namespace {

// the query kernels' budget: 64 VGPRs, 8 waves per SIMD; QUERY_STACK_LDS x 4 B x 64 lanes = 5 KiB of LDS per wave
constexpr int CWAVES_PER_SIMD = 8;

struct ClosestArgs {
  const float4* points;           // (q, R)
  uint32_t* hits;                 // MirtHit: 6 words
  float4* features;               // nullable: (P, 1), (n, 0)
  long long n;
  const float4* nodes;            // record heap (scene_dev.h)
  const uint32_t* unit_prim;
  const float4* tri_verts;        // file order: p0, p1, p2 of every triangle
  const PlaneDev* planes; int num_planes;
  uint32_t root_ref;              // the exact records' root (REF_NONE: no primitive)
  uint32_t prim_base16;
  float coord_max;                // largest coordinate magnitude of the scene box
  int lds_depth;                  // stack entries kept in LDS (<= QUERY_STACK_LDS)
};

__global__ void __launch_bounds__(QUERY_BLOCK, CWAVES_PER_SIMD) closest_points_kernel(const ClosestArgs a)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];             // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * QUERY_BLOCK;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(a.nodes);
  const ConstPlanes planes = const_planes(a.planes);
  for (long long i = (long long)blockIdx.x * QUERY_BLOCK + tid; i < a.n; i += stride) {
    const float4 row = a.points[i];
    const f3 q = mk3(row.x, row.y, row.z);
    const float R = row.w;
    // (x - x is 0 for a finite x and NaN for an infinity or a NaN)
    const bool live = R > 0.0f && (q.x - q.x) == 0.0f && (q.y - q.y) == 0.0f && (q.z - q.z) == 0.0f;
    float best = R;                  // the smallest admitted distance so far; without a winner, the radius
    uint32_t refbest = REF_NONE;     // the winner, a primitive record of the heap ...
    int plane_id = -1;               // ... or a plane
    if (live) {
      for (int j = 0; j < a.num_planes; ++j) {
        const f3 N = normalize(mk3(planes[j].nx, planes[j].ny, planes[j].nz));
        const float dist = fabsf(dot(N, q - mk3(planes[j].px, planes[j].py, planes[j].pz)));
        if (dist < best) { best = dist; plane_id = j; }      // (an equal distance: the lower index stays)
      }
    }
    if (live && a.root_ref != REF_NONE) {
      const float sigma = row_sigma(largest_abs(q), a.coord_max);
      float reach = best + sigma;
      float bound2 = reach * reach;      // a box farther than this (squared) holds nothing that wins or ties
      uint32_t cur = a.root_ref;
      int sp = 0;
      for (;;) {
        const float4* rec = reinterpret_cast<const float4*>(heap + (cur << 4));
        bool pop;
        if (cur & REF_LEAF) {
          float dist;
          uint32_t id = 0u;
          if (cur & REF_TRI) {
            id = a.unit_prim[(cur & REF_OFFMASK) - a.prim_base16] & 0x7fffffffu;
            dist = length(q - triangle_point(a.tri_verts, id, q));
          } else {
            const float4 s = rec[0];
            dist = fabsf(length(q - mk3(s.x, s.y, s.z)) - s.w);
          }
          bool better = dist < best;
          // (a tie with the winner: (kind, id) decides)
          if (dist == best && (plane_id >= 0 || refbest != REF_NONE)) better = wins_tie(cur, id, plane_id, refbest, a.unit_prim, a.prim_base16);
          if (better) {
            best = dist; refbest = cur; plane_id = -1;
            reach = best + sigma;
            bound2 = reach * reach;
          }
          pop = true;
        } else {
          const float4 b0 = rec[0], b1 = rec[1], b2 = rec[2];
          const uint2 ch = *reinterpret_cast<const uint2*>(rec + 3);
          const float l2 = box_dist2(b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, q);
          const float r2 = box_dist2(b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, q);
          const bool hl = !(l2 > bound2), hr = !(r2 > bound2);
          const bool right_first = r2 < l2;      // the nearer child first
          if (hl && hr) {
            // (stack_push and stack_pop of query_walk.h, written out: as calls they move this loop's blocks)
            const uint32_t later = right_first ? ch.x : ch.y;
            if (sp < a.lds_depth) lds_stack[sp * QUERY_BLOCK + tid] = later;
            else spill[(sp - a.lds_depth) & (STACK_TOTAL - 1)] = later;
            ++sp;
          }
          cur = (hl && hr) ? (right_first ? ch.y : ch.x) : (hl ? ch.x : ch.y);
          pop = !(hl || hr);
        }
        if (pop) {
          if (sp == 0) break;
          --sp;
          cur = sp < a.lds_depth ? lds_stack[sp * QUERY_BLOCK + tid] : spill[(sp - a.lds_depth) & (STACK_TOTAL - 1)];
        }
      }
    }
    // the winner's record: its point and normal by the header's operations (the loop kept the distance only).  The three formulas
    // are closest_multi.hip's and overlap.hip's, written out here too: through one function they move 938 of this kernel's 1039
    // instruction lines
    float t = -1.0f;
    uint32_t kind = MIRT_HIT_NONE, id = 0u;
    f3 P = mk3(0.0f, 0.0f, 0.0f), n = P;
    const bool hit = plane_id >= 0 || refbest != REF_NONE;
    if (plane_id >= 0) {
      const f3 N = normalize(mk3(planes[plane_id].nx, planes[plane_id].ny, planes[plane_id].nz));
      const float s = dot(N, q - mk3(planes[plane_id].px, planes[plane_id].py, planes[plane_id].pz));
      P = q - N * s;
      n = s < 0.0f ? -N : N;
      kind = MIRT_HIT_PLANE; id = (uint32_t)plane_id;
    } else if (refbest != REF_NONE) {
      id = a.unit_prim[(refbest & REF_OFFMASK) - a.prim_base16] & 0x7fffffffu;
      const float4* rec = a.nodes + (refbest & REF_OFFMASK);
      if (refbest & REF_TRI) {
        const float4 q0 = rec[0], q1 = rec[1];
        const f3 nor = mk3(q0.w, q1.x, q1.y);
        P = triangle_point(a.tri_verts, id, q);
        n = dot(q - P, nor) < 0.0f ? -nor : nor;
        kind = MIRT_HIT_TRIANGLE;
      } else {
        const float4 s = rec[0];
        const f3 c = mk3(s.x, s.y, s.z), v = q - c;
        const f3 u = normalize(v);
        P = c + u * s.w;
        n = length(v) < s.w ? -u : u;
        kind = MIRT_HIT_SPHERE;
      }
    }
    if (hit) t = best;
    // (store_hit of query_walk.h, written out like the stack above: section 6q)
    uint32_t* const h = a.hits + 6 * i;
    h[0] = __float_as_uint(t);
    h[1] = kind;
    h[2] = id;
    h[3] = __float_as_uint(n.x);
    h[4] = __float_as_uint(n.y);
    h[5] = __float_as_uint(n.z);
    if (a.features) {
      a.features[2 * i] = make_float4(P.x, P.y, P.z, hit ? 1.0f : 0.0f);
      a.features[2 * i + 1] = make_float4(n.x, n.y, n.z, 0.0f);
    }
  }
}

} // namespace

int closest_points(MirtScene* sc, const void* d_points, int64_t n, void* d_hits, void* d_features, uint32_t flags, hipStream_t stream)
{
  bool go = false;
  const int rc = check_closest_points(d_points, n, d_hits, d_features, flags, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  ClosestArgs q;
  q.points = reinterpret_cast<const float4*>(d_points);
  q.hits = reinterpret_cast<uint32_t*>(d_hits);
  q.features = reinterpret_cast<float4*>(d_features);
  q.n = n;
  fill_scene_args(q, sc);
  return launch_rows(sc, closest_points_kernel, CWAVES_PER_SIMD, &sc->closest_blocks, n, q, stream);
}

} // namespace mirt
