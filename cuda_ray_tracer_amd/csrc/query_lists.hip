// Ray and ball lists on a built scene (include_ext/mirt_query_lists.h): EVERY surface a ray crosses or a ball
// touches, as words kind << 30 | id (and, if asked for, the t or dist of each) into the segments of offsets the caller made -- the
// fill steps of count (the count-only call of mirt_multihit.h / mirt_contacts.h), exclusive scan (the overlap-list extension's
// offsets call), fill.
//
// ray_list_kernel<VALUES>   the loop of multihit_kernel<0> (multihit.hip), written out here: the planes through scalar loads, the
//                           walk over the exact records with box_pair at tmax, left child first, triangle_hit / sphere_hit and the
//                           1e-6 < t < tmax admission -- with a write cursor in place of the counter.  The bound never shrinks, so
//                           the set does not depend on the visiting order; left child first makes the ORDER of a row the scene's
//                           leaf order.
// ball_list_kernel<VALUES>  the count-mode walk of contacts_kernel<0> (closest_multi.hip), written out here: the planes, then the
//                           squared point-box distance of both children against (R + sigma)^2 -- the bound is the row's radius for
//                           the whole walk, so the same subtrees are pruned whichever child comes first -- with the LEFT child
//                           first instead of the nearer one, and the cursor in place of the counter.
// Both walks are copies and not calls of one function with the kernels they come from: folding those loops into shared functions
// moved the existing kernels and cost them their speed (section 6y), and they stay byte for byte what they were.
//
// The cursor a lane carries across the walk is a pointer to the row's next word and the room left in its segment (list_cursor.h:
// the rule of overlap_list.hip's fill), read once per row by a live row only.  A value goes to the word's index of the value
// array: its address is the word's plus the distance between the two arrays, the same for every lane (a scalar), so the cursor of
// the instance with values is no wider.  VALUES is a template parameter, not a null test at each word: section 6z has the
// compiler's report of both instances.  A sphere's id is a unit_prim load for every admitted sphere.
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "query_walk.h"
#include "point_query.h"
#include "list_cursor.h"
#include "../../include_ext/mirt_query_lists.h"

#include <cmath>

namespace mirt {
namespace {

// Waves per SIMD the instances are compiled for (section 6z has the compiler's report).
constexpr int RAY_LIST_WAVES = 8;
constexpr int BALL_LIST_WAVES = 8;

struct QueryListArgs {
  const float4* rows;             // rays: MirtRay (o, tmax), (d, pad); balls: (q, R)
  const long long* offsets;       // [n + 1]
  uint32_t* words;                // [capacity]
  long long value_delta;          // bytes from words to the value array (VALUES instances)
  long long capacity;
  long long n;
  const float4* nodes;            // record heap (scene_dev.h)
  const uint32_t* unit_prim;
  const float4* tri_verts;        // file order: p0, p1, p2 of every triangle (balls)
  const PlaneDev* planes; int num_planes;
  uint32_t root_ref;              // the exact records' root (REF_NONE: no primitive)
  uint32_t prim_base16;
  float coord_max;                // largest coordinate magnitude of the scene box (balls)
  int lds_depth;                  // stack entries kept in LDS (<= QUERY_STACK_LDS)
};

// A row's cursor: where its next word goes and how many more its segment takes (list_room).  An admitted surface's word goes to
// the cursor, its value to the same index of the value array.
template <bool VALUES>
struct ValueCursor {
  uint32_t* out; uint32_t room;
  MIRT_DEV void emit(uint32_t word, float value, long long value_delta)
  {
    if (room) {
      *out = word;
      if (VALUES) *reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(out) + value_delta) = value;
      ++out; --room;
    }
  }
};
template <bool VALUES>
MIRT_DEV ValueCursor<VALUES> row_cursor(const QueryListArgs& a, long long i)
{
  const ListRoom r = list_room(a.offsets, a.capacity, i);
  ValueCursor<VALUES> c;
  c.room = r.room;
  c.out = a.words + r.beg;
  return c;
}
MIRT_DEV uint32_t prim_word(const QueryListArgs& a, uint32_t cur)
{
  const uint32_t id = a.unit_prim[(cur & REF_OFFMASK) - a.prim_base16] & 0x7fffffffu;
  return ((cur & REF_TRI) ? ((uint32_t)MIRT_HIT_TRIANGLE << 30) : ((uint32_t)MIRT_HIT_SPHERE << 30)) | id;
}

template <bool VALUES>
__global__ void __launch_bounds__(QUERY_BLOCK, RAY_LIST_WAVES) ray_list_kernel(const QueryListArgs q)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];                     // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * QUERY_BLOCK;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(q.nodes);
  const ConstPlanes planes = const_planes(q.planes);
  const float tmin = 0.0001f;
  for (long long i = (long long)blockIdx.x * QUERY_BLOCK + tid; i < q.n; i += stride) {
    const float4 r0 = q.rows[2 * i], r1 = q.rows[2 * i + 1];
    const f3 o = mk3(r0.x, r0.y, r0.z);
    const float tmax = r0.w;
    const f3 d = normalize(mk3(r1.x, r1.y, r1.z));      // Ray(eye, dir, bounce), object.cuh:69
    if (!ray_is_live(tmax, d)) continue;                // (a dead row writes nothing and does not read its offsets)
    ValueCursor<VALUES> at = row_cursor<VALUES>(q, i);
    // multihit_kernel<0>'s plane loop (multihit.hip): checkPlane, the bound being tmax
    for (int j = 0; j < q.num_planes; ++j) {
      const f3 pnor = mk3(planes[j].nx, planes[j].ny, planes[j].nz);
      const float t = dot(mk3(planes[j].px, planes[j].py, planes[j].pz) - o, pnor) / dot(d, pnor);
      if (!(t <= 1e-6f) && t > EPSILON && t < (float)(INT_MAX - 10) && t < tmax) at.emit(((uint32_t)MIRT_HIT_PLANE << 30) | (uint32_t)j, t, q.value_delta);
    }
    if (q.root_ref == REF_NONE) continue;
    // multihit_kernel<0>'s walk (multihit.hip), the cursor in place of the counter
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
        if (hit && t > 1e-6f && t < tmax) at.emit(prim_word(q, cur), t, q.value_delta);
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
}

template <bool VALUES>
__global__ void __launch_bounds__(QUERY_BLOCK, BALL_LIST_WAVES) ball_list_kernel(const QueryListArgs a)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];             // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * QUERY_BLOCK;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(a.nodes);
  const ConstPlanes planes = const_planes(a.planes);
  for (long long i = (long long)blockIdx.x * QUERY_BLOCK + tid; i < a.n; i += stride) {
    const float4 row = a.rows[i];
    const f3 q = mk3(row.x, row.y, row.z);
    const float R = row.w;
    // (x - x is 0 for a finite x and NaN for an infinity or a NaN)
    const bool live = R > 0.0f && (q.x - q.x) == 0.0f && (q.y - q.y) == 0.0f && (q.z - q.z) == 0.0f;
    if (!live) continue;                   // (a dead row writes nothing and does not read its offsets)
    ValueCursor<VALUES> at = row_cursor<VALUES>(a, i);
    // contacts_kernel<0>'s plane loop (closest_multi.hip)
    for (int j = 0; j < a.num_planes; ++j) {
      const f3 N = normalize(mk3(planes[j].nx, planes[j].ny, planes[j].nz));
      const float dist = fabsf(dot(N, q - mk3(planes[j].px, planes[j].py, planes[j].pz)));
      if (dist < R) at.emit(((uint32_t)MIRT_HIT_PLANE << 30) | (uint32_t)j, dist, a.value_delta);
    }
    if (a.root_ref == REF_NONE) continue;
    // contacts_kernel<0>'s walk in count mode (closest_multi.hip) -- the bound is R from the first box to the last -- with the
    // left child first instead of the nearer one, and the cursor in place of the counter
    const float sigma = row_sigma(largest_abs(q), a.coord_max);
    const float reach = R + sigma;
    const float bound2 = reach * reach;      // a box farther than this (squared) holds nothing nearer than R
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
        if (dist < R) {
          // (a triangle's id is loaded anyway: its vertices are in file order; a sphere's for an admitted sphere only)
          if (!(cur & REF_TRI)) id = a.unit_prim[(cur & REF_OFFMASK) - a.prim_base16] & 0x7fffffffu;
          at.emit(((cur & REF_TRI) ? ((uint32_t)MIRT_HIT_TRIANGLE << 30) : ((uint32_t)MIRT_HIT_SPHERE << 30)) | id, dist, a.value_delta);
        }
        pop = true;
      } else {
        const float4 b0 = rec[0], b1 = rec[1], b2 = rec[2];
        const uint2 ch = *reinterpret_cast<const uint2*>(rec + 3);
        const float l2 = box_dist2(b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, q);
        const float r2 = box_dist2(b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, q);
        const bool hl = !(l2 > bound2), hr = !(r2 > bound2);
        if (hl && hr) stack_push(lds_stack, spill, a.lds_depth, tid, sp, ch.y);
        cur = hl ? ch.x : ch.y;
        pop = !(hl || hr);
      }
      if (pop) {
        if (sp == 0) break;
        cur = stack_pop(lds_stack, spill, a.lds_depth, tid, sp);
      }
    }
  }
}

void fill_list_args(QueryListArgs& q, const MirtScene* sc, const void* d_rows, int64_t n, const int64_t* d_offsets, uint32_t* d_words, const float* d_values,
                    int64_t capacity)
{
  q.rows = reinterpret_cast<const float4*>(d_rows);
  q.offsets = reinterpret_cast<const long long*>(d_offsets);
  q.words = d_words;
  q.value_delta = d_values ? (long long)((intptr_t)d_values - (intptr_t)d_words) : 0;
  q.capacity = capacity;
  q.n = n;
  fill_scene_args(q, sc);
}

} // namespace

int ray_list(MirtScene* sc, const void* d_rays, int64_t num_rays, const int64_t* d_offsets, uint32_t* d_words, float* d_t, int64_t capacity, uint32_t flags,
             hipStream_t stream)
{
  bool go = false;
  const int rc = check_ray_list(d_rays, num_rays, d_offsets, d_words, d_t, capacity, flags, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  QueryListArgs q;
  fill_list_args(q, sc, d_rays, num_rays, d_offsets, d_words, d_t, capacity);
  if (d_t) return launch_rows(sc, ray_list_kernel<true>, RAY_LIST_WAVES, &sc->ray_list_blocks[1], num_rays, q, stream);
  return launch_rows(sc, ray_list_kernel<false>, RAY_LIST_WAVES, &sc->ray_list_blocks[0], num_rays, q, stream);
}

int ball_list(MirtScene* sc, const void* d_points, int64_t n, const int64_t* d_offsets, uint32_t* d_words, float* d_dist, int64_t capacity, uint32_t flags,
              hipStream_t stream)
{
  bool go = false;
  const int rc = check_ball_list(d_points, n, d_offsets, d_words, d_dist, capacity, flags, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  QueryListArgs q;
  fill_list_args(q, sc, d_points, n, d_offsets, d_words, d_dist, capacity);
  if (d_dist) return launch_rows(sc, ball_list_kernel<true>, BALL_LIST_WAVES, &sc->ball_list_blocks[1], n, q, stream);
  return launch_rows(sc, ball_list_kernel<false>, BALL_LIST_WAVES, &sc->ball_list_blocks[0], n, q, stream);
}

} // namespace mirt
