// Triangle overlap queries on a built scene (include_ext2/mirt_overlap_tris.h): EVERY plane, sphere and
// triangle a caller's triangle touches -- their number per row (mirt_overlap_triangles; with MIRT_TRIS_ANY whether there is one) and
// their words kind << 30 | id in the builder's order (mirt_triangle_list).  The offsets between the two are the overlap lists' scan.
//
// tri_walk                  the shape of overlap_walk.h's walk with the narrow phase of tri_tests.h at the leaves: left child first
//                           (the ORDER of a row's words is the scene's leaf order), a child visited when its box meets the row's
//                           vertex bounds grown by sigma on every axis (negated compares: a NaN visits), the single latch,
//                           stack_push / stack_pop.  The header's clauses (0) and (i) are exact bounds tests, so the pruning
//                           cannot lose a candidate.  What an admitted candidate does is the action's.
// overlap_tris_kernel<ANY>  one lane = one row (grid-stride over the batch): the nine floats loaded once, the planes from scalar
//                           loads, the walk with a counter; ANY ends at the first admitted surface.
// triangle_list_kernel      the same with list_cursor.h's bounded cursor in place of the counter.
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "query_walk.h"
#include "point_query.h"
#include "tri_tests.h"
#include "list_cursor.h"
#include "../../include_ext2/mirt_overlap_tris.h"

#include <cmath>

namespace mirt {
namespace {

// Waves per SIMD the three instances are compiled for: the largest at which the compiler reports no VGPR spill (90 / 90 / 94 VGPRs;
// at 6 waves the count instances spill 8 registers and the fill 42.  DESIGN.md section 6aa has the report).
constexpr int TRIS_WAVES = 5;

struct OverlapTrisArgs {
  const float* tris;              // [n][9]: a, b, c
  uint32_t* counts;               // [n] (the count kernels)
  const long long* offsets;       // [n + 1] (the fill)
  uint32_t* words;                // [capacity]
  long long capacity;
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

// What an admitted candidate does is the caller's action, a struct held by value (the walks return it): act.plane(j) for plane j,
// act.leaf(cur, id) for a sphere or triangle -- cur the leaf's reference, id a triangle's file-order id (a sphere's is a unit_prim
// load the action makes if it wants it); both return whether the row ends there.
// the planes the row meets, in index order
template <class Act>
MIRT_DEV Act tri_planes(ConstPlanes planes, int num_planes, f3 a, f3 b, f3 c, Act act)
{
  for (int j = 0; j < num_planes; ++j) {
    const f3 N = normalize(mk3(planes[j].nx, planes[j].ny, planes[j].nz));
    if (tri_meets_plane(N, mk3(planes[j].px, planes[j].py, planes[j].pz), a, b, c)) {
      if (act.plane((uint32_t)j)) break;
    }
  }
  return act;
}

// The spheres and triangles the row (a, a + ub, a + uc; bounds [lo, hi]) meets, in the scene's leaf order.  root_ref is no REF_NONE.
template <class Act>
MIRT_DEV Act tri_walk(const unsigned char* heap, const uint32_t* unit_prim, const float4* tri_verts, uint32_t prim_base16, uint32_t root_ref,
                       float coord_max, int lds_depth, uint32_t* lds_stack, uint32_t* spill, int tid, f3 lo, f3 hi, f3 a, f3 ub, f3 uc, Act act)
{
  const float sigma = row_sigma(fmaxf(largest_abs(lo), largest_abs(hi)), coord_max);
  uint32_t cur = root_ref;
  int sp = 0;
  for (;;) {
    const float4* rec = reinterpret_cast<const float4*>(heap + (cur << 4));
    bool pop;
    if (cur & REF_LEAF) {
      uint32_t id = 0u;
      bool pass;
      if (cur & REF_TRI) {
        id = unit_prim[(cur & REF_OFFMASK) - prim_base16] & 0x7fffffffu;
        const float4* v = tri_verts + 3 * (size_t)id;
        const float4 pa = v[0], pb = v[1], pc = v[2];
        pass = tri_meets_triangle(lo, hi, a, ub, uc, mk3(pa.x, pa.y, pa.z), mk3(pb.x, pb.y, pb.z), mk3(pc.x, pc.y, pc.z));
      } else {
        const float4 s = rec[0];
        pass = tri_meets_sphere(lo, hi, a, ub, uc, mk3(s.x, s.y, s.z), s.w);
      }
      if (pass) {
        if (act.leaf(cur, id)) break;
      }
      pop = true;
    } else {
      const float4 b0 = rec[0], b1 = rec[1], b2 = rec[2];
      const uint2 ch = *reinterpret_cast<const uint2*>(rec + 3);
      // hi + sigma and lo - sigma are made here, from a copy of sigma the compiler cannot see through: hoisted out of the walk
      // they are six registers held across every leaf's test (as in overlap_walk.h)
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
    // one latch for every path (an empty statement the compiler may not duplicate; it emits nothing): overlap_walk.h says why
    asm volatile("");
  }
  return act;
}

// the count: every admitted candidate is one more; ANY: the first ends the row
template <bool ANY>
struct Counter {
  uint32_t count;
  MIRT_DEV bool plane(uint32_t) { ++count; return ANY; }
  MIRT_DEV bool leaf(uint32_t, uint32_t) { ++count; return ANY; }
};

// the fill: an admitted candidate's word goes to the row's cursor while its segment has room (list_cursor.h)
struct TriCursor {
  uint32_t* out; uint32_t room;
  const uint32_t* unit_prim; uint32_t prim_base16;
  MIRT_DEV void emit(uint32_t word)
  {
    if (room) { *out++ = word; --room; }
  }
  MIRT_DEV bool plane(uint32_t j) { emit(((uint32_t)MIRT_HIT_PLANE << 30) | j); return false; }
  MIRT_DEV bool leaf(uint32_t cur, uint32_t id)
  {
    if (!(cur & REF_TRI)) id = unit_prim[(cur & REF_OFFMASK) - prim_base16] & 0x7fffffffu;
    emit(((cur & REF_TRI) ? ((uint32_t)MIRT_HIT_TRIANGLE << 30) : ((uint32_t)MIRT_HIT_SPHERE << 30)) | id);
    return false;
  }
};

template <bool ANY>
__global__ void __launch_bounds__(QUERY_BLOCK, TRIS_WAVES) overlap_tris_kernel(const OverlapTrisArgs q)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];             // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * QUERY_BLOCK;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(q.nodes);
  const ConstPlanes planes = const_planes(q.planes);
  for (long long i = (long long)blockIdx.x * QUERY_BLOCK + tid; i < q.n; i += stride) {
    const TriRow t = tri_row(q.tris, i);
    Counter<ANY> at;
    at.count = 0u;
    if (t.live) {
      at = tri_planes(planes, q.num_planes, t.a, t.b, t.c, at);
      if (q.root_ref != REF_NONE && !(ANY && at.count != 0u)) {
        at = tri_walk(heap, q.unit_prim, q.tri_verts, q.prim_base16, q.root_ref, q.coord_max, q.lds_depth, lds_stack, spill, tid, t.lo, t.hi, t.a,
                      t.b - t.a, t.c - t.a, at);
      }
    }
    q.counts[i] = at.count;      // (a dead row: 0; ANY: the first admitted candidate ended the row at 1)
  }
}

__global__ void __launch_bounds__(QUERY_BLOCK, TRIS_WAVES) triangle_list_kernel(const OverlapTrisArgs q)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];             // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * QUERY_BLOCK;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(q.nodes);
  const ConstPlanes planes = const_planes(q.planes);
  for (long long i = (long long)blockIdx.x * QUERY_BLOCK + tid; i < q.n; i += stride) {
    const TriRow t = tri_row(q.tris, i);
    if (!t.live) continue;           // (a dead row writes nothing)
    const ListRoom r = list_room(q.offsets, q.capacity, i);
    TriCursor at;
    at.room = r.room;
    at.out = q.words + r.beg;
    at.unit_prim = q.unit_prim; at.prim_base16 = q.prim_base16;
    at = tri_planes(planes, q.num_planes, t.a, t.b, t.c, at);
    if (q.root_ref == REF_NONE) continue;
    tri_walk(heap, q.unit_prim, q.tri_verts, q.prim_base16, q.root_ref, q.coord_max, q.lds_depth, lds_stack, spill, tid, t.lo, t.hi, t.a, t.b - t.a,
             t.c - t.a, at);
  }
}

} // namespace

int overlap_triangles(MirtScene* sc, const void* d_tris, int64_t n, uint32_t* d_counts, uint32_t flags, hipStream_t stream)
{
  bool go = false;
  const int rc = check_overlap_triangles(d_tris, n, d_counts, flags, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  OverlapTrisArgs q;
  q.tris = reinterpret_cast<const float*>(d_tris);
  q.counts = d_counts;
  q.offsets = nullptr; q.words = nullptr; q.capacity = 0;
  q.n = n;
  fill_scene_args(q, sc);
  if (flags & MIRT_TRIS_ANY) return launch_rows(sc, overlap_tris_kernel<true>, TRIS_WAVES, &sc->overlap_tris_blocks[1], n, q, stream);
  return launch_rows(sc, overlap_tris_kernel<false>, TRIS_WAVES, &sc->overlap_tris_blocks[0], n, q, stream);
}

int triangle_list(MirtScene* sc, const void* d_tris, int64_t n, const int64_t* d_offsets, uint32_t* d_words, int64_t capacity, hipStream_t stream)
{
  bool go = false;
  const int rc = check_triangle_list(d_tris, n, d_offsets, d_words, capacity, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  OverlapTrisArgs q;
  q.tris = reinterpret_cast<const float*>(d_tris);
  q.counts = nullptr;
  q.offsets = reinterpret_cast<const long long*>(d_offsets);
  q.words = d_words;
  q.capacity = capacity;
  q.n = n;
  fill_scene_args(q, sc);
  return launch_rows(sc, triangle_list_kernel, TRIS_WAVES, &sc->overlap_tris_blocks[2], n, q, stream);
}

} // namespace mirt
