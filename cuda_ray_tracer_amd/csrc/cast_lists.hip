// Cast lists on a built scene (include_ext3/mirt_cast_lists.h): EVERY surface a moving ball touches along its
// path -- their number per row (mirt_cast_counts) and their words kind << 30 | id in the builder's order, with the contact
// parameter t of each if asked for (mirt_cast_list).  The offsets between the two are the overlap lists' scan.  Like the other
// queries they read the scene only and touch no render context, counter, hand-out table or RNG table.
//
// cast_row                  one row's walk, inlined into the three kernels: the planes from scalar loads, then the stack walk of
//                           sphere_cast_kernel (spherecast.hip) over the exact 64-byte records -- box_interval of both children,
//                           grown by r + sigma -- with what a list needs and a first contact does not: the bound is the row's
//                           tmax + tmax * TAU from the first box to the last, so the same subtrees are left out whichever child
//                           comes first; the LEFT child is visited first, which makes the order of a row the scene's leaf order;
//                           there is no winner and no tie state.  A leaf's t comes from cast_tests.h, the functions of the cast
//                           kernel, and is admitted when 0 <= t < tmax.  A leaf reached through its parent has passed the header's
//                           clause (0) on its own box there; a root that is a leaf has no box and is visited untested, as the
//                           header says.  The stack is the query kernels': [entry][lane] in LDS, deeper entries in the lane's
//                           private array.
// cast_count_kernel         one lane = one row (grid-stride over the batch); an admitted candidate adds one.
// cast_list_kernel<VALUES>  the same with list_cursor.h's bounded cursor in place of the counter.  A value goes to the word's index
//                           of the value array: its address is the word's plus the distance between the two arrays, the same for
//                           every lane.  VALUES is a template parameter, not a null test at each word (section 6z says why).
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "query_walk.h"
#include "point_query.h"
#include "cast_tests.h"
#include "list_cursor.h"
#include "../../include_ext3/mirt_cast_lists.h"

#include <cmath>

namespace mirt {
namespace {

// Waves per SIMD the instances are compiled for (DESIGN.md section 6ab has the compiler's report).
constexpr int CAST_LIST_WAVES = 5;

struct CastListArgs {
  const float4* casts;            // (o, tmax), (d, r)
  uint32_t* counts;               // [n] (the count kernel)
  const long long* offsets;       // [n + 1] (the fill kernels)
  uint32_t* words;                // [capacity]
  long long value_delta;          // bytes from words to the value array (the VALUES instance)
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

// the row rule of mirt_spherecast.h: the ball, its tmax, and whether the row is live
MIRT_DEV bool cast_row_of(const CastListArgs& a, long long i, Ball& k, float& tmax)
{
  const float4 r0 = a.casts[2 * i], r1 = a.casts[2 * i + 1];
  k.o = mk3(r0.x, r0.y, r0.z);
  k.d = normalize(mk3(r1.x, r1.y, r1.z));
  k.r = r1.w;
  tmax = r0.w;
  // (x - x is 0 for a finite x and NaN for an infinity or a NaN)
  return ray_is_live(tmax, k.d) && k.r >= 0.0f && (k.r - k.r) == 0.0f && finite3(r0);
}

// A live row's set in the header's order: emit(word, t) for every member, as it is met.
template <class E>
MIRT_DEV void cast_row(const CastListArgs& a, const Ball& k, float tmax, uint32_t* lds_stack, uint32_t* spill, int tid, E& emit)
{
  const ConstPlanes planes = const_planes(a.planes);
  for (int j = 0; j < a.num_planes; ++j) {
    const f3 N = normalize(mk3(planes[j].nx, planes[j].ny, planes[j].nz));
    const float t = plane_cast(N, mk3(planes[j].px, planes[j].py, planes[j].pz), k);
    if (t >= 0.0f && t < tmax) emit(((uint32_t)MIRT_HIT_PLANE << 30) | (uint32_t)j, t);
  }
  if (a.root_ref == REF_NONE) return;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(a.nodes);
  const f3 inv = mk3(1.0f / k.d.x, 1.0f / k.d.y, 1.0f / k.d.z);
  const float sigma = row_sigma(largest_abs(k.o), a.coord_max, k.r);
  const float grow = k.r + sigma;
  const float bound = tmax + tmax * TAU;   // the row's, from the first box to the last: a box entered later holds no member
  uint32_t cur = a.root_ref;
  int sp = 0;
  for (;;) {
    const float4* rec = reinterpret_cast<const float4*>(heap + (cur << 4));
    bool pop;
    if (cur & REF_LEAF) {
      float t;
      uint32_t id = 0u;
      if (cur & REF_TRI) {
        id = a.unit_prim[(cur & REF_OFFMASK) - a.prim_base16] & 0x7fffffffu;
        const float4* v = a.tri_verts + 3 * (size_t)id;
        const float4 va = v[0], vb = v[1], vc = v[2];
        const float4 q0 = rec[0], q1 = rec[1];
        t = triangle_cast(mk3(va.x, va.y, va.z), mk3(vb.x, vb.y, vb.z), mk3(vc.x, vc.y, vc.z), mk3(q0.w, q1.x, q1.y), k);
      } else {
        t = sphere_cast(rec[0], k);
      }
      if (t >= 0.0f && t < tmax) {
        // (a triangle's id is loaded anyway: its vertices are in file order; a sphere's for an admitted sphere only)
        if (!(cur & REF_TRI)) id = a.unit_prim[(cur & REF_OFFMASK) - a.prim_base16] & 0x7fffffffu;
        emit(((cur & REF_TRI) ? ((uint32_t)MIRT_HIT_TRIANGLE << 30) : ((uint32_t)MIRT_HIT_SPHERE << 30)) | id, t);
      }
      pop = true;
    } else {
      const float4 b0 = rec[0], b1 = rec[1], b2 = rec[2];
      const uint2 ch = *reinterpret_cast<const uint2*>(rec + 3);
      float el, ll, er, lr;
      box_interval(b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, k.o, inv, grow, el, ll);
      box_interval(b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, k.o, inv, grow, er, lr);
      const bool hl = !(el > fminf(ll, bound)), hr = !(er > fminf(lr, bound));
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

struct CountEmit {
  uint32_t count;
  MIRT_DEV void operator()(uint32_t, float) { ++count; }
};

// A row's cursor: where its next word goes and how many more its segment takes (list_room).  An admitted surface's word goes to
// the cursor, its value to the same index of the value array.
template <bool VALUES>
struct ListEmit {
  uint32_t* out; uint32_t room; long long value_delta;
  MIRT_DEV void operator()(uint32_t word, float t)
  {
    if (room) {
      *out = word;
      if (VALUES) *reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(out) + value_delta) = t;
      ++out; --room;
    }
  }
};

__global__ void __launch_bounds__(QUERY_BLOCK, CAST_LIST_WAVES) cast_count_kernel(const CastListArgs a)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];             // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * QUERY_BLOCK;
  for (long long i = (long long)blockIdx.x * QUERY_BLOCK + tid; i < a.n; i += stride) {
    Ball k;
    float tmax;
    CountEmit emit;
    emit.count = 0u;
    if (cast_row_of(a, i, k, tmax)) cast_row(a, k, tmax, lds_stack, spill, tid, emit);
    a.counts[i] = emit.count;
  }
}

template <bool VALUES>
__global__ void __launch_bounds__(QUERY_BLOCK, CAST_LIST_WAVES) cast_list_kernel(const CastListArgs a)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];             // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * QUERY_BLOCK;
  for (long long i = (long long)blockIdx.x * QUERY_BLOCK + tid; i < a.n; i += stride) {
    Ball k;
    float tmax;
    if (!cast_row_of(a, i, k, tmax)) continue;      // (a dead row writes nothing and does not read its offsets)
    const ListRoom r = list_room(a.offsets, a.capacity, i);
    ListEmit<VALUES> emit;
    emit.out = a.words + r.beg;
    emit.room = r.room;
    emit.value_delta = a.value_delta;
    cast_row(a, k, tmax, lds_stack, spill, tid, emit);
  }
}

} // namespace

int cast_counts(MirtScene* sc, const void* d_casts, int64_t n, uint32_t* d_counts, uint32_t flags, hipStream_t stream)
{
  bool go = false;
  const int rc = check_cast_counts(d_casts, n, d_counts, flags, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  CastListArgs q;
  q.casts = reinterpret_cast<const float4*>(d_casts);
  q.counts = d_counts;
  q.offsets = nullptr; q.words = nullptr; q.value_delta = 0; q.capacity = 0;
  q.n = n;
  fill_scene_args(q, sc);
  return launch_rows(sc, cast_count_kernel, CAST_LIST_WAVES, &sc->cast_list_blocks[0], n, q, stream);
}

int cast_list(MirtScene* sc, const void* d_casts, int64_t n, const int64_t* d_offsets, uint32_t* d_words, float* d_t, int64_t capacity, uint32_t flags,
              hipStream_t stream)
{
  bool go = false;
  const int rc = check_cast_list(d_casts, n, d_offsets, d_words, d_t, capacity, flags, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  CastListArgs q;
  q.casts = reinterpret_cast<const float4*>(d_casts);
  q.counts = nullptr;
  q.offsets = reinterpret_cast<const long long*>(d_offsets);
  q.words = d_words;
  q.value_delta = d_t ? (long long)((intptr_t)d_t - (intptr_t)d_words) : 0;
  q.capacity = capacity;
  q.n = n;
  fill_scene_args(q, sc);
  if (d_t) return launch_rows(sc, cast_list_kernel<true>, CAST_LIST_WAVES, &sc->cast_list_blocks[2], n, q, stream);
  return launch_rows(sc, cast_list_kernel<false>, CAST_LIST_WAVES, &sc->cast_list_blocks[1], n, q, stream);
}

} // namespace mirt
