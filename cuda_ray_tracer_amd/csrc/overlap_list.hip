// Overlap lists on a built scene (include_ext/mirt_overlap_list.h): EVERY surface a box touches, as offsets
// and one array of words -- count (the count-only call of mirt_overlap.h), exclusive scan (mirt_list_offsets), fill
// (mirt_overlap_list).
//
// offsets_kernel<WRITE>     the LBVH build's placement scan (tri_scan_kernel / scan_sums_kernel, lbvh_build.hip) over 64-bit sums:
// offset_sums_kernel        a block's LIST_TILE counts summed per thread and scanned over the block (block_scan.h); the block
//                           totals scanned by one block that loops over them with a carry; then every block again, writing
//                           offsets[j] for its counts and, the block of the last count, offsets[n].  A batch of one tile is the
//                           third launch alone.  Sums of the counts in index order: no order of arrival is observable.
// overlap_list_kernel       overlap.hip's walk (overlap_walk.h: the planes from scalar loads, the stack walk over the exact
//                           records, left child first, sigma, the leaf tests of overlap_tests.h and the dist == dist admission)
//                           with a write cursor in place of the counter.  Left child first is what the ORDER of a
//                           row's words depends on: it is the scene's leaf order.  The cursor a lane carries across the walk is
//                           a pointer to the row's next word and the room left in its segment [offsets[i], min(offsets[i + 1],
//                           capacity)), read once per row: three registers where the count-only kernel has one, and still that
//                           instance's 80 VGPRs and 6 waves per SIMD (section 6x has the compiler's report, and the measured
//                           alternative that reads the segment again at each word).  A word is stored only while there is
//                           room: offsets from other counts truncate a row, they never move a store outside [0, capacity).
//                           A sphere's id is a unit_prim load for every admitted sphere.
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "query_walk.h"
#include "point_query.h"
#include "block_scan.h"
#include "overlap_walk.h"
#include "list_cursor.h"
#include "../../include_ext/mirt_overlap_list.h"

#include <cmath>

namespace mirt {
namespace {

// ---- the offsets ---------------------------------------------------------------------------------------------------------------------
constexpr int LIST_BLOCK = 256;
constexpr int LIST_ITEMS = 8, LIST_TILE = LIST_BLOCK * LIST_ITEMS;      // counts per workgroup
typedef unsigned long long u64;

inline long long list_blocks(long long n) { return (n + LIST_TILE - 1) / LIST_TILE; }

// WRITE false: block b's total into sums[b].  WRITE true: the offsets, each block starting from sums[b] (null: one block, from 0).
template <bool WRITE>
__global__ void __launch_bounds__(LIST_BLOCK) offsets_kernel(long long n, const uint32_t* __restrict__ counts, u64* __restrict__ sums,
                                                             long long* __restrict__ offsets)
{
  __shared__ u64 sh[LIST_BLOCK];
  const long long base = (long long)blockIdx.x * LIST_TILE + (long long)threadIdx.x * LIST_ITEMS;
  uint32_t c[LIST_ITEMS];
  u64 s = 0;
#pragma unroll
  for (int k = 0; k < LIST_ITEMS; ++k) {
    c[k] = (base + k < n) ? counts[base + k] : 0u;
    s += c[k];
  }
  u64 total;
  u64 run = block_exclusive_scan<LIST_BLOCK>(s, sh, &total);
  if (!WRITE) { if (threadIdx.x == 0) sums[blockIdx.x] = total; return; }
  if (sums) run += sums[blockIdx.x];            // exclusive prefix of the blocks before this one
#pragma unroll
  for (int k = 0; k < LIST_ITEMS; ++k) {
    const long long j = base + k;
    if (j < n) offsets[j] = (long long)run;
    run += c[k];
    if (j == n - 1) offsets[n] = (long long)run;
  }
}

// one block: sums -> exclusive prefix, in place (any number of them: the loop carries)
__global__ void __launch_bounds__(LIST_BLOCK) offset_sums_kernel(u64* __restrict__ sums, long long nb)
{
  __shared__ u64 sh[LIST_BLOCK];
  u64 carry = 0;
  for (long long b0 = 0; b0 < nb; b0 += LIST_BLOCK) {
    const long long i = b0 + threadIdx.x;
    const u64 v = (i < nb) ? sums[i] : 0ull;
    u64 total;
    const u64 ex = block_exclusive_scan<LIST_BLOCK>(v, sh, &total);
    if (i < nb) sums[i] = carry + ex;
    carry += total;
  }
}

// ---- the fill ------------------------------------------------------------------------------------------------------------------------
constexpr int LIST_WAVES = 6;      // (waves per SIMD: the count-only instance's, overlap.hip)

struct OverlapListArgs {
  const float4* boxes;            // (lo, _) (hi, _)
  const long long* offsets;       // [n + 1]
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

// A row's cursor: where its next word goes and how many more its segment takes (list_cursor.h's list_room: the rule the ray and
// ball fills of query_lists.hip share).
// It is the walk's action (overlap_walk.h): an admitted candidate's word kind << 30 | id goes to the cursor.
struct Cursor {
  uint32_t* out; uint32_t room;
  const uint32_t* unit_prim; uint32_t prim_base16;
  MIRT_DEV void emit(uint32_t word)
  {
    if (room) { *out++ = word; --room; }
  }
  MIRT_DEV void plane(float, uint32_t j) { emit(((uint32_t)MIRT_HIT_PLANE << 30) | j); }
  MIRT_DEV bool leaf(float, uint32_t cur, uint32_t id)
  {
    if (!(cur & REF_TRI)) id = unit_prim[(cur & REF_OFFMASK) - prim_base16] & 0x7fffffffu;
    emit(((cur & REF_TRI) ? ((uint32_t)MIRT_HIT_TRIANGLE << 30) : ((uint32_t)MIRT_HIT_SPHERE << 30)) | id);
    return false;
  }
};
MIRT_DEV Cursor row_cursor(const OverlapListArgs& a, long long i)
{
  const ListRoom r = list_room(a.offsets, a.capacity, i);
  Cursor c;
  c.room = r.room;
  c.out = a.words + r.beg;
  c.unit_prim = a.unit_prim; c.prim_base16 = a.prim_base16;
  return c;
}

__global__ void __launch_bounds__(QUERY_BLOCK, LIST_WAVES) overlap_list_kernel(const OverlapListArgs a)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];             // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * QUERY_BLOCK;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(a.nodes);
  const ConstPlanes planes = const_planes(a.planes);
  for (long long i = (long long)blockIdx.x * QUERY_BLOCK + tid; i < a.n; i += stride) {
    const BoxRow b = box_row(a.boxes, i);
    if (!b.live) continue;           // (a dead row writes nothing)
    Cursor at = row_cursor(a, i);
    at =overlap_planes(planes, a.num_planes, b.m, b.h, at);
    if (a.root_ref == REF_NONE) continue;
    overlap_walk(heap, a.unit_prim, a.tri_verts, a.prim_base16, a.root_ref, a.coord_max, a.lds_depth, lds_stack, spill, tid, b.lo, b.hi, b.m, b.h, at);
  }
}

} // namespace

int64_t list_offsets_work_bytes(int64_t n)
{
  return n > LIST_TILE ? (int64_t)sizeof(u64) * list_blocks(n) : 0;
}

int list_offsets(MirtScene* sc, const uint32_t* d_counts, int64_t n, int64_t* d_offsets, void* d_work, hipStream_t stream)
{
  (void)sc;      // (the device and the error conventions: api.hip has made the device current)
  // (a count the checks refuse has no work bytes: nothing is computed from it)
  const size_t work = (n >= 0 && n <= (1ll << 40)) ? (size_t)list_offsets_work_bytes(n) : 0;
  bool go = false;
  const int rc = check_list_offsets(d_counts, n, d_offsets, d_work, work, &go);
  if (rc != MIRT_OK) return rc;
  long long* const offsets = reinterpret_cast<long long*>(d_offsets);
  if (!go) { MIRT_HIP(hipMemsetAsync(d_offsets, 0, sizeof(int64_t), stream)); return MIRT_OK; }      // (n == 0: the total alone)
  const long long nb = list_blocks(n);
  u64* const sums = work ? reinterpret_cast<u64*>(d_work) : nullptr;
  if (sums) {
    hipLaunchKernelGGL(offsets_kernel<false>, dim3((unsigned)nb), dim3(LIST_BLOCK), 0, stream, (long long)n, d_counts, sums, offsets);
    hipLaunchKernelGGL(offset_sums_kernel, dim3(1), dim3(LIST_BLOCK), 0, stream, sums, nb);
  }
  hipLaunchKernelGGL(offsets_kernel<true>, dim3((unsigned)nb), dim3(LIST_BLOCK), 0, stream, (long long)n, d_counts, sums, offsets);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

int overlap_list(MirtScene* sc, const void* d_boxes, int64_t n, const int64_t* d_offsets, uint32_t* d_words, int64_t capacity, hipStream_t stream)
{
  bool go = false;
  const int rc = check_overlap_list(d_boxes, n, d_offsets, d_words, capacity, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  OverlapListArgs q;
  q.boxes = reinterpret_cast<const float4*>(d_boxes);
  q.offsets = reinterpret_cast<const long long*>(d_offsets);
  q.words = d_words;
  q.capacity = capacity;
  q.n = n;
  fill_scene_args(q, sc);
  return launch_rows(sc, overlap_list_kernel, LIST_WAVES, &sc->overlap_list_blocks, n, q, stream);
}

} // namespace mirt
