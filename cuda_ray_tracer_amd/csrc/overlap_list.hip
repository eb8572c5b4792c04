// Overlap lists on a built scene (include_ext/mirt_overlap_list.h): EVERY surface a box touches, as offsets
// and one array of words -- count (the count-only call of mirt_overlap.h), exclusive scan (mirt_list_offsets), fill
// (mirt_overlap_list).
//
// offsets_kernel<WRITE>     the LBVH build's placement scan (tri_scan_kernel / scan_sums_kernel, lbvh_build.hip) over 64-bit sums:
// offset_sums_kernel        a block's LIST_TILE counts summed per thread and scanned over the block (block_scan.h); the block
//                           totals scanned by one block that loops over them with a carry; then every block again, writing
//                           offsets[j] for its counts and, the block of the last count, offsets[n].  A batch of one tile is the
//                           third launch alone.  Sums of the counts in index order: no order of arrival is observable.
// overlap_list_kernel       overlap.hip's count-only walk -- the planes from scalar loads, the stack walk over the exact records,
//                           left child first, the same sigma, stack and leaf tests (overlap_tests.h) and the same dist == dist
//                           admission -- with a write cursor in place of the counter.  Left child first is what the ORDER of a
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
#include "overlap_tests.h"
#include "../../include_ext/mirt_overlap_list.h"

#include <cmath>
#include <string>

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

// A row's cursor: where its next word goes and how many more its segment [beg, min(lim, capacity)) takes -- none if the segment
// begins below 0, at or beyond the capacity or after its own end.  (A row admits fewer than 2^32 candidates, so a longer
// segment's room may stop there.)
struct Cursor { uint32_t* out; uint32_t room; };
MIRT_DEV Cursor row_cursor(const OverlapListArgs& a, long long i)
{
  const long long beg = a.offsets[i], lim = a.offsets[i + 1];
  const long long end = lim < a.capacity ? lim : a.capacity;
  Cursor c;
  c.room = (beg >= 0 && beg < end) ? (uint32_t)(end - beg > 0xffffffffll ? 0xffffffffll : end - beg) : 0u;
  c.out = a.words + (c.room ? beg : 0);
  return c;
}
MIRT_DEV void emit(Cursor& c, uint32_t word)
{
  if (c.room) { *c.out++ = word; --c.room; }
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
    const float4 r0 = a.boxes[2 * i], r1 = a.boxes[2 * i + 1];
    const f3 lo = mk3(r0.x, r0.y, r0.z), hi = mk3(r1.x, r1.y, r1.z);
    // (x - x is 0 for a finite x and NaN for an infinity or a NaN)
    const bool live = (lo.x - lo.x) == 0.0f && (lo.y - lo.y) == 0.0f && (lo.z - lo.z) == 0.0f && (hi.x - hi.x) == 0.0f && (hi.y - hi.y) == 0.0f &&
                      (hi.z - hi.z) == 0.0f && lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z;
    if (!live) continue;             // (a dead row writes nothing)
    const f3 m = (lo + hi) * 0.5f, h = (hi - lo) * 0.5f;
    Cursor at = row_cursor(a, i);
    for (int j = 0; j < a.num_planes; ++j) {
      const f3 N = normalize(mk3(planes[j].nx, planes[j].ny, planes[j].nz));
      const float s = dot(N, m - mk3(planes[j].px, planes[j].py, planes[j].pz));
      const float e = (h.x * fabsf(N.x) + h.y * fabsf(N.y)) + h.z * fabsf(N.z);
      if (fabsf(s) <= e) emit(at, ((uint32_t)MIRT_HIT_PLANE << 30) | (uint32_t)j);      // (s is then no NaN, and dist = fabsf(s) is none)
    }
    if (a.root_ref == REF_NONE) continue;
    const float sigma = (fmaxf(max3(fabsf(lo.x), fabsf(lo.y), fabsf(lo.z)), max3(fabsf(hi.x), fabsf(hi.y), fabsf(hi.z))) + a.coord_max) * SLACK;
    uint32_t cur = a.root_ref;
    int sp = 0;
    for (;;) {
      const float4* rec = reinterpret_cast<const float4*>(heap + (cur << 4));
      bool pop;
      if (cur & REF_LEAF) {
        float dist = 0.0f;
        uint32_t id = 0u;
        bool pass;
        if (cur & REF_TRI) {
          id = a.unit_prim[(cur & REF_OFFMASK) - a.prim_base16] & 0x7fffffffu;
          const float4* v = a.tri_verts + 3 * (size_t)id;
          const float4 pa = v[0], pb = v[1], pc = v[2];
          const f3 ta = mk3(pa.x, pa.y, pa.z), tb = mk3(pb.x, pb.y, pb.z), tc = mk3(pc.x, pc.y, pc.z);
          pass = triangle_overlaps(m, h, ta, tb, tc);
          if (pass) {
            // (the vertices are loaded again, through an id the compiler cannot see through, as in overlap.hip: section 6w)
            asm volatile("" : "+v"(id));
            dist = length(m - triangle_point(a.tri_verts, id, m));
          }
        } else {
          const float4 s = rec[0];
          const f3 c = mk3(s.x, s.y, s.z);
          pass = sphere_overlaps(lo, hi, c, s.w);
          if (pass) dist = fabsf(length(m - c) - s.w);
        }
        if (pass && dist == dist) {          // (a NaN dist is not admitted)
          if (!(cur & REF_TRI)) id = a.unit_prim[(cur & REF_OFFMASK) - a.prim_base16] & 0x7fffffffu;
          emit(at, ((cur & REF_TRI) ? ((uint32_t)MIRT_HIT_TRIANGLE << 30) : ((uint32_t)MIRT_HIT_SPHERE << 30)) | id);
        }
        pop = true;
      } else {
        const float4 b0 = rec[0], b1 = rec[1], b2 = rec[2];
        const uint2 ch = *reinterpret_cast<const uint2*>(rec + 3);
        // (hi + sigma and lo - sigma made here from a copy of sigma the compiler cannot see through, as in overlap.hip: section 6w)
        float sg = sigma;
        asm volatile("" : "+v"(sg));
        const f3 los = mk3(lo.x - sg, lo.y - sg, lo.z - sg), his = mk3(hi.x + sg, hi.y + sg, hi.z + sg);
        const bool hl = !(b0.x > his.x) && !(b0.y < los.x) && !(b0.z > his.y) && !(b0.w < los.y) && !(b1.x > his.z) && !(b1.y < los.z);
        const bool hr = !(b1.z > his.x) && !(b1.w < los.x) && !(b2.x > his.y) && !(b2.y < los.y) && !(b2.z > his.z) && !(b2.w < los.z);
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

} // namespace

int64_t list_offsets_work_bytes(int64_t n)
{
  return n > LIST_TILE ? (int64_t)sizeof(u64) * list_blocks(n) : 0;
}

int list_offsets(MirtScene* sc, const uint32_t* d_counts, int64_t n, int64_t* d_offsets, void* d_work, hipStream_t stream)
{
  (void)sc;      // (the device and the error conventions: api.hip has made the device current)
  const char* const who = "mirt_list_offsets";
  if (n < 0) { set_error(std::string(who) + ": negative n"); return MIRT_ERR_ARG; }
  if (n > (1ll << 40)) { set_error(std::string(who) + ": n above 2^40"); return MIRT_ERR_ARG; }
  const size_t work = (size_t)list_offsets_work_bytes(n);
  if (!d_offsets || (n > 0 && !d_counts) || (work && !d_work)) {
    set_error(std::string(who) + ": null buffer (d_offsets; d_counts when n > 0; d_work when mirt_list_offsets_work_bytes(n) > 0)"); return MIRT_ERR_ARG;
  }
  if (!is_aligned(4, (const char*)d_counts) || !is_aligned(8, (const char*)d_offsets, (const char*)(work ? d_work : nullptr))) {
    set_error(std::string(who) + ": d_counts must be 4-byte aligned, d_offsets and d_work 8-byte aligned"); return MIRT_ERR_ARG;
  }
  const void* const ptr[3] = {d_counts, d_offsets, d_work};
  const size_t bytes[3] = {4 * (size_t)n, 8 * ((size_t)n + 1), work};
  for (int x = 0; x < 3; ++x) {
    for (int y = x + 1; y < 3; ++y) {
      if (bytes[x] && bytes[y] && overlaps(ptr[x], bytes[x], ptr[y], bytes[y])) {
        set_error(std::string(who) + ": d_counts, d_offsets and d_work must not overlap each other"); return MIRT_ERR_ARG;
      }
    }
  }
  long long* const offsets = reinterpret_cast<long long*>(d_offsets);
  if (n == 0) { MIRT_HIP(hipMemsetAsync(d_offsets, 0, sizeof(int64_t), stream)); return MIRT_OK; }      // (the total alone)
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
  const char* const who = "mirt_overlap_list";
  if (n < 0) { set_error(std::string(who) + ": negative n"); return MIRT_ERR_ARG; }
  if (capacity < 0) { set_error(std::string(who) + ": negative capacity"); return MIRT_ERR_ARG; }
  if ((n > 0 && (!d_boxes || !d_offsets)) || (capacity > 0 && !d_words)) {
    set_error(std::string(who) + ": null buffer (d_boxes and d_offsets when n > 0; d_words when capacity > 0)"); return MIRT_ERR_ARG;
  }
  if (!is_aligned(16, (const char*)d_boxes) || !is_aligned(8, (const char*)d_offsets) || !is_aligned(4, (const char*)d_words)) {
    set_error(std::string(who) + ": d_boxes must be 16-byte aligned, d_offsets 8-byte aligned, d_words 4-byte aligned"); return MIRT_ERR_ARG;
  }
  // (a range of no bytes -- n == 0, capacity == 0 -- overlaps nothing)
  const void* const ptr[3] = {d_boxes, d_offsets, d_words};
  const size_t bytes[3] = {32 * (size_t)n, n > 0 ? 8 * ((size_t)n + 1) : 0, 4 * (size_t)capacity};
  for (int x = 0; x < 3; ++x) {
    for (int y = x + 1; y < 3; ++y) {
      if (bytes[x] && bytes[y] && overlaps(ptr[x], bytes[x], ptr[y], bytes[y])) {
        set_error(std::string(who) + ": d_boxes, d_offsets and d_words must not overlap each other"); return MIRT_ERR_ARG;
      }
    }
  }
  if (!sc->built) { set_error(std::string(who) + ": call mirt_build_lbvh first"); return MIRT_ERR_STATE; }
  if (n == 0 || capacity == 0) return MIRT_OK;      // (no row, or no word any row could write)
  OverlapListArgs q;
  q.boxes = reinterpret_cast<const float4*>(d_boxes);
  q.offsets = reinterpret_cast<const long long*>(d_offsets);
  q.words = d_words;
  q.capacity = capacity;
  q.n = n;
  q.nodes = sc->nodes; q.unit_prim = sc->unit_prim;
  q.tri_verts = sc->tri_verts;
  q.planes = sc->planes; q.num_planes = sc->d.num_planes;
  q.root_ref = sc->root_ref; q.prim_base16 = sc->prim_base / 16u;
  q.coord_max = sc->coord_max;
  q.lds_depth = query_lds_depth(sc);
  const int grid = query_grid_blocks(sc, overlap_list_kernel, LIST_WAVES, &sc->overlap_list_blocks);
  hipLaunchKernelGGL(overlap_list_kernel, dim3(row_launch(n, grid)), dim3(QUERY_BLOCK), 0, stream, q);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

} // namespace mirt
