// Box overlap queries on a built scene (include_ext/mirt_overlap.h: mirt_overlap_boxes): for each row, an
// axis-aligned box [lo, hi], ALL the planes, spheres and triangles whose surface meets the box -- the k nearest to the box's centre m
// in (dist, kind, id) order, and their number.  The header defines both over the scene's arrays, so the order of the visits is free
// and a subtree may be left out whenever none of its candidates can pass its test.
//
// overlap_kernel<CAP, ANY>  one lane = one row (grid-stride over the batch).  The planes from scalar loads, then a stack walk over
//                       the exact 64-byte records, left child first: a child is visited when its box meets the row's grown by the
//                       header's sigma on every axis (negated compares: a NaN visits).  There is no shrinking bound: what is visited
//                       depends on the row alone, except that ANY ends the walk at the first admitted candidate.  A leaf is the
//                       header's test -- a sphere's two squared distances against rs^2, a triangle's thirteen axes in four groups
//                       of one running boolean each, the three box axes first (cheapest, and they reject most) -- and, for a candidate that passes,
//                       mirt_closest.h's dist at m: a NaN dist (a triangle without area, zero divided by zero) is not admitted,
//                       so every instance computes it, the count-only ones for that test alone.  What a lane carries beside the
//                       row and the stack pointer is the count and its CAP best as contact keys (key_list.h), ascending, in
//                       registers.  A sphere's id costs a unit_prim load, made for a candidate that is admitted and not beyond the
//                       list's last distance; a triangle's id is loaded anyway (its vertices are in file order).  A call with k
//                       below CAP starts with CAP - k keys of 0, below every real key: they stay in front, so the last slot is
//                       always the k-th best and no slot is indexed at run time.  The loop keeps keys only: the records and feature
//                       rows are made after the walk by mirt_closest.h's operations at q = m.
//                       CAP = 0: no list at all (count-only; with ANY the count is 0 or 1).
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "query_walk.h"
#include "point_query.h"
#include "key_list.h"
#include "overlap_tests.h"
#include "../../include_ext/mirt_overlap.h"

#include <cmath>

namespace mirt {
namespace {

// Waves per SIMD an instance is compiled for: the largest at which the compiler reports no VGPR spill (80 / 94 / 104 / 113 VGPRs;
// DESIGN.md section 6w has the report).  The triangle's test, not the list, sets the floor: the count-only instance spills six
// registers at 7 waves.
constexpr int overlap_waves(int cap) { return cap == 0 ? 6 : cap == 1 ? 5 : 4; }

struct OverlapArgs {
  const float4* boxes;            // (lo, _) (hi, _)
  uint32_t* hits;                 // MirtHit: 6 words, k per row
  uint32_t* counts;               // (may be null)
  float4* features;               // nullable: (P, 1), (n, 0), k per row
  long long n;
  int k;
  const float4* nodes;            // record heap (scene_dev.h)
  const uint32_t* unit_prim;
  const float4* spheres;          // file order: (c, r) -- what the heap's sphere records are copies of
  const float4* tris;             // file order: 3 x float4 per triangle (the normal is read here)
  const float4* tri_verts;        // file order: p0, p1, p2 of every triangle
  const PlaneDev* planes; int num_planes;
  uint32_t root_ref;              // the exact records' root (REF_NONE: no primitive)
  uint32_t prim_base16;
  float coord_max;                // largest coordinate magnitude of the scene box
  int lds_depth;                  // stack entries kept in LDS (<= QUERY_STACK_LDS)
};

template <int CAP, bool ANY>
__global__ void __launch_bounds__(QUERY_BLOCK, overlap_waves(CAP)) overlap_kernel(const OverlapArgs a)
{
  static_assert(!ANY || CAP == 0, "MIRT_OVERLAP_ANY is a count-only call");
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
    const f3 m = (lo + hi) * 0.5f, h = (hi - lo) * 0.5f;
    KeyList<CAP> best;
#pragma unroll
    for (int j = 0; j < CAP; ++j) best.key[j] = j < CAP - a.k ? 0ull : KEY_NONE;
    uint32_t count = 0u;
    if (live) {
      for (int j = 0; j < a.num_planes; ++j) {
        const f3 N = normalize(mk3(planes[j].nx, planes[j].ny, planes[j].nz));
        const float s = dot(N, m - mk3(planes[j].px, planes[j].py, planes[j].pz));
        const float e = (h.x * fabsf(N.x) + h.y * fabsf(N.y)) + h.z * fabsf(N.z);
        if (fabsf(s) <= e) {       // (s is then no NaN, and dist = fabsf(s) is none)
          ++count;
          best.insert(contact_key(fabsf(s), MIRT_HIT_PLANE, (uint32_t)j));
        }
      }
    }
    if (live && a.root_ref != REF_NONE && !(ANY && count != 0u)) {
      // The walk of overlap_walk.h (overlap_list.hip uses it), written out: as a call the count-only and the record instances run
      // 0.8 to 1.8 % slower on the voxel grids of tools/overlap_bench.py, more than the parent's run spread.
      // A change to the pruning or to the degenerate-triangle rule goes into both.
      const float sigma = row_sigma(fmaxf(largest_abs(lo), largest_abs(hi)), a.coord_max);
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
              // (the vertices are loaded again, through an id the compiler cannot see through: kept from the test above they are
              // nine registers more at the kernel's peak, section 6w)
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
            ++count;
            if (ANY) break;
            // (a distance above the list's last cannot enter it; an equal one may, by its kind and id)
            if (CAP > 0 && !(__float_as_uint(dist) > (uint32_t)(best.key[CAP > 0 ? CAP - 1 : 0] >> 32))) {
              if (!(cur & REF_TRI)) id = a.unit_prim[(cur & REF_OFFMASK) - a.prim_base16] & 0x7fffffffu;
              best.insert(contact_key(dist, (cur & REF_TRI) ? MIRT_HIT_TRIANGLE : MIRT_HIT_SPHERE, id));
            }
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
    if (a.counts) a.counts[i] = ANY ? (count != 0u ? 1u : 0u) : count;      // (several planes may have admitted the row)
    if (CAP > 0) {
      // the k records, nearest first: each key's point and normal by mirt_closest.h's operations at q = m (the loop kept the distance only)
      for (int j = a.k; j < CAP; ++j) best.pop_front();      // (the keys of 0 in front of a list with k below CAP)
      uint32_t* hp = a.hits + 6 * (i * a.k);
      float4* f = a.features ? a.features + 2 * (i * a.k) : nullptr;
      for (int j = 0; j < a.k; ++j, hp += 6) {
        const unsigned long long key = best.pop_front();
        const uint32_t low = (uint32_t)key;
        float t = -1.0f;
        uint32_t kind = MIRT_HIT_NONE, id = 0u;
        f3 P = mk3(0.0f, 0.0f, 0.0f), n = P;
        const bool hit = key != KEY_NONE;
        if (hit) {
          t = __uint_as_float((uint32_t)(key >> 32));
          kind = low >> 30;
          id = low & KEY_ID;
          if (kind == MIRT_HIT_PLANE) {
            const f3 N = normalize(mk3(planes[id].nx, planes[id].ny, planes[id].nz));
            const float s = dot(N, m - mk3(planes[id].px, planes[id].py, planes[id].pz));
            P = m - N * s;
            n = s < 0.0f ? -N : N;
          } else if (kind == MIRT_HIT_TRIANGLE) {
            const float4 q0 = a.tris[3 * (size_t)id], q1 = a.tris[3 * (size_t)id + 1];
            const f3 nor = mk3(q0.w, q1.x, q1.y);
            P = triangle_point(a.tri_verts, id, m);
            n = dot(m - P, nor) < 0.0f ? -nor : nor;
          } else {
            const float4 s = a.spheres[id];
            const f3 c = mk3(s.x, s.y, s.z), v = m - c;
            const f3 u = normalize(v);
            P = c + u * s.w;
            n = length(v) < s.w ? -u : u;
          }
        }
        store_hit(hp, t, kind, id, n);
        if (f) {
          f[0] = make_float4(P.x, P.y, P.z, hit ? 1.0f : 0.0f);
          f[1] = make_float4(n.x, n.y, n.z, 0.0f);
          f += 2;
        }
      }
    }
  }
}

} // namespace

int overlap_boxes(MirtScene* sc, const void* d_boxes, int64_t n, int k, void* d_hits, uint32_t* d_counts, void* d_features, uint32_t flags,
                  hipStream_t stream)
{
  bool go = false;
  const int rc = check_overlap_boxes(d_boxes, n, k, d_hits, d_counts, d_features, flags, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  OverlapArgs q;
  q.boxes = reinterpret_cast<const float4*>(d_boxes);
  q.hits = reinterpret_cast<uint32_t*>(d_hits);
  q.counts = d_counts;
  q.features = k > 0 ? reinterpret_cast<float4*>(d_features) : nullptr;
  q.n = n;
  q.k = k;
  fill_scene_args(q, sc);
  q.spheres = sc->spheres; q.tris = sc->tris;
  if (flags & MIRT_OVERLAP_ANY) return launch_rows(sc, overlap_kernel<0, true>, overlap_waves(0), &sc->overlap_blocks[1], n, q, stream);
  // the smallest instance that holds k (overlap_blocks: count, any, capacity 1, 4, 8)
  return with_capacity(k, [&](auto cap, int slot) {
    constexpr int CAP = decltype(cap)::value;
    return launch_rows(sc, overlap_kernel<CAP, false>, overlap_waves(CAP), &sc->overlap_blocks[slot ? slot + 1 : 0], n, q, stream);
  });
}

} // namespace mirt
