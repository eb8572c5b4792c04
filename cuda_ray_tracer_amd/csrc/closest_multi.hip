// Contact queries on a built scene (include_ext/mirt_contacts.h: mirt_closest_points_multi): for each row
// (q, R) the k nearest of ALL the planes, spheres and triangles nearer than R, in (dist, kind, id) order, and their number.  The
// header defines both over the scene's arrays, so the order of the visits is free and a subtree may be left out whenever none of
// its candidates can enter the answer.
//
// contacts_kernel<CAP>  one lane = one row (grid-stride over the batch): the walk of closest_points_kernel (closest.hip) with the
//                       list of multihit_kernel (multihit.hip).  The planes from scalar loads, then the best-first stack walk over
//                       the exact 64-byte records: the squared point-box distance of both children against (B + sigma)^2, the
//                       nearer child first, the other pushed.  With counts asked for, B is the row's radius for the whole walk
//                       (every candidate nearer than R has to be met); without them B is the radius until the list holds k keys
//                       and the list's largest distance from then on.  sigma is mirt_closest.h's slack, once per row.
//                       What a lane carries beside the row and the stack pointer is the count and its CAP best as 64-bit keys,
//                       ascending, in registers (key_list.h): high word dist's bits (non-negative: they order as unsigned
//                       integers), low word kind << 30 | file-order id -- one unsigned compare is the header's whole order.  A
//                       triangle's id is loaded anyway (its vertices are in file order); a sphere's costs a unit_prim load,
//                       made for a candidate that is admitted and not beyond the list's last distance.  Capacity 1 does without
//                       it: its sphere keys hold the record's unit, and the compare loads both ids only between two spheres at
//                       the same distance, as closest_points_kernel does on a tie (the eager load cost it up to 26 %, the
//                       compare with a branch costs capacity 4 more than the load: section 6s).  A call with k below CAP
//                       starts with CAP - k keys of 0, below every real key: they stay in front, so the last slot is always
//                       the k-th best and no slot is indexed at run time.  The loop keeps keys only: the records and feature
//                       rows are made after the walk by mirt_closest.h's operations.
//                       CAP = 0 is the count-only instance: no list at all.
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "query_walk.h"
#include "point_query.h"
#include "key_list.h"
#include "../../include_ext/mirt_contacts.h"

#include <cmath>
#include <string>

namespace mirt {
namespace {

// Waves per SIMD an instance is compiled for: 8 is what the LDS stack allows (20 KiB per block, 8 blocks per CU) and what the
// count-only instance reaches within 64 VGPRs; the list takes two registers per key (DESIGN.md section 6s has the compiler's report).
constexpr int contacts_waves(int cap) { return cap == 0 ? 8 : cap == 1 ? 7 : cap == 4 ? 6 : 5; }

struct ContactsArgs {
  const float4* points;           // (q, R)
  uint32_t* hits;                 // MirtHit: 6 words, k per row
  uint32_t* counts;               // (may be null)
  float4* features;               // nullable: (P, 1), (n, 0), k per row
  long long n;
  int k;
  const float4* nodes;            // record heap (scene_dev.h)
  const uint32_t* unit_prim;
  const float4* spheres;          // file order: (c, r) -- what the heap's sphere records are copies of (capacities 4 and 8 read them by id)
  const float4* tris;             // file order: 3 x float4 per triangle, what the heap's triangle records are copies of (the normal is read here)
  const float4* tri_verts;        // file order: p0, p1, p2 of every triangle
  const PlaneDev* planes; int num_planes;
  uint32_t root_ref;              // the exact records' root (REF_NONE: no primitive)
  uint32_t prim_base16;
  float coord_max;                // largest coordinate magnitude of the scene box
  int lds_depth;                  // stack entries kept in LDS (<= QUERY_STACK_LDS)
};

template <int CAP>
__global__ void __launch_bounds__(QUERY_BLOCK, contacts_waves(CAP)) contacts_kernel(const ContactsArgs a)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];             // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * QUERY_BLOCK;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(a.nodes);
  const ConstPlanes planes = const_planes(a.planes);
  const bool shrink = CAP > 0 && a.counts == nullptr;      // the bound follows the list's last key
  // Capacity 1: a sphere's key holds its record's unit and the ids are loaded only to break a tie, as closest_points_kernel does.
  // Capacities 4 and 8: the key holds the id, loaded for every sphere that reaches the list -- there the chain's compares with a
  // branch each cost more than the load (4 to 33 % at capacity 4; at capacity 8 they spill scalar registers; section 6s).
  constexpr bool ID_ON_TIE = CAP == 1;
  // the header's order on a sphere's key x and a key y: two spheres at the same distance are told apart by their file-order ids,
  // everything else by the keys (capacity 1, whose sphere keys hold units)
  const auto less = [&a](unsigned long long x, unsigned long long y) {
    if (((x ^ y) >> 30) != 0ull || ((uint32_t)x >> 30) != (uint32_t)MIRT_HIT_SPHERE) return x < y;      // (the chain carries other kinds too)
    return (a.unit_prim[(uint32_t)x & KEY_ID] & 0x7fffffffu) < (a.unit_prim[(uint32_t)y & KEY_ID] & 0x7fffffffu);
  };
  for (long long i = (long long)blockIdx.x * QUERY_BLOCK + tid; i < a.n; i += stride) {
    const float4 row = a.points[i];
    const f3 q = mk3(row.x, row.y, row.z);
    const float R = row.w;
    // (x - x is 0 for a finite x and NaN for an infinity or a NaN)
    const bool live = R > 0.0f && (q.x - q.x) == 0.0f && (q.y - q.y) == 0.0f && (q.z - q.z) == 0.0f;
    KeyList<CAP> best;
#pragma unroll
    for (int j = 0; j < CAP; ++j) best.key[j] = j < CAP - a.k ? 0ull : KEY_NONE;
    uint32_t count = 0u;
    float B = R;                     // no candidate at a distance above B can enter the answer
    if (live) {
      for (int j = 0; j < a.num_planes; ++j) {
        const f3 N = normalize(mk3(planes[j].nx, planes[j].ny, planes[j].nz));
        const float dist = fabsf(dot(N, q - mk3(planes[j].px, planes[j].py, planes[j].pz)));
        if (dist < R) {
          ++count;
          best.insert(contact_key(dist, MIRT_HIT_PLANE, (uint32_t)j));
        }
      }
      if (shrink) {
        const uint32_t last = (uint32_t)(best.key[CAP > 0 ? CAP - 1 : 0] >> 32);
        B = last == 0xffffffffu ? R : __uint_as_float(last);
      }
    }
    if (live && a.root_ref != REF_NONE) {
      const float sigma = row_sigma(largest_abs(q), a.coord_max);
      float reach = B + sigma;
      float bound2 = reach * reach;      // a box farther than this (squared) holds nothing that enters the answer
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
            ++count;
            // (a distance above the list's last cannot enter it; an equal one may, by its kind and id)
            if (CAP > 0 && !(__float_as_uint(dist) > (uint32_t)(best.key[CAP > 0 ? CAP - 1 : 0] >> 32))) {
              const uint32_t unit = (cur & REF_OFFMASK) - a.prim_base16;
              if (!(cur & REF_TRI)) id = ID_ON_TIE ? unit : a.unit_prim[unit] & 0x7fffffffu;
              const unsigned long long x = contact_key(dist, (cur & REF_TRI) ? MIRT_HIT_TRIANGLE : MIRT_HIT_SPHERE, id);
              if (ID_ON_TIE && !(cur & REF_TRI)) best.insert(x, less);
              else best.insert(x);
              if (shrink) {
                const uint32_t last = (uint32_t)(best.key[CAP > 0 ? CAP - 1 : 0] >> 32);
                B = last == 0xffffffffu ? R : __uint_as_float(last);
                reach = B + sigma;
                bound2 = reach * reach;
              }
            }
          }
          pop = true;
        } else {
          const float4 b0 = rec[0], b1 = rec[1], b2 = rec[2];
          const uint2 ch = *reinterpret_cast<const uint2*>(rec + 3);
          const float l2 = box_dist2(b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, q);
          const float r2 = box_dist2(b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, q);
          const bool hl = !(l2 > bound2), hr = !(r2 > bound2);
          const bool right_first = r2 < l2;      // the nearer child first
          if (hl && hr) stack_push(lds_stack, spill, a.lds_depth, tid, sp, right_first ? ch.x : ch.y);
          cur = (hl && hr) ? (right_first ? ch.y : ch.x) : (hl ? ch.x : ch.y);
          pop = !(hl || hr);
        }
        if (pop) {
          if (sp == 0) break;
          cur = stack_pop(lds_stack, spill, a.lds_depth, tid, sp);
        }
      }
    }
    if (a.counts) a.counts[i] = count;
    if (CAP > 0) {
      // the k records, nearest first: each key's point and normal by mirt_closest.h's operations (the loop kept the distance only).
      // overlap.hip has the same loop, written out in both: as one function it moves capacity 1, 4 and 8 here (995, 606 and 1262
      // instruction lines), and capacity 8 was then up to 1.6 % slower, more than the parent's run spread
      for (int j = a.k; j < CAP; ++j) best.pop_front();      // (the keys of 0 in front of a list with k below CAP)
      uint32_t* h = a.hits + 6 * (i * a.k);
      float4* f = a.features ? a.features + 2 * (i * a.k) : nullptr;
      for (int j = 0; j < a.k; ++j, h += 6) {
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
            const float s = dot(N, q - mk3(planes[id].px, planes[id].py, planes[id].pz));
            P = q - N * s;
            n = s < 0.0f ? -N : N;
          } else if (kind == MIRT_HIT_TRIANGLE) {
            const float4 q0 = a.tris[3 * (size_t)id], q1 = a.tris[3 * (size_t)id + 1];
            const f3 nor = mk3(q0.w, q1.x, q1.y);
            P = triangle_point(a.tri_verts, id, q);
            n = dot(q - P, nor) < 0.0f ? -nor : nor;
          } else {
            const float4 s = ID_ON_TIE ? a.nodes[a.prim_base16 + id] : a.spheres[id];      // (the key holds the record's unit, or the id)
            if (ID_ON_TIE) id = a.unit_prim[id] & 0x7fffffffu;
            const f3 c = mk3(s.x, s.y, s.z), v = q - c;
            const f3 u = normalize(v);
            P = c + u * s.w;
            n = length(v) < s.w ? -u : u;
          }
        }
        store_hit(h, t, kind, id, n);
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

int closest_points_multi(MirtScene* sc, const void* d_points, int64_t n, int k, void* d_hits, uint32_t* d_counts, void* d_features, uint32_t flags,
                         hipStream_t stream)
{
  bool go = false;
  const int rc = check_closest_points_multi(d_points, n, k, d_hits, d_counts, d_features, flags, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  ContactsArgs q;
  q.points = reinterpret_cast<const float4*>(d_points);
  q.hits = reinterpret_cast<uint32_t*>(d_hits);
  q.counts = d_counts;
  q.features = k > 0 ? reinterpret_cast<float4*>(d_features) : nullptr;
  q.n = n;
  q.k = k;
  fill_scene_args(q, sc);
  q.spheres = sc->spheres; q.tris = sc->tris;
  // the smallest instance that holds k
  return with_capacity(k, [&](auto cap, int slot) {
    constexpr int CAP = decltype(cap)::value;
    return launch_rows(sc, contacts_kernel<CAP>, contacts_waves(CAP), &sc->contacts_blocks[slot], n, q, stream);
  });
}

} // namespace mirt
