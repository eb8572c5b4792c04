// Sphere casts on a built scene (include_ext/mirt_spherecast.h: mirt_cast_spheres): for each row the first
// contact of a ball of radius r whose centre travels along a ray -- the admitted candidate with the smallest (t, kind, id), which
// the header defines over the scene's arrays, so the order of the visits is free.  Like the other queries it reads the scene only
// and touches no render context, counter, hand-out table or RNG table.
//
// sphere_cast_kernel<ANY>  one lane = one row (grid-stride over the batch).  The planes from scalar loads, then a stack walk over the
//                          exact 64-byte node records: a slab test of the centre ray against both children's boxes grown by
//                          r + sigma, over [0, best + tau], the child with the nearer entry first, the other pushed.  best starts
//                          at the row's tmax and shrinks with every admitted candidate; sigma and tau are the header's slacks.
//                          The loop keeps (t, ref) only; the winner's point and normal are made after it, by the header's
//                          operations.  ANY (MIRT_CAST_ANY_HIT): the walk ends at the first admitted candidate.  The stack is the
//                          query kernels': [entry][lane] in LDS, deeper entries in the lane's private array.
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "query_walk.h"
#include "point_query.h"
#include "cast_tests.h"
#include "../../include_ext/mirt_spherecast.h"

#include <cmath>

namespace mirt {
namespace {

// the compiler's report decides: at 5 waves per SIMD both instances take the 96 VGPRs there are and spill
// nothing; at 6 (80 VGPRs) they spill 11 and 12 registers, at 8 (64) about 30
constexpr int SWAVES_PER_SIMD = 5;

struct CastArgs {
  const float4* casts;            // (o, tmax), (d, r)
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

template <bool ANY>
__global__ void __launch_bounds__(QUERY_BLOCK, SWAVES_PER_SIMD) sphere_cast_kernel(const CastArgs a)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];             // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * QUERY_BLOCK;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(a.nodes);
  const ConstPlanes planes = const_planes(a.planes);
  for (long long i = (long long)blockIdx.x * QUERY_BLOCK + tid; i < a.n; i += stride) {
    const float4 r0 = a.casts[2 * i], r1 = a.casts[2 * i + 1];
    Ball k;
    k.o = mk3(r0.x, r0.y, r0.z);
    k.d = normalize(mk3(r1.x, r1.y, r1.z));
    k.r = r1.w;
    const float tmax = r0.w;
    // (x - x is 0 for a finite x and NaN for an infinity or a NaN)
    const bool live = ray_is_live(tmax, k.d) && k.r >= 0.0f && (k.r - k.r) == 0.0f && finite3(r0);
    float best = tmax;               // the smallest admitted t so far; without a winner, tmax
    uint32_t refbest = REF_NONE;     // the winner, a primitive record of the heap ...
    int plane_id = -1;               // ... or a plane
    if (live) {
      for (int j = 0; j < a.num_planes; ++j) {
        const f3 N = normalize(mk3(planes[j].nx, planes[j].ny, planes[j].nz));
        const float t = plane_cast(N, mk3(planes[j].px, planes[j].py, planes[j].pz), k);
        if (t >= 0.0f && t < best) { best = t; plane_id = j; }      // (an equal t: the lower index stays)
      }
    }
    // (a cast for any contact that a plane already answers needs no walk)
    if (live && a.root_ref != REF_NONE && !(ANY && plane_id >= 0)) {
      const f3 inv = mk3(1.0f / k.d.x, 1.0f / k.d.y, 1.0f / k.d.z);
      const float sigma = row_sigma(largest_abs(k.o), a.coord_max, k.r);
      const float grow = k.r + sigma;
      float bound = best + best * TAU;     // a box the centre enters later than this holds nothing that wins or ties
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
          bool better = t >= 0.0f && t < best;
          // (a tie with the winner: (kind, id) decides)
          if (t == best && (plane_id >= 0 || refbest != REF_NONE)) better = wins_tie(cur, id, plane_id, refbest, a.unit_prim, a.prim_base16);
          if (better) {
            best = t; refbest = cur; plane_id = -1;
            bound = best + best * TAU;
            if (ANY) break;
          }
          pop = true;
        } else {
          const float4 b0 = rec[0], b1 = rec[1], b2 = rec[2];
          const uint2 ch = *reinterpret_cast<const uint2*>(rec + 3);
          float el, ll, er, lr;
          box_interval(b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, k.o, inv, grow, el, ll);
          box_interval(b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, k.o, inv, grow, er, lr);
          const bool hl = !(el > fminf(ll, bound)), hr = !(er > fminf(lr, bound));
          const bool right_first = er < el;      // the child with the nearer entry first
          if (hl && hr) {
            // (stack_push and stack_pop of query_walk.h, written out as closest.hip does: DESIGN.md section 6q)
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
    // the winner's record: the centre at contact, the candidate's closest point to it, the push-out direction
    float t = -1.0f;
    uint32_t kind = MIRT_HIT_NONE, id = 0u;
    f3 P = mk3(0.0f, 0.0f, 0.0f), n = P;
    const bool hit = plane_id >= 0 || refbest != REF_NONE;
    if (hit) {
      t = best;
      const f3 Cw = k.o + k.d * t;
      if (plane_id >= 0) {
        const f3 N = normalize(mk3(planes[plane_id].nx, planes[plane_id].ny, planes[plane_id].nz));
        const float s = dot(N, Cw - mk3(planes[plane_id].px, planes[plane_id].py, planes[plane_id].pz));
        P = Cw - N * s;
        kind = MIRT_HIT_PLANE; id = (uint32_t)plane_id;
      } else {
        id = a.unit_prim[(refbest & REF_OFFMASK) - a.prim_base16] & 0x7fffffffu;
        if (refbest & REF_TRI) {
          P = triangle_point(a.tri_verts, id, Cw);
          kind = MIRT_HIT_TRIANGLE;
        } else {
          const float4 s = a.nodes[refbest & REF_OFFMASK];
          const f3 c = mk3(s.x, s.y, s.z);
          P = c + normalize(Cw - c) * s.w;
          kind = MIRT_HIT_SPHERE;
        }
      }
      n = normalize(Cw - P);
    }
    store_hit(a.hits + 6 * i, t, kind, id, n);
    if (a.features) {
      a.features[2 * i] = make_float4(P.x, P.y, P.z, hit ? 1.0f : 0.0f);
      a.features[2 * i + 1] = make_float4(n.x, n.y, n.z, 0.0f);
    }
  }
}

} // namespace

int cast_spheres(MirtScene* sc, const void* d_casts, int64_t n, void* d_hits, void* d_features, uint32_t flags, hipStream_t stream)
{
  bool go = false;
  const int rc = check_cast_spheres(d_casts, n, d_hits, d_features, flags, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  CastArgs q;
  q.casts = reinterpret_cast<const float4*>(d_casts);
  q.hits = reinterpret_cast<uint32_t*>(d_hits);
  q.features = reinterpret_cast<float4*>(d_features);
  q.n = n;
  fill_scene_args(q, sc);
  return (flags & MIRT_CAST_ANY_HIT) ? launch_rows(sc, sphere_cast_kernel<true>, SWAVES_PER_SIMD, &sc->spherecast_blocks[1], n, q, stream)
                                     : launch_rows(sc, sphere_cast_kernel<false>, SWAVES_PER_SIMD, &sc->spherecast_blocks[0], n, q, stream);
}

} // namespace mirt
