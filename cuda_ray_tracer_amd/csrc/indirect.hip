// Indirect light at surface points (include/mirt_indirect.h: mirt_indirect_light): one diffuse bounce.  K
// directions of a caller's table, turned into the frame of each row's normal as mirt_hemisphere_visibility turns them, are traced to
// their closest hit within a radius; every hit point receives mirt_direct_light's raw sum of the scene's lights, times the diffuse
// weight of the material it lies on; the weighted terms are summed over the directions.  Like the other two surface-point queries
// it reads the scene only and touches no render context, counter, hand-out table or RNG table.
//
// indirect_light_kernel  the shape of hemisphere_visibility_kernel (visibility.hip): one lane = one (row, direction) pair.  G is
//                      the next power of two >= K: a wave serves 64 / G rows at a time (grid-stride, a wave-uniform trip count),
//                      lane g G + k owns direction k of the wave's row g, lanes with k >= K idle.
//                      phase 1: the lane builds its gather ray and does the closest-hit walk of trace_rays_kernel<false>
//                               (query.hip), planes and the mapping to the file-order id included.
//                      phase 2: a lane that hit keeps its hit point, the hit's normal and the index of the hit's material, and
//                               runs the light loop of mirt_direct_light at that point: light li in iteration li, the facing test,
//                               the any-hit walk of trace_rays_kernel<true> for the shadow ray, the term added in light order.
//                               Lanes that missed, or that the light does not face, idle through the iteration's walk.
//                      phase 3: rho of the hit's material, w from the table; one ballot of "hit" is the wave's 64-bit word, of
//                               which a row's mask is its G-bit field; the four channels are summed by the xor-butterfly whose
//                               order the header fixes, and the group's first lane writes them.
//                      Both walks are walk<ANY> of query_walk.h, which light.hip uses too, and the choice of the winner and
//                      its normal are the helpers query.hip uses (section 6n).
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "query_walk.h"
#include "../../include/mirt_indirect.h"

#include <cmath>

namespace mirt {
namespace {

// IWAVES_PER_SIMD is a lower bound for the compiler, not the 8 of the other query kernels: this one carries the hit point, the hit's
// normal, the sum and the material index across the shadow walks, and under a bound of 8 (64 VGPRs) it spills 12 of them.  Under
// this bound it takes 72 VGPRs without a spill: 7 waves per SIMD.
// (QUERY_STACK_LDS x 4 B x 64 lanes = 5 KiB of LDS per wave, as in the other query kernels)
constexpr int IWAVES_PER_SIMD = 6;
constexpr uint32_t MAT_NONE = 0xffffffffu;     // the gather ray hit nothing
constexpr uint32_t MAT_PLANE = 0x80000000u;    // | plane index; else the index into mats (spheres, then triangles)

struct IndirectArgs {
  const float4* features;         // mirt_hit_features rows: (P, hit), (n, _)
  const float4* dirs;             // K rows (lx, ly, lz, w)
  const float2* rot;              // nullable: n rows (c, r)
  float4* out;
  unsigned long long* mask;       // nullable
  long long n;
  const float4* nodes;            // record heap (scene_dev.h)
  const uint32_t* unit_prim;
  const float4* mats;             // 3 x float4 per primitive: spheres first, then triangles
  const PlaneDev* planes; int num_planes;
  uint32_t root_ref;              // the exact records' root (REF_NONE: no primitive)
  uint32_t prim_base16;
  int num_spheres;
  const LightDev* suns; int num_suns;
  const LightDev* bulbs; int num_bulbs;
  float radius;
  int num_dirs;                   // K
  int lds_depth;                  // stack entries kept in LDS (<= QUERY_STACK_LDS)
  int gshift;                     // G = 1 << gshift lanes per row
};

// The kernel's arguments as they lie in the kernarg segment.  What only one phase needs -- the row and table pointers, the id and
// material tables, the light arrays, the outputs -- is read through this pointer where it is needed, from a copy of the pointer the
// compiler cannot tie to the others, so that it occupies no scalar registers across the walks (as HotArgs keeps RenderArgs out of
// the trace kernel's loop, scene_dev.h).  The walks' own arguments are read from the by-value struct as usual.
typedef const IndirectArgs __attribute__((address_space(4))) * KernArgs;
__device__ __forceinline__ KernArgs fresh(KernArgs p) { asm volatile("" : "+s"(p)); return p; }

__global__ void __launch_bounds__(QUERY_BLOCK, IWAVES_PER_SIMD) indirect_light_kernel(const IndirectArgs q)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];                     // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int G = 1 << q.gshift;
  const int rows_per_wave = 64 >> q.gshift;
  const KernArgs ka = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(q.nodes);
  // (the same for every lane of a wave: the loop below is uniform, so that every lane reaches the ballot and the exchange)
  const long long wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (QUERY_BLOCK / 64) + (threadIdx.x >> 6)));
  const long long stride = (long long)gridDim.x * (QUERY_BLOCK / 64) * rows_per_wave;
  for (long long base = wave * rows_per_wave; base < q.n; base += stride) {
    // (as in hemisphere_visibility_kernel: what a lane derives from its index is derived again in every pass, and again after every
    // walk, from a copy of the index the compiler cannot tie to the others, so that none of it lives across the passes or a walk)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int k = tid & (G - 1);                          // this lane's direction
    const int group = (tid & 63) >> q.gshift;             // ... and its row among the wave's
    const long long row = base + group;
    const bool in_range = row < q.n;
    const KernArgs a1 = fresh(ka);
    float4 f0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), f1 = f0;
    if (in_range) { const float4* const features = a1->features; f0 = features[2 * row]; f1 = features[2 * row + 1]; }
    const bool hit_row = f0.w != 0.0f;
    // ---- phase 1: the gather ray and its closest hit ---------------------------------------------------------------------------
    bool missed = false;                                  // a direction of the table that found nothing: its term is (0, 0, 0, w)
    uint32_t matref = MAT_NONE;
    f3 P2 = mk3(0.0f, 0.0f, 0.0f), n2 = P2;
    if (hit_row && k < a1->num_dirs) {
      // the origin and the frame of mirt_visibility.h
      const f3 P = mk3(f0.x, f0.y, f0.z), ng = mk3(f1.x, f1.y, f1.z);
      const f3 N = normalize(ng);
      const f3 o = P + ng * EPSILON;
      const float s = copysignf(1.0f, N.z);
      const float a = -1.0f / (s + N.z);
      const float b = (N.x * N.y) * a;
      const f3 T = mk3(1.0f + ((s * N.x) * N.x) * a, s * b, (-s) * N.x);
      const f3 B = mk3(b, s + (N.y * N.y) * a, -N.y);
      const float4 dk = a1->dirs[k];
      float x = dk.x, y = dk.y;
      const float2* const rot = a1->rot;
      if (rot) {
        const float2 cr = rot[row];
        x = cr.x * dk.x - cr.y * dk.y;
        y = cr.y * dk.x + cr.x * dk.y;
      }
      const f3 dl = (T * x + B * y) + N * dk.z;
      const f3 d = normalize(dl);                          // Ray(eye, dir, bounce), object.cuh:69 -- as mirt_trace_rays does it
      const float tmax = q.radius;
      float tbest, tplane;
      uint32_t refbest;
      int plane_id;
      walk<false>(heap, q.root_ref, q.planes, q.num_planes, o, d, tmax, lds_stack, spill, q.lds_depth, tid, tbest, refbest, tplane, plane_id);
      const Nearest w = nearest_of<false>(tbest, refbest, tplane, plane_id, tmax);
      missed = !w.report;
      if (w.report) {
        const KernArgs a2 = fresh(ka);
        const float t = w.t;
        // mirt_hit_features' point, and ObjectInfo.normal of the winner as mirt_trace_rays reports it
        P2 = mk3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z);
        if (w.use_bvh) {
          const uint32_t id = a2->unit_prim[(refbest & REF_OFFMASK) - a2->prim_base16] & 0x7fffffffu;
          n2 = prim_normal(q.nodes, refbest, t, o, d);
          matref = (refbest & REF_TRI) ? (uint32_t)a2->num_spheres + id : id;
        } else {
          n2 = plane_normal(q.planes, plane_id, d);
          matref = MAT_PLANE | (uint32_t)plane_id;
        }
      }
    }
    // ---- phase 2: mirt_direct_light with MIRT_LIGHT_RAW at (P2, n2), the lights in the scene's order -----------------------------
    f3 acc = mk3(0.0f, 0.0f, 0.0f);
    const int nlights = fresh(ka)->num_suns + fresh(ka)->num_bulbs;
    for (int li = 0; li < nlights; ++li) {
      if (matref == MAT_NONE) continue;
      int tidw = threadIdx.x;
      asm volatile("" : "+v"(tidw));
      const KernArgs a3 = fresh(ka);
      const int num_suns = a3->num_suns;
      const bool is_sun = li < num_suns;
      const LightDev* const lt = is_sun ? a3->suns + li : a3->bulbs + (li - num_suns);
      const f3 N = normalize(n2);
      const f3 o = P2 + n2 * EPSILON;
      float tmax = INFINITY;
      f3 L, d;
      if (is_sun) {
        L = mk3(lt->nx, lt->ny, lt->nz);
        d = normalize(mk3(lt->x, lt->y, lt->z));
      } else {
        const f3 bd = mk3(lt->x, lt->y, lt->z) - P2;
        tmax = length(bd);
        L = normalize(bd);
        d = L;
      }
      const float lam = dot(N, L);
      if (lam > 0.0f) {
        float tbest, tplane;
        uint32_t refbest;
        int plane_id;
        walk<true>(heap, q.root_ref, q.planes, q.num_planes, o, d, tmax, lds_stack, spill, q.lds_depth, tidw, tbest, refbest, tplane, plane_id);
        // what the query reports as kind != 0: an occluder of the tree or a plane, nearer than tmax
        const bool occluded = (refbest != REF_NONE && tbest < tmax) || (plane_id >= 0 && tplane < tmax);
        if (!occluded) {
          // getColorSun / getColorBulb (helper.cu) for an object colour of 1, without the exposure curve
          f3 term = mk3(lt->r * lam, lt->g * lam, lt->b * lam);
          if (!is_sun) {
            const float i2 = 1.0f / (tmax * tmax);
            term = term * i2;
          }
          acc = mk3(acc.x + term.x, acc.y + term.y, acc.z + term.z);
        }
      }
    }
    // ---- phase 3: this direction's term, the mask and the sum --------------------------------------------------------------------
    int tid2 = threadIdx.x;
    asm volatile("" : "+v"(tid2));
    const int k2 = tid2 & (G - 1);
    float ex = 0.0f, ey = 0.0f, ez = 0.0f, ew = 0.0f;
    const bool hit = matref != MAT_NONE;
    const KernArgs a4 = fresh(ka);
    if (hit) {
      // the diffuse weight of the reference's mix (draw.cu:277-280): (1 - shininess) (1 - trans) colour
      Mat mt;
      if (matref & MAT_PLANE) {
        mt = plane_mat(q.planes[matref & ~MAT_PLANE]);
      } else {
        mt = load_mat(a4->mats, matref);
      }
      const float rr = ((1.0f - mt.shininess.x) * (1.0f - mt.trans.x)) * mt.color.x;
      const float rg = ((1.0f - mt.shininess.y) * (1.0f - mt.trans.y)) * mt.color.y;
      const float rb = ((1.0f - mt.shininess.z) * (1.0f - mt.trans.z)) * mt.color.z;
      const float w = a4->dirs[k2].w;
      ex = w * (rr * acc.x); ey = w * (rg * acc.y); ez = w * (rb * acc.z);
    } else if (missed) {
      ew = a4->dirs[k2].w;
    }
    const unsigned long long word = __ballot(hit);
    const int lane2 = tid2 & 63, group2 = lane2 >> q.gshift;
    const unsigned long long field = ((word >> (group2 << q.gshift)) << (64 - G)) >> (64 - G);
    // the xor-butterfly inside the group (draw.cu:181-189): every lane of the group ends with the same sum
    for (int off = G >> 1; off > 0; off >>= 1) {
      const float px = __shfl_xor(ex, off), py = __shfl_xor(ey, off), pz = __shfl_xor(ez, off), pw = __shfl_xor(ew, off);
      ex = ex + px; ey = ey + py; ez = ez + pz; ew = ew + pw;
    }
    const long long row2 = base + group2;
    if (row2 < q.n && k2 == 0) {
      a4->out[row2] = make_float4(ex, ey, ez, ew);
      unsigned long long* const mask = a4->mask;
      if (mask) mask[row2] = field;
    }
  }
}

} // namespace

int indirect_light(MirtScene* sc, const void* d_features, int64_t n, const void* d_dirs, int num_dirs, const void* d_rot, float radius,
                   void* d_out_f32, uint64_t* d_hit_mask, uint32_t flags, hipStream_t stream)
{
  bool go = false;
  const int rc = check_table_query("mirt_indirect_light", "d_hit_mask", d_features, n, d_dirs, num_dirs, d_rot, radius, d_out_f32, d_hit_mask, flags, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  IndirectArgs q;
  q.features = reinterpret_cast<const float4*>(d_features);
  q.dirs = reinterpret_cast<const float4*>(d_dirs);
  q.rot = reinterpret_cast<const float2*>(d_rot);
  q.out = reinterpret_cast<float4*>(d_out_f32);
  q.mask = reinterpret_cast<unsigned long long*>(d_hit_mask);
  q.n = n;
  q.nodes = sc->nodes; q.unit_prim = sc->unit_prim;
  q.mats = sc->mats;
  q.planes = sc->planes; q.num_planes = sc->d.num_planes;
  q.root_ref = sc->root_ref; q.prim_base16 = sc->prim_base / 16u;
  q.num_spheres = sc->Ns;
  q.suns = sc->suns; q.num_suns = sc->d.num_suns;
  q.bulbs = sc->bulbs; q.num_bulbs = sc->d.num_bulbs;
  q.radius = radius;
  q.num_dirs = num_dirs;
  q.lds_depth = query_lds_depth(sc);
  const GroupLaunch g = group_launch(n, num_dirs, query_grid_blocks(sc, indirect_light_kernel, IWAVES_PER_SIMD, &sc->indirect_blocks));
  q.gshift = g.gshift;
  hipLaunchKernelGGL(indirect_light_kernel, dim3(g.blocks), dim3(QUERY_BLOCK), 0, stream, q);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

} // namespace mirt
