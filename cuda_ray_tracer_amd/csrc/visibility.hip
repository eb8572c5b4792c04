// Hemisphere visibility at surface points (include/mirt_visibility.h: mirt_hemisphere_visibility): which of
// K directions of a caller's table, turned into the frame of each row's normal, are free of geometry within a radius, their
// weighted sum (the unnormalised bent normal and the visible weight) and the mask.  Like the ray queries and the direct light it
// reads the scene only and touches no render context, counter, hand-out table or RNG table.
//
// hemisphere_visibility_kernel  the shape of direct_light_kernel (light.hip): one lane = one (row, direction) pair.  G is the next
//                      power of two >= K: a wave serves 64 / G rows at a time (grid-stride, a wave-uniform trip count), lane
//                      g G + k owns direction k of the wave's row g, lanes with k >= K idle.  A lane builds its ray and does the
//                      any-hit walk of trace_rays_kernel<true> (query.hip), written out here: walk<true> of query_walk.h, which
//                      light.hip and indirect.hip use, measured up to 0.7 % slower in this kernel (section 6n).  One ballot
//                      of "visible" is the wave's 64-bit word, of which a row's mask is its G-bit field; the four channels are summed by an
//                      xor-butterfly inside the group, whose order the header fixes, so every lane of a group ends with the same
//                      bits and the group's first lane writes them.
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "../../include/mirt_visibility.h"

#include <cmath>

namespace mirt {
namespace {

// the query kernel's budget: 64 VGPRs, 8 waves per SIMD; QUERY_STACK_LDS x 4 B x 64 lanes = 5 KiB of LDS per wave
constexpr int VWAVES_PER_SIMD = 8;

struct VisArgs {
  const float4* features;         // mirt_hit_features rows: (P, hit), (n, _)
  const float4* dirs;             // K rows (lx, ly, lz, w)
  const float2* rot;              // nullable: n rows (c, r)
  float4* out;
  unsigned long long* mask;       // nullable
  long long n;
  const float4* nodes;            // record heap (scene_dev.h)
  const PlaneDev* planes; int num_planes;
  uint32_t root_ref;              // the exact records' root (REF_NONE: no primitive)
  float radius;
  int num_dirs;                   // K
  int lds_depth;                  // stack entries kept in LDS (<= QUERY_STACK_LDS)
  int gshift;                     // G = 1 << gshift lanes per row
};

__global__ void __launch_bounds__(QUERY_BLOCK, VWAVES_PER_SIMD) hemisphere_visibility_kernel(const VisArgs q)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];                     // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int G = 1 << q.gshift;
  const int rows_per_wave = 64 >> q.gshift;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(q.nodes);
  const float tmin = 0.0001f;
  // (the same for every lane of a wave: the loop below is uniform, so that every lane reaches the ballot and the exchange)
  const long long wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (QUERY_BLOCK / 64) + (threadIdx.x >> 6)));
  const long long stride = (long long)gridDim.x * (QUERY_BLOCK / 64) * rows_per_wave;
  for (long long base = wave * rows_per_wave; base < q.n; base += stride) {
    // (as in direct_light_kernel: what a lane derives from its index is derived again in every pass, and again after the walk,
    // from a copy of the index the compiler cannot tie to the others, so that none of it lives across the passes or the walk)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    // (likewise the uniform tests on these two are made where they are needed, not kept in scalar register pairs from before the loop)
    uint32_t root_ref = q.root_ref;
    int num_planes = q.num_planes;
    asm volatile("" : "+s"(root_ref), "+s"(num_planes));
    const int k = tid & (G - 1);                          // this lane's direction
    const int group = (tid & 63) >> q.gshift;             // ... and its row among the wave's
    const long long row = base + group;
    const bool in_range = row < q.n;
    float4 f0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), f1 = f0;
    if (in_range) { f0 = q.features[2 * row]; f1 = q.features[2 * row + 1]; }
    const bool hit_row = f0.w != 0.0f;
    bool visible = false;
    f3 u = mk3(0.0f, 0.0f, 0.0f);
    if (hit_row && k < q.num_dirs) {
      // the origin of diffuseLight's shadow rays (draw.cu:340, 346) and the frame of the normal (Duff et al. 2017)
      const f3 P = mk3(f0.x, f0.y, f0.z), ng = mk3(f1.x, f1.y, f1.z);
      const f3 N = normalize(ng);
      const f3 o = P + ng * EPSILON;
      const float s = copysignf(1.0f, N.z);
      const float a = -1.0f / (s + N.z);
      const float b = (N.x * N.y) * a;
      const f3 T = mk3(1.0f + ((s * N.x) * N.x) * a, s * b, (-s) * N.x);
      const f3 B = mk3(b, s + (N.y * N.y) * a, -N.y);
      const float4 dk = q.dirs[k];
      float x = dk.x, y = dk.y;
      if (q.rot) {
        const float2 cr = q.rot[row];
        x = cr.x * dk.x - cr.y * dk.y;
        y = cr.y * dk.x + cr.x * dk.y;
      }
      const f3 dl = (T * x + B * y) + N * dk.z;
      const f3 d = normalize(dl);                          // Ray(eye, dir, bounce), object.cuh:69 -- as mirt_trace_rays does it
      u = d;
      const float tmax = q.radius;
      // ---- the any-hit query of trace_rays_kernel<true> (query.hip) for the ray (o, tmax, d) --------------------------------
      const bool live = tmax > 0.0f && (fabsf(d.x) + fabsf(d.y) + fabsf(d.z)) > 0.0f;
      float tplane = INFINITY, tbest = INFINITY;
      int plane_id = -1;
      uint32_t refbest = REF_NONE;
      if (live) nearest_plane(q.planes, num_planes, o, d, tplane, plane_id);
      // an occlusion query that a plane already answers needs no walk
      if (live && root_ref != REF_NONE && !(plane_id >= 0 && tplane < tmax)) {
        const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        uint32_t cur = root_ref;
        int sp = 0;
        for (;;) {
          const float4* rec = reinterpret_cast<const float4*>(heap + (cur << 4));
          bool pop;
          if (cur & REF_LEAF) {
            // intersect_leaf_primitives, bvh_traversal.cu:47-89
            float t = 0.0f;
            bool hit;
            if (cur & REF_TRI) {
              hit = triangle_hit(rec[0], rec[1], rec[2], o, d, t);
            } else {
              float tc, t_far;
              hit = sphere_hit(rec[0], o, d, t, tc, t_far);
            }
            const bool closer = closer_hit(hit, t, tbest, cur & REF_OFFMASK, refbest);
            tbest = closer ? t : tbest;
            refbest = closer ? cur : refbest;
            if (closer && t < tmax) break;                  // the first occluder ends an occlusion query
            pop = true;
          } else {
            // hit_aabb_adapted on both children, left first (bvh_traversal.cu:11-44, 149-157)
            const float4 b0 = rec[0], b1 = rec[1], b2 = rec[2];
            const uint2 ch = *reinterpret_cast<const uint2*>(rec + 3);
            bool hl, hr;
            float tel, ter;
            box_pair(b0, b1, b2, o.x, o.y, o.z, inv.x, inv.y, inv.z, tbest, tmin, hl, hr, tel, ter);
            if (hl && hr) {
              // (the tree is at most 58 levels deep, DESIGN.md section 1: sp stays below STACK_TOTAL; the mask only bounds the index)
              if (sp < q.lds_depth) lds_stack[sp * QUERY_BLOCK + tid] = ch.y;
              else spill[(sp - q.lds_depth) & (STACK_TOTAL - 1)] = ch.y;
              ++sp;
            }
            cur = hl ? ch.x : ch.y;
            pop = !(hl || hr);
          }
          if (pop) {
            if (sp == 0) break;
            --sp;
            cur = sp < q.lds_depth ? lds_stack[sp * QUERY_BLOCK + tid] : spill[(sp - q.lds_depth) & (STACK_TOTAL - 1)];
          }
        }
      }
      // what the query reports as kind != 0: an occluder of the tree or a plane, nearer than tmax
      const bool occluded = (refbest != REF_NONE && tbest < tmax) || (plane_id >= 0 && tplane < tmax);
      visible = !occluded;
    }
    // this direction's term: the weight times the unit direction, and the weight
    int tid2 = threadIdx.x;
    asm volatile("" : "+v"(tid2));
    const int k2 = tid2 & (G - 1);
    float ex = 0.0f, ey = 0.0f, ez = 0.0f, ew = 0.0f;
    if (visible) {
      const float w = q.dirs[k2].w;
      ex = w * u.x; ey = w * u.y; ez = w * u.z; ew = w;
    }
    const unsigned long long word = __ballot(visible);
    const int lane2 = tid2 & 63, group2 = lane2 >> q.gshift;
    const unsigned long long field = ((word >> (group2 << q.gshift)) << (64 - G)) >> (64 - G);
    // the xor-butterfly inside the group (draw.cu:181-189): every lane of the group ends with the same sum
    for (int off = G >> 1; off > 0; off >>= 1) {
      const float px = __shfl_xor(ex, off), py = __shfl_xor(ey, off), pz = __shfl_xor(ez, off), pw = __shfl_xor(ew, off);
      ex = ex + px; ey = ey + py; ez = ez + pz; ew = ew + pw;
    }
    const long long row2 = base + group2;
    if (row2 < q.n && k2 == 0) {
      q.out[row2] = make_float4(ex, ey, ez, ew);
      if (q.mask) q.mask[row2] = field;
    }
  }
}

} // namespace

int hemisphere_visibility(MirtScene* sc, const void* d_features, int64_t n, const void* d_dirs, int num_dirs, const void* d_rot, float radius,
                          void* d_out_f32, uint64_t* d_vis_mask, uint32_t flags, hipStream_t stream)
{
  bool go = false;
  const int rc = check_table_query("mirt_hemisphere_visibility", "d_vis_mask", d_features, n, d_dirs, num_dirs, d_rot, radius, d_out_f32, d_vis_mask, flags, sc->built, &go);
  if (rc != MIRT_OK || !go) return rc;
  VisArgs q;
  q.features = reinterpret_cast<const float4*>(d_features);
  q.dirs = reinterpret_cast<const float4*>(d_dirs);
  q.rot = reinterpret_cast<const float2*>(d_rot);
  q.out = reinterpret_cast<float4*>(d_out_f32);
  q.mask = reinterpret_cast<unsigned long long*>(d_vis_mask);
  q.n = n;
  q.nodes = sc->nodes;
  q.planes = sc->planes; q.num_planes = sc->d.num_planes;
  q.root_ref = sc->root_ref;
  q.radius = radius;
  q.num_dirs = num_dirs;
  q.lds_depth = query_lds_depth(sc);
  const GroupLaunch g = group_launch(n, num_dirs, query_grid_blocks(sc, hemisphere_visibility_kernel, VWAVES_PER_SIMD, &sc->vis_blocks));
  q.gshift = g.gshift;
  hipLaunchKernelGGL(hemisphere_visibility_kernel, dim3(g.blocks), dim3(QUERY_BLOCK), 0, stream, q);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

} // namespace mirt
