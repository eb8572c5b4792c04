// Ray queries on a built scene (include/mirt.h: mirt_trace_rays, mirt_camera_rays): the reference's hitNearest (draw.cu:292-318)
// for rays a caller supplies, its occlusion test (diffuseLight's shadow rays, draw.cu:347-352, 365-370), and the primary rays of
// a frame.  Not a path of the render: it reads the scene only and touches no render context, counter or hand-out order.
//
// trace_rays_kernel   one lane = one ray (grid-stride over the batch): the planes (checkPlane, draw.cu:581-615), then the walk
//                     of traverse_lbvh (bvh_traversal.cu:92-183) over the exact 64-byte node records, left child first -- the
//                     reference's own walk, so no vetting and no second walk is ever needed.  A lane carries the ray, 1/d, the
//                     best distance and record and a stack pointer; the stack lives in LDS ([entry][lane]), entries deeper
//                     than QUERY_STACK_LDS in a per-lane private array (scratch) that the bundled scenes rarely reach.
//                     light.hip and indirect.hip take this walk from query_walk.h; here it is written out, because as a
//                     function it cost the closest-hit kernel 21 to 37 %.
// camera_rays_kernel  one lane = one pixel: the ray sample 0 of the pixel starts with in the render (init_sample_core +
//                     primary_ray), before the Ray constructor normalises its direction.
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "query_walk.h"

#include <cmath>
#include <cstring>
#include <string>

namespace mirt {
namespace {

// 64 VGPRs: 8 waves per SIMD, 32 per CU.  LDS: QUERY_STACK_LDS x 4 B x 64 lanes = 5 KiB per wave, 160 KiB per CU at full occupancy.
constexpr int QWAVES_PER_SIMD = 8;

struct QueryArgs {
  const float4* rays;             // MirtRay: (o, tmax), (d, pad)
  uint32_t* hits;                 // MirtHit: 6 words
  long long num_rays;
  const float4* nodes;            // record heap (scene_dev.h)
  const uint32_t* unit_prim;
  const PlaneDev* planes; int num_planes;
  uint32_t root_ref;              // the exact records' root (REF_NONE: no primitive)
  uint32_t prim_base16;
  int lds_depth;                  // stack entries kept in LDS (<= QUERY_STACK_LDS)
};

template <bool ANY>
__global__ void __launch_bounds__(QUERY_BLOCK, QWAVES_PER_SIMD) trace_rays_kernel(const QueryArgs q)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];                     // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int tid = threadIdx.x;
  const long long stride = (long long)gridDim.x * QUERY_BLOCK;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(q.nodes);
  const float tmin = 0.0001f;
  for (long long i = (long long)blockIdx.x * QUERY_BLOCK + tid; i < q.num_rays; i += stride) {
    const float4 r0 = q.rays[2 * i], r1 = q.rays[2 * i + 1];
    const f3 o = mk3(r0.x, r0.y, r0.z);
    const float tmax = r0.w;
    const f3 d = normalize(mk3(r1.x, r1.y, r1.z));      // Ray(eye, dir, bounce), object.cuh:69
    const bool live = ray_is_live(tmax, d);
    float tplane = INFINITY, tbest = INFINITY;
    int plane_id = -1;
    uint32_t refbest = REF_NONE;
    if (live) nearest_plane(q.planes, q.num_planes, o, d, tplane, plane_id);
    // an occlusion query that a plane already answers needs no walk
    if (live && q.root_ref != REF_NONE && !(ANY && plane_id >= 0 && tplane < tmax)) {
      const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
      uint32_t cur = q.root_ref;
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
          if (ANY && closer && t < tmax) break;           // the first occluder ends an occlusion query
          pop = true;
        } else {
          // hit_aabb_adapted on both children, left first (bvh_traversal.cu:11-44, 149-157)
          const float4 b0 = rec[0], b1 = rec[1], b2 = rec[2];
          const uint2 ch = *reinterpret_cast<const uint2*>(rec + 3);
          bool hl, hr;
          float tel, ter;
          box_pair(b0, b1, b2, o.x, o.y, o.z, inv.x, inv.y, inv.z, tbest, tmin, hl, hr, tel, ter);
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
    const Nearest w = nearest_of<ANY>(tbest, refbest, tplane, plane_id, tmax);
    const bool report = w.report;
    const float t = w.t;
    uint32_t kind = 0u, id = 0u;
    f3 n = mk3(0.0f, 0.0f, 0.0f);
    if (report) {
      // the winner's file-order id, its normal and MirtHit's kind
      if (w.use_bvh) {
        id = q.unit_prim[(refbest & REF_OFFMASK) - q.prim_base16] & 0x7fffffffu;
        n = prim_normal(q.nodes, refbest, t, o, d);
        kind = (refbest & REF_TRI) ? MIRT_HIT_TRIANGLE : MIRT_HIT_SPHERE;
      } else {
        n = plane_normal(q.planes, plane_id, d);
        id = (uint32_t)plane_id;
        kind = MIRT_HIT_PLANE;
      }
    }
    store_hit(q.hits + 6 * i, report ? t : -1.0f, kind, id, n);
  }
}

// init_sample_core (sample 0 of local pixel i of the part) + primary_dir
__global__ void __launch_bounds__(QUERY_BLOCK) camera_rays_kernel(const RenderArgs a, float4* __restrict__ rays, long long num_pixels)
{
  const long long i = (long long)blockIdx.x * QUERY_BLOCK + threadIdx.x;
  if (i >= num_pixels) return;
  // local pixel of the part -> frame pixel, as init_sample_core does it (a part has < 2^31 pixels: checked by camera_rays)
  const uint32_t stripe_pixels = (uint32_t)a.stripe_rows * (uint32_t)a.width;
  const uint32_t lp = (uint32_t)i;
  const uint32_t ls = lp / stripe_pixels;
  const uint32_t within = lp - ls * stripe_pixels;
  const uint32_t gs = ls * (uint32_t)a.num_parts + (uint32_t)a.part;
  const uint32_t wy = within / (uint32_t)a.width;
  const int py = (int)(gs * (uint32_t)a.stripe_rows + wy);
  const int px = (int)(within - wy * (uint32_t)a.width);
  const uint32_t pixel = (uint32_t)py * (uint32_t)a.width + (uint32_t)px;
  Xorwow rng;
  rng.v0 = rng.v1 = rng.v2 = rng.v3 = rng.v4 = rng.d = 0; rng.bm_flag = 0; rng.bm_extra = 0.0f;
  // curand_init(1234 + pixel, 0, 0) for spp > 1 (draw.cu:162), curand_init(1234, pixel, 0) otherwise (draw.cu:105): the tables
  // camera_rays loaded say which
  if (a.needs_rng) xw_init(rng, a.rng, pixel, 0u);
  float fx = (float)px, fy = (float)py;
  if (a.spp >= 1) {
    const float jx = randD(-0.5f, 0.5f, rng);
    const float jy = randD(-0.5f, 0.5f, rng);
    fx = (float)px + jx; fy = (float)py + jy;
  }
  const RayS r = primary_dir(a, fx, fy, rng);
  // hitNearest answers a bounce-0 ray with nothing (draw.cu:294)
  rays[2 * i] = make_float4(r.o.x, r.o.y, r.o.z, r.bounce == 0 ? 0.0f : INFINITY);
  rays[2 * i + 1] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
}

} // namespace

int trace_rays(MirtScene* sc, const void* d_rays, int64_t num_rays, void* d_hits, uint32_t flags, hipStream_t stream)
{
  if ((flags & ~(uint32_t)MIRT_QUERY_ANY_HIT) != 0u) { set_error("mirt_trace_rays: unknown flag bits"); return MIRT_ERR_ARG; }
  if (num_rays < 0) { set_error("mirt_trace_rays: negative num_rays"); return MIRT_ERR_ARG; }
  if (num_rays > 0 && (!d_rays || !d_hits)) { set_error("mirt_trace_rays: null buffer"); return MIRT_ERR_ARG; }
  if (((uintptr_t)d_rays & 15u) != 0u || ((uintptr_t)d_hits & 3u) != 0u) {
    set_error("mirt_trace_rays: d_rays must be 16-byte aligned, d_hits 4-byte aligned"); return MIRT_ERR_ARG;
  }
  if (!sc->built) { set_error("mirt_trace_rays: call mirt_build_lbvh first"); return MIRT_ERR_STATE; }
  if (num_rays == 0) return MIRT_OK;
  query_grid_blocks(sc, trace_rays_kernel<false>, QWAVES_PER_SIMD, &sc->query_blocks);      // (both instances run on the closest-hit instance's grid)
  QueryArgs q;
  q.rays = reinterpret_cast<const float4*>(d_rays);
  q.hits = reinterpret_cast<uint32_t*>(d_hits);
  q.num_rays = num_rays;
  fill_walk_args(q, sc);
  return (flags & MIRT_QUERY_ANY_HIT) ? launch_rows(sc, trace_rays_kernel<true>, QWAVES_PER_SIMD, &sc->query_blocks, num_rays, q, stream)
                                      : launch_rows(sc, trace_rays_kernel<false>, QWAVES_PER_SIMD, &sc->query_blocks, num_rays, q, stream);
}

int camera_rays(MirtScene* sc, const MirtRenderParams* p, void* d_rays, hipStream_t stream)
{
  const int64_t npix = render_num_pixels(p);
  if (npix < 0 || p->spp < 0) { set_error("mirt_camera_rays: bad parameters"); return MIRT_ERR_ARG; }
  if (npix > 0 && !d_rays) { set_error("mirt_camera_rays: null buffer"); return MIRT_ERR_ARG; }
  if (((uintptr_t)d_rays & 15u) != 0u) { set_error("mirt_camera_rays: d_rays must be 16-byte aligned"); return MIRT_ERR_ARG; }
  bool go = false;
  int rc = check_frame("mirt_camera_rays", p, npix, &go);
  if (rc != MIRT_OK || !go) return rc;
  RenderArgs a;
  memset(&a, 0, sizeof(a));
  fill_camera(a, sc, p);
  a.spp = p->spp;
  // the primary ray consumes random numbers for the jitter (spp >= 1) and the lens (depth of field), nothing else
  a.needs_rng = (p->spp >= 1) || (sc->d.dof_focus != 0.0f && !sc->d.fisheye && !sc->d.panorama);
  if (a.needs_rng) {
    // spp > 1: sample 0's tables -- any cached sample table covers it (a render's larger one is not evicted); else the per-pixel
    // tables of the frame
    rc = ensure_rng_tables(&sc->rng, p->spp > 1 ? 1 : 0, (long long)p->width * p->height, stream, &a.rng, true);
    if (rc != MIRT_OK) return rc;
  }
  const int blocks = (int)((npix + QUERY_BLOCK - 1) / QUERY_BLOCK);
  hipLaunchKernelGGL(camera_rays_kernel, dim3(blocks), dim3(QUERY_BLOCK), 0, stream, a, reinterpret_cast<float4*>(d_rays), (long long)npix);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

} // namespace mirt
