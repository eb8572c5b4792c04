// Direct light at surface points (include/mirt_light.h: mirt_direct_light): the reference's diffuseLight
// (draw.cu:329-377) for an object colour of (1,1,1) and roughness 0, as a query on a built scene.  Every light of the scene is
// shadow-tested from every row of a mirt_hit_features buffer.  Like the ray queries it reads the scene only and touches no render
// context, counter, hand-out table or RNG table.
//
// direct_light_kernel  one lane = one (row, light) pair.  With L lights, G is the next power of two >= max(L, 1): a wave serves
//                      64 / G rows at a time (grid-stride), lane g G + li owns light li of the wave's row g, lanes with li >= L
//                      idle.  A lane does the facing test, then the any-hit walk of its one shadow ray -- the walk of
//                      trace_rays_kernel<true> (query.hip): walk<true> of query_walk.h, which indirect.hip uses too (DESIGN.md
//                      section 6n).
//                      The lane of a light that reaches the point then computes that light's term; one
//                      ballot of "facing and not occluded" is the wave's 64-bit word, of which a row's mask is its G-bit field;
//                      and the terms are summed in light order, every lane of a group fetching term li of its group in step
//                      li.  The sum order is fixed by construction, so the result's bits do not depend on this shape.
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"
#include "query_walk.h"
#include "../../include/mirt_light.h"

#include <cmath>

namespace mirt {
namespace {

// the query kernel's budget: 64 VGPRs, 8 waves per SIMD; QUERY_STACK_LDS x 4 B x 64 lanes = 5 KiB of LDS per wave
constexpr int LWAVES_PER_SIMD = 8;

struct LightArgs {
  const float4* features;         // mirt_hit_features rows: (P, hit), (n, _)
  float4* out;
  unsigned long long* mask;       // nullable
  long long n;
  const float4* nodes;            // record heap (scene_dev.h)
  const PlaneDev* planes; int num_planes;
  uint32_t root_ref;              // the exact records' root (REF_NONE: no primitive)
  const LightDev* suns; int num_suns;
  const LightDev* bulbs; int num_bulbs;
  float expose;                   // (+inf, which set_expose leaves a term at, also stands for MIRT_LIGHT_RAW)
  int lds_depth;                  // stack entries kept in LDS (<= QUERY_STACK_LDS)
  int gshift;                     // G = 1 << gshift lanes per row
};

__global__ void __launch_bounds__(QUERY_BLOCK, LWAVES_PER_SIMD) direct_light_kernel(const LightArgs q)
{
  __shared__ uint32_t lds_stack[QUERY_STACK_LDS * QUERY_BLOCK];
  uint32_t spill[STACK_TOTAL];                     // (entries lds_depth.. of the lane's stack: the rarely taken spill path)
  const int G = 1 << q.gshift;
  const int rows_per_wave = 64 >> q.gshift;
  const int nlights = q.num_suns + q.num_bulbs;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(q.nodes);
  // (the same for every lane of a wave: the loop below is uniform, so that every lane reaches the ballot and the exchange)
  const long long wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (QUERY_BLOCK / 64) + (threadIdx.x >> 6)));
  const long long stride = (long long)gridDim.x * (QUERY_BLOCK / 64) * rows_per_wave;
  for (long long base = wave * rows_per_wave; base < q.n; base += stride) {
    // (what a lane derives from its index -- its light, its row -- is derived again in every pass, and again after the walk, from
    // a copy of the index the compiler cannot tie to the others: nothing of it then stays in registers across the passes or the
    // walk, which is what keeps the kernel within the 64 registers of 8 waves per SIMD)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    // (likewise the uniform tests on these two are made where they are needed, not kept in scalar register pairs from before the loop)
    uint32_t root_ref = q.root_ref;
    int num_planes = q.num_planes;
    asm volatile("" : "+s"(root_ref), "+s"(num_planes));
    const int li = tid & (G - 1);                         // this lane's light
    const int group = (tid & 63) >> q.gshift;             // ... and its row among the wave's
    const bool is_sun = li < q.num_suns;
    const LightDev* const lt = is_sun ? q.suns + li : q.bulbs + (li - q.num_suns);
    const long long row = base + group;
    const bool in_range = row < q.n;
    float4 f0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), f1 = f0;
    if (in_range) { f0 = q.features[2 * row]; f1 = q.features[2 * row + 1]; }
    const bool hit_row = f0.w != 0.0f;
    bool lit = false;
    float lam = 0.0f, tmax = INFINITY;
    if (hit_row && li < nlights) {
      // diffuseLight's prologue and the shadow ray of light li (draw.cu:340, 346 / 362-363)
      const f3 P = mk3(f0.x, f0.y, f0.z), ng = mk3(f1.x, f1.y, f1.z);
      const f3 N = normalize(ng);
      const f3 o = P + ng * EPSILON;
      f3 L, d;
      light_ray(lt, is_sun, P, L, d, tmax);
      lam = dot(N, L);
      if (lam > 0.0f) {
        // the any-hit query of trace_rays_kernel<true> (query.hip) for the ray (o, tmax, d)
        float tbest, tplane;
        uint32_t refbest;
        int plane_id;
        walk<true>(heap, root_ref, q.planes, num_planes, o, d, tmax, lds_stack, spill, q.lds_depth, tid, tbest, refbest, tplane, plane_id);
        // what the query reports as kind != 0: an occluder of the tree or a plane, nearer than tmax
        const bool occluded = (refbest != REF_NONE && tbest < tmax) || (plane_id >= 0 && tplane < tmax);
        lit = !occluded;
      }
    }
    // this light's term (getColorSun / getColorBulb, helper.cu, for an object colour of 1)
    int tid2 = threadIdx.x;
    asm volatile("" : "+v"(tid2));
    const int li2 = tid2 & (G - 1);
    const bool is_sun2 = li2 < q.num_suns;
    f3 term = mk3(0.0f, 0.0f, 0.0f);
    if (lit) {
      const LightDev* const lt2 = is_sun2 ? q.suns + li2 : q.bulbs + (li2 - q.num_suns);
      const float cr = lt2->r * lam, cg = lt2->g * lam, cb = lt2->b * lam;
      term = mk3(set_expose(cr, q.expose), set_expose(cg, q.expose), set_expose(cb, q.expose));
      if (!is_sun2) {
        const float i2 = 1.0f / (tmax * tmax);
        term = term * i2;
      }
    }
    const int lane2 = tid2 & 63, group2 = lane2 >> q.gshift;
    const unsigned long long field = group_field(lit, lane2, q.gshift);
    // the sum in light order: in step k every lane fetches term k of its group (only the group's first lane keeps the result)
    f3 acc = mk3(0.0f, 0.0f, 0.0f);
    const int first = lane2 & ~(G - 1);
    for (int k = 0; k < nlights; ++k) {
      const float tr = __shfl(term.x, first + k), tg = __shfl(term.y, first + k), tb = __shfl(term.z, first + k);
      const bool on = ((field >> k) & 1ull) != 0ull;
      acc.x = on ? acc.x + tr : acc.x;
      acc.y = on ? acc.y + tg : acc.y;
      acc.z = on ? acc.z + tb : acc.z;
    }
    const long long row2 = base + group2;
    if (row2 < q.n && li2 == 0) {
      q.out[row2] = make_float4(acc.x, acc.y, acc.z, hit_row ? 1.0f : 0.0f);
      if (q.mask) q.mask[row2] = field;
    }
  }
}

} // namespace

int direct_light(MirtScene* sc, const void* d_features, int64_t n, void* d_out_f32, uint64_t* d_lit_mask, uint32_t flags, hipStream_t stream)
{
  if ((flags & ~(uint32_t)MIRT_LIGHT_RAW) != 0u) { set_error("mirt_direct_light: unknown flag bits"); return MIRT_ERR_ARG; }
  if (n < 0) { set_error("mirt_direct_light: negative n"); return MIRT_ERR_ARG; }
  if (n > 0 && (!d_features || !d_out_f32)) { set_error("mirt_direct_light: null buffer"); return MIRT_ERR_ARG; }
  if (n > 0 && (!is_aligned(16, d_features, d_out_f32) || !is_aligned(8, d_lit_mask))) {
    set_error("mirt_direct_light: d_features and d_out_f32 must be 16-byte aligned, d_lit_mask 8-byte aligned"); return MIRT_ERR_ARG;
  }
  if (n >= (1ll << 56)) { set_error("mirt_direct_light: too many rows"); return MIRT_ERR_ARG; }
  const size_t N = (size_t)n;
  if (n > 0 && (overlaps(d_out_f32, 16 * N, d_features, 32 * N) ||
                (d_lit_mask && (overlaps(d_lit_mask, 8 * N, d_features, 32 * N) || overlaps(d_lit_mask, 8 * N, d_out_f32, 16 * N))))) {
    set_error("mirt_direct_light: d_out_f32 and d_lit_mask must not overlap d_features or each other"); return MIRT_ERR_ARG;
  }
  if (!sc->built) { set_error("mirt_direct_light: call mirt_build_lbvh first"); return MIRT_ERR_STATE; }
  if (n == 0) return MIRT_OK;
  LightArgs q;
  q.features = reinterpret_cast<const float4*>(d_features);
  q.out = reinterpret_cast<float4*>(d_out_f32);
  q.mask = reinterpret_cast<unsigned long long*>(d_lit_mask);
  q.n = n;
  q.nodes = sc->nodes;
  q.planes = sc->planes; q.num_planes = sc->d.num_planes;
  q.root_ref = sc->root_ref;
  q.suns = sc->suns; q.num_suns = sc->d.num_suns;
  q.bulbs = sc->bulbs; q.num_bulbs = sc->d.num_bulbs;
  q.expose = (flags & MIRT_LIGHT_RAW) ? INFINITY : sc->d.expose;
  q.lds_depth = query_lds_depth(sc);
  const int nlights = q.num_suns + q.num_bulbs;      // (at most 64: mirt_scene_create)
  const GroupLaunch g = group_launch(n, nlights, query_grid_blocks(sc, direct_light_kernel, LWAVES_PER_SIMD, &sc->light_blocks));
  q.gshift = g.gshift;
  hipLaunchKernelGGL(direct_light_kernel, dim3(g.blocks), dim3(QUERY_BLOCK), 0, stream, q);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

} // namespace mirt
