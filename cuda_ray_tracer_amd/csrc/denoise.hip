// Image-space denoising of a frame (include/mirt.h: mirt_hit_features, mirt_denoise, mirt_denoise_work_bytes; DESIGN.md section
// 6f).  Not in the reference, which writes the sample mean as it is.  An edge-avoiding a-trous wavelet filter (Dammertz et al.
// 2010) steered by the first-hit geometry of the ray queries and by the per-pixel variance estimate the adaptive-sampling
// moments give (the weights of Schied et al. 2017, without the temporal part).  Nothing here reads a scene's records, a render
// context, a counter or a hand-out table.
//
// hit_features_kernel    one lane per ray: (P, hit), (n, 0) from the ray and its closest-hit record.
// denoise_prepare_kernel one lane per pixel: mean colour S / n and the variance of the mean (mirt_select_pixels' e:
//                        variance_of_mean, device_common.h).
// denoise_iter_kernel    one lane per pixel, a 64 x 4 pixel tile per block (tile_xy, device_common.h; one wave per row of the tile:
//                        a wave's loads of a tap are 64 consecutive pixels, 1 KiB of colour, 2 KiB of features): the 3 x 3 variance prefilter,
//                        then the 25 taps at distance s, from global memory (the L1 / L2 serve the reuse between neighbours;
//                        DESIGN.md section 6f has the measurement against a tile staged in LDS, or says that there is none).
//                        No atomics, no LDS, no communication between lanes: every output depends on its inputs only, so the
//                        result does not depend on timing.
#include "scene_dev.h"
#include "host_scene.h"

#include <cmath>

namespace mirt {
namespace {

constexpr int DBLOCK = 256;
static_assert(TILE_W * TILE_H == DBLOCK, "denoise_iter_kernel: one lane per pixel of the tile");

__global__ void __launch_bounds__(DBLOCK) hit_features_kernel(const float4* __restrict__ rays, const uint32_t* __restrict__ hits, long long n,
                                                               float4* __restrict__ features)
{
  const long long i = (long long)blockIdx.x * DBLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t* const h = hits + 6 * i;
  float4 f0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), f1 = f0;
  if (h[1] != (uint32_t)MIRT_HIT_NONE) hit_feature_rows(rays[2 * i], rays[2 * i + 1], h, f0, f1);
  features[2 * i] = f0;
  features[2 * i + 1] = f1;
}

__global__ void __launch_bounds__(DBLOCK) denoise_prepare_kernel(const float4* __restrict__ accum, const float4* __restrict__ accum_sq,
                                                                  const uint32_t* __restrict__ counts, long long n, float4* __restrict__ colour,
                                                                  float* __restrict__ variance)
{
  const long long i = (long long)blockIdx.x * DBLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = counts[i];
  float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float v = 0.0f;
  if (k != 0u) {
    const float4 S = accum[i];
    const float nf = (float)k;
    c = make_float4(S.x / nf, S.y / nf, S.z / nf, S.w / nf);
    if (k >= 2u) {
      const float4 Q = accum_sq[i];
      v = fmaxf(variance_of_mean(S.x, Q.x, nf), fmaxf(variance_of_mean(S.y, Q.y, nf), variance_of_mean(S.z, Q.z, nf)));
    }
  }
  colour[i] = c;
  variance[i] = v;
}

struct IterArgs {
  const float4* colour_in; const float* var_in;
  const float4* features;
  float4* colour_out; float* var_out;
  int width, height, step;
  float sigma_c, sigma_n, sigma_p;
};

__global__ void __launch_bounds__(DBLOCK) denoise_iter_kernel(const IterArgs a)
{
  int x, y;
  tile_xy(x, y);
  if (x >= a.width || y >= a.height) return;
  const long long W = a.width;
  const long long p = (long long)y * W + x;
  const float4 cp = a.colour_in[p];
  if (!finite3(cp)) {      // a non-finite pixel is neither filtered nor spread
    a.colour_out[p] = cp;
    a.var_out[p] = a.var_in[p];
    return;
  }
  // the variance the colour weight is scaled by: 3 x 3, (1 2 1; 2 4 2; 1 2 1) / 16, coordinates clamped, summed in row-major order
  float g = 0.0f;
  {
    const int xm = x > 0 ? x - 1 : 0, xp = x + 1 < a.width ? x + 1 : x;
    const int ym = y > 0 ? y - 1 : 0, yp = y + 1 < a.height ? y + 1 : y;
    const float* const r0 = a.var_in + (long long)ym * W;
    const float* const r1 = a.var_in + (long long)y * W;
    const float* const r2 = a.var_in + (long long)yp * W;
    g = 0.0625f * r0[xm];
    g = g + 0.125f * r0[x];
    g = g + 0.0625f * r0[xp];
    g = g + 0.125f * r1[xm];
    g = g + 0.25f * r1[x];
    g = g + 0.125f * r1[xp];
    g = g + 0.0625f * r2[xm];
    g = g + 0.125f * r2[x];
    g = g + 0.0625f * r2[xp];
  }
  const float den_c = a.sigma_c * sqrtf(g) + 1e-10f;
  const float4 fp0 = a.features[2 * p], fp1 = a.features[2 * p + 1];
  const bool hit_p = fp0.w != 0.0f;
  const f3 Pp = mk3(fp0.x, fp0.y, fp0.z), np_ = mk3(fp1.x, fp1.y, fp1.z);
  float sw = 0.0f, sv = 0.0f;
  float4 sc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float kern[3] = {0.375f, 0.25f, 0.0625f};
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = y + a.step * dy;
    if (qy < 0 || qy >= a.height) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + a.step * dx;
      if (qx < 0 || qx >= a.width) continue;
      const float h = kern[dx < 0 ? -dx : dx] * kern[dy < 0 ? -dy : dy];
      const long long q = (long long)qy * W + qx;
      const float4 cq = a.colour_in[q];
      if (!finite3(cq)) continue;
      float e = 0.0f;      // the centre's exponent is 0 by definition
      if (dx != 0 || dy != 0) {
        const float4 fq0 = a.features[2 * q];
        const bool hit_q = fq0.w != 0.0f;
        if (hit_p != hit_q) continue;
        float a_n = 0.0f, a_p = 0.0f;
        if (hit_p) {
          const float4 fq1 = a.features[2 * q + 1];
          a_n = fmaxf(0.0f, 1.0f - dot(np_, mk3(fq1.x, fq1.y, fq1.z))) / a.sigma_n;
          const f3 D = mk3(fq0.x, fq0.y, fq0.z) - Pp;
          const float len = length(D);
          a_p = len == 0.0f ? 0.0f : fabsf(dot(np_, D)) / (a.sigma_p * len);
        }
        const float a_c = fmaxf(fmaxf(fabsf(cp.x - cq.x), fabsf(cp.y - cq.y)), fabsf(cp.z - cq.z)) / den_c;
        const float t = (a_n + a_p) + a_c;
        if (t != t) continue;
        e = fminf(t, 87.0f);
      }
      const float w = h * dm_expf(-e);
      sw = sw + w;
      sc.x = sc.x + w * cq.x; sc.y = sc.y + w * cq.y; sc.z = sc.z + w * cq.z; sc.w = sc.w + w * cq.w;
      sv = sv + (w * w) * a.var_in[q];
    }
  }
  a.colour_out[p] = make_float4(sc.x / sw, sc.y / sw, sc.z / sw, sc.w / sw);
  a.var_out[p] = sv / (sw * sw);
}

} // namespace

int hit_features(MirtScene* sc, const void* d_rays, const void* d_hits, int64_t n, void* d_features, hipStream_t stream)
{
  if (n < 0) { set_error("mirt_hit_features: negative n"); return MIRT_ERR_ARG; }
  if (n > 0 && (!d_rays || !d_hits || !d_features)) { set_error("mirt_hit_features: null buffer"); return MIRT_ERR_ARG; }
  if (!is_aligned(16, d_rays, d_features) || !is_aligned(4, d_hits)) {
    set_error("mirt_hit_features: d_rays and d_features must be 16-byte aligned, d_hits 4-byte aligned"); return MIRT_ERR_ARG;
  }
  if (n >= 0x7fffffffll * DBLOCK) { set_error("mirt_hit_features: too many rays"); return MIRT_ERR_ARG; }
  if (!sc->built) { set_error("mirt_hit_features: call mirt_build_lbvh first"); return MIRT_ERR_STATE; }
  if (n == 0) return MIRT_OK;
  hipLaunchKernelGGL(hit_features_kernel, dim3((unsigned)((n + DBLOCK - 1) / DBLOCK)), dim3(DBLOCK), 0, stream, (const float4*)d_rays, (const uint32_t*)d_hits,
                     (long long)n, (float4*)d_features);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

size_t denoise_work_bytes(const MirtRenderParams* p)
{
  const int64_t n = p ? render_num_pixels(p) : -1;
  if (n < 0 || p->num_parts != 1) return 0;
  return (size_t)n * 40u;      // two float4 colour buffers, two float variance buffers
}

int denoise(const MirtRenderParams* p, const void* d_accum, const void* d_accum_sq, const uint32_t* d_counts, const void* d_features, int iterations,
            float sigma_c, float sigma_n, float sigma_p, void* d_work, void* d_out, hipStream_t stream)
{
  const int64_t n = render_num_pixels(p);
  if (n < 0) { set_error("mirt_denoise: bad render parameters"); return MIRT_ERR_ARG; }
  if (p->num_parts != 1) { set_error("mirt_denoise: whole frames only (num_parts must be 1: a striped part has no neighbours across stripes)"); return MIRT_ERR_ARG; }
  if (iterations < 0 || iterations > 8) { set_error("mirt_denoise: iterations must be in [0, 8]"); return MIRT_ERR_ARG; }
  if (!positive_finite(sigma_c) || !positive_finite(sigma_n) || !positive_finite(sigma_p)) {
    set_error("mirt_denoise: sigma_c, sigma_n and sigma_p must be finite and positive"); return MIRT_ERR_ARG;
  }
  if (!d_accum || !d_accum_sq || !d_counts || !d_features || !d_work || !d_out) { set_error("mirt_denoise: null pointer"); return MIRT_ERR_ARG; }
  if (!is_aligned(16, d_accum, d_accum_sq, d_features, d_work, d_out) || !is_aligned(4, d_counts)) {
    set_error("mirt_denoise: the float buffers must be 16-byte aligned, d_counts 4-byte aligned"); return MIRT_ERR_ARG;
  }
  if (n >= 0x7fffffffll || p->height > 65535 * TILE_H) { set_error("mirt_denoise: frame too large"); return MIRT_ERR_ARG; }
  const size_t N = (size_t)n;
  const struct { const void* ptr; size_t bytes; } inputs[4] = {{d_accum, 16 * N}, {d_accum_sq, 16 * N}, {d_counts, 4 * N}, {d_features, 32 * N}};
  for (const auto& in : inputs) {
    if (overlaps(d_out, 16 * N, in.ptr, in.bytes) || overlaps(d_work, 40 * N, in.ptr, in.bytes)) {
      set_error("mirt_denoise: d_out and d_work must not overlap an input"); return MIRT_ERR_ARG;
    }
  }
  if (overlaps(d_out, 16 * N, d_work, 40 * N)) { set_error("mirt_denoise: d_out and d_work must not overlap"); return MIRT_ERR_ARG; }
  if (n == 0) return MIRT_OK;
  float4* const colour[2] = {(float4*)d_work, (float4*)d_work + N};
  float* const var[2] = {(float*)((float4*)d_work + 2 * N), (float*)((float4*)d_work + 2 * N) + N};
  hipLaunchKernelGGL(denoise_prepare_kernel, dim3((unsigned)((n + DBLOCK - 1) / DBLOCK)), dim3(DBLOCK), 0, stream, (const float4*)d_accum,
                     (const float4*)d_accum_sq, d_counts, (long long)n, iterations == 0 ? (float4*)d_out : colour[0], var[0]);
  const dim3 grid = tile_grid(p->width, p->height);
  for (int i = 0; i < iterations; ++i) {
    IterArgs a;
    a.colour_in = colour[i & 1]; a.var_in = var[i & 1];
    a.features = (const float4*)d_features;
    a.colour_out = i == iterations - 1 ? (float4*)d_out : colour[(i + 1) & 1]; a.var_out = var[(i + 1) & 1];
    a.width = p->width; a.height = p->height; a.step = 1 << i;
    a.sigma_c = sigma_c; a.sigma_n = sigma_n; a.sigma_p = sigma_p;
    hipLaunchKernelGGL(denoise_iter_kernel, grid, dim3(DBLOCK), 0, stream, a);
  }
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

} // namespace mirt
