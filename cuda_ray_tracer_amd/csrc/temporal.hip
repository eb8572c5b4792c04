// Temporal accumulation (include/mirt.h: mirt_scene_get_spheres, mirt_scene_get_triangles, mirt_prev_features,
// mirt_temporal_accumulate).  Not in the reference, which renders every frame from nothing.  The previous
// frame's per-pixel moments are carried to the surface points this frame's pixels see (reprojection through the previous camera
// and the previous geometry), validated against the previous frame's hit features with the denoiser's normal and plane terms,
// and added to this frame's moments -- the result is again (accum, accum_sq, counts), which mirt_denoise, mirt_select_pixels and
// mirt_finalize_counts consume as they are.  Nothing here touches a render context, a counter or a hand-out table.
//
// get_spheres_kernel / get_triangles_kernel  one lane per primitive: the scene's file-order arrays back out, the inverse of update.hip.
// prev_features_kernel      one lane per ray: hit_features' rows (hit_feature_rows, device_common.h), then what moved replaced by
//                           the hit point and normal as they were in the previous geometry.
// temporal_kernel           one lane per pixel, a 64 x 4 pixel tile per block (tile_xy, device_common.h; one wave per row of the tile: a
//                           wave's own-pixel traffic is consecutive 16-byte loads and stores); the four bilinear taps of the
//                           history are gathers from global memory that neighbouring lanes share through the L1 / L2.  No atomics,
//                           no LDS, no communication between lanes: every output depends on its inputs only.  A lane reads the
//                           current-frame buffers at its own pixel only and before it writes, so the outputs may be those buffers.
#include "scene_dev.h"
#include "host_scene.h"

#include <cmath>
#include <string>

namespace mirt {
namespace {

constexpr int TBLOCK = 256;
static_assert(TILE_W * TILE_H == TBLOCK, "temporal_kernel: one lane per pixel of the tile");

__global__ __launch_bounds__(TBLOCK) void get_spheres_kernel(const float4* __restrict__ spheres, float4* __restrict__ out, int count)
{
  const int i = (int)(blockIdx.x * TBLOCK + threadIdx.x);
  if (i >= count) return;
  out[i] = spheres[i];
}

// 9 floats out per triangle (4-byte aligned: dword stores)
__global__ __launch_bounds__(TBLOCK) void get_triangles_kernel(const float4* __restrict__ verts, float* __restrict__ out, int count)
{
  const int i = (int)(blockIdx.x * TBLOCK + threadIdx.x);
  if (i >= count) return;
  const float4* const v = verts + 3 * (size_t)i;
  const float4 p0 = v[0], p1 = v[1], p2 = v[2];
  float* const o = out + 9 * (size_t)i;
  o[0] = p0.x; o[1] = p0.y; o[2] = p0.z;
  o[3] = p1.x; o[4] = p1.y; o[5] = p1.z;
  o[6] = p2.x; o[7] = p2.y; o[8] = p2.z;
}

__global__ void __launch_bounds__(TBLOCK) prev_features_kernel(const float4* __restrict__ rays, const uint32_t* __restrict__ hits, long long n,
                                                                const float4* __restrict__ spheres, int num_spheres, const float4* __restrict__ tris,
                                                                int num_tris, const float4* __restrict__ prev_xyzr, const float* __restrict__ prev_verts,
                                                                float4* __restrict__ features)
{
  const long long i = (long long)blockIdx.x * TBLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t* const h = hits + 6 * i;
  const uint32_t kind = h[1], id = h[2];
  float4 f0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), f1 = f0;
  if (kind != (uint32_t)MIRT_HIT_NONE) {
    hit_feature_rows(rays[2 * i], rays[2 * i + 1], h, f0, f1);
    const f3 P = mk3(f0.x, f0.y, f0.z), nr = mk3(f1.x, f1.y, f1.z);
    if (kind == (uint32_t)MIRT_HIT_SPHERE && prev_xyzr) {
      if (id >= (uint32_t)num_spheres) {
        f0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f); f1 = f0;
      } else {
        const float4 s = spheres[id], sp = prev_xyzr[id];
        const f3 u = (P - mk3(s.x, s.y, s.z)) / s.w;
        const float qx = u.x * sp.w, qy = u.y * sp.w, qz = u.z * sp.w;
        f0 = make_float4(sp.x + qx, sp.y + qy, sp.z + qz, 1.0f);
      }
    } else if (kind == (uint32_t)MIRT_HIT_TRIANGLE && prev_verts) {
      if (id >= (uint32_t)num_tris) {
        f0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f); f1 = f0;
      } else {
        const float4 t0 = tris[3 * (size_t)id], t1 = tris[3 * (size_t)id + 1], t2 = tris[3 * (size_t)id + 2];
        const f3 p0 = mk3(t0.x, t0.y, t0.z), nor = mk3(t0.w, t1.x, t1.y), e1 = mk3(t1.z, t1.w, t2.x), e2 = mk3(t2.y, t2.z, t2.w);
        const f3 v = P - p0;
        const float b1 = dot(e1, v), b2 = dot(e2, v);
        const float* const pv = prev_verts + 9 * (size_t)id;
        const f3 q0 = mk3(pv[0], pv[1], pv[2]), q1 = mk3(pv[3], pv[4], pv[5]), q2 = mk3(pv[6], pv[7], pv[8]);
        const f3 d1 = q1 - q0, d2 = q2 - q0;
        const f3 a = mk3(b1 * d1.x, b1 * d1.y, b1 * d1.z), b = mk3(b2 * d2.x, b2 * d2.y, b2 * d2.z);
        const f3 Q = (q0 + a) + b;
        f3 nn = normalize(cross(d1, d2));
        if (dot(nr, nor) < 0.0f) nn = -nn;
        f0 = make_float4(Q.x, Q.y, Q.z, 1.0f);
        f1 = make_float4(nn.x, nn.y, nn.z, 0.0f);
      }
    }
  }
  features[2 * i] = f0;
  features[2 * i + 1] = f1;
}

struct TemporalArgs {
  const float4* accum; const float4* accum_sq; const uint32_t* counts;      // this frame (may be the outputs)
  const float4* prev_features;
  const float4* hist_accum; const float4* hist_accum_sq; const uint32_t* hist_counts;
  const float4* hist_features;
  float4* out_accum; float4* out_accum_sq; uint32_t* out_counts;
  int width, height;
  uint32_t max_history;
  float sigma_n, sigma_p;
  f3 eye, forward, right, up;      // the previous camera
};

// One axis of the reprojected position: snapped to a pixel centre within 1 / 1024, split into the first tap's coordinate and the
// second tap's weight.  false: both taps are outside [0, size) (or the position is a NaN).
MIRT_DEV bool split_axis(float x, int size, int* first, float* frac)
{
  const float r = rintf(x);
  if (fabsf(x - r) <= 0.0009765625f) x = r;
  if (!(x > -1.0f && x < (float)size)) return false;      // floor(x) in [-1, size - 1] (x == -1: the only tap inside has weight 0)
  const float fl = floorf(x);
  *first = (int)fl;
  *frac = x - fl;
  return true;
}

__global__ void __launch_bounds__(TBLOCK) temporal_kernel(const TemporalArgs a)
{
  int x, y;
  tile_xy(x, y);
  if (x >= a.width || y >= a.height) return;
  const long long W = a.width;
  const long long p = (long long)y * W + x;
  const float4 cS = a.accum[p], cQ = a.accum_sq[p];
  const uint32_t ck = a.counts[p];
  float4 hS = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hQ = hS;
  uint32_t hk = 0u;
  const float4 g0 = a.prev_features[2 * p];
  if (g0.w != 0.0f) {
    const float4 g1 = a.prev_features[2 * p + 1];
    const f3 P = mk3(g0.x, g0.y, g0.z), nP = mk3(g1.x, g1.y, g1.z);
    const f3 v = P - a.eye;
    const float f = dot(v, a.forward) / dot(a.forward, a.forward);
    int x0 = 0, y0 = 0;
    float tx = 0.0f, ty = 0.0f;
    bool inside = f > 0.0f && (f - f) == 0.0f;
    if (inside) {
      const float max_dim = fmaxf((float)a.width, (float)a.height);
      const float sx = dot(v, a.right) / dot(a.right, a.right) / f;
      const float sy = dot(v, a.up) / dot(a.up, a.up) / f;
      const float fx = (sx * max_dim + (float)a.width) / 2.0f;
      const float fy = ((float)a.height - sy * max_dim) / 2.0f;
      inside = split_axis(fx, a.width, &x0, &tx);
      inside = split_axis(fy, a.height, &y0, &ty) && inside;
      if (inside) {
        const float foot = length(v) * 2.0f / max_dim;
        const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty};
        float4 tS[4], tQ[4];
        float tw[4];
        uint32_t tk[4];
        float sw = 0.0f;
        uint32_t kmin = 0xffffffffu;
        int exact = -1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int t = 2 * j + i;
            tw[t] = 0.0f;      // (0: the tap is dropped)
            tk[t] = 0u;
            tS[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); tQ[t] = tS[t];
            const int qx = x0 + i, qy = y0 + j;
            if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height) continue;
            const float w = wx[i] * wy[j];
            if (w == 0.0f) continue;
            const long long q = (long long)qy * W + qx;
            const uint32_t kq = a.hist_counts[q];
            if (kq == 0u) continue;
            const float4 Sq = a.hist_accum[q], Qq = a.hist_accum_sq[q];
            if (!finite3(Sq) || !finite3(Qq)) continue;
            const float4 fq0 = a.hist_features[2 * q];
            if (fq0.w == 0.0f) continue;
            const float4 fq1 = a.hist_features[2 * q + 1];
            const float c = 1.0f - dot(nP, mk3(fq1.x, fq1.y, fq1.z));
            const float a_n = (c < 0.0f ? 0.0f : c) / a.sigma_n;      // (a NaN stays one)
            const f3 D = mk3(fq0.x, fq0.y, fq0.z) - P;
            const float a_p = fabsf(dot(nP, D)) / (a.sigma_p * fmaxf(length(D), foot));
            if (!(a_n + a_p <= 1.0f)) continue;      // (also a NaN)
            tw[t] = w; tk[t] = kq; tS[t] = Sq; tQ[t] = Qq;
            sw = sw + w;
            kmin = kq < kmin ? kq : kmin;
            if (w == 1.0f) exact = t;
          }
        }
        if (exact >= 0) {      // the position is a pixel centre: that pixel's history as it is (the other taps had weight 0)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (t == exact) { hS = tS[t]; hQ = tQ[t]; hk = tk[t]; }
        } else if (sw != 0.0f) {
          float4 ms = make_float4(0.0f, 0.0f, 0.0f, 0.0f), mq = ms;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            if (tw[t] == 0.0f) continue;
            const float wn = tw[t] / sw;
            const float kf = (float)tk[t];
            ms.x = ms.x + wn * (tS[t].x / kf); ms.y = ms.y + wn * (tS[t].y / kf); ms.z = ms.z + wn * (tS[t].z / kf); ms.w = ms.w + wn * (tS[t].w / kf);
            mq.x = mq.x + wn * (tQ[t].x / kf); mq.y = mq.y + wn * (tQ[t].y / kf); mq.z = mq.z + wn * (tQ[t].z / kf); mq.w = mq.w + wn * (tQ[t].w / kf);
          }
          hk = kmin;
          const float kh = (float)hk;
          hS = make_float4(ms.x * kh, ms.y * kh, ms.z * kh, ms.w * kh);
          hQ = make_float4(mq.x * kh, mq.y * kh, mq.z * kh, mq.w * kh);
        }
        if (hk > a.max_history) {
          const float s = (float)a.max_history / (float)hk;
          hS = make_float4(hS.x * s, hS.y * s, hS.z * s, hS.w * s);
          hQ = make_float4(hQ.x * s, hQ.y * s, hQ.z * s, hQ.w * s);
          hk = a.max_history;
        }
      }
    }
  }
  if (hk == 0u) {      // no history: the frame's own moments, bit for bit (x + 0 would turn -0 into +0)
    a.out_accum[p] = cS;
    a.out_accum_sq[p] = cQ;
    a.out_counts[p] = ck;
    return;
  }
  a.out_accum[p] = make_float4(cS.x + hS.x, cS.y + hS.y, cS.z + hS.z, cS.w + hS.w);
  a.out_accum_sq[p] = make_float4(cQ.x + hQ.x, cQ.y + hQ.y, cQ.z + hQ.z, cQ.w + hQ.w);
  a.out_counts[p] = ck + hk;
}

f3 host3(const MirtVec3& v) { f3 r; r.x = v.x; r.y = v.y; r.z = v.z; return r; }

} // namespace

int get_spheres(MirtScene* sc, int first, int count, void* d_xyzr_out, hipStream_t stream)
{
  bool go = false;
  const int rc = check_range("mirt_scene_get_spheres", d_xyzr_out, first, count, sc->Ns, 16, &go);
  if (rc != MIRT_OK || !go) return rc;
  hipLaunchKernelGGL(get_spheres_kernel, dim3((unsigned)((count + TBLOCK - 1) / TBLOCK)), dim3(TBLOCK), 0, stream, sc->spheres + first,
                     static_cast<float4*>(d_xyzr_out), count);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

int get_triangles(MirtScene* sc, int first, int count, void* d_verts_out, hipStream_t stream)
{
  bool go = false;
  const int rc = check_range("mirt_scene_get_triangles", d_verts_out, first, count, sc->Nt, 4, &go);
  if (rc != MIRT_OK || !go) return rc;
  hipLaunchKernelGGL(get_triangles_kernel, dim3((unsigned)((count + TBLOCK - 1) / TBLOCK)), dim3(TBLOCK), 0, stream, sc->tri_verts + 3 * (size_t)first,
                     static_cast<float*>(d_verts_out), count);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

int prev_features(MirtScene* sc, const void* d_rays, const void* d_hits, int64_t n, const void* d_prev_xyzr, const void* d_prev_verts, void* d_features,
                  hipStream_t stream)
{
  if (n < 0) { set_error("mirt_prev_features: negative n"); return MIRT_ERR_ARG; }
  if (n > 0 && (!d_rays || !d_hits || !d_features)) { set_error("mirt_prev_features: null buffer"); return MIRT_ERR_ARG; }
  if (!is_aligned(16, d_rays, d_features, d_prev_xyzr) || !is_aligned(4, d_hits, d_prev_verts)) {
    set_error("mirt_prev_features: d_rays, d_features and d_prev_xyzr must be 16-byte aligned, d_hits and d_prev_verts 4-byte aligned"); return MIRT_ERR_ARG;
  }
  if (n >= 0x7fffffffll * TBLOCK) { set_error("mirt_prev_features: too many rays"); return MIRT_ERR_ARG; }
  if (!sc->built) { set_error("mirt_prev_features: call mirt_build_lbvh first"); return MIRT_ERR_STATE; }
  if (n == 0) return MIRT_OK;
  hipLaunchKernelGGL(prev_features_kernel, dim3((unsigned)((n + TBLOCK - 1) / TBLOCK)), dim3(TBLOCK), 0, stream, (const float4*)d_rays, (const uint32_t*)d_hits,
                     (long long)n, sc->spheres, sc->Ns, sc->tris, sc->Nt, (const float4*)d_prev_xyzr, (const float*)d_prev_verts, (float4*)d_features);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

int temporal_accumulate(const MirtRenderParams* p, const MirtCamera* prev_camera, const void* d_accum, const void* d_accum_sq, const uint32_t* d_counts,
                        const void* d_prev_features, const void* d_hist_accum, const void* d_hist_accum_sq, const uint32_t* d_hist_counts,
                        const void* d_hist_features, int max_history, float sigma_n, float sigma_p, void* d_out_accum, void* d_out_accum_sq,
                        uint32_t* d_out_counts, hipStream_t stream)
{
  const char* const who = "mirt_temporal_accumulate";
  const int64_t n = render_num_pixels(p);
  if (n < 0) { set_error(std::string(who) + ": bad render parameters"); return MIRT_ERR_ARG; }
  if (p->num_parts != 1) { set_error(std::string(who) + ": whole frames only (num_parts must be 1: a reprojected pixel may land in another stripe)"); return MIRT_ERR_ARG; }
  if (prev_camera->fisheye != 0 || prev_camera->panorama != 0 || prev_camera->dof_focus != 0.0f) {
    set_error(std::string(who) + ": prev_camera must be a pinhole (fisheye, panorama and dof_focus 0)"); return MIRT_ERR_ARG;
  }
  if (max_history < 1) { set_error(std::string(who) + ": max_history must be at least 1"); return MIRT_ERR_ARG; }
  if (!positive_finite(sigma_n) || !positive_finite(sigma_p)) { set_error(std::string(who) + ": sigma_n and sigma_p must be finite and positive"); return MIRT_ERR_ARG; }
  if (!d_accum || !d_accum_sq || !d_counts || !d_prev_features || !d_hist_accum || !d_hist_accum_sq || !d_hist_counts || !d_hist_features || !d_out_accum ||
      !d_out_accum_sq || !d_out_counts) {
    set_error(std::string(who) + ": null pointer"); return MIRT_ERR_ARG;
  }
  if (!is_aligned(16, d_accum, d_accum_sq, d_prev_features, d_hist_accum, d_hist_accum_sq, d_hist_features, d_out_accum, d_out_accum_sq) ||
      !is_aligned(4, d_counts, d_hist_counts, d_out_counts)) {
    set_error(std::string(who) + ": the float buffers must be 16-byte aligned, the counts 4-byte aligned"); return MIRT_ERR_ARG;
  }
  const size_t N = (size_t)n;
  struct Range { const void* ptr; size_t bytes; };
  const Range outs[3] = {{d_out_accum, 16 * N}, {d_out_accum_sq, 16 * N}, {d_out_counts, 4 * N}};
  const Range cur[3] = {{d_accum, 16 * N}, {d_accum_sq, 16 * N}, {d_counts, 4 * N}};
  const Range others[5] = {{d_prev_features, 32 * N}, {d_hist_accum, 16 * N}, {d_hist_accum_sq, 16 * N}, {d_hist_counts, 4 * N}, {d_hist_features, 32 * N}};
  for (int o = 0; o < 3; ++o) {
    for (int c = 0; c < 3; ++c) {
      if (o == c && outs[o].ptr == cur[c].ptr) continue;      // in place: a lane reads its own pixel only, before it writes
      if (overlaps(outs[o].ptr, outs[o].bytes, cur[c].ptr, cur[c].bytes)) {
        set_error(std::string(who) + ": an output may be exactly its own current-frame buffer; any other overlap with an input is refused"); return MIRT_ERR_ARG;
      }
    }
    for (const Range& in : others) {
      if (overlaps(outs[o].ptr, outs[o].bytes, in.ptr, in.bytes)) {
        set_error(std::string(who) + ": an output must not overlap d_prev_features or a history buffer"); return MIRT_ERR_ARG;
      }
    }
    for (int o2 = o + 1; o2 < 3; ++o2) {
      if (overlaps(outs[o].ptr, outs[o].bytes, outs[o2].ptr, outs[o2].bytes)) { set_error(std::string(who) + ": the outputs must not overlap each other"); return MIRT_ERR_ARG; }
    }
  }
  // (after the pointer checks, so that a caller -- or a test without a device -- learns of a bad pointer first)
  if (n >= 0x7fffffffll || p->height > 65535 * TILE_H) { set_error(std::string(who) + ": frame too large"); return MIRT_ERR_ARG; }
  if (n == 0) return MIRT_OK;
  TemporalArgs a;
  a.accum = (const float4*)d_accum; a.accum_sq = (const float4*)d_accum_sq; a.counts = d_counts;
  a.prev_features = (const float4*)d_prev_features;
  a.hist_accum = (const float4*)d_hist_accum; a.hist_accum_sq = (const float4*)d_hist_accum_sq; a.hist_counts = d_hist_counts;
  a.hist_features = (const float4*)d_hist_features;
  a.out_accum = (float4*)d_out_accum; a.out_accum_sq = (float4*)d_out_accum_sq; a.out_counts = d_out_counts;
  a.width = p->width; a.height = p->height;
  a.max_history = (uint32_t)max_history;
  a.sigma_n = sigma_n; a.sigma_p = sigma_p;
  a.eye = host3(prev_camera->eye); a.forward = host3(prev_camera->forward); a.right = host3(prev_camera->right); a.up = host3(prev_camera->up);
  hipLaunchKernelGGL(temporal_kernel, tile_grid(p->width, p->height), dim3(TBLOCK), 0, stream, a);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

} // namespace mirt
