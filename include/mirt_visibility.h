/* mirt_visibility.h -- extension of mirt.h: hemisphere visibility at surface points (ambient occlusion, sky irradiance, bent normals).
 *
 * One entry point more than mirt.h declares, in a header of its own so that mirt.h, mirt_light.h and the binding tables held to
 * them stay as they are.  libmirt.so exports the symbol beside the others; callers detect the feature by
 * the symbol (MIRT_VERSION stays 3).  Everything mirt.h says about handles, device pointers, streams and status codes holds here.
 */
#ifndef MIRT_VISIBILITY_H
#define MIRT_VISIBILITY_H

#include "mirt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- hemisphere visibility: which of K directions above each of n surface points are free of geometry within a radius ---------- */
/* d_features: n rows of mirt_hit_features' layout, (Px, Py, Pz, hit) (nx, ny, nz, _), 32 B each, 16-byte aligned: the rows that
 *             call wrote, or rows the caller made for points of its own (probes, texels).  The last word of a row is not read.
 * d_dirs:     K = num_dirs rows (lx, ly, lz, w), float4, device memory, 16-byte aligned: a direction in the row's local frame, z
 *             along the normal, and a weight.  Taken as given (any length, any sign).  1 <= K <= 64.
 * d_rot:      NULL, or n float2 (c, r), 8-byte aligned: a rotation of the table about the normal for each row, taken as given
 *             (the caller brings the cosine and the sine; no trigonometry and no random number is made on the device).
 * radius:     how far a ray looks: positive, or +inf.
 * d_out_f32:  n float4, 16-byte aligned: (bx, by, bz, a).
 * d_vis_mask: NULL, or n uint64, 8-byte aligned: bit k of word i is set when direction k is unoccluded at point i.
 * flags:      must be 0.
 *
 * All arithmetic is float32 with one IEEE rounding per operation (no fused multiply-add), IEEE division and square root;
 * normalize is vec3::normalize (vec3.cuh:72-82: (0, 0, 0) when the length is below 1e-6, else each component times 1 / length);
 * dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z; a vector times a scalar is taken per component.  Row i:
 *     hit == 0: out = (0, 0, 0, 0), mask = 0; nothing is traced.  Otherwise
 *     ng = (nx, ny, nz), taken as given;  N = normalize(ng);  o = P + ng * 0.001f  (the product rounded, then the sum: draw.cu:346)
 *     s = copysignf(1.0f, N.z);  a = -1.0f / (s + N.z);  b = (N.x * N.y) * a
 *     T = (1.0f + ((s * N.x) * N.x) * a,  s * b,  (-s) * N.x)
 *     B = (b,  s + (N.y * N.y) * a,  -N.y)                               (Duff et al. 2017, the branch-free orthonormal basis)
 *     direction k, (lx, ly, lz, w) = d_dirs[k]:
 *         d_rot == NULL: x = lx, y = ly.  Otherwise (c, r) = d_rot[i]:  x = c * lx - r * ly;  y = r * lx + c * ly
 *         d = (T * x + B * y) + N * lz
 *         the ray is MirtRay{o, tmax = radius, d}; direction k is VISIBLE exactly when mirt_trace_rays with MIRT_QUERY_ANY_HIT
 *             reports kind == 0 for it (planes first, the exact 64-byte records, the reference's order; a d that normalises to 0
 *             or NaN is a miss, hence visible)
 *         u = normalize(d);  e_k = visible ? (w * u.x, w * u.y, w * u.z, w) : (+0, +0, +0, +0);  bit k of the mask = visible
 *     G = the next power of two >= K;  e_k = +0 for K <= k < G
 *     for off = G/2, G/4, ..., 1:  every e_k = e_k + e_(k xor off), all k at once, per channel  (xor-butterfly, as draw.cu:181-189)
 *     out = e_0
 * A channel that is NaN (a NaN in the normal, the table or the rotation) is some NaN: its sign and payload are not specified.
 *
 * With weights that sum to 1, a is the visible fraction of the hemisphere -- one minus the ambient occlusion -- and (bx, by, bz)
 * the unnormalised bent normal; with the weights set to a sky's radiance times the solid-angle measure, a is the sky's irradiance.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per (row, direction)
 * pair; the order of the sum is the one above whatever the number of lanes, so the result does not depend on timing.  Reads the
 * scene only -- record heap and planes -- and touches no render context, MirtStats counter, hand-out table or random-number
 * table: it may run on another stream while a frame is in flight.  Ordering a query in flight before mirt_scene_set_planes or a
 * geometry update is the caller's duty, as for mirt_trace_rays.
 * n == 0: MIRT_OK, nothing launched.  MIRT_ERR_ARG (all checked on the host, before any device work): null scene; n < 0;
 * num_dirs outside 1..64; a radius that is NaN or <= 0; non-zero flags; with n > 0 a null or misaligned d_features, d_dirs or
 * d_out_f32, or a misaligned d_rot or d_vis_mask; d_out_f32 (16 n bytes) or d_vis_mask (8 n) overlapping d_features (32 n),
 * d_dirs (16 K), d_rot (8 n) or each other.  MIRT_ERR_STATE before mirt_build_lbvh. */
int mirt_hemisphere_visibility(MirtScene* sc, const void* d_features, int64_t n, const void* d_dirs, int num_dirs, const void* d_rot,
                               float radius, void* d_out_f32, uint64_t* d_vis_mask, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_VISIBILITY_H */
