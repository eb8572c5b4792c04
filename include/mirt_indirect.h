/* mirt_indirect.h -- extension of mirt.h: indirect light at surface points (one diffuse bounce, gathered on the device).
 *
 * One entry point more than mirt.h declares, in a header of its own so that mirt.h, mirt_light.h, mirt_visibility.h and the binding
 * tables held to them stay as they are.  libmirt.so exports the symbol beside the others; callers detect
 * the feature by the symbol (MIRT_VERSION stays 3).  Everything mirt.h says about handles, device pointers, streams and status
 * codes holds here.
 */
#ifndef MIRT_INDIRECT_H
#define MIRT_INDIRECT_H

#include "mirt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- indirect light: what K directions above each of n surface points see of the scene's directly lit surfaces ---------------- */
/* The term the reference calls globalIllumination (draw.cu:540-568), without its random numbers: the directions come from the
 * caller's table, and the surface a direction finds is shaded by its diffuse term alone.
 *
 * d_features, d_dirs (K = num_dirs rows (lx, ly, lz, w), 1 <= K <= 64), d_rot, radius and the alignment rules: exactly as in
 *             mirt_hemisphere_visibility (mirt_visibility.h).
 * d_out_f32:  n float4, 16-byte aligned: (r, g, b, a).
 * d_hit_mask: NULL, or n uint64, 8-byte aligned: bit k of word i is set when direction k hit something at point i.
 * flags:      must be 0.
 *
 * All arithmetic is float32 with one IEEE rounding per operation (no fused multiply-add), IEEE division and square root; normalize
 * and dot are those of mirt_light.h and mirt_visibility.h.  Row i:
 *     hit == 0: out = (0, 0, 0, 0), mask = 0; nothing is traced.  Otherwise
 *     N, o, T, B, the rotation and d of direction k are those of mirt_visibility.h, operation for operation.
 *     direction k, (lx, ly, lz, w) = d_dirs[k]:
 *         the gather ray is MirtRay{o, tmax = radius, d}, answered as mirt_trace_rays with flags 0 answers it: the exact 64-byte
 *             records, the reference's order, the planes afterwards, reported only if t < tmax.  The answer is a MirtHit
 *             (t, kind, id, n2).
 *         kind == 0 (a d that normalises to 0 or NaN included):  e_k = (+0, +0, +0, w);  bit k of the mask is clear.  Otherwise
 *         u = normalize(d);  P2_c = o_c + t * u_c  (the product rounded, then the sum: mirt_hit_features' expression)
 *         D = (D_r, D_g, D_b) is the acc that mirt_direct_light with MIRT_LIGHT_RAW computes for the row (P2, 1) (n2, _), every
 *             operation as mirt_light.h gives it: every sun, then every bulb, in the scene's order; N2 = normalize(n2); the facing
 *             rule !(lam > 0); the shadow origin P2 + n2 * 0.001f; a bulb's bd = point - P2, tmax = tl and 1.0f / (tl * tl); the
 *             terms added in light order.  The exposure curve is never applied: it is a tone curve on a final colour, and a
 *             gather sums radiance.  A caller applies it to the result if wanted.
 *         rho_ch = ((1.0f - shininess_ch) * (1.0f - trans_ch)) * colour_ch, from the material of primitive (kind, id) -- sphere,
 *             triangle or plane -- as the scene holds it now: the diffuse weight of the reference's mix (draw.cu:277-280, 561-563)
 *             without the reflect and refract terms (a mirror or a glass surface bounces no diffuse light) and without roughness,
 *             whose perturbation of the normal draws random numbers: it is taken as 0, as mirt_direct_light takes it.
 *         L_ch = rho_ch * D_ch;  e_k = (w * L_r, w * L_g, w * L_b, +0);  bit k of the mask is set
 *     G = the next power of two >= K;  e_k = +0 for K <= k < G
 *     the xor-butterfly of mirt_visibility.h: for off = G/2, G/4, ..., 1: every e_k = e_k + e_(k xor off), all k at once, per channel
 *     out = e_0
 * A channel that is NaN is some NaN, as in mirt_visibility.h: its sign and payload are not specified.
 *
 * Two things follow.  (1) a, and the complement of the hit mask within its K bits, are bit for bit the a channel and the mask that
 * mirt_hemisphere_visibility gives for the same arguments: the any-hit and the closest-hit query report the same boolean for the
 * same tmax.  (2) With visibility.cosine_directions(K) (w = 1 / K), (r, g, b) estimates the bounced irradiance over pi: a caller
 * multiplies by the receiving surface's own diffuse colour.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per (row, direction) pair;
 * the order of every sum is the one above whatever the number of lanes, so the result does not depend on timing.  Reads the scene
 * only -- record heap, planes, materials, light arrays -- and touches no render context, MirtStats counter, hand-out table or
 * random-number table: it may run on another stream while a frame is in flight.  Ordering a query in flight before a geometry,
 * plane, light or material update (mirt_scene_update_sphere_materials, mirt_scene_update_triangle_materials, mirt_scene_set_planes:
 * this is the first query that reads materials) is the caller's duty, as for mirt_trace_rays.
 * n == 0: MIRT_OK, nothing launched.  MIRT_ERR_ARG (all checked on the host, before any device work): null scene; n < 0;
 * num_dirs outside 1..64; a radius that is NaN or <= 0; non-zero flags; with n > 0 a null or misaligned d_features, d_dirs or
 * d_out_f32, or a misaligned d_rot or d_hit_mask; d_out_f32 (16 n bytes) or d_hit_mask (8 n) overlapping d_features (32 n),
 * d_dirs (16 K), d_rot (8 n) or each other.  MIRT_ERR_STATE before mirt_build_lbvh. */
int mirt_indirect_light(MirtScene* sc, const void* d_features, int64_t n, const void* d_dirs, int num_dirs, const void* d_rot,
                        float radius, void* d_out_f32, uint64_t* d_hit_mask, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_INDIRECT_H */
