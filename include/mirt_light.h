/* mirt_light.h -- extension of mirt.h: direct light at surface points.
 *
 * One entry point more than mirt.h declares, in a header of its own so that mirt.h and the binding table held to it stay as they
 * are.  libmirt.so exports the symbol beside the others; callers detect the feature by the symbol
 * (MIRT_VERSION stays 3).  Everything mirt.h says about handles, device pointers, streams and status codes holds here.
 */
#ifndef MIRT_LIGHT_H
#define MIRT_LIGHT_H

#include "mirt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- direct light: every light of the scene, shadow-tested, at n surface points -------------------- */
/* The reference's diffuseLight (draw.cu:329-377) for an object colour of (1, 1, 1) and roughness 0 -- the one part of its shading
 * that is a pure function of (point, normal, lights, scene) and draws no random number -- offered as a query on a built scene.
 *
 * d_features: n rows of mirt_hit_features' layout, (Px, Py, Pz, hit) (nx, ny, nz, _), 32 B each, 16-byte aligned: the rows that
 *             call wrote, or rows the caller made for points of its own (probes, texels).  The last word of a row is not read.
 * d_out_f32:  n float4, 16-byte aligned.
 * d_lit_mask: NULL, or n uint64, 8-byte aligned: bit li of word i is set when light li reaches point i.
 * flags:      0 or MIRT_LIGHT_RAW.
 *
 * All arithmetic is float32 with one IEEE rounding per operation (no fused multiply-add), IEEE division and square root;
 * normalize is vec3::normalize (vec3.cuh:72-82: (0, 0, 0) when the length is below 1e-6, else each component times 1 / length);
 * dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z; length(u) = sqrtf(dot(u, u)).  Row i:
 *     hit == 0: out = (0, 0, 0, 0), mask = 0; nothing is traced.  Otherwise
 *     ng = (nx, ny, nz), taken as given;  N = normalize(ng);  o = P + ng * 0.001f  (the product rounded, then the sum: draw.cu:346)
 *     acc = (0, 0, 0), mask = 0.  The lights in the scene's order, suns 0 .. num_suns - 1, then the bulbs; light li is bit li of
 *     the mask (a scene has at most 64 lights):
 *       sun j:   L = normalize(dir) as the scene holds it (computed once on the host, the same operations);  lam = dot(N, L)
 *                !(lam > 0): the light adds nothing and no ray is traced -- the query's own rule; it equals the reference's
 *                    fmaxf(lam, 0) factor whenever the light's colour is finite (the condition of the render's skip_unlit)
 *                the shadow ray is MirtRay{o, tmax = +inf, d = dir}; it is occluded exactly when mirt_trace_rays with
 *                    MIRT_QUERY_ANY_HIT reports kind != 0 for it (planes first, the exact 64-byte records, the reference's order)
 *                occluded: nothing is added.  Otherwise c_ch = colour_ch * lam for r, g, b;
 *                    e_ch = c_ch with MIRT_LIGHT_RAW, else setExpose (helper.cu:40-45) with the scene's current MirtShading.expose:
 *                    expose == +inf ? c_ch : (float)(1.0 - (double)expf(-expose * c_ch)), expf the library's own (mirt_probe_math
 *                    which = 1);
 *                    acc_ch = acc_ch + e_ch;  bit li is set
 *       bulb k:  bd = point - P  (from P, not from o: draw.cu:362);  tl = length(bd);  L = normalize(bd);  lam = dot(N, L)
 *                the same facing rule
 *                the shadow ray is MirtRay{o, tmax = tl, d = bd}: occluded exactly when the any-hit query reports a hit (t < tl)
 *                not occluded: i2 = 1.0f / (tl * tl);  acc_ch = acc_ch + e_ch * i2, e_ch as for a sun;  bit li is set
 *     out = (acc_r, acc_g, acc_b, 1)
 * A scene without lights therefore writes (0, 0, 0, hit != 0).
 *
 * The object colour of diffuseLight is left out, which is the colour (1, 1, 1).  So on a scene whose materials are matte white
 * (colour 1, shininess 0, trans 0, roughness 0), with gi 0 and bounces >= 1, the float4 of the first-hit point of a pixel's camera
 * ray -- mirt_camera_rays, a closest-hit mirt_trace_rays, mirt_hit_features, then this call -- is, bit for bit, that pixel's RGBA
 * in mirt_render's d_rgba_f32 at spp 0: shootPrimaryRay's weights reduce to 0 + 0 + 1 * 1 * diffuse, the render's hit point is
 * t * d + o, the expression mirt_hit_features uses, and a light the normal faces away from adds +0 in the render.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per (row, light) pair; the
 * terms of a row are added in light order whatever the number of lanes, so the result does not depend on timing.  Reads the scene
 * only -- record heap, planes, light arrays, expose -- and touches no render context, MirtStats counter, hand-out table or
 * random-number table: it may run on another stream while a frame is in flight.  Ordering a query in flight before
 * mirt_scene_set_lights, mirt_scene_set_planes or a geometry update is the caller's duty, as for mirt_trace_rays.
 * n == 0: MIRT_OK, nothing launched.  MIRT_ERR_ARG (all checked on the host, before any device work): null scene; n < 0; a null
 * or misaligned buffer with n > 0 (d_lit_mask may be NULL); unknown flag bits; d_out_f32 or d_lit_mask overlapping the feature
 * range (32 n bytes) or each other (16 n, 8 n bytes).  MIRT_ERR_STATE before mirt_build_lbvh. */
#define MIRT_LIGHT_RAW 1u
int mirt_direct_light(MirtScene* sc, const void* d_features, int64_t n, void* d_out_f32, uint64_t* d_lit_mask, uint32_t flags,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_LIGHT_H */
