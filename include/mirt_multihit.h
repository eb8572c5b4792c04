/* mirt_multihit.h -- extension of mirt.h: multi-hit ray queries on a built scene (the k nearest hits along a ray and the number of all).
 *
 * One entry point more than mirt.h declares, in a header of its own so that mirt.h, mirt_light.h, mirt_visibility.h,
 * mirt_indirect.h, mirt_closest.h and the binding tables held to them stay as they are.  libmirt.so exports
 * the symbol beside the others; callers detect the feature by the symbol (MIRT_VERSION stays 3).  Everything mirt.h says about
 * handles, device pointers, streams and status codes holds here.
 */
#ifndef MIRT_MULTIHIT_H
#define MIRT_MULTIHIT_H

#include "mirt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIRT_MULTIHIT_MAX_K 8

/* ---- multi-hit: for each ray every plane, sphere and triangle it meets before tmax -- the k nearest as records, and how many ----- */
/* d_rays:   num_rays MirtRay rows, device memory, 16-byte aligned, as for mirt_trace_rays: (o, tmax), (d, pad); d is normalised
 *           once by vec3::normalize ((0, 0, 0) when its length is below 1e-6, else each component times 1 / length).
 * k:        0 to MIRT_MULTIHIT_MAX_K: the records per ray.
 * d_hits:   num_rays * k MirtHit records (24 B each, 4-byte aligned); ray i's j-th nearest hit is record i * k + j.  All k records
 *           of every ray are always written; the slots past the ray's hits are the miss record of mirt_trace_rays (t = -1, kind =
 *           MIRT_HIT_NONE, id = 0, n = (0, 0, 0)).  May be NULL only when k == 0.
 * d_counts: NULL (unless k == 0), or num_rays uint32, 4-byte aligned: the number of ALL admitted hits of the ray.  It may exceed k.
 * flags:    must be 0.
 *
 * All arithmetic is float32 with one IEEE rounding per operation (no fused multiply-add), IEEE division and square root.
 * dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z; sums and differences of vectors and a scalar times a vector are taken per component.
 *
 * Rays that are not live.  A ray with tmax <= 0 or NaN, or whose direction normalises to (0, 0, 0) or holds a NaN, is not live:
 * count 0 and k miss records.  This is mirt_trace_rays' rule.
 *
 * The admitted set S of a live ray (o, d, tmax) is what the reference's walk (hitNearest, draw.cu:292-318; traverse_lbvh,
 * bvh_traversal.cu:92-183) accepts when its bound is held at tmax and never shrinks:
 *   Planes.  Plane j (nor, point of MirtPlane j) is admitted (checkPlane, draw.cu:581-615, as each plane is tested) when
 *       t = dot(point - o, nor) / dot(d, nor)
 *       !(t <= 1e-6)  and  t > 0.001  and  t < 2147483648.0f  and  t < tmax.
 *   Tree.  The root of the scene's tree (mirt_get_tree) is entered untested.  A child box is entered when
 *       te < tx  and  te < tmax  and  tx > 1e-4,
 *     te and tx being hit_aabb_adapted's values (bvh_traversal.cu:11-44) over the exact float32 box: per axis
 *       a = (min - o) * (1 / d),  b = (max - o) * (1 / d)   (the difference rounded, then the product; 1 / d one division),
 *       te = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz)),  tx = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)).
 *     A leaf reached this way is admitted when its primitive test reports a hit with 1e-6 < t < tmax:
 *     Sphere (c, r), checkSphereIntersectionSoA (struct.cu:64-109):
 *       cr0 = c - o;  inside = dot(cr0, cr0) < r * r;  tc = dot(cr0, d);  dv = (o + tc * d) - c;  d2 = dot(dv, dv)
 *       toff = sqrtf(r * r - d2);  t = inside ? tc + toff : tc - toff
 *       hit = !(!inside && tc < 0) && !(!inside && r * r < d2)
 *     Triangle (p0, nor, e1, e2 of the scene's record), checkTriangleIntersectionSoA (struct.cu:111-163):
 *       denom = dot(d, nor);  t = dot(p0 - o, nor) / denom;  ip = t * d + o
 *       b1 = dot(e1, ip - p0);  b2 = dot(e2, ip - p0);  b0 = (1 - b1) - b2
 *       hit = !(fabsf(denom) < 1e-9) && !(t <= 0.001) && b0 >= -0.001 && b1 >= -0.001 && b2 >= -0.001
 *   No bound changes during the walk, so S does not depend on the visiting order: an implementation may visit the boxes in any order.
 *
 * The answer is defined by the tree, not by the scene's arrays.  A float32 triangle hit in the barycentric tolerance band, or a hit
 * far from the origin, can lie outside every box that holds its primitive (DESIGN.md sections 1 and 7.4), and no bounded slack makes
 * a box walk equal to a brute force over the arrays.  This is the position mirt_trace_rays takes: the reference's result by
 * construction.
 *
 * Order.  The hits of S ascend by (t, class, index): t compared as floats; on an exact tie a plane comes before a sphere or a
 * triangle (hitNearest: the tree's hit wins only when strictly nearer); among planes the lower index first; among spheres and
 * triangles the earlier sorted leaf first (the leaf order of mirt_get_tree -- the reference's left-first walk keeps the first of a tie).
 *
 * What is written.  The records are the first min(k, |S|) hits of that order, then misses; the count is |S|.  kind, id (file order
 * within the kind; a plane's index) and the normal are exactly what mirt_trace_rays writes for that primitive at that t, p = t d + o:
 *   sphere:   normalize(inside ? c - p : p - c);   triangle: dot(d, nor) < 0 ? nor : -nor;   plane: dot(nor, d) < 0 ? nor : -nor.
 *
 * Relation to mirt_trace_rays.  Call a ray regular when, for every primitive whose test above accepts it with t < tmax, the primitive
 * is in S and its t is greater than te of every box on its path from the root.  On a regular ray record 0 is the record
 * mirt_trace_rays (closest hit, same tmax) gives, bit for bit, and count > 0 is the MIRT_QUERY_ANY_HIT boolean.  On other rays the two
 * walks may differ: hitNearest's shrinking bound, and its first bound of +inf rather than tmax, cull differently within an ulp.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per ray.  Reads the scene
 * only -- record heap and planes -- and touches no render context, MirtStats counter, hand-out table or random-number table: it may
 * run on another stream while a frame is in flight.  Ordering a query in flight before mirt_scene_set_planes or a geometry update is
 * the caller's duty, as for mirt_trace_rays.
 * num_rays == 0: MIRT_OK, nothing launched, nothing written.  MIRT_ERR_ARG (all checked on the host, before any device work): null
 * scene; num_rays < 0; k outside 0..MIRT_MULTIHIT_MAX_K; non-zero flags; with num_rays > 0 a null d_rays, a null d_hits with k > 0, a
 * null d_counts with k == 0; a misaligned buffer; d_hits (24 * num_rays * k bytes), d_counts (4 * num_rays) or d_rays (32 * num_rays)
 * overlapping each other.  MIRT_ERR_STATE before mirt_build_lbvh (and between a geometry update and its rebuild).  Every message
 * names mirt_trace_rays_multi. */
int mirt_trace_rays_multi(MirtScene* sc, const void* d_rays, int64_t num_rays, int k, void* d_hits, uint32_t* d_counts, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_MULTIHIT_H */
