/* mirt_closest.h -- extension of mirt.h: closest-point queries on a built scene (the nearest surface to a point, within a radius).
 *
 * One entry point more than mirt.h declares, in a header of its own so that mirt.h, mirt_light.h, mirt_visibility.h,
 * mirt_indirect.h and the binding tables held to them stay as they are.  libmirt.so exports the symbol beside
 * the others; callers detect the feature by the symbol (MIRT_VERSION stays 3).  Everything mirt.h says about handles, device
 * pointers, streams and status codes holds here.
 */
#ifndef MIRT_CLOSEST_H
#define MIRT_CLOSEST_H

#include "mirt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- closest points: for each of n points the nearest plane, sphere or triangle of the scene nearer than the row's radius ------ */
/* d_points:   n rows (qx, qy, qz, R), float4, device memory, 16-byte aligned: the point q and the row's search radius R (positive,
 *             or +inf), the way MirtRay carries tmax.
 * d_hits:     n MirtHit records (24 B each, 4-byte aligned): t is the distance, kind / id are as mirt_trace_rays reports them
 *             (file order within the kind; a plane is MIRT_HIT_PLANE with its index), n is the surface normal at the closest point,
 *             turned towards q.  A miss is (t = -1, kind = MIRT_HIT_NONE, id = 0, n = (0, 0, 0)), as a ray's.
 * d_features: NULL, or n rows of mirt_hit_features' layout, (Px, Py, Pz, 1) (nx, ny, nz, 0), 32 B each, 16-byte aligned, written
 *             with two 16-byte stores: P is the closest point, n the normal of the hit record.  A miss writes eight +0.  The rows
 *             are what mirt_direct_light, mirt_hemisphere_visibility and mirt_indirect_light take.
 * flags:      must be 0.
 *
 * All arithmetic is float32 with one IEEE rounding per operation (no fused multiply-add), IEEE division and square root.
 * dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z;  length(v) = sqrtf(dot(v, v));  normalize is vec3::normalize as in mirt_visibility.h:
 * (0, 0, 0) when the length is below 1e-6, else each component times 1 / length.  Sums and differences of vectors and a vector
 * times a scalar are taken per component, one rounding each; -v flips each sign bit (so -(+0) is -0).
 *
 * Row rule.  A row with !(R > 0) (zero, negative, NaN), or with a NaN or infinite coordinate, is a miss.  Otherwise EVERY plane,
 * sphere and triangle of the scene is a candidate with a distance dist, a point P and a normal n as below.  A candidate is admitted
 * when dist < R (a NaN dist never is).  The answer is the admitted candidate with the smallest (dist, kind, id), compared
 * lexicographically -- dist as floats, then kind (sphere 1 < triangle 2 < plane 3), then the index -- and a miss if none is
 * admitted.  The answer is so defined by the scene's arrays alone, not by the tree, its boxes or any visiting order: an
 * implementation may visit the candidates in any order and leave out any it can prove loses.
 *
 * Plane j (kind 3; nor, point of MirtPlane j):
 *     N = normalize(nor);  s = dot(N, q - point);  dist = fabsf(s)
 *     P = q - N * s;       n = s < 0 ? -N : N
 * Sphere (c, r) (kind 1):
 *     v = q - c;  l = length(v);  dist = fabsf(l - r)
 *     u = normalize(v);  P = c + u * r;  n = l < r ? -u : u
 *     (q within 1e-6 of the centre: u = (0, 0, 0), so P = c and n is zero in every component -- -0 for r > l -- and dist =
 *     fabsf(l - r), which is r to rounding)
 * Triangle (kind 2): a, b, c = p0, p1, p2 of the file-order vertex array (what mirt_scene_get_triangles reads), nor the normal of
 * the scene's record (MirtTriangle.nor; after mirt_scene_update_triangles the one that call computed).  The closest point by
 * Voronoi region (Ericson, Real-Time Collision Detection, section 5.1.5), in this order, the first region that matches wins:
 *     ab = b - a;  ac = c - a;  ap = q - a;  d1 = dot(ab, ap);  d2 = dot(ac, ap)
 *         d1 <= 0 && d2 <= 0:                 P = a
 *     bp = q - b;  d3 = dot(ab, bp);  d4 = dot(ac, bp)
 *         d3 >= 0 && d4 <= d3:                P = b
 *     vc = d1 * d4 - d3 * d2
 *         vc <= 0 && d1 >= 0 && d3 <= 0:      P = a + ab * (d1 / (d1 - d3))
 *     cp = q - c;  d5 = dot(ab, cp);  d6 = dot(ac, cp)
 *         d6 >= 0 && d5 <= d6:                P = c
 *     vb = d5 * d2 - d1 * d6
 *         vb <= 0 && d2 >= 0 && d6 <= 0:      P = a + ac * (d2 / (d2 - d6))
 *     va = d3 * d6 - d5 * d4;  e = d4 - d3;  f = d5 - d6
 *         va <= 0 && e >= 0 && f >= 0:        P = b + (c - b) * (e / (e + f))
 *     otherwise  den = 1 / ((va + vb) + vc);  P = (a + ab * (vb * den)) + ac * (vc * den)
 *     w = q - P;  dist = length(w);  n = dot(w, nor) < 0 ? -nor : nor
 * A triangle without area is not special: where these operations divide zero by zero its dist is NaN and it is never admitted;
 * where a vertex or an edge region matches first it is a candidate like any other (its nor is (0, 0, 0), so n is).
 *
 * Pruning (informative; it cannot change the answer).  The kernel walks the scene's tree and leaves a subtree out when the point's
 * distance to the subtree's box exceeds the best admitted distance so far -- R at the start -- by MORE than a slack
 *     sigma = 2^-18 * (max(|qx|, |qy|, |qz|) + C),   C the largest coordinate magnitude of the scene's box,
 * computed once per row: a float32 leaf box does not bound the float32 distance of its own primitive (a sphere's box is c -+ r
 * rounded, a computed P may leave its triangle's box by a rounding), and sigma exceeds every rounding between the two (DESIGN.md
 * section 6o has the count; it holds for coordinates between 2^-40 and 2^40 in magnitude and for triangles whose barycentric sum
 * (va + vb) + vc is not itself rounding noise).  A subtree whose box distance equals the best is visited: the (kind, id) tie-break
 * needs it.  The children are visited nearer box first.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per row.  Reads the scene
 * only -- record heap, vertex array and planes -- and touches no render context, MirtStats counter, hand-out table or random-number
 * table: it may run on another stream while a frame is in flight.  Ordering a query in flight before mirt_scene_set_planes or a
 * geometry update is the caller's duty, as for mirt_trace_rays.
 * n == 0: MIRT_OK, nothing launched.  MIRT_ERR_ARG (all checked on the host, before any device work): null scene; n < 0; non-zero
 * flags; with n > 0 a null or misaligned d_points or d_hits, or a misaligned d_features; d_hits (24 n bytes) or d_features (32 n)
 * overlapping d_points (16 n) or each other.  MIRT_ERR_STATE before mirt_build_lbvh (and between a geometry update and its
 * rebuild).  Every message names mirt_closest_points. */
int mirt_closest_points(MirtScene* sc, const void* d_points, int64_t n, void* d_hits, void* d_features, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_CLOSEST_H */
