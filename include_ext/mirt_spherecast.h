/* mirt_spherecast.h -- extension of mirt.h: sphere casts on a built scene (how far a ball travels along a direction before it
 * touches a surface, and where it touches).
 *
 * One entry point more than mirt.h declares, in a header of its own so that mirt.h, the extension headers under include/ and the
 * binding tables held to them stay as they are (section 6s says why this header lies in include_ext/).
 * libmirt.so exports the symbol beside the others; callers detect the feature by the symbol (MIRT_VERSION stays 3).  Everything
 * mirt.h says about handles, device pointers, streams and status codes holds here.
 */
#ifndef MIRT_SPHERECAST_H
#define MIRT_SPHERECAST_H

#include "../include/mirt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIRT_CAST_ANY_HIT 1u

/* ---- sphere casts: for each of n rows the first contact of a ball of radius r, its centre travelling from o along d, with a plane,
 * sphere or triangle of the scene ------------------------------------------------------------------------------------------------ */
/* d_casts:    n rows in MirtRay's layout, (ox, oy, oz, tmax) (dx, dy, dz, r), 32 B each, device memory, 16-byte aligned: the `pad`
 *             word carries the ball's radius r, the way MirtRay carries tmax.
 * d_hits:     n MirtHit records (24 B each, 4-byte aligned): t is the distance the ball's CENTRE travels along the unit direction
 *             until the first contact -- 0 when the ball touches or overlaps a surface at the start --, kind / id are as
 *             mirt_trace_rays reports them (file order within the kind; a plane is MIRT_HIT_PLANE with its index), n is the contact
 *             normal defined below.  A miss is (t = -1, kind = MIRT_HIT_NONE, id = 0, n = (0, 0, 0)), as a ray's.
 * d_features: NULL, or n rows of mirt_hit_features' layout, (Px, Py, Pz, 1) (nx, ny, nz, 0), 32 B each, 16-byte aligned, written
 *             with two 16-byte stores: P is the contact point on the surface, n the normal of the hit record.  A miss writes eight
 *             +0.  The rows are what mirt_direct_light, mirt_hemisphere_visibility and mirt_indirect_light take.
 * flags:      0 or MIRT_CAST_ANY_HIT.
 *
 * Arithmetic: mirt_closest.h's, word for word -- float32 with one IEEE rounding per operation (no fused multiply-add), IEEE
 * division and square root; dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z; length(v) = sqrtf(dot(v, v)); normalize: (0, 0, 0) when the
 * length is below 1e-6, else each component times 1 / length; vector sums, differences and a vector times a scalar per component,
 * one rounding each.  -x flips the sign bit.  A comparison with a NaN is false.
 *
 * Row rule.  d^ = normalize(d), as mirt_trace_rays takes a direction.  A row is live when tmax > 0, r >= 0 and r is finite, every
 * coordinate of o is finite, and |d^.x| + |d^.y| + |d^.z| > 0 (a direction shorter than 1e-6, or with a NaN or an infinity, is
 * not).  Any other row is a miss.  The centre at parameter t is
 *     C(t) = o + d^ * t            (the product rounded, then the sum).
 * Surfaces are two-sided and hollow, as in mirt_closest.h: a ball inside a large sphere meets it from inside, a plane is met from
 * either side.  EVERY plane, sphere and triangle of the scene is a candidate with a parameter t as below, or none.  A candidate is
 * admitted when 0 <= t < tmax (a NaN never is).  The answer is the admitted candidate with the smallest (t, kind, id), compared
 * lexicographically -- t as floats, then kind (sphere 1 < triangle 2 < plane 3), then the index -- and a miss if none is admitted.
 * The answer is so defined by the scene's arrays alone, never by the tree, its boxes or any visiting order: an implementation
 * may visit the candidates in any order and leave out any it can prove loses.  All candidates the ball overlaps at the start tie
 * at t = 0, and (kind, id) alone picks among them: mirt_closest_points_multi (mirt_contacts.h) with R = r lists the whole contact
 * set.
 *
 * Helpers: the centre's ray against the ball (p, R), in the closest-approach form (a discriminant b^2 - c loses the grazing cases):
 *     m = p - o;  a = dot(m, d^);  w = m - d^ * a;  h2 = R * R - dot(w, w)
 *     entry(p, R) = a - sqrtf(h2), none if !(h2 >= 0)
 *     exit(p, R)  = a + sqrtf(h2 < 0 ? 0 : h2)
 * Sphere (c, rs) (kind 1):
 *     l = length(o - c);  g = l - rs
 *     fabsf(g) <= r:  t = 0
 *     g > 0:          t = entry(c, rs + r)
 *     otherwise:      t = exit(c, rs - r)
 * Plane rule for a unit normal N and a point of the plane:
 *     s = dot(N, o - point)
 *     fabsf(s) <= r:  t = 0
 *     otherwise  dn = dot(N, d^)
 *     s > 0 && dn < 0:  t = (r - s) / dn
 *     s < 0 && dn > 0:  t = (-r - s) / dn
 *     otherwise none
 * Plane j (kind 3; nor, point of MirtPlane j): the plane rule with N = normalize(nor).
 * Triangle (kind 2): a, b, c = p0, p1, p2 of the file-order vertex array, nor the normal of the scene's record, both as in
 * mirt_closest.h.  P0 = mirt_closest.h's closest point of the triangle for q = o.
 *     length(o - P0) <= r:  t = 0
 *     otherwise t is the smallest of seven pieces; a piece counts only with t >= 0 (a NaN does not); none if no piece counts
 *     face:      tf = the plane rule with N = nor, point = a; it counts when dot(nor, nor) > 0 and mirt_closest.h's region walk for
 *                q = C(tf) falls through to its last case (none of its six vertex and edge tests matches)
 *     vertices:  entry(a, r), entry(b, r), entry(c, r)
 *     edges (a, b), (a, c), (b, c), each as (p, q):
 *         e = q - p;  ee = dot(e, e);  m = o - p;  u = dot(m, e) / ee;  k = dot(d^, e) / ee
 *         mp = m - e * u;  dp = d^ - e * k;  A = dot(dp, dp);  t0 = -dot(mp, dp) / A
 *         wv = mp + dp * t0;  h2 = r * r - dot(wv, wv);  t = t0 - sqrtf(h2 / A)
 *         it counts when ee != 0, A != 0, h2 >= 0 and 0 <= u + t * k <= 1
 * Each piece lies inside the Minkowski sum of the triangle and the ball, and together they cover its boundary, so the first entry
 * into any piece is the first contact.  The record's nor is (0, 0, 0) for every triangle whose cross product is shorter than 1e-6
 * (normalize's threshold): triangles without area, but also small ones and slivers of positive area.  A zero nor names no plane
 * (the plane rule would give s = 0 and t = 0 at any distance), so such a triangle has no face piece and is met by its edges and
 * vertices alone: a ball wider than the triangle meets them within w * w / (2 r) of the face, w the triangle's width; a smaller
 * ball, and a ray (r = 0), can pass through its interior.  A triangle without area is otherwise not special: it is the segment or
 * point its pieces make, and a NaN is never admitted.
 *
 * The winner's record.  Cw = C(t); P is mirt_closest.h's P of THAT candidate for q = Cw (a plane: Cw - N * dot(N, Cw - point); a
 * sphere: c + normalize(Cw - c) * rs; a triangle: its closest point); n = normalize(Cw - P), the direction that pushes the ball
 * out of the surface -- (0, 0, 0) when that vector is shorter than 1e-6, as for r = 0.
 *
 * MIRT_CAST_ANY_HIT.  kind != MIRT_HIT_NONE exactly when the call without the flag says so.  The record is that of AN admitted
 * candidate, made as above from its own t; it need not be the first.  The walk may end at the first admitted candidate it meets.
 *
 * Pruning (informative; it cannot change the answer).  The kernel tests the planes, then walks the scene's tree and leaves a
 * subtree out when the centre's ray misses the subtree's box grown on every side by r + sigma, or enters it later than
 * best + tau, best the smallest admitted t so far -- tmax at the start:
 *     sigma = 2^-18 * ((max(|ox|, |oy|, |oz|) + C) + r),   C the largest coordinate magnitude of the scene's box
 *     tau   = 2^-20 * best
 * At a candidate's computed t the centre is r from the primitive up to a few roundings of |o| + C + r -- the closest-approach
 * forms keep that error linear where t itself is ill-conditioned --, so it lies in every ancestor's box grown by r plus those
 * roundings and those of a sphere's own float32 box; sigma is 64 units in the last place of |o| + C + r and exceeds their sum
 * and the roundings of the slab test's own differences, and tau exceeds the three relative roundings of a slab parameter
 * (DESIGN.md section 6v has the count; it holds for coordinates between 2^-40 and 2^40 in magnitude).  The count does not cover
 * an edge piece whose path runs nearly along the edge -- A below 2^-4 with r below the foot's overshoot 5 * 2^-24 (|o| + C + r) /
 * sqrtf(A) --: there the claim that pruning cannot change the answer is made on the strength of tests alone (casts along and
 * nearly along triangle edges give the brute force's bits, in the CPU walk and on the device), not of the count.  A box entered exactly at the bound is visited: the (kind, id) tie-break needs it.  The
 * child entered earlier is visited first.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per row.  Reads the scene
 * only -- record heap, vertex array and planes -- and touches no render context, MirtStats counter, hand-out table or random-number
 * table: it may run on another stream while a frame is in flight.  Ordering a query in flight before mirt_scene_set_planes or a
 * geometry update is the caller's duty, as for mirt_trace_rays.
 * n == 0: MIRT_OK, nothing launched (on a built scene: the state is checked before n).  MIRT_ERR_ARG (all checked on the host, before any device work): null scene; n < 0; flag bits
 * other than MIRT_CAST_ANY_HIT; with n > 0 a null d_casts or d_hits; a misaligned d_casts, d_hits or d_features; d_hits (24 n bytes)
 * or d_features (32 n) overlapping d_casts (32 n) or each other.  MIRT_ERR_STATE before mirt_build_lbvh (and between a geometry
 * update and its rebuild).  Every message names mirt_cast_spheres. */
int mirt_cast_spheres(MirtScene* sc, const void* d_casts, int64_t n, void* d_hits, void* d_features, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_SPHERECAST_H */
