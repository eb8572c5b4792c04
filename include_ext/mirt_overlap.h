/* mirt_overlap.h -- extension of mirt.h: box overlap queries on a built scene (the surfaces an axis-aligned box touches, and how
 * many).
 *
 * One entry point more than mirt.h declares, in a header of its own so that mirt.h, the extension headers under include/ and the
 * binding tables held to them stay as they are (section 6s says why this header lies in include_ext/).
 * libmirt.so exports the symbol beside the others; callers detect the feature by the symbol (MIRT_VERSION stays 3).  Everything
 * mirt.h says about handles, device pointers, streams and status codes holds here.
 */
#ifndef MIRT_OVERLAP_H
#define MIRT_OVERLAP_H

#include "../include/mirt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIRT_OVERLAP_MAX_K 8
#define MIRT_OVERLAP_ANY   1u

/* ---- box overlaps: for each of n axis-aligned boxes every plane, sphere and triangle whose SURFACE meets the box -- the k nearest to
 * the box's centre as records, and how many there are ------------------------------------------------------------------------------ */
/* d_boxes:    n rows in MirtRay's layout, (lox, loy, loz, _) (hix, hiy, hiz, _), 32 B each, device memory, 16-byte aligned: the box
 *             [lo, hi].  The two `_` words are ignored.
 * k:          0 to MIRT_OVERLAP_MAX_K: the records per row.
 * d_hits:     n * k MirtHit records (24 B each, 4-byte aligned); row i's j-th record is record i * k + j.  All k records of every row
 *             are always written; the slots past the row's surfaces are the miss record (t = -1, kind = MIRT_HIT_NONE, id = 0,
 *             n = (0, 0, 0)) -- exactly mirt_closest_points_multi's layout (mirt_contacts.h).  May be NULL only when k == 0.
 * d_counts:   n uint32, 4-byte aligned: the number of ALL admitted candidates of the row.  It may exceed k.  May be NULL only when
 *             k > 0.
 * d_features: NULL, or n * k rows of mirt_hit_features' layout, (Px, Py, Pz, 1) (nx, ny, nz, 0), 32 B each, 16-byte aligned, written
 *             with two 16-byte stores; row i * k + j belongs to record i * k + j.  A miss slot is eight +0.  The rows are what
 *             mirt_direct_light, mirt_hemisphere_visibility and mirt_indirect_light take.  Not touched when k == 0.
 * flags:      0 or MIRT_OVERLAP_ANY.  MIRT_OVERLAP_ANY requires k == 0 and a non-null d_counts; the count written is then 1 when
 *             the row has an admitted candidate and 0 when it has none -- 1 exactly when the call without the flag writes a non-zero
 *             count --, and the walk may end at the first admitted candidate.
 *
 * Arithmetic: mirt_closest.h's, word for word -- float32 with one IEEE rounding per operation (no fused multiply-add), IEEE
 * division and square root; dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z; length(v) = sqrtf(dot(v, v)); normalize: (0, 0, 0) when the
 * length is below 1e-6, else each component times 1 / length; vector sums, differences and a vector times a scalar per component,
 * one rounding each.  |x| = fabsf(x) clears the sign bit.  fminf and fmaxf return the other operand when one is a NaN; their results
 * are only ever compared or squared below, so the sign of a zero they return does not matter.  A comparison with a NaN is false,
 * and every test below is a conjunction of <= and >= (never a negated >), so a NaN never admits a candidate.
 *
 * Row rule.  A row is live when all six coordinates are finite and lo.x <= hi.x, lo.y <= hi.y, lo.z <= hi.z.  A box without volume
 * (a rectangle, a segment, a point: lo == hi on some axes) is live.  Any other row has count 0 and k miss records.
 *
 * Box quantities, per component:   m = (lo + hi) * 0.5      h = (hi - lo) * 0.5
 *
 * Candidates.  EVERY plane, sphere and triangle of the scene is a candidate.  Surfaces are hollow and two-sided, as in
 * mirt_closest.h: a box strictly inside a sphere, away from its surface, does not touch that sphere.  The set is defined by the
 * scene's arrays alone, never by the tree, its boxes or a visiting order.  A candidate passes its overlap test as follows.
 *
 * Sphere (c, rs) (kind 1), per axis a of x, y, z:
 *     dn.a = fmaxf(fmaxf(lo.a - c.a, c.a - hi.a), 0)          (the box's nearest point to c, per axis)
 *     df.a = fmaxf(fabsf(c.a - lo.a), fabsf(hi.a - c.a))      (its farthest corner from c, per axis)
 *     dmin2 = dot(dn, dn);  dmax2 = dot(df, df);  rr = rs * rs
 *     passes when  dmin2 <= rr && dmax2 >= rr                 (the box reaches the surface and is not wholly inside it)
 *
 * Plane j (kind 3; nor, point of MirtPlane j):
 *     N = normalize(nor);  s = dot(N, m - point)
 *     e = (h.x * |N.x| + h.y * |N.y|) + h.z * |N.z|
 *     passes when  fabsf(s) <= e
 *
 * Triangle (kind 2): a, b, c = p0, p1, p2 of the file-order vertex array (what mirt_scene_get_triangles reads).  Thirteen axes
 * (Akenine-Moller, Fast 3D Triangle-Box Overlap Testing, 2001); the triangle passes when every axis passes.  With x, y, z numbered
 * 0, 1, 2 and u[k] the k-th component of u:
 *     v0 = a - m;  v1 = b - m;  v2 = c - m;  f0 = v1 - v0;  f1 = v2 - v1;  f2 = v0 - v2
 *   Box axis k = 0, 1, 2:
 *     mn = fminf(fminf(v0[k], v1[k]), v2[k]);  mx = fmaxf(fmaxf(v0[k], v1[k]), v2[k])
 *     passes when  mn <= h[k] && mx >= -h[k]
 *   Face:
 *     nn.x = f0.y * f1.z - f0.z * f1.y;  nn.y = f0.z * f1.x - f0.x * f1.z;  nn.z = f0.x * f1.y - f0.y * f1.x
 *     d = dot(nn, v0);  r = (h.x * |nn.x| + h.y * |nn.y|) + h.z * |nn.z|
 *     passes when  fabsf(d) <= r
 *     (the scene record's nor is not used here.  A triangle without area has nn = (0, 0, 0) and passes: it is tested as the segment
 *     or the point its other axes describe)
 *   Edge axes: for f = f0, f1, f2 in turn and k = 0, 1, 2, with k1 = (k + 1) % 3 and k2 = (k + 2) % 3:
 *     p0 = v0[k2] * f[k1] - v0[k1] * f[k2];  p1 = v1[k2] * f[k1] - v1[k1] * f[k2];  p2 = v2[k2] * f[k1] - v2[k1] * f[k2]
 *     rr = h[k1] * |f[k2]| + h[k2] * |f[k1]|
 *     mn = fminf(fminf(p0, p1), p2);  mx = fmaxf(fmaxf(p0, p1), p2)
 *     passes when  mn <= rr && mx >= -rr
 *
 * Admission.  Each candidate carries mirt_closest.h's dist, P and n for the point q = m ("Plane j", "Sphere (c, r)", "Triangle",
 * operation by operation).  A candidate is admitted when it passes its overlap test and its dist is not a NaN (a triangle without
 * area whose closest-point operations divide zero by zero is the one way to a NaN dist on finite coordinates: it is not admitted).
 * A is the set of the row's admitted candidates.
 *
 * Order.  The candidates of A ascend by (dist, kind, id), compared lexicographically, in mirt_contacts.h's order: dist as floats, then
 * kind (sphere 1 < triangle 2 < plane 3), then the index within the kind (file order; a plane's index).
 *
 * What is written.  The records are the first min(k, |A|) candidates of that order, then misses; the count is |A| (with
 * MIRT_OVERLAP_ANY: |A| > 0).  Each record is exactly what mirt_closest_points writes for that candidate at q = m: t = dist, kind,
 * file-order id, the normal turned towards m; the feature row is (P, 1) (n, 0).  P is the point of the surface nearest the box's
 * CENTRE.  It may lie outside the box: a box that a large triangle crosses near one corner has its P on the triangle, nearest m, not
 * necessarily within [lo, hi].  Two identical primitives both appear, the lower id first.  Neither d_counts nor k changes which
 * candidates are admitted.
 *
 * Pruning (informative; it cannot change the answer).  The planes come first.  Then the kernel walks the scene's tree and visits a
 * child with box [bmin, bmax] when, on every axis,
 *     !(bmin > hi + sigma) && !(bmax < lo - sigma)            (a NaN therefore visits)
 *     sigma = 2^-18 * (max(|lo.x|, |lo.y|, |lo.z|, |hi.x|, |hi.y|, |hi.z|) + C),   C the largest coordinate magnitude of the scene's box,
 * computed once per row, hi + sigma and lo - sigma once per row as well.  sigma exceeds every rounding between a primitive's test
 * above and its own float32 boxes (m, h and v = p - m against a leaf's planes; a sphere's c -+ rs planes; the pad of a refit):
 * DESIGN.md section 6w has the count, which holds for coordinates between 2^-40 and 2^40 in magnitude, as in section 6o.  There is no
 * shrinking bound in this query: k and d_counts do not change which subtrees are visited; only MIRT_OVERLAP_ANY ends a walk early.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per row.  Reads the scene
 * only -- record heap, the file-order sphere, triangle and vertex arrays and the planes -- and touches no render context, MirtStats
 * counter, hand-out table or random-number table: it may run on another stream while a frame is in flight.  Ordering a query in
 * flight before mirt_scene_set_planes or a geometry update is the caller's duty, as for mirt_trace_rays.
 * n == 0 on a built scene: MIRT_OK, nothing launched, nothing written.  MIRT_ERR_ARG (all checked on the host, before any device
 * work): null scene; n < 0; k outside 0..MIRT_OVERLAP_MAX_K; unknown flag bits; MIRT_OVERLAP_ANY with k != 0; with n > 0 a null
 * d_boxes, a null d_hits with k > 0, a null d_counts with k == 0; a misaligned buffer; any two of the ranges d_boxes (32 n bytes),
 * d_hits (24 n k), d_counts (4 n), d_features (32 n k) overlapping.  MIRT_ERR_STATE before mirt_build_lbvh (and between a geometry
 * update and its rebuild).  Every message names mirt_overlap_boxes. */
int mirt_overlap_boxes(MirtScene* sc, const void* d_boxes, int64_t n, int k, void* d_hits, uint32_t* d_counts, void* d_features, uint32_t flags,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_OVERLAP_H */
