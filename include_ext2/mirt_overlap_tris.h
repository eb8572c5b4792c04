/* mirt_overlap_tris.h -- extension of mirt.h: triangle overlap queries on a built scene (EVERY surface a caller's triangle touches,
 * as a count per row and as offsets and one array of words).
 *
 * Two entry points more than mirt.h declares, in a header of its own so that mirt.h, the other extension headers and the binding
 * tables held to them stay as they are (the header lies in include_ext2/ because the test that lists include/
 * and include_ext/ holds its own table of them).  libmirt.so exports the symbols beside the others; callers detect the feature by
 * the symbols (MIRT_VERSION stays 3).  Everything mirt.h says about handles, device pointers, streams and status codes holds here.
 *
 * The box query answers "what touches this triangle's bounding box", a broad phase.  This is the narrow phase: triangle against
 * plane, against sphere surface and against triangle.  A list is made in three steps, as a box list is: count
 * (mirt_overlap_triangles, flags = 0), exclusive scan (the scan of the overlap lists, unchanged: any count per row makes offsets),
 * fill (mirt_triangle_list) -- with one read of the total, offsets[n], between the last two if the caller sizes the words by it.
 */
#ifndef MIRT_OVERLAP_TRIS_H
#define MIRT_OVERLAP_TRIS_H

#include "../include/mirt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mirt_overlap_triangles: the walk ends at the first admitted surface, and the count is 1 or 0 */
#define MIRT_TRIS_ANY 1u

/* ---- rows --------------------------------------------------------------------------------------------------------------------------
 * d_tris: n rows of nine floats, a.x a.y a.z b.x b.y b.z c.x c.y c.z, 36 B each, device memory, 4-byte aligned: the layout
 * mirt_scene_get_triangles writes, so that call's buffer is a row array as it is (a mesh against itself).
 *
 * ---- the set -----------------------------------------------------------------------------------------------------------------------
 * A_i, the admitted set of row i, is defined over the scene's arrays -- every plane, every sphere, every triangle, in file order --
 * and never over the tree.  All arithmetic is float32 with one rounding per operation (no fused multiply-add), in the operand order
 * written here: dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z; cross(u, v) = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x);
 * length(u) = sqrtf(dot(u, u)); min3(x, y, z) = fminf(fminf(x, y), z) and max3 likewise with fmaxf (they pass over a NaN operand).
 *
 * Live row.  All nine coordinates are finite (x - x == 0), and with u_b = b - a, u_c = c - a, n1 = cross(u_b, u_c) the value
 * m1 = dot(n1, n1) is finite (m1 - m1 == 0) and m1 > 0.  A row without area -- a point, a segment, a sliver whose n1 rounds to
 * zero -- is dead, as is one whose m1 overflows.  A dead row admits nothing: its count is 0 and it writes no word.
 * The row's bounds are rlo = the componentwise min3 and rhi = the componentwise max3 of a, b, c: exact.
 *
 * Common origin.  The sphere and the triangle tests subtract the row's a from every point first (one rounding per component), and
 * the row's own vertices are then 0, u_b, u_c.  A scene vertex with the bits of a row vertex therefore becomes the very float
 * vector the row's vertex is, and projects to the same float on every axis.  PROPERTY: a scene triangle with area that shares a
 * vertex (hence also one that shares an edge) with a live row, bit for bit, is always admitted -- whatever else rounding does --
 * provided no axis below overflows to an infinity.  (The plane test has no second body to agree with and uses the vertices as
 * given.)
 *
 * Plane j (point p_j, normal n_j).  N = normalize(n_j) as mirt_closest.h has it; s_v = dot(N, v - p_j) for v = a, b, c.  Admitted
 * iff min3(s_a, s_b, s_c) <= 0 && max3(s_a, s_b, s_c) >= 0 and none of the three is a NaN (s_v == s_v): the vertices lie on both
 * sides, or one on the plane.  A NaN admits nothing.
 *
 * Sphere (centre ctr, radius rs): the surface, hollow, as in the box query.  Admitted iff all of
 *   (0) the sphere's box meets the row's bounds: with lo_k = ctr[k] - rs, hi_k = ctr[k] + rs, swapped if lo_k <= hi_k is false --
 *       the very operations mirt_build_lbvh makes a sphere's leaf box with -- lo_k <= rhi[k] && hi_k >= rlo[k] on all three axes;
 *   (1) dn <= rs, where C = ctr - a, P = mirt_closest.h's closest point of the triangle (0, u_b, u_c) to C, region by region, and
 *       dn = length(C - P);
 *   (2) df >= rs, where df = max3(length(0 - C), length(u_b - C), length(u_c - C)): some vertex is not inside.
 * A triangle wholly inside a sphere does not touch it.  Clause (0) is part of the definition on purpose: for a sliver row the
 * interior branch of the closest point divides by a sum that has cancelled, and P may then lie far from the triangle, so "dn <= rs"
 * alone does not imply that the sphere's box comes near the row's bounds.  With (0) the set is one a walk can prune for exactly.
 *
 * Triangle (p, q, r).  P = p - a, Q = q - a, R = r - a.  Admitted iff all of
 *   (i)   its bounds meet the row's: min3(p[k], q[k], r[k]) <= rhi[k] && max3(p[k], q[k], r[k]) >= rlo[k] on all three axes, from
 *         the vertices as given (exact, closed);
 *   (ii)  with f0 = Q - P, f1 = R - Q, f2 = R - P and n2 = cross(f0, f2), m2 = dot(n2, n2) is finite and m2 > 0 (a scene triangle
 *         without area touches nothing);
 *   (iii) none of the SEVENTEEN AXES separates the two, in this order, with e0 = u_b, e1 = u_c - u_b, e2 = u_c:
 *           1       n1 = cross(u_b, u_c)
 *           2       n2
 *           3..11   cross(e_i, f_j), i = 0, 1, 2 outer, j = 0, 1, 2 inner
 *           12..14  cross(n1, e_i), i = 0, 1, 2
 *           15..17  cross(n2, f_j), j = 0, 1, 2
 *         An axis L separates iff rmax < smin || smax < rmin, where rmin = min3(0, dot(L, u_b), dot(L, u_c)), rmax = max3 of the
 *         same three (the row's a projects to 0), smin = min3(dot(L, P), dot(L, Q), dot(L, R)) and smax = max3 of those.  Touching
 *         counts; a zero axis projects everything to 0 and never separates; the last six decide the coplanar case.
 * The result is the conjunction, so an implementation may leave at the first clause that fails.  Clause (i) is part of the
 * definition on purpose: a leaf's box contains its triangle's vertex bounds, so pruning by boxes is exact.
 *
 * ---- pruning (for the record; it cannot change the set) ---------------------------------------------------------------------------
 * The kernel walks the tree, left child first, and visits a child when its box meets [rlo - sigma, rhi + sigma] on every axis
 * (negated compares: a NaN visits), sigma = 2^-18 (the largest coordinate magnitude of the row + that of the scene's box).  Clauses
 * (0) and (i) make every admitted primitive's leaf box meet [rlo, rhi] itself, and a parent's box holds its children's.
 *
 * ---- order, words, writes ---------------------------------------------------------------------------------------------------------
 * A word is kind << 30 | id: MIRT_HIT_SPHERE 1, MIRT_HIT_TRIANGLE 2, MIRT_HIT_PLANE 3 and the file-order id (a plane's index).
 * The order within a row is the builder's: first the planes of A_i, ascending by index; then the spheres and triangles of A_i in
 * the scene's LEAF ORDER, the order mirt_build_lbvh sorts the primitives into (ascending 30-bit Morton code of the centroid, ties in
 * input order; mirt_get_tree's refs are that order; a left-child-first stack walk emits exactly it).  The SET is defined by the
 * scene's arrays alone; the ORDER within a row is the builder's.  A caller who wants (kind, id) order sorts each segment's words
 * ascending as unsigned numbers.  A rebuild after a geometry update may reorder a row.
 */

/* d_counts: n uint32, 4-byte aligned: d_counts[i] = |A_i|; with MIRT_TRIS_ANY 1 if A_i is not empty, else 0.  A dead row writes 0.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per row.  Reads the scene
 * only and touches no render context.  n == 0 on a built scene: MIRT_OK, nothing launched.  MIRT_ERR_ARG (all checked on the host,
 * before any device work): null scene; n < 0; flag bits other than MIRT_TRIS_ANY; with n > 0 a null d_tris or d_counts; a
 * misaligned buffer; the ranges d_tris (36 n bytes) and d_counts (4 n) overlapping.  MIRT_ERR_STATE before mirt_build_lbvh (and
 * between a geometry update and its rebuild).  Every message names mirt_overlap_triangles. */
int mirt_overlap_triangles(MirtScene* sc, const void* d_tris, int64_t n, uint32_t* d_counts, uint32_t flags, void* stream);

/* d_offsets: n + 1 int64, 8-byte aligned: row i's segment of d_words is [d_offsets[i], d_offsets[i + 1]).
 * d_words:   capacity uint32, 4-byte aligned.  May be NULL only when capacity == 0.
 *
 * What is written.  Writes are bounded by the caller's offsets and capacity, not by what the walk finds:
 *   row i writes the first min(|A_i|, d_offsets[i + 1] - d_offsets[i]) words of its order, from d_words[d_offsets[i]] on;
 *   no word is written at an index >= capacity or < 0: a row whose segment starts at or beyond capacity writes nothing;
 *   offsets that came from other counts, or a d_words smaller than the total, therefore truncate rows and never write outside
 *   [0, capacity); a segment longer than |A_i| keeps its tail untouched; a row that is not live writes nothing.
 * With offsets scanned from the counts of the same rows on the same scene, and capacity >= d_offsets[n], every segment is filled
 * exactly.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per row.  Touches no render
 * context.  n == 0 on a built scene: MIRT_OK, nothing launched, nothing written (capacity == 0 likewise).  MIRT_ERR_ARG (all checked
 * on the host, before any device work): null scene; n < 0; capacity < 0; with n > 0 a null d_tris or a null d_offsets; a null
 * d_words with capacity > 0; a misaligned buffer; any two of the ranges d_tris (36 n bytes), d_offsets (8 (n + 1)), d_words
 * (4 capacity) overlapping.  MIRT_ERR_STATE before mirt_build_lbvh (and between a geometry update and its rebuild).  Every message
 * names mirt_triangle_list. */
int mirt_triangle_list(MirtScene* sc, const void* d_tris, int64_t n, const int64_t* d_offsets, uint32_t* d_words, int64_t capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_OVERLAP_TRIS_H */
