/* mirt_cast_lists.h -- extension of mirt.h: cast lists on a built scene (EVERY surface a moving ball touches along its path, as a
 * count per row and as words in the segments of the caller's offsets, with the contact parameter t of each if asked for).
 *
 * Two entry points more than mirt.h declares, in a header of its own so that mirt.h, the other extension headers and the binding
 * tables held to them stay as they are (the header lies in include_ext3/ because the tests that list
 * include/, include_ext/ and include_ext2/ hold their own tables of them; later extensions may join this folder).  libmirt.so exports
 * the symbols beside the others; callers detect the feature by the symbols (MIRT_VERSION stays 3).  Everything mirt.h says about
 * handles, device pointers, streams and status codes holds here.
 *
 * mirt_cast_spheres (include_ext/mirt_spherecast.h) answers with the first contact of a row, or with some contact.  A list is made
 * in three steps, as the other lists are: count (mirt_cast_counts), exclusive scan (mirt_list_offsets of the overlap-list extension,
 * unchanged: any count per row makes offsets), fill (mirt_cast_list) -- with one read of the total, offsets[n], between the last two
 * if the caller sizes the arrays by it.
 */
#ifndef MIRT_CAST_LISTS_H
#define MIRT_CAST_LISTS_H

#include "../include/mirt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- rows --------------------------------------------------------------------------------------------------------------------------
 * d_casts: n rows in the layout of include_ext/mirt_spherecast.h ("d_casts"): (ox, oy, oz, tmax) (dx, dy, dz, r), 32 B each, device
 * memory, 16-byte aligned.  A row is live by that header's "Row rule", unchanged.  A row that is not live counts 0 and writes nothing.
 *
 * ---- the set -----------------------------------------------------------------------------------------------------------------------
 * Nothing about a candidate's parameter is restated here.  Row i's set L_i is made of the candidates of
 * include_ext/mirt_spherecast.h, section "Row rule" and the candidate paragraphs after it ("Helpers", "Sphere", "Plane rule",
 * "Plane j", "Triangle"): the arithmetic, d^ = normalize(d), the parameter t of a plane, of a sphere and of a triangle in its seven
 * pieces, and the admission 0 <= t < tmax, a NaN never.
 *   A plane is in L_i when that header admits it.
 *   A sphere or a triangle is in L_i when that header admits it AND clause (0) below holds for it.
 * A surface appears ONCE, with the parameter of its FIRST contact: 0 when the ball touches or overlaps it at the start.  A sphere
 * gives one word, also for r = 0 and also when the path goes through it: this is not the pair of crossings a ray list holds for a
 * sphere (entry and exit are not both listed; the exit parameter is not part of this extension).
 *
 * Clause (0): the bound that makes the set one a walk can prune for exactly.  It applies when the scene holds two or more
 * spheres and triangles together (the only primitive of a scene has no box in the tree and is always a candidate).  With
 *     C      the largest coordinate magnitude of the scene's box (of all spheres' and triangles' boxes)
 *     sigma  = ((max(|ox|, |oy|, |oz|) + C) + r) * 2^-18          grow = r + sigma
 *     bound  = tmax + tmax * 2^-20                                  (+inf stays +inf)
 *     inv    = (1 / d^.x, 1 / d^.y, 1 / d^.z)
 * and the primitive's OWN BUILDER BOX [lo, hi] -- a sphere's: lo_k = c[k] - rs, hi_k = c[k] + rs, swapped if lo_k <= hi_k is false;
 * a triangle's: lo_k = fminf(fminf(p0[k], p1[k]), p2[k]), hi_k likewise with fmaxf, and where hi_k - lo_k < 0.01f then lo_k - 0.01f and
 * hi_k + 0.01f in their place; the very operations mirt_build_lbvh makes a leaf's box with --, per axis k
 *     a_k = ((lo_k - grow) - o_k) * inv_k        b_k = ((hi_k + grow) - o_k) * inv_k
 *     enter = fmaxf(fmaxf(fmaxf(fminf(a_x, b_x), fminf(a_y, b_y)), fminf(a_z, b_z)), 0)
 *     leave = fminf(fminf(fmaxf(a_x, b_x), fmaxf(a_y, b_y)), fmaxf(a_z, b_z))
 * (fminf and fmaxf pass over a NaN operand), clause (0) holds when enter > fminf(leave, bound) is false: the centre's ray meets
 * the primitive's box, grown by r + sigma, within [0, bound].  This is the slab test of mirt_spherecast.h's "Pruning", made on the
 * primitive's own box with the bound held at tmax.
 * Why it is part of the definition: that header's count shows that an admitted candidate's centre at t lies in its box grown by
 * r + sigma -- so that clause (0) removes nothing --, except for an edge piece whose path runs nearly along the edge, where it
 * rests on tests alone.  A first contact may rest on that; a list must emit EVERY member, so the bound is carried here instead, and
 * the set is a function of the scene's arrays and the row alone: it does not depend on the tree, its inner boxes or any visiting
 * order.  (Subtraction, and multiplication by the fixed inv_k, are monotone in float32, and an inner box of the tree holds its
 * children's bit for bit: the interval of an inner box contains its descendants', so a walk that tests every box by these operations
 * visits every member.)  No difference has been observed between L_i and the plain admitted set.
 *
 * |L_i| is the count mirt_cast_counts writes.  Sorted by (t, kind, id), L_i begins with the (t, kind, id) of mirt_cast_spheres'
 * record for the row, bit for bit, and L_i is empty exactly where that call misses: a sphere or triangle that call's kernel
 * reports has passed this very test on its own box with a bound no larger, so it is in L_i; that it is the smallest of L_i is
 * that header's pruning claim.  MIRT_CAST_ANY_HIT's record names a member of L_i with its t, likewise.
 *
 * ---- words, values, order ---------------------------------------------------------------------------------------------------------
 * A word is kind << 30 | id: MIRT_HIT_SPHERE 1, MIRT_HIT_TRIANGLE 2, MIRT_HIT_PLANE 3 and the file-order id (a plane's index) -- the
 * word of the overlap-list extension.
 * A value.  d_t[j] is, for the word at d_words[j], the candidate's t on that row, bit for bit the t mirt_spherecast.h defines (what
 * mirt_cast_spheres' record carries when that surface is the first).  It is written wherever, and only where, its word is written.
 * The order within a row is fixed, and it is the builder's:
 *   first the planes of L_i, ascending by index;
 *   then the spheres and triangles of L_i in the scene's LEAF ORDER, the order mirt_build_lbvh sorts the primitives into: ascending
 *   by the 30-bit Morton code of the centroid in the scene's box, ties in input order.  mirt_get_tree's refs are that order.  (A
 *   left-child-first stack walk of the tree emits exactly it.)
 * One pass, and no sort per row.  A rebuild after a geometry update may reorder a row.  Every t of L_i is non-negative, so its bits
 * order as unsigned integers: a sort of a row by t's bits << 32 | word is exactly (t, kind, id), mirt_spherecast.h's order.
 *
 * ---- what is written --------------------------------------------------------------------------------------------------------------
 * Writes are bounded by the caller's offsets and capacity, not by what the walk finds (the rule of the overlap-list extension):
 *   row i writes the first min(|L_i|, d_offsets[i + 1] - d_offsets[i]) words of its order, and their values if asked for, from
 *   index d_offsets[i] on;
 *   nothing is written at an index >= capacity or < 0: a row whose segment starts at or beyond capacity writes nothing;
 *   offsets that came from other counts, or arrays smaller than the total, therefore truncate rows and never write outside
 *   [0, capacity); a segment longer than the row's set keeps its tail untouched; a row that is not live writes nothing and does not
 *   read its offsets.
 * With offsets made from the counts of the same rows on the same scene, and capacity >= d_offsets[n], every segment is filled
 * exactly.
 */

/* d_counts: n uint32, 4-byte aligned: d_counts[i] = |L_i|.  A row that is not live writes 0.
 * flags:    must be 0.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per row.  Reads the scene
 * only -- record heap, vertex array and planes -- and touches no render context, MirtStats counter, hand-out table or random-number
 * table: it may run on another stream while a frame is in flight.  Ordering a query in flight before mirt_scene_set_planes or a
 * geometry update is the caller's duty.
 * n == 0 on a built scene: MIRT_OK, nothing launched.  MIRT_ERR_ARG (all checked on the host, before any device work): null scene;
 * non-zero flags; n < 0; with n > 0 a null d_casts or d_counts; a misaligned buffer; the ranges d_casts (32 n bytes) and d_counts
 * (4 n) overlapping.  MIRT_ERR_STATE before mirt_build_lbvh (and between a geometry update and its rebuild).  Every message names
 * mirt_cast_counts. */
int mirt_cast_counts(MirtScene* sc, const void* d_casts, int64_t n, uint32_t* d_counts, uint32_t flags, void* stream);

/* d_offsets: n + 1 int64, 8-byte aligned: row i's segment of d_words (and of d_t) is [d_offsets[i], d_offsets[i + 1]).
 * d_words:   capacity uint32, 4-byte aligned.  May be NULL only when capacity == 0.
 * d_t:       NULL, or capacity float32, 4-byte aligned: the value of every word, at the word's index.
 * flags:     must be 0.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per row.  Reads the scene
 * only, like the count, and touches no render context.
 * n == 0 on a built scene: MIRT_OK, nothing launched, nothing written (capacity == 0 likewise).  MIRT_ERR_ARG (all checked on the
 * host, before any device work): null scene; non-zero flags; n < 0; capacity < 0; with n > 0 a null d_casts or a null d_offsets; a
 * null d_words with capacity > 0; a misaligned buffer; any two of the ranges d_casts (32 n bytes), d_offsets (8 (n + 1)), d_words
 * (4 capacity), d_t (4 capacity, when given) overlapping (ranges that only touch do not overlap).  MIRT_ERR_STATE before
 * mirt_build_lbvh (and between a geometry update and its rebuild).  Every message names mirt_cast_list. */
int mirt_cast_list(MirtScene* sc, const void* d_casts, int64_t n, const int64_t* d_offsets, uint32_t* d_words, float* d_t, int64_t capacity,
                   uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_CAST_LISTS_H */
