/* mirt_query_lists.h -- extension of mirt.h: ray and ball lists on a built scene (EVERY surface a ray crosses or a ball touches, as
 * words in the segments of the caller's offsets, with the t or dist of each if asked for).
 *
 * Two entry points more than mirt.h declares, in a header of its own so that mirt.h, the other extension headers and the binding
 * tables held to them stay as they are (section 6s says why this header lies in include_ext/).  libmirt.so
 * exports the symbols beside the others; callers detect the feature by the symbols (MIRT_VERSION stays 3).  Everything mirt.h says
 * about handles, device pointers, streams and status codes holds here.
 *
 * The multi-hit ray query of mirt_multihit.h and the contact query of mirt_contacts.h answer with at most eight records per row and
 * a count that may exceed them.  A list is made in three steps:
 *   count   the count-only call of mirt_multihit.h (rays) or of mirt_contacts.h (balls): k = 0, flags = 0;
 *   scan    the offsets call of the overlap-list extension, unchanged: any per-row count makes offsets;
 *   fill    one of the two calls below,
 * with one read of the total, offsets[n], between the last two if the caller sizes the arrays by it.
 */
#ifndef MIRT_QUERY_LISTS_H
#define MIRT_QUERY_LISTS_H

#include "../include/mirt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the two fills: for each row the words of ALL the planes, spheres and triangles of the row's set, and their values ------------- */
/* d_rays:    num_rays rows in mirt_multihit.h's layout ("d_rays"), 32 B each, 16-byte aligned.
 * d_points:  n rows in mirt_contacts.h's layout ("d_points"), 16 B each, 16-byte aligned.
 * d_offsets: rows + 1 int64, 8-byte aligned: row i's segment of d_words (and of d_t / d_dist) is [d_offsets[i], d_offsets[i + 1]).
 * d_words:   capacity uint32, 4-byte aligned.  May be NULL only when capacity == 0.
 * d_t, d_dist: NULL, or capacity float32, 4-byte aligned: the value of every word, at the word's index.
 * flags:     must be 0.
 *
 * The set.  Nothing about it is restated here.
 *   Rays.   Row i's set is S of mirt_multihit.h, sections "Rays that are not live" and "The admitted set S": the live-ray rule, the
 *           planes, the tree-defined walk with the bound held at tmax, the leaf tests and the arithmetic, unchanged.  |S| is the
 *           count that header's count-only call writes.  Like it, the set is defined by the scene's tree.
 *   Balls.  Row i's set is A of mirt_contacts.h, section "Candidates are not redefined here": the row rule, dist of a plane, a
 *           sphere and a triangle, and the admission dist < R, a NaN dist never.  |A| is the count that header's count-only call
 *           writes.  The set is defined by the scene's arrays alone, never by the tree.
 *
 * A word.  kind << 30 | id: the kind (MIRT_HIT_SPHERE 1, MIRT_HIT_TRIANGLE 2, MIRT_HIT_PLANE 3) and the file-order id (a plane's
 * index) a MirtHit of that surface carries -- the word of the overlap-list extension, and the low word of mirt_contacts.h's order.
 *
 * A value.  d_t[j] / d_dist[j] is, for the word at d_words[j], the t (rays) or dist (balls) that the record call's MirtHit carries
 * for that surface on that row, bit for bit.  It is written wherever, and only where, its word is written.  It is what lets a
 * caller order a row.
 *
 * The order within a row is fixed, and it is the builder's:
 *   first the planes of the set, ascending by index;
 *   then the spheres and triangles of the set in the scene's LEAF ORDER, the order mirt_build_lbvh sorts the primitives into:
 *   ascending by the 30-bit Morton code of the centroid in the scene's box, ties in input order (the sort is stable).
 *   mirt_get_tree's refs are that order.  (A left-child-first stack walk of the tree emits exactly it; neither set depends on the
 *   order of the visits.)
 * One pass, and no sort per row.  A rebuild after a geometry update may reorder a row (the set changes only as the geometry does).
 * That order is also the tie order of both record calls, so a caller orders a row with one sort:
 *   Rays.   A STABLE sort of a row by the bits of t (every t of S is positive: the bits order as unsigned integers) is exactly
 *           mirt_multihit.h's (t, class, index) order.
 *   Balls.  A sort of a row by dist's bits << 32 | word (dist is non-negative) is exactly mirt_contacts.h's (dist, kind, id) order.
 *
 * What is written.  Writes are bounded by the caller's offsets and capacity, not by what the walk finds:
 *   row i writes the first min(|set|, d_offsets[i + 1] - d_offsets[i]) words of its order, and their values if asked for, from
 *   index d_offsets[i] on;
 *   nothing is written at an index >= capacity or < 0: a row whose segment starts at or beyond capacity writes nothing;
 *   offsets that came from other counts, or arrays smaller than the total, therefore truncate rows and never write outside
 *   [0, capacity); a segment longer than the row's set keeps its tail untouched; a row that is not live writes nothing and does not
 *   read its offsets.
 * With offsets made from the counts of the same rows on the same scene, and capacity >= d_offsets[rows], every segment is filled
 * exactly.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per row.  Reads the scene
 * only, like the record calls, and touches no render context: it may run on another stream while a frame is in flight.
 * rows == 0 on a built scene: MIRT_OK, nothing launched, nothing written (capacity == 0 likewise).  MIRT_ERR_ARG (all checked on
 * the host, before any device work): null scene; non-zero flags; rows < 0; capacity < 0; with rows > 0 a null d_rays / d_points or a
 * null d_offsets; a null d_words with capacity > 0; a misaligned buffer; any two of the ranges d_rays (32 num_rays bytes) /
 * d_points (16 n), d_offsets (8 (rows + 1)), d_words (4 capacity), d_t / d_dist (4 capacity, when given) overlapping.
 * MIRT_ERR_STATE before mirt_build_lbvh (and between a geometry update and its rebuild).  Every message names its entry point. */
int mirt_ray_list(MirtScene* sc, const void* d_rays, int64_t num_rays, const int64_t* d_offsets, uint32_t* d_words, float* d_t, int64_t capacity,
                  uint32_t flags, void* stream);
int mirt_ball_list(MirtScene* sc, const void* d_points, int64_t n, const int64_t* d_offsets, uint32_t* d_words, float* d_dist, int64_t capacity,
                   uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_QUERY_LISTS_H */
