/* mirt_overlap_list.h -- extension of mirt.h: overlap lists on a built scene (EVERY surface an axis-aligned box touches, as offsets
 * and one array of words).
 *
 * Three entry points more than mirt.h declares, in a header of its own so that mirt.h, the other extension headers and the binding
 * tables held to them stay as they are (section 6s says why this header lies in include_ext/).  libmirt.so
 * exports the symbols beside the others; callers detect the feature by the symbols (MIRT_VERSION stays 3).  Everything mirt.h says
 * about handles, device pointers, streams and status codes holds here.
 *
 * The box query of mirt_overlap.h answers with at most eight records per row and a count that may exceed them.  A list is made in
 * three steps: count (the count-only call of mirt_overlap.h: k = 0, flags = 0), exclusive scan (mirt_list_offsets), fill
 * (mirt_overlap_list) -- with one read of the total, offsets[n], between the last two if the caller sizes the array of words by it.
 */
#ifndef MIRT_OVERLAP_LIST_H
#define MIRT_OVERLAP_LIST_H

#include "../include/mirt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- offsets: the exclusive prefix sums of n counts, and their total ---------------------------------------------------------------- */
/* The bytes of d_work a mirt_list_offsets call of n counts needs (host arithmetic: 8 bytes per 2048 counts, the block partials): 0
 * for n <= 2048 -- d_work may then be NULL -- and for a negative n. */
int64_t mirt_list_offsets_work_bytes(int64_t n);

/* d_counts:   n uint32, device memory, 4-byte aligned: what the count-only call of mirt_overlap.h, or any other count per row, wrote.
 * d_offsets:  n + 1 int64, 8-byte aligned: d_offsets[0] = 0 and d_offsets[i + 1] = d_offsets[i] + d_counts[i] for i < n, the total
 *             last.  The sums are 64-bit throughout: a total past 2^32 is exact.
 * d_work:     mirt_list_offsets_work_bytes(n) bytes, 8-byte aligned; NULL when that is 0.
 *
 * The result is a function of the counts alone: every sum is taken in index order, and no order of arrival is observable.  The
 * call is not tied to boxes: any per-row count makes offsets.  It does not read the scene's geometry and needs no built scene;
 * sc names the device and the error conventions.
 * At most three kernel launches (one for n <= 2048), asynchronous on `stream`; no allocation, no synchronisation, no atomics.
 * n == 0: d_offsets[0] = 0 is written (an asynchronous 8-byte fill), nothing launched.  MIRT_ERR_ARG (all checked on the host,
 * before any device work): null scene; n < 0 or n > 2^40; a null d_offsets; with n > 0 a null d_counts; a null d_work when
 * mirt_list_offsets_work_bytes(n) > 0; a misaligned buffer; any two of the ranges d_counts (4 n bytes), d_offsets (8 (n + 1)),
 * d_work overlapping.  Every message names mirt_list_offsets. */
int mirt_list_offsets(MirtScene* sc, const uint32_t* d_counts, int64_t n, int64_t* d_offsets, void* d_work, void* stream);

/* ---- the fill: for each of n axis-aligned boxes the words of ALL the planes, spheres and triangles whose surface meets the box ------ */
/* d_boxes:    n rows in mirt_overlap.h's layout ("d_boxes"), 32 B each, 16-byte aligned.
 * d_offsets:  n + 1 int64, 8-byte aligned: row i's segment of d_words is [d_offsets[i], d_offsets[i + 1]).
 * d_words:    capacity uint32, 4-byte aligned.  May be NULL only when capacity == 0.
 *
 * The set.  Row rule, candidates, overlap tests, admission (the NaN dist rule included) and arithmetic are mirt_overlap.h's,
 * sections "Row rule", "Candidates", "Admission" and "Arithmetic", unchanged: A_i is that header's admitted set of row i, and
 * |A_i| the count its count-only call writes.  The set is defined by the scene's arrays alone, never by the tree.
 *
 * A word.  kind << 30 | id: the kind (MIRT_HIT_SPHERE 1, MIRT_HIT_TRIANGLE 2, MIRT_HIT_PLANE 3) and the file-order id (a plane's
 * index) a MirtHit of that surface carries -- the low word of mirt_contacts.h's order key.
 *
 * The order within a row is fixed, and it is the builder's:
 *   first the planes of A_i, ascending by index;
 *   then the spheres and triangles of A_i in the scene's LEAF ORDER, the order mirt_build_lbvh sorts the primitives into: ascending
 *   by the 30-bit Morton code of the centroid in the scene's box, ties in input order (the sort is stable).  mirt_get_tree's refs
 *   are that order.  (A left-child-first stack walk of the tree emits exactly it.)
 * The SET is defined by the scene's arrays alone; the ORDER within a row is the builder's: one pass, and no sort per row.  A caller
 * who wants (kind, id) order sorts each segment's words ascending as unsigned numbers.  A rebuild after a geometry update may
 * reorder a row (the set changes only as the geometry does).
 *
 * What is written.  Writes are bounded by the caller's offsets and capacity, not by what the walk finds:
 *   row i writes the first min(|A_i|, d_offsets[i + 1] - d_offsets[i]) words of its order, from d_words[d_offsets[i]] on;
 *   no word is written at an index >= capacity or < 0: a row whose segment starts at or beyond capacity writes nothing;
 *   offsets that came from other counts, or a d_words smaller than the total, therefore truncate rows and never write outside
 *   [0, capacity); a segment longer than |A_i| keeps its tail untouched; a row that is not live writes nothing.
 * With offsets made by mirt_list_offsets from the counts of the same boxes on the same scene, and capacity >= d_offsets[n], every
 * segment is filled exactly.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per row.  Reads the scene
 * only, like mirt_overlap.h's call, and touches no render context: it may run on another stream while a frame is in flight.
 * n == 0 on a built scene: MIRT_OK, nothing launched, nothing written (capacity == 0 likewise).  MIRT_ERR_ARG (all checked on the
 * host, before any device work): null scene; n < 0; capacity < 0; with n > 0 a null d_boxes or a null d_offsets; a null d_words
 * with capacity > 0; a misaligned buffer; any two of the ranges d_boxes (32 n bytes), d_offsets (8 (n + 1)), d_words
 * (4 capacity) overlapping.  MIRT_ERR_STATE before mirt_build_lbvh (and between a geometry update and its rebuild).  Every message
 * names mirt_overlap_list. */
int mirt_overlap_list(MirtScene* sc, const void* d_boxes, int64_t n, const int64_t* d_offsets, uint32_t* d_words, int64_t capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_OVERLAP_LIST_H */
