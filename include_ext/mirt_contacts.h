/* mirt_contacts.h -- extension of mirt.h: contact queries on a built scene (the k nearest surfaces to a point within a radius, and the
 * number of all of them).
 *
 * One entry point more than mirt.h declares, in a header of its own so that mirt.h, the extension headers under include/ and the
 * binding tables held to them stay as they are (which also says why this header lies in include_ext/).
 * libmirt.so exports the symbol beside the others; callers detect the feature by the symbol (MIRT_VERSION stays 3).  Everything
 * mirt.h says about handles, device pointers, streams and status codes holds here.
 */
#ifndef MIRT_CONTACTS_H
#define MIRT_CONTACTS_H

#include "../include/mirt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MIRT_CONTACTS_MAX_K 8

/* ---- contacts: for each of n points every plane, sphere and triangle nearer than the row's radius -- the k nearest as records, and
 * how many there are --------------------------------------------------------------------------------------------------------------- */
/* d_points:   n rows (qx, qy, qz, R), float4, device memory, 16-byte aligned, exactly as for mirt_closest_points (mirt_closest.h):
 *             the point q and the row's radius R (positive, or +inf).
 * k:          0 to MIRT_CONTACTS_MAX_K: the records per row.
 * d_hits:     n * k MirtHit records (24 B each, 4-byte aligned); row i's j-th nearest surface is record i * k + j.  All k records of
 *             every row are always written; the slots past the row's surfaces are the miss record (t = -1, kind = MIRT_HIT_NONE,
 *             id = 0, n = (0, 0, 0)).  May be NULL only when k == 0.
 * d_counts:   NULL (unless k == 0), or n uint32, 4-byte aligned: the number of ALL admitted candidates of the row.  It may exceed k.
 * d_features: NULL, or n * k rows of mirt_hit_features' layout, (Px, Py, Pz, 1) (nx, ny, nz, 0), 32 B each, 16-byte aligned, written
 *             with two 16-byte stores; row i * k + j belongs to record i * k + j.  A miss slot is eight +0.  The rows are what
 *             mirt_direct_light, mirt_hemisphere_visibility and mirt_indirect_light take.  Not touched when k == 0.
 * flags:      must be 0.
 *
 * Candidates are not redefined here.  mirt_closest.h's paragraphs hold word for word:
 *   its arithmetic (float32, one IEEE rounding per operation, dot, length, normalize);
 *   its row rule: a row with !(R > 0) (zero, negative, NaN), or with a NaN or infinite coordinate, has count 0 and k miss records;
 *   dist, P and n of a plane, a sphere and a triangle, operation by operation ("Plane j", "Sphere (c, r)", "Triangle");
 *   admission: a candidate is admitted when dist < R, a NaN dist never.
 * A is the set of the row's admitted candidates.  It is defined by the scene's arrays alone, never by the tree, its boxes or a
 * visiting order.
 *
 * Order.  The candidates of A ascend by (dist, kind, id), compared lexicographically: dist as floats, then kind (sphere 1 <
 * triangle 2 < plane 3), then the index within the kind (file order; a plane's index).
 *
 * What is written.  The records are the first min(k, |A|) candidates of that order, then misses; the count is |A|.  Each record's
 * t (= dist), kind, id and n, and the feature row's P, are exactly what mirt_closest_points writes for that candidate.  Two
 * identical primitives both appear, at the same dist, the lower id first -- which mirt_closest_points can never show.
 *
 * Relation to mirt_closest_points.  With k == 1, record 0 and feature row 0 of every row are mirt_closest_points' record and feature
 * row for the same (q, R), bit for bit, on every row without exception: both are defined over the arrays with the same order.
 *
 * Pruning (informative; it cannot change the answer).  The kernel walks the scene's tree, the children nearer box first, and leaves
 * a subtree out when the squared distance of q to the subtree's box exceeds (B + sigma)^2, with mirt_closest.h's slack
 *     sigma = 2^-18 * (max(|qx|, |qy|, |qz|) + C),   C the largest coordinate magnitude of the scene's box.
 * With d_counts given, B is R for the whole walk: every candidate nearer than R must be counted.  With d_counts == NULL, B is R
 * until the list holds k entries; after that it is the list's largest dist, and it shrinks as the list improves.  A box at exactly
 * the bound is visited: the (kind, id) tie-break needs it.  The slack bounds a candidate's computed dist against its own boxes
 *  whichever threshold is compared, under mirt_closest.h's conditions on the coordinates.  A count with
 * R = +inf visits every leaf of the tree: ask for counts with the radius the contact needs.
 *
 * One kernel launch, asynchronous on `stream`; no allocation, no synchronisation, no atomics.  One lane per row.  Reads the scene
 * only -- record heap, the file-order sphere, triangle and vertex arrays and the planes -- and touches no render context, MirtStats
 * counter, hand-out table or random-number table: it may run on another stream while a frame is in flight.  Ordering a query in
 * flight before mirt_scene_set_planes or a geometry update is the caller's duty, as for mirt_trace_rays.
 * n == 0: MIRT_OK, nothing launched, nothing written.  MIRT_ERR_ARG (all checked on the host, before any device work): null scene;
 * n < 0; k outside 0..MIRT_CONTACTS_MAX_K; non-zero flags; with n > 0 a null d_points, a null d_hits with k > 0, a null d_counts with
 * k == 0; a misaligned buffer; any two of the ranges d_points (16 n bytes), d_hits (24 n k), d_counts (4 n), d_features (32 n k)
 * overlapping.  MIRT_ERR_STATE before mirt_build_lbvh (and between a geometry update and its rebuild).  Every message names
 * mirt_closest_points_multi. */
int mirt_closest_points_multi(MirtScene* sc, const void* d_points, int64_t n, int k, void* d_hits, uint32_t* d_counts, void* d_features, uint32_t flags,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_CONTACTS_H */
