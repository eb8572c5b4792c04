// Render on the device: replaces render() and the render kernels of draw.cu:94-239 together with the device code
// they call (shootPrimaryRay/hitNearest/diffuseLight/reflectionLight/refractionLight/globalIllumination/checkPlane,
// draw.cu:260-659; traverse_lbvh, bvh_traversal.cu:11-183; Ray::Ray and the primitive tests, struct.cu:16-163).
//
// trace_kernel    one lane = one sample.  A persistent grid walks the samples; every lane runs a small state machine
//                 (the reference's mutually recursive shading functions turned into an explicit ray-tree walk) around ONE
//                 shared BVH traversal loop, so that primary, shadow, reflection, refraction and GI rays of different
//                 lanes are traversed together.  Traversal stack: 32 entries per lane in LDS ([entry][lane], conflict
//                 free), spilling to global memory above that.  Nodes are 64-byte two-child records.  A workgroup
//                 is one wave; the loop header (who traverses, who waits, is the wave draining, are enough primitive
//                 tests pending) runs once per four traversal steps; only what the loop touches is passed by value.
// resolve_tree_kernel / resolve_kernel
//                 mirt_render's pixels: sum the samples in the reference's xor-butterfly order (draw.cu:181-189), mean, sRGB,
//                 quantise (draw.cu:129-132 for spp <= 1, draw.cu:9-11,202-205 otherwise); one lane per sample when
//                 the butterfly fits a wave, one thread per pixel otherwise.  (mirt_render_accumulate's sums go through
//                 adaptive.hip's resolve_moments, as do mirt_finalize's pixels.)
// order_kernel    sorts the frame's sample chunks by their measured cost: later frames hand them out longest first.
//
// The ray tree is evaluated top-down (every ray carries the product of the mixing weights above it) instead of the
// reference's bottom-up recursion; geometry and random-number consumption are identical, colours agree to rounding.
#include "scene_dev.h"
#include "host_scene.h"
#include "shade_common.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace mirt {
namespace {

constexpr int RBLOCK = 256;
constexpr int MAX_SPP = 4096;         // resolve_kernel's partial-sum stack holds log2(4096) + 1 entries
constexpr int MAX_SLAB_ARGS = 4;      // device copies of RenderArgs a context cycles through (one per slab in flight on its stream)
// (TRACE_BLOCK, STACK_LDS and the chunk sizes: render_plan.h, where the call plan reads them)
#ifndef MIRT_WAVES_PER_SIMD
#define MIRT_WAVES_PER_SIMD 4   // 128 VGPRs: measured best (2: 86 ms, 3: 76 ms, 4: 68 ms, 5: 79 ms on tenthousand 1080p16)
#endif
// The quantised walk found a triangle hit it is about to accept (scene_dev.h): does the reference's walk reach this leaf?  Yes,
// provably, if the triangle's exact leaf box passes the order-independent clauses of hit_aabb_adapted (bvh_traversal.cu:11-44)
// and the ray enters it before the hit: every ancestor's exact box contains the leaf box and the slab arithmetic is monotone in
// the box planes, so t_enter(ancestor) <= t_enter(leaf) < t <= the best distance at the time the ancestor was tested, and each of
// those tests passed.  A hit outside its box (the triangle test accepts up to 0.001 outside the triangle, struct.cu:155) does
// not qualify: the ray is then walked again over the exact records.  Rare: the scene-sized arguments come through `ap`.
MIRT_DEV bool triangle_leaf_reached(const RenderArgs* __restrict__ ap, uint32_t off16, const f3& o, const f3& d, float t, float tmin, f3& inv)
{
  const RenderArgs* aq = ap;
  asm volatile("" : "+s"(aq));
  const uint32_t id = aq->unit_prim[off16 - aq->prim_base16] & 0x7fffffffu;
  const float4 b0 = aq->tri_boxes[2 * (size_t)id], b1 = aq->tri_boxes[2 * (size_t)id + 1];
  inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  const float tx1 = (b0.x - o.x) * inv.x, tx2 = (b0.y - o.x) * inv.x;
  const float ty1 = (b0.z - o.y) * inv.y, ty2 = (b0.w - o.y) * inv.y;
  const float tz1 = (b1.x - o.z) * inv.z, tz2 = (b1.y - o.z) * inv.z;
  const float te = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
  const float tx = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
  return te < tx && tx > tmin && te < t;
}

// QN: the walk starts on the 32-byte quantised node records (scene_dev.h); SPECX: SPEC_NOTRI / SPEC_NOBULB / SPEC_NOPEND of
// shade_common.h.  With QN and triangles a lane can also be on the 64-byte exact records (S.qsx == 0: its ray is being walked
// again, triangle_leaf_reached); then S.inv holds 1 / d.
// With QN on a scene that has triangles the quantised records are the wide ones (WIDE, scene_dev.h): a step tests the boxes of
// the node's four grandchildren and descends two levels.
// SPECX & SPEC_LDS_STACK: the traversal stack never leaves LDS -- push and pop have no arm for the global spill area, and an
// empty stack is a REF_NONE at its bottom, not a count of zero.  Selected by the plan (render_plan.h, lds_only) for a binary
// walk over a tree whose depth proves that the entries fit; see MIRT_PUSH below.
// SPECX & SPEC_START_LDS (with SPEC_LDS_STACK, on the sphere-only quantised records, no point lights): the loop header's ray
// start reads nothing through the vector memory path.  What that arm looks at -- root reference, counts of planes and suns,
// shadow-ray mode -- and the sun record each lane indexes are written once per wave into the first stack slot's 256 bytes of
// LDS; the stack itself starts one slot later and has START_LDS_SLOTS slots, which the plan has shown to be enough (start_lds).
constexpr int SPEC_LDS_STACK = 8;
constexpr int SPEC_START_LDS = 16;
// a sun as the loop header's ray start reads it from LDS: LightDev's direction and reciprocal
struct SunLds { float nx, ny, nz, ix, iy, iz; };
struct StartLdsArgs : HotArgs { const SunLds* suns; };      // (hides HotArgs::suns: batch_next indexes whichever it is given)
static_assert(sizeof(SunLds) == 24 && offsetof(LightDev, ix) == offsetof(LightDev, nx) + 12, "six consecutive words of a LightDev");
template <bool COUNT, int TABLES, bool QN, int SPECX = 0>
__global__ void __launch_bounds__(TRACE_BLOCK, MIRT_WAVES_PER_SIMD) trace_kernel(const RenderArgs* __restrict__ ap, const HotArgs h)
{
  constexpr bool LDS_ONLY = (SPECX & SPEC_LDS_STACK) != 0;
  // ONE_START: the shade loop issues one ray start per pass for the lanes of both its arms (below; batch_next reads it off SPEC:
  // shade_common.h, batch_setup).  The LDS-only kernels over the quantised records take it.  The others keep a start in either arm,
  // and with it the code they had: with one start, the kernels whose stack can spill gained spill instructions inside the
  // traversal loop, and the LDS-only exact-record kernel lost 2.7 % on redchair.txt at 3840 x 2160 x 64.
  constexpr bool ONE_START = LDS_ONLY && QN;
  constexpr int SPEC = (SPECX & ~(SPEC_LDS_STACK | SPEC_START_LDS)) | (ONE_START ? SPEC_ONE_START : 0);
  constexpr bool START_LDS = (SPECX & SPEC_START_LDS) != 0;
  // CUR_MARK: inside the traversal loop's steps a lane that is not traversing holds S.cur == REF_NONE, and the steps read that
  // instead of S.trav (a bool the compiler keeps as a byte per lane: moves, a select in the pop and a mask rebuilt per step).
  // REF_NONE has the REF_LEAF bit, so "(int)S.cur >= 0" is "traversing, at an internal node" in one compare.  S.trav is brought
  // up to date once per header pass, after the steps; everything outside them reads S.trav as before.  Only the kernel that
  // starts rays from LDS takes this form: in the other LDS-only sphere kernel it put scalar-register spill reloads back into the
  // loop.
  constexpr bool CUR_MARK = START_LDS;
  static_assert(!CUR_MARK || LDS_ONLY, "the pop that empties an LDS-only stack yields REF_NONE");
  static_assert((REF_NONE & REF_LEAF) != 0, "REF_NONE reads as a leaf reference");
  constexpr bool NOTRI = (SPEC & SPEC_NOTRI) != 0;
  constexpr bool WIDE = QN && !NOTRI;
  static_assert(!START_LDS || (LDS_ONLY && QN && NOTRI && (SPEC & SPEC_NOBULB) != 0), "the ray-start block holds suns only, and its room comes from a stack that cannot spill");
  constexpr int HEAD_AT = 0, SUNS_AT = 16, STACK_AT = START_LDS ? TRACE_BLOCK * 4 : 0;      // START_LDS: the ray-start block in slot 0's bytes, the stack after it
  static_assert(!(LDS_ONLY && WIDE), "the wide walk pushes up to three entries per step: the depth of the tree does not bound its stack");
  // a finished shadow ray towards a point light that hit something, in a walk that is not the reference's own: the hit is vetted
  // by the shade phase before batch_next reads "occluded" off it (hit_needs_literal_walk); no such lanes in a kernel without bulbs
#define MIRT_HELD (QN && !(SPEC & SPEC_NOBULB) && h.reach_check && S.batch_pending && !S.trav && S.li >= h.num_suns && S.li < h.num_suns + h.num_bulbs && \
                   S.refbest != REF_NONE)
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[STACK_LDS * TRACE_BLOCK * 4];     // traversal stacks: STACK_LDS x TRACE_BLOCK words
  // The random-number state (8 words per lane) is only touched in the shade phase: it lives here during traversal so
  // that it does not occupy registers across the hot loop (the kernel runs at the 128-VGPR edge of 4 waves per SIMD).
  __shared__ uint4 lds_rng[2][TRACE_BLOCK];
  // Likewise eight words of shading state that the traversal loop and its batch transitions never touch (radiance so far,
  // alpha, the diffuse weight, the node's index of refraction).
  __shared__ uint4 lds_park[2][TRACE_BLOCK];
  uint32_t* const lds_stack = reinterpret_cast<uint32_t*>(lds_raw + STACK_AT);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  (void)lane;
  const unsigned char* const heap = reinterpret_cast<const unsigned char*>(h.nodes);
  // (32-bit: the grid has far fewer than 2^31 threads; the 64-bit products below are formed where they are used)
  const uint32_t gid32 = blockIdx.x * (uint32_t)TRACE_BLOCK + (uint32_t)tid;
  const long long gid = (long long)gid32;
  const long long gthreads = (long long)(gridDim.x * (uint32_t)TRACE_BLOCK);
  Counters cn = {0, 0, 0, 0, 0, 0, 0, 0, 0};

  // Work distribution: the sample range is cut into chunks of 2^chunk_shift consecutive samples (16 pixels at 16 spp); a wave
  // takes the next chunk from a global counter whenever its local one is used up (one atomic per chunk), so waves that
  // draw cheap samples simply draw more of them -- this is what keeps the tail short when a GPU renders only a stripe set.
  unsigned long long c_next = 0, c_end = 0;   // wave-uniform: this wave's current chunk
  bool exhausted = false;                      // wave-uniform: the global counter has run past the frame

  Lane S;
  lane_reset(S);

  lds_rng[0][tid] = make_uint4(0, 0, 0, 0);
  lds_rng[1][tid] = make_uint4(0, 0, 0, 0);
  lds_park[0][tid] = make_uint4(0, 0, 0, 0);
  lds_park[1][tid] = make_uint4(0, 0, 0, __float_as_uint(1.458f));
  if (START_LDS) {
    // once per wave: the head (root reference, planes, suns, shadow-ray mode) and six words per sun (the plan: num_suns <=
    // START_LDS_SUNS; a workgroup is one wave)
    static_assert(TRACE_BLOCK == 64 && 6 * START_LDS_SUNS <= TRACE_BLOCK, "one pass of the wave fills the block");
    if (tid == 0) *reinterpret_cast<uint4*>(lds_raw + HEAD_AT) = make_uint4(ap->root_ref, (uint32_t)ap->num_planes, (uint32_t)ap->num_suns, (uint32_t)ap->shadow_anyhit);
    if (tid < 6 * START_LDS_SUNS)
      reinterpret_cast<float*>(lds_raw + SUNS_AT)[tid] = tid < 6 * ap->num_suns ? (&ap->suns[tid / 6].nx)[tid % 6] : 0.0f;
    __syncthreads();
  }
  for (;;) {
    // ================= shade / refill phase: lanes that are not traversing =================
    // The shade phase reads the frame's RenderArgs through a pointer the optimiser cannot see through, so that those
    // values are (scalar-)loaded here and do not live in registers across the traversal loop.
    const RenderArgs* aq = ap;
    asm volatile("" : "+s"(aq));
    const RenderArgs& a = *aq;
    // A lane whose nearest-hit walk ended on a sphere the reference may never have tested (hit_needs_literal_walk: a few rays per
    // frame) has its ray walked again here, the reference's way, before the hit is shaded below -- while the sixteen parked words
    // of the lane are still in LDS: with them in registers the walk's own pushed spills into the whole shade phase (+1..3 %).
    // (the lanes vetted are exactly those the loop below lets advance() consume: none is looked at twice)
    // (a batch lane: its reflection ray, or a shadow ray towards a point light -- one that hit something is left to this phase
    // by the traversal loop's header, MIRT_HELD)
    // (LDS_ONLY: every ray this phase starts finds the empty stack's REF_NONE on top -- the lanes that may start one are those
    // that are not traversing now; a ray that ended on an any-hit exit left its entries behind)
    if (LDS_ONLY && !S.trav) S.tos = REF_NONE;
    if (a.reach_check && !S.trav && S.g >= 0 && !(exhausted && S.batch_pending && !MIRT_HELD) && (!S.batch_pending || S.li >= a.num_suns)) {
      if (hit_needs_literal_walk<QN>(a, S)) walk_literally<COUNT, NOTRI>(a, S, cn, gid, gthreads);
    }
    {
      const uint4 r0 = lds_rng[0][tid], r1 = lds_rng[1][tid];
      S.rng.v0 = r0.x; S.rng.v1 = r0.y; S.rng.v2 = r0.z; S.rng.v3 = r0.w;
      S.rng.v4 = r1.x; S.rng.d = r1.y; S.rng.bm_extra = __uint_as_float(r1.z); S.rng.bm_flag = (int)r1.w;
      const uint4 p0 = lds_park[0][tid], p1 = lds_park[1][tid];
      S.L = mk3(__uint_as_float(p0.x), __uint_as_float(p0.y), __uint_as_float(p0.z)); S.alpha = __uint_as_float(p0.w);
      S.wD = mk3(__uint_as_float(p1.x), __uint_as_float(p1.y), __uint_as_float(p1.z)); S.Hior = __uint_as_float(p1.w);
    }
    // (once the frame's queue is empty the first ray of a new batch is started by the traversal loop's header instead)
    // One pass serves the whole wave in the common case (1.03 passes per shade phase on the headline frame): a lane whose batch
    // ended with the ray that just finished -- its reflection ray, or the last shadow ray of a node without one -- learns so from
    // batch_next and is shaded by the SAME pass's advance(), next to the lanes that arrived without a batch.  (With the second arm
    // an `else` those two or three lanes came back for a pass of their own: 1.59 executions of the whole advance() stream per shade
    // phase.)  Every lane still goes through the same calls in the same order.  The loop is written wave-uniform, the lanes'
    // conditions inside it: as a per-lane `while` around the two `if`s the same code spilled 180 registers in two of the kernels.
    for (;;) {
      const bool live = !S.trav && S.g >= 0 && !(exhausted && S.batch_pending && !MIRT_HELD);
      if (__ballot(live) == 0) break;
      // Both arms only set a ray up; one start_ray -- the quantised-axis set-up and the plane loop -- serves every lane that got
      // one in this pass.  (With a start of its own in either arm the first arm, 4.7 lanes per execution on the headline frame,
      // paid for a whole ray start that the same pass issued again a few hundred instructions later.)  A shadow ray that a plane
      // answers leaves the lane not traversing with its batch pending: the next pass serves it.
      if (ONE_START) {
        bool go = false;
        if (live && S.batch_pending) go = batch_setup<COUNT, RenderArgs, SPEC>(a, S, cn);
        if (live && !go && !S.trav && !S.batch_pending) go = advance_setup<COUNT, SPEC>(a, S, cn, gid, gthreads);
        if (go) start_ray<COUNT, true, QN>(a, S, cn);
      } else {
        if (live && S.batch_pending) batch_next<COUNT, QN, RenderArgs, SPEC>(a, S, cn);
        if (live && !S.trav && !S.batch_pending) advance<COUNT, QN, SPEC>(a, S, cn, gid, gthreads);
      }
    }
    if (!exhausted) {
      // lanes without a sample take new ones -- once init_k of them wait, or when the wave has nothing else to do: starting a
      // sample (RNG stream set-up, camera ray) costs the wave the same instructions for one lane as for forty
      const unsigned long long need = __ballot(!S.trav && S.g < 0);
      if (need && (__popcll(need) >= a.init_k || __ballot(S.trav || S.batch_pending) == 0)) {
        const int want = __popcll(need);
        const unsigned long long nsamples = (unsigned long long)a.num_samples;
        const unsigned long long chunk = 1ull << a.chunk_shift;
        const unsigned long long nchunks = (nsamples + chunk - 1) >> a.chunk_shift;
        const int r = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
        int given = 0;
        long long my = -1;
        while (given < want) {
          if (c_next >= c_end) {
            unsigned long long k = 0;
            if (lane == 0) {
              k = atomicAdd(a.work_counter, 1ull);
              // longest-first hand-out order measured on an earlier frame (any order gives the same pixels)
              if (k < nchunks && a.chunk_order) k = a.chunk_order[k];
            }
            k = __shfl(k, 0);
            if (k >= nchunks) {
              // Every wave fetches past the end exactly once (and never again): the last one to do so puts both counters back
              // to zero for the next launch on this context -- no memset between launches.
              if (lane == 0 && atomicAdd(a.work_counter + 4, 1ull) == (unsigned long long)gridDim.x * (TRACE_BLOCK / 64) - 1ull) {
                a.work_counter[4] = 0ull;
                a.work_counter[0] = 0ull;
              }
              exhausted = true;
              break;
            }
            c_next = k << a.chunk_shift;
            c_end = (c_next + chunk < nsamples) ? c_next + chunk : nsamples;
          }
          const int avail = (int)(c_end - c_next);
          const int take = (want - given < avail) ? want - given : avail;
          if (!S.trav && S.g < 0 && r >= given && r < given + take) my = (long long)c_next + (r - given);
          c_next += (unsigned long long)take;
          given += take;
        }
        // (sched = 2: the hand-out position names its sample through the cost-ordered table)
        if (my >= 0) init_sample<COUNT, TABLES, QN>(a, S, cn, a.sample_order ? (long long)a.sample_order[my] : my);
      }
    }
    lds_rng[0][tid] = make_uint4(S.rng.v0, S.rng.v1, S.rng.v2, S.rng.v3);
    lds_rng[1][tid] = make_uint4(S.rng.v4, S.rng.d, __float_as_uint(S.rng.bm_extra), (uint32_t)S.rng.bm_flag);
    lds_park[0][tid] = make_uint4(__float_as_uint(S.L.x), __float_as_uint(S.L.y), __float_as_uint(S.L.z), __float_as_uint(S.alpha));
    lds_park[1][tid] = make_uint4(__float_as_uint(S.wD.x), __float_as_uint(S.wD.y), __float_as_uint(S.wD.z), __float_as_uint(S.Hior));
    if (__ballot(S.trav || S.batch_pending) == 0) {
      if (exhausted && __ballot(S.g >= 0) == 0) break;
      continue;
    }

    // ================= traversal phase: traverse_lbvh, bvh_traversal.cu:92-183 =================
    const float tmin = 0.0001f;
    for (;;) {
      const unsigned long long tm = __ballot(S.trav);
      // lanes whose batch ray finished and whose next one this header may start (not MIRT_HELD ones: the shade phase vets them)
      const bool pend = !S.trav && S.batch_pending && !MIRT_HELD;
      const unsigned long long bm = __ballot(pend);
      if (tm == 0 && bm == 0) break;
      // leave when enough lanes are waiting to shade (they cannot progress while the wave keeps traversing); a wave with
      // few live lanes (the drain at the end of the frame) does not wait for company: there the critical path is one
      // lane's bounce chain
      // lanes that wait: to shade, or (finished) for a new sample while the frame still has some
      const int nwait = __popcll(__ballot(!S.trav && !pend && (S.g >= 0 || !exhausted)));
      const int nlive = __popcll(__ballot(S.g >= 0));
      const bool drain = exhausted && nlive <= h.drain_lanes;
      if (nwait >= h.refill_k || (drain && nwait > 0)) break;
      // lanes whose batch ray finished move on to the next ray of their batch (cheap; done in groups)
      if (bm != 0 && (__popcll(bm) >= h.batch_k || tm == 0 || drain)) {
        if (START_LDS) {
          // The values the arm merely looks at and the sun record each lane indexes come from the wave's LDS block: no
          // vector-memory load, no wait on one, before start_ray.  Planes and the records' grid stay scalar loads through `h`.
          if (pend) {
            const uint4 hd = *reinterpret_cast<const uint4*>(lds_raw + HEAD_AT);
            StartLdsArgs hh;
            static_cast<HotArgs&>(hh) = h;
            hh.root_ref = __builtin_amdgcn_readfirstlane(hd.x); hh.num_planes = (int)__builtin_amdgcn_readfirstlane(hd.y);
            hh.num_suns = (int)__builtin_amdgcn_readfirstlane(hd.z); hh.num_bulbs = 0; hh.shadow_anyhit = (int)__builtin_amdgcn_readfirstlane(hd.w);
            hh.suns = reinterpret_cast<const SunLds*>(lds_raw + SUNS_AT);
            batch_next<COUNT, QN, StartLdsArgs, SPEC>(hh, S, cn);
            S.tos = REF_NONE;      // (the next ray's empty stack)
          }
        } else if (LDS_ONLY) {
          // This kernel keeps only the arm's data pointers that are read through (planes, the records' grid) in scalar registers.
          // The values the arm merely looks at -- the root reference, the counts of planes and lights, the shadow-ray mode -- and
          // the light array's address are read where the arm runs, through the same opaque pointer as the shade phase: four
          // scalar loads issued together, one level deep.  Passed by value they, and the loop-invariant conditions the compiler
          // derives from them, did not fit the scalar registers across the traversal loop and were reloaded from spill lanes in
          // every execution of the arm.  (All of them read through the pointer, planes and grid included, is two dependent loads
          // deep and was measured slower than the reloads: DESIGN.md section 4.)
          if (pend) {
            const RenderArgs* hq = ap;
            asm volatile("" : "+s"(hq));
            HotArgs hh = h;
            hh.suns = hq->suns; hh.root_ref = hq->root_ref; hh.num_planes = hq->num_planes; hh.num_suns = hq->num_suns; hh.num_bulbs = hq->num_bulbs;
            hh.shadow_anyhit = hq->shadow_anyhit;
            batch_next<COUNT, QN, HotArgs, SPEC>(hh, S, cn);
            S.tos = REF_NONE;      // (the next ray's empty stack)
          }
        } else {
          if (pend) batch_next<COUNT, QN, HotArgs, SPEC>(h, S, cn);
        }
      }
      // A wave executes the node path and the primitive path one after the other whenever its lanes are split between
      // them, and with ~45 live lanes nearly every iteration has a lane or two at a primitive.  So lanes that reach a
      // primitive wait until leaf_k of them have one pending (or nothing else is left to do): the primitive code then
      // runs in a fraction of the iterations.  Each ray still performs exactly the same sequence of steps.
      // (nothing reads S.cur of a lane that is not traversing: a ray start overwrites it, the shade phase goes by S.refbest)
      if (CUR_MARK && !S.trav) S.cur = REF_NONE;
      const bool leaf0 = S.trav && (S.cur & REF_LEAF) != 0;
      const unsigned long long lm = __ballot(leaf0);
      const bool do_leaf0 = __popcll(lm) >= h.leaf_k || __ballot(S.trav && !leaf0) == 0 || drain;
      // `reps` steps per pass through the header above: the bookkeeping is amortised; a lane whose ray ends in the first
      // step idles through the others, and a primitive reached in a later step waits for the next pass
      // (LDS_ONLY: the count is made opaque here, so that what the compiler derives from it for the loop below -- the count less
      // the peeled first step -- is computed per pass and not kept, in a spilled scalar register, across the kernel)
      int reps = h.reps;
      if (LDS_ONLY) asm volatile("" : "+s"(reps));
      for (int rep = 0; rep < reps; ++rep) {
      const bool leaf = (CUR_MARK ? S.cur != REF_NONE : S.trav) && (S.cur & REF_LEAF) != 0;
      const bool do_leaf = rep == 0 && do_leaf0;
      if (CUR_MARK ? (int)S.cur >= 0 || (leaf && do_leaf) : S.trav && (!leaf || do_leaf)) {
        if (COUNT) ++S.steps;      // (scheduling statistic: the frames that measure their chunks run the counting kernels)
        // one record per step: a node (64 B: two child boxes + two child references) or a primitive (sphere 16 B,
        // triangle 48 B), addressed by one scalar base (the record heap) + a 32-bit byte offset.  Each kind loads the
        // quarters it needs inside its own branch: no merged/zero-filled registers between the two paths.
        const float4* rec = reinterpret_cast<const float4*>(heap + (S.cur << 4));
        bool pop = false;
        if (leaf) {
          // intersect_leaf_primitives, bvh_traversal.cu:47-89
          float t = 0.0f;
          bool hit = false;
          const float4 q0 = rec[0];
          const bool tri = !NOTRI && (S.cur & REF_TRI) != 0;
          if (tri) {
            if (COUNT) cn.tri_tests++;
            const float4 q1 = rec[1], q2 = rec[2];
            hit = triangle_hit(q0, q1, q2, S.o, S.d, t);
          } else {
            if (COUNT) cn.sphere_tests++;
            float tc, t_far;
            hit = sphere_hit(q0, S.o, S.d, t, tc, t_far);
            if (QN && hit && (NOTRI || S.qsx != 0u)) hit = sphere_leaf_box_admits(q0, S.o, S.d, tc, t_far);
          }
          // (S.trav is true here)
          bool closer = closer_hit(hit, t, S.tbest, S.cur & REF_OFFMASK, S.refbest);
          if (QN && !NOTRI && closer && tri && S.qsx != 0u) {
            f3 inv;
            if (!triangle_leaf_reached(ap, S.cur & REF_OFFMASK, S.o, S.d, t, tmin, inv)) {
              // walk this ray again from the root, over the exact records (node 0 sits at heap offset 0), left child first
              closer = false;
              S.inv = inv; S.qsx = 0u;
              S.tos = 0u; S.sp = 1;      // (the pop below makes the root the current node)
              S.tbest = INFINITY; S.refbest = REF_NONE;
            }
          }
          S.tbest = closer ? t : S.tbest;
          S.refbest = closer ? S.cur : S.refbest;
          // any-hit exit (LDS_ONLY: the entries it leaves on the stack go at the next ray start, S.tos = REF_NONE)
          pop = !(closer && S.shadow && t < S.limit);
          if (CUR_MARK) { if (!pop) S.cur = REF_NONE; }
          else S.trav = pop;
        } else {
          if (COUNT) cn.internal_visits++;
          // hit_aabb_adapted, bvh_traversal.cu:11-44, on both children
          // (the empty asm keeps the compiler from merging this branch's first load with the primitive branch's and
          // waiting for it before the other three are issued)
          uint32_t noff = S.cur << 4;
          asm volatile("" : "+v"(noff));
          const float4* nrec = reinterpret_cast<const float4*>(heap + noff);
          bool hl, hr;
          float tel, ter;
          uint32_t lref, rref;
          // push `v`: the previous top of stack goes to memory, the new top stays in a register.  With n entries on the stack,
          // entry k < n sits in slot k and entry n is S.tos (slot 0 only ever receives the dead S.tos of an empty stack), so
          // the slot to write is simply the current depth.
          // Capacity without the spill area: pushes at depths 0 .. lds_depth - 1 stay in LDS, so lds_depth entries -- the top in
          // S.tos, entries 1 .. lds_depth - 1 in the slots of their number.  STACK_LDS_CAPACITY (render_plan.h) is that with
          // lds_depth = STACK_LDS, all the slots there are.
          // LDS_ONLY: the plan has shown that the entries fit.  This binary walk pushes at most one sibling per internal node on
          // the path from the root to the current node and pops it before it leaves that node's subtree, so the entries pending
          // never exceed the internal nodes on that path: at most D, the tree's depth counted in internal nodes (lbvh_build.hip),
          // and D <= STACK_LDS_CAPACITY.  An empty stack has REF_NONE in S.tos; the first push moves it to slot 0 and the pop
          // that empties the stack brings it back, so "the popped reference is REF_NONE" ends the walk.
#define MIRT_PUSH(v) do { if (LDS_ONLY || S.sp < h.lds_depth) lds_stack[S.sp * TRACE_BLOCK + tid] = S.tos; \
                          else h.stack_spill[(size_t)(S.sp - h.lds_depth) * gthreads + gid] = S.tos; \
                          S.tos = (v); ++S.sp; if (COUNT) cn.max_stack = max(cn.max_stack, (uint32_t)S.sp); } while (0)
          if (WIDE && S.qsx != 0u) {
            // four 16-byte requests: the boxes of up to four grandchildren in the reference's visiting order, their references.
            // The first one hit is descended, the others are pushed last first -- the reference's depth-first order over a
            // superset of the nodes it visits (it tests the children of the right child only when that is popped, against a
            // best distance that may have shrunk meanwhile).  The last push is the common one below.
            const uint4 w0 = *reinterpret_cast<const uint4*>(nrec), w1 = *reinterpret_cast<const uint4*>(nrec + 1);
            const uint4 w2 = *reinterpret_cast<const uint4*>(nrec + 2), w3 = *reinterpret_cast<const uint4*>(nrec + 3);
            const bool h0 = box_q(w0.x, w0.y, w0.z, S.inv, S.qb, S.qc, S.qsx, S.qsy, S.qsz, S.tbest, tmin);
            const bool h1 = box_q(w0.w, w1.x, w1.y, S.inv, S.qb, S.qc, S.qsx, S.qsy, S.qsz, S.tbest, tmin);
            const bool h2 = box_q(w1.z, w1.w, w2.x, S.inv, S.qb, S.qc, S.qsx, S.qsy, S.qsz, S.tbest, tmin);
            const bool h3 = box_q(w2.y, w2.z, w2.w, S.inv, S.qb, S.qc, S.qsx, S.qsy, S.qsz, S.tbest, tmin);
            uint32_t cand = w3.w;
            bool have = h3;
            if (h2 && have) MIRT_PUSH(cand);
            cand = h2 ? w3.z : cand; have = have || h2;
            if (h1 && have) MIRT_PUSH(cand);
            cand = h1 ? w3.y : cand; have = have || h1;
            hl = h0 || have; hr = h0 && have;
            lref = h0 ? w3.x : cand; rref = cand;
            tel = 0.0f; ter = 0.0f;
          } else if (QN && NOTRI) {
            // two 16-byte requests: twelve grid coordinates and the child references; every node of a sphere-only scene may be
            // descended near child first
            const uint4 w0 = *reinterpret_cast<const uint4*>(nrec), w1 = *reinterpret_cast<const uint4*>(nrec + 1);
            box_pair_q(w0, w1.x, w1.y, S.inv, S.qb, S.qc, S.qsx, S.qsy, S.qsz, S.tbest, tmin, hl, hr, tel, ter);
            lref = w1.z; rref = w1.w;
            order_children(hl, hr, tel, ter, NODE_SWAP_ANY | NODE_SWAP_PURE, h.swap_mask, lref, rref);
          } else {
            const float4 q0 = nrec[0], q1 = nrec[1], q2 = nrec[2];
            const uint4 ch = *reinterpret_cast<const uint4*>(nrec + 3);      // child references, NODE_SWAP_* flags
            box_pair(q0, q1, q2, S.o.x, S.o.y, S.o.z, S.inv.x, S.inv.y, S.inv.z, S.tbest, tmin, hl, hr, tel, ter);
            lref = ch.x; rref = ch.y;
            // (with QN every lane in this branch is walking its ray again: the reference's order, left first)
            if (!QN) order_children(hl, hr, tel, ter, ch.z, h.swap_mask, lref, rref);
          }
          // first child next, push the second (bvh_traversal.cu:149-157: left, right), written with selects: one short
          // branch for the push
          const bool both = hl && hr;
          // (no depth check: the stack cannot outgrow STACK_TOTAL.  A Karras tree over 30-bit codes with the index tie-break of
          // lbvh_builder.cu:76-101 is a radix tree over (code, index) keys of 30 + ceil(log2 N) bits, N < 2^28 (checked at scene
          // creation), so it is at most 58 levels deep, and the walk keeps at most one pending sibling per level.  The
          // reference's "stack overflow" warning, bvh_traversal.cu:154-164, is unreachable for the same reason.  LDS_ONLY: the
          // same one-sibling-per-level argument with the built tree's own depth D in place of 58, at MIRT_PUSH above.)
          if (both) MIRT_PUSH(rref);
#undef MIRT_PUSH
          S.cur = hl ? lref : (hr ? rref : S.cur);
          pop = !(hl || hr);
        }
        if (pop) {
          // an empty stack ends the traversal; otherwise the top becomes the current node and the new top is reloaded
          // (a dead read of slot 0 when the stack is now empty)
          if (LDS_ONLY) {
            // (the walk ends on the REF_NONE below the entries; popping it leaves the depth at zero and reads slot 0 again)
            S.cur = S.tos;
            if (!CUR_MARK) S.trav = S.cur != REF_NONE;
            S.sp = (int)__builtin_elementwise_sub_sat((uint32_t)S.sp, 1u);
            S.tos = lds_stack[S.sp * TRACE_BLOCK + tid];
          } else {
            S.trav = S.sp != 0;
            S.cur = S.tos;
            S.sp = S.sp > 0 ? S.sp - 1 : 0;
            S.tos = lds_stack[(S.sp < h.lds_depth ? S.sp : 0) * TRACE_BLOCK + tid];
            if (S.sp >= h.lds_depth) S.tos = h.stack_spill[(size_t)(S.sp - h.lds_depth) * gthreads + gid];
          }
        }
      }
      }
      if (CUR_MARK) S.trav = S.cur != REF_NONE;
    }
  }

  if (COUNT) flush_counters(cn, ap->counters, tid);
}
#undef MIRT_HELD

// (to_srgb8, draw.cu:9-11, and mean_of: device_common.h)
// draw.cu:129-132: plain float -> unsigned char conversion
MIRT_DEV unsigned char to_uchar_trunc(float f)
{
  if (!(f > 0.0f)) return 0;
  if (f >= 255.0f) return 255;
  return (unsigned char)f;
}

// pixel_color_accum / uchar conversion, draw.cu:191-205 (spp > 1) and draw.cu:120-135 (spp <= 1)
MIRT_DEV void write_pixel(const ResolveArgs& a, long long lq, const float4 sum)
{
  const long long lp = a.pixel_base + lq;
  const float4 m = a.count > 1 ? mean_of(sum, a.count) : sum;
  if (a.rgba_f32) a.rgba_f32[lp] = m;
  uchar4 o;
  if (a.spp <= 1) {
    o.x = to_uchar_trunc(rgb_to_srgb(m.x) * 255);
    o.y = to_uchar_trunc(rgb_to_srgb(m.y) * 255);
    o.z = to_uchar_trunc(rgb_to_srgb(m.z) * 255);
    o.w = to_uchar_trunc(m.w * 255);
  } else {
    o = to_srgb8(m);
  }
  reinterpret_cast<uchar4*>(a.rgba8)[lp] = o;
}

// spp <= 1, and the fallback for P > 64: one thread per pixel
__global__ void __launch_bounds__(RBLOCK) resolve_kernel(const ResolveArgs a)
{
  const long long lp = (long long)blockIdx.x * RBLOCK + threadIdx.x;
  if (lp >= a.num_local_pixels) return;
  float4 m;
  if (a.count <= 1) {
    m = a.samples[lp];
  } else {
    int P = 1, lg = 0;
    while (P < a.count) { P <<= 1; ++lg; }
    m = butterfly_sum<false>(a.samples + lp * a.count, a.count, P, lg);
  }
  write_pixel(a, lp, m);
}

// The same sum for P <= 64 with one lane per sample: coalesced 16-byte loads, then literally the reference's butterfly
// `for (mask = P/2; mask > 0; mask /= 2) v += shfl_xor(v, mask)` (draw.cu:181-189) inside each group of P lanes; the
// group's lane 0 parks its sum in LDS and the first threads of the block finish the block's pixels (full waves in the
// sRGB code instead of one lane in P).
constexpr int TBLOCK = 1024;
__global__ void __launch_bounds__(TBLOCK) resolve_tree_kernel(const ResolveArgs a, int P, int lg)
{
  __shared__ float4 sums[TBLOCK / 2];
  const int tid = threadIdx.x;
  const int ppb = TBLOCK >> lg;                       // pixels per block
  const int si = tid & (P - 1);
  const long long lp = (long long)blockIdx.x * ppb + (tid >> lg);
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (lp < a.num_local_pixels && si < a.count) v = a.samples[lp * a.count + si];
  for (int mask = P >> 1; mask > 0; mask >>= 1) {
    v.x += __shfl_xor(v.x, mask); v.y += __shfl_xor(v.y, mask); v.z += __shfl_xor(v.z, mask); v.w += __shfl_xor(v.w, mask);
  }
  if (si == 0) sums[tid >> lg] = v;
  __syncthreads();
  const long long lq = (long long)blockIdx.x * ppb + tid;
  if (tid < ppb && lq < a.num_local_pixels) write_pixel(a, lq, sums[tid]);
}

// Local pixel lp of part `part_id`'s compact buffer -> its place in the frame: the part holds its stripes (stripe i = rows
// [i stripe_rows, (i + 1) stripe_rows), owned by part i % num_parts) in increasing order, each row-major (include/mirt.h,
// MirtRenderParams).  init_sample_core does the same arithmetic in 32 bits.
__host__ __device__ inline void part_pixel_xy(long long lp, int width, int stripe_rows, int num_parts, int part_id, long long& x, long long& y)
{
  const long long stripe_pixels = (long long)stripe_rows * width;
  const long long ls = lp / stripe_pixels, within = lp - ls * stripe_pixels;
  const long long gs = ls * num_parts + part_id;
  y = gs * stripe_rows + within / width;
  x = within % width;
}

__global__ void __launch_bounds__(RBLOCK) scatter_kernel(const uchar4* __restrict__ part, uchar4* __restrict__ frame, long long n,
                                                         int width, int height, int stripe_rows, int num_parts, int part_id)
{
  const long long lp = (long long)blockIdx.x * RBLOCK + threadIdx.x;
  if (lp >= n) return;
  long long x, y;
  part_pixel_xy(lp, width, stripe_rows, num_parts, part_id, x, y);
  frame[y * width + x] = part[lp];
}

__global__ void probe_math_kernel(int which, int n, const float* __restrict__ in, float* __restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = in[i];
  float y;
  switch (which) {
    case 0: y = dm_logf(x); break;
    case 1: y = dm_expf(x); break;
    case 2: y = dm_sinf(x); break;
    case 3: y = dm_cosf(x); break;
    case 4: y = dm_powf(x, 1 / 2.4f); break;
    case 5: y = rgb_to_srgb(x); break;
    case 6: y = sqrtf(x); break;
    case 7: y = 1.0f / x; break;
    default: y = x;
  }
  out[i] = y;
}

// mirt_probe_qbox (mirt.h): one case per thread through the builder's qlo / qhi and the walk's quantised_axis, box_pair,
// box_pair_q (the packed box as the left child, then as the right one) and box_q.  The grid's step and 2^60 / step are computed as
// pack_qnodes_kernel computes them (lbvh_build.hip), 1 / d and the three axes as start_ray<QN> does (shade_common.h).
__global__ void probe_qbox_kernel(int n, const float* __restrict__ in, uint32_t* __restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* c = in + 20 * (size_t)i;
  const float tmin = 0.0001f;
  float smin[3], step[3], lim[3];
  uint32_t lo[3], hi[3], w[3];
  for (int k = 0; k < 3; ++k) {
    smin[k] = c[k];
    const float range = c[3 + k] - smin[k];
    step[k] = range > 0.0f ? range / QGRID : 1.0f;
    lim[k] = QINV_STEPS / step[k];
    lo[k] = qlo(c[6 + k], smin[k], step[k]);
    hi[k] = qhi(c[9 + k], smin[k], step[k]);
    w[k] = lo[k] | (hi[k] << 16);
  }
  const f3 o = mk3(c[12], c[13], c[14]), d = mk3(c[15], c[16], c[17]);
  const float tbest = c[18];
  const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  f3 A, Cn, Cf;
  uint32_t sx, sy, sz;
  quantised_axis(smin[0], step[0], lim[0], o.x, inv.x, A.x, Cn.x, Cf.x, sx);
  quantised_axis(smin[1], step[1], lim[1], o.y, inv.y, A.y, Cn.y, Cf.y, sy);
  quantised_axis(smin[2], step[2], lim[2], o.z, inv.z, A.z, Cn.z, Cf.z, sz);
  // the other child of the pair: some other box (every coordinate differs from the tested one's)
  const uint32_t v[3] = {w[0] ^ 0x5a5aa5a5u, w[1] ^ 0x0ff0f00fu, w[2] ^ 0xa5a55a5au};
  bool hit[4], other;
  float te[3], te_other;
  // the exact box as the left child of a 64-byte record (the right child: the same box)
  const float4 q0 = make_float4(c[6], c[9], c[7], c[10]), q1 = make_float4(c[8], c[11], c[6], c[9]), q2 = make_float4(c[7], c[10], c[8], c[11]);
  box_pair(q0, q1, q2, o.x, o.y, o.z, inv.x, inv.y, inv.z, tbest, tmin, hit[0], other, te[0], te_other);
  box_pair_q(make_uint4(w[0], w[1], w[2], v[0]), v[1], v[2], A, Cn, Cf, sx, sy, sz, tbest, tmin, hit[1], other, te[1], te_other);
  box_pair_q(make_uint4(v[0], v[1], v[2], w[0]), w[1], w[2], A, Cn, Cf, sx, sy, sz, tbest, tmin, other, hit[2], te_other, te[2]);
  hit[3] = box_q(w[0], w[1], w[2], A, Cn, Cf, sx, sy, sz, tbest, tmin);
  uint32_t* r = out + 20 * (size_t)i;
  for (int k = 0; k < 3; ++k) { r[k] = lo[k]; r[3 + k] = hi[k]; r[14 + k] = __float_as_uint(step[k]); r[17 + k] = __float_as_uint(lim[k]); }
  for (int k = 0; k < 4; ++k) r[6 + k] = hit[k] ? 1u : 0u;
  for (int k = 0; k < 3; ++k) r[10 + k] = __float_as_uint(te[k]);
  r[13] = 0u;
}

// out[i*draws + k]: k-th raw 32-bit draw of stream i.  mode 0: curand_init(1234 + i/spp.., ...) is exercised through
// xw_init exactly as the trace kernel does: pixel = i / spp, sample = i % spp (spp > 1) or pixel = i (spp <= 1).
__global__ void probe_xorwow_kernel(RngTablesDev t, int spp, int nstreams, int draws, uint32_t* __restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nstreams) return;
  Xorwow s;
  if (spp > 1) xw_init(s, t, (uint32_t)(i / spp), (uint32_t)(i % spp));
  else xw_init(s, t, (uint32_t)i, 0u);
  for (int k = 0; k < draws; ++k) out[(size_t)i * draws + k] = xw_next(s);
}

// ---- longest-first scheduling: order the frame's chunks by the cost measured on a previous frame ------------------------
constexpr int SORT_BINS = 1024;
MIRT_DEV uint32_t cost_bin(uint32_t c) { const uint32_t b = c >> 3; return b < (uint32_t)SORT_BINS ? (uint32_t)(SORT_BINS - 1) - b : 0u; }   // bin 0 = most expensive
// One block: the per-bin counters are LDS atomics (global atomics on a handful of hot bins -- half the frame is sky --
// ran at ~90 per microsecond), and each thread walks a contiguous run of chunks and adds a run of equal bins at once.
__global__ void __launch_bounds__(SORT_BINS) order_kernel(const uint32_t* __restrict__ cost, uint32_t n, uint32_t* __restrict__ order)
{
  __shared__ uint32_t bins[SORT_BINS];
  const int t = threadIdx.x;
  bins[t] = 0;
  __syncthreads();
  const uint32_t per = (n + SORT_BINS - 1) / SORT_BINS;
  const uint32_t lo = min(n, (uint32_t)t * per), hi = min(n, lo + per);
  {
    uint32_t cb = 0, cnt = 0;
    for (uint32_t i = lo; i < hi; ++i) {
      const uint32_t b = cost_bin(cost[i]);
      if (cnt && b != cb) { atomicAdd(&bins[cb], cnt); cnt = 0; }
      cb = b; ++cnt;
    }
    if (cnt) atomicAdd(&bins[cb], cnt);
  }
  __syncthreads();
  const uint32_t own = bins[t];
  for (int o = 1; o < SORT_BINS; o <<= 1) {
    const uint32_t x = (t >= o) ? bins[t - o] : 0;
    __syncthreads();
    bins[t] += x;
    __syncthreads();
  }
  const uint32_t excl = bins[t] - own;
  __syncthreads();
  bins[t] = excl;
  __syncthreads();
  {
    uint32_t cb = 0, cnt = 0, first = lo;
    for (uint32_t i = lo; i <= hi; ++i) {
      const uint32_t b = (i < hi) ? cost_bin(cost[i]) : 0xffffffffu;
      if (cnt && b != cb) {
        const uint32_t base = atomicAdd(&bins[cb], cnt);
        for (uint32_t k = 0; k < cnt; ++k) order[base + k] = first + k;
        cnt = 0;
      }
      if (cnt == 0) first = i;
      cb = b; ++cnt;
    }
  }
}

// mirt_probe_sched which = 0: cost_key itself, one value per thread
__global__ void probe_cost_key_kernel(int n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = cost_key(in[i]);
}

int64_t local_pixels(const MirtRenderParams* p)
{
  if (p->width <= 0 || p->height <= 0 || p->stripe_rows <= 0 || p->num_parts <= 0 || p->part < 0 || p->part >= p->num_parts) return -1;
  const int64_t nstripes = ((int64_t)p->height + p->stripe_rows - 1) / p->stripe_rows;
  int64_t rows = 0;
  for (int64_t s = p->part; s < nstripes; s += p->num_parts) {
    const int64_t r0 = s * p->stripe_rows;
    const int64_t r1 = r0 + p->stripe_rows < p->height ? r0 + p->stripe_rows : p->height;
    rows += r1 - r0;
  }
  return rows * p->width;
}

} // namespace

// sample_tables >= 1: tables of the sequence skips of sample indices [0, sample_tables) (curand_init(1234 + pixel, sample, 0));
// 0: the per-pixel tables of curand_init(1234, pixel, 0).  allow_larger: tables for more sample indices serve as well.
int ensure_rng_tables(RngCache* rc, int sample_tables, long long frame_pixels, hipStream_t stream, RngTablesDev* out, bool allow_larger)
{
  const int spp = sample_tables;
  const long long key = spp >= 1 ? (long long)spp : -frame_pixels;
  if (rc->key != key && !(allow_larger && spp >= 1 && rc->key >= key)) {
    if (spp >= 1) build_sample_tables(spp, rc->host);
    else build_pixel_tables(frame_pixels, 1234, rc->host);
    MIRT_HIP(hipDeviceSynchronize());   // (not grow(): another stream may still be reading the old tables)
    rng_cache_free(rc);
    const RngTables& t = rc->host;
    MIRT_TRY(rc->A.alloc(t.A.size() / 4, "rc->A")); MIRT_HIP(hipMemcpy(rc->A, t.A.data(), t.A.size() * 4, hipMemcpyHostToDevice));      // (A: whole uint4)
    MIRT_TRY(rc->B.alloc(t.B.size(), "rc->B")); MIRT_HIP(hipMemcpy(rc->B, t.B.data(), t.B.size() * 4, hipMemcpyHostToDevice));
    MIRT_TRY(rc->K.alloc(t.K.size(), "rc->K")); MIRT_HIP(hipMemcpy(rc->K, t.K.data(), t.K.size() * 4, hipMemcpyHostToDevice));
    MIRT_TRY(rc->R2.alloc(t.R2.size(), "rc->R2"));
    if (!t.R2.empty()) MIRT_HIP(hipMemcpy(rc->R2, t.R2.data(), t.R2.size() * 4, hipMemcpyHostToDevice));
    rc->key = key;
  }
  const RngTables& t = rc->host;
  out->A = rc->A; out->B = rc->B; out->K = rc->K; out->R2 = rc->R2;
  out->mode = t.mode; out->chunk_bits = t.chunk_bits; out->nin_words = t.nin_words; out->nchunks = t.nchunks; out->d0 = t.d0;
  return MIRT_OK;
}

// (the tables go back with their owner; a cache without a key is made again by the next call)
void rng_cache_free(RngCache* rc)
{
  rc->key = -1;
}

// One call of mirt_render / mirt_render_accumulate.  The part's pixels are rendered in slabs of at most 2^slab_log2 samples,
// so the per-sample workspace is bounded (4 GiB by default) whatever the frame: BASELINE config 5 (3840x2160 x 256 spp,
// 2.1 G samples) takes 8 slabs instead of a 34 GB buffer.  Each slab is a trace launch + a resolve launch; a slab boundary
// costs one drain of the persistent grid (~1-2 ms per 64 M samples).
//   d_accum == null: pixels are written (mean, sRGB, quantise);  sample_first must be 0 and sample_count max(spp, 1)
//   d_accum != null: the sum of each pixel's samples [sample_first, sample_first + sample_count) is ADDED to d_accum (adaptive.hip,
//                    resolve_moments)
//   ax != null (with d_accum): mirt_render_accumulate_pixels -- the second moment and the counts are added as well, and with
//                    ax->list only the listed pixels are rendered: every launch hands out, through RenderArgs::sample_order, the
//                    samples of the listed pixels of its slab (adaptive.hip) instead of the scene's measured order, to the same
//                    trace kernels.  The workspace stays indexed by the slab's dense sample number.
// What the call decides without the device is plan_call's (render_plan.h); render_impl, at the end, carries the plan out
// through the steps below, in this order.
struct RenderCall {
  MirtScene* sc; const MirtRenderParams* p;
  void* d_rgba8; void* d_rgba_f32; void* d_accum; const AdaptiveArgs* ax;      // outputs; the list and moments of ..._accumulate_pixels
  int sample_first, sample_count;
  hipStream_t stream;
  bool sparse() const { return ax && ax->list; }
  bool count() const { return (p->flags & MIRT_RENDER_COUNTERS) != 0; }
};

// The first thing that plans a call: it settles the facts -- after a material update in place the primitives' share of
// any_trans / any_rough / colors_finite is known only to the device, and this waits, once, for the update's reduction
// (update_shading.hip) -- and recombines them with the host's share (planes, lights, exposure).
// The measurement of a sample order in flight (sample_table_finish), once its event has passed: the order is usable, and the
// counts its call copied to the pinned words give the scene's primitive tests per internal-node visit.  No wait: a call that
// finds the event still pending goes on without the order and without the ratio.  `wait`: mirt_get_sample_order.
static int sample_order_landed(MirtScene* sc, bool wait = false)
{
  if (!sc->so_busy) return MIRT_OK;
  if (wait) MIRT_HIP(hipEventSynchronize(sc->so_ev));
  else if (hipEventQuery(sc->so_ev) != hipSuccess) return MIRT_OK;
  sc->so_busy = false;
  const unsigned long long* n = sc->so_counts_host;      // internal visits, sphere tests, triangle tests
  sc->so_ratio = (n && !sc->so_ratio_stale && n[0] > 0) ? (float)((double)(n[1] + n[2]) / (double)n[0]) : -1.0f;
  sc->so_ratio_stale = false;
  return MIRT_OK;
}

static int scene_facts(MirtScene* sc, SceneFacts* out)
{
  int rc = settle_facts(sc);
  if (rc != MIRT_OK) return rc;
  rc = sample_order_landed(sc);
  if (rc != MIRT_OK) return rc;
  SceneFacts f;
  f.prim_ratio = sc->so_ratio;
  f.N = sc->N; f.Nt = sc->Nt; f.grid_ok = sc->grid_ok; f.tree_depth = sc->tree_depth;
  f.has_quantised = sc->root_ref_q != REF_NONE; f.has_wide = sc->root_ref_w != REF_NONE;
  f.colors_finite = sc->colors_finite; f.any_trans = sc->any_trans; f.any_rough = sc->any_rough;
  f.gi = sc->d.gi; f.bounces = sc->d.bounces; f.num_suns = sc->d.num_suns; f.num_bulbs = sc->d.num_bulbs;
  *out = f;
  return MIRT_OK;
}

// step 1: the call's arguments.  MIRT_OK with *npix = 0: an empty part, nothing to do.
static int check_call(const RenderCall& c, int64_t* npix)
{
  const char* who = c.ax ? "mirt_render_accumulate_pixels" : (c.d_accum ? "mirt_render_accumulate" : "mirt_render");
  *npix = 0;
  if (!c.sc->built) { set_error(std::string(who) + ": call mirt_build_lbvh first"); return MIRT_ERR_STATE; }
  const int64_t n = local_pixels(c.p);
  if (n < 0 || c.p->spp < 0 || (!c.d_rgba8 && !c.d_accum)) { set_error(std::string(who) + ": bad parameters"); return MIRT_ERR_ARG; }
  if (c.sample_first < 0 || c.sample_count < 1 || (long long)c.sample_first + c.sample_count > MAX_SPP) {
    set_error(std::string(who) + ": more than 4096 samples per pixel (mirt_render_accumulate renders any number in several calls of at most 4096)"); return MIRT_ERR_ARG;
  }
  bool go = false;
  const int rc = check_frame(who, c.p, n, &go);
  if (rc != MIRT_OK || !go) return rc;
  if (c.sparse() && c.sc->opt.wavefront != 0) { set_error(std::string(who) + ": a pixel list is not supported with wavefront = 1 (the trace / shade kernel pair does not hand samples out through a table)"); return MIRT_ERR_ARG; }
  *npix = n;
  return MIRT_OK;
}

// step 2: the persistent grid of the call's trace launches
static int size_grid(MirtScene* sc, const CallPlan& pl, bool count, hipStream_t stream)
{
  if (!sc->grid_blocks && persistent_grid_blocks(sc->device, trace_kernel<false, 8, false>, TRACE_BLOCK, 4 * 256 / TRACE_BLOCK, &sc->grid_blocks) != hipSuccess)
    sc->grid_blocks = 1024;      // per scene, i.e. per device
  const int blocks_cached = sc->grid_blocks;
  const long long want_blocks = (pl.launch_samples_max + TRACE_BLOCK - 1) / TRACE_BLOCK;
  int blocks = (int)(want_blocks < blocks_cached ? want_blocks : blocks_cached);
  // A small frame (one GPU's stripe set of an 8-GPU job) rendered while another frame is in flight gets half the grid:
  // every wave ends with a drain -- its last samples, few live lanes, 0.5-2.5 ms -- during which it holds its slot, and
  // with two half-grid frames resident at a time there are half as many drains per frame (1/8 of 1080p x 16: 5.8 -> 5.4
  // ms per frame; no gain from 1/4 of a frame up, a loss for a frame rendered alone).
  if (!count && blocks == blocks_cached && pl.launch_samples_max < 20ll * blocks_cached * TRACE_BLOCK) {
    for (int i = 0; i < MIRT_MAX_FRAMES; ++i) {
      const RenderCtx& c = sc->ctx[i];
      if (c.used && c.stream != stream && hipEventQuery(c.ev3) == hipErrorNotReady) { blocks = blocks_cached > 1 ? blocks_cached / 2 : 1; break; }   // (a frame on this same stream does not overlap)
    }
  }
  if (sc->opt.trace_waves >= 1 && sc->opt.trace_waves <= blocks_cached) blocks = sc->opt.trace_waves;
  return blocks;
}

// the finished frame's trace-kernel time goes into the running mean (mirt_get_stats), once
int fold_trace_time(MirtScene* sc, RenderCtx& cx)
{
  if (cx.timed) return MIRT_OK;
  float ms = 0.0f;
  int rc = trace_ms_of(cx, &ms);
  if (rc != MIRT_OK) return rc;
  sc->trace_ms_sum += ms; sc->trace_frames += 1; cx.timed = true;
  return MIRT_OK;
}

// step 3: this frame's context; wait for the frame that used it MIRT_MAX_FRAMES renders ago (the frame counter moves only
// once the frame is actually issued, at the end of render_impl)
static int take_context(MirtScene* sc, RenderCtx** out)
{
  RenderCtx& cx = sc->ctx[sc->frame_no % MIRT_MAX_FRAMES];
  *out = &cx;
  if (!cx.used) return MIRT_OK;
  MIRT_HIP(hipEventSynchronize(cx.ev3));
  return fold_trace_time(sc, cx);
}

// step 4: the context's buffers, at least as large as this call needs them
static int ensure_workspace(const RenderCall& c, RenderCtx& cx, const CallPlan& pl, int blocks)
{
  const hipStream_t stream = c.stream;
  const size_t gthreads = (size_t)blocks * TRACE_BLOCK;
  const size_t samples = (size_t)pl.slab_samples_max;
  const size_t spill_need = (size_t)STACK_TOTAL_WIDE * gthreads;      // (the wide walk pushes up to three entries per two levels)
  const size_t pending_need = (size_t)pl.pending_slots * PENDING_WORDS * gthreads;
  MIRT_TRY(cx.samples.grow(samples, stream, "samples"));
  MIRT_TRY(cx.stack_spill.grow(spill_need, stream, "stack_spill"));
  if (c.sparse()) {
    MIRT_TRY(cx.sp_list.grow((size_t)c.ax->num_listed, stream, "sp_list"));
    MIRT_TRY(cx.sp_table.grow((size_t)pl.launch_samples_max, stream, "sp_table"));
    MIRT_TRY(cx.sp_blocks.grow(sparse_blocks_words(c.ax->num_listed), stream, "sp_blocks"));
  }
  MIRT_TRY(cx.pending.grow(pending_need, stream, "pending"));
  if (c.sc->opt.wavefront == 0 && !cx.args_dev) MIRT_TRY(cx.args_dev.alloc(MAX_SLAB_ARGS, "args_dev"));
  // one event pair per trace launch: a call of several slabs reports the SUM of its launches, not a bracket that would take in
  // the resolve kernels between them
  while ((int)cx.slab_ev.size() < 2 * pl.nslabs) { Event e; MIRT_TRY(e.create()); cx.slab_ev.push_back(std::move(e)); }
  return MIRT_OK;
}

// step 5: the kernel arguments every slab of the call shares (the slab's own are launch_slab's; the hand-out order's follow)
static int fill_args(const RenderCall& c, RenderCtx& cx, const CallPlan& pl, int chunk_shift, RenderArgs& a, HotArgs& h)
{
  MirtScene* sc = c.sc;
  const Options& opt = sc->opt;
  memset(&a, 0, sizeof(a));
  fill_camera(a, sc, c.p);
  a.gi = sc->d.gi; a.spp = pl.args_spp; a.expose = sc->d.expose;
  a.sample_first = c.sample_first; a.sample_count = c.sample_count; a.seed_per_pixel = pl.per_pixel_seed ? 1 : 0;
  a.nodes = sc->nodes; a.unit_prim = sc->unit_prim; a.mats = sc->mats;
  a.root_ref = pl.qn ? (pl.notri ? sc->root_ref_q : sc->root_ref_w) : sc->root_ref;
  a.num_spheres = sc->Ns; a.num_prims = sc->N;
  a.qparams = pl.qn ? sc->qparams : nullptr;
  a.tri_boxes = sc->tri_boxes;
  a.prim_base16 = sc->prim_base / 16u;
  a.swap_mask = pl.swap_mask; a.skip_unlit = pl.skip_unlit; a.shadow_anyhit = pl.shadow_anyhit;
  a.reach_check = pl.reach_check;
  a.reach_slack = 4.76837158203125e-07f * sc->coord_max;
  a.nonfinite_colours = sc->colors_finite ? 0 : 1;
  a.planes = sc->planes; a.num_planes = sc->d.num_planes;
  a.suns = sc->suns; a.num_suns = sc->d.num_suns;
  a.bulbs = sc->bulbs; a.num_bulbs = sc->d.num_bulbs;
  // random numbers are consumed only by jitter (spp >= 1), depth of field, rough normals and GI
  a.needs_rng = (a.spp >= 1) || (sc->d.dof_focus != 0.0f && !sc->d.fisheye && !sc->d.panorama) || pl.shading_rng;
  if (a.needs_rng) {
    int rc = ensure_rng_tables(&sc->rng, pl.rng_sample_tables, (long long)c.p->width * c.p->height, c.stream, &a.rng, c.d_accum != nullptr);
    if (rc != MIRT_OK) return rc;
  }
  a.samples = cx.samples;
  a.stack_spill = cx.stack_spill;
  a.pending = cx.pending; a.pending_slots = pl.pending_slots;
  a.counters = c.count() ? cx.counters : nullptr;
  a.overflow = cx.counters + 9;
  a.work_counter = cx.counters + 8;
  a.lds_depth = pl.lds_depth;
  a.refill_k = opt.wavefront != 0 ? opt.wf_refill_k : pl.refill_k;
  a.drain_lanes = opt.drain_lanes; a.init_k = pl.init_k; a.batch_k = pl.batch_k;
  a.chunk_shift = chunk_shift;
  h.nodes = a.nodes; h.root_ref = a.root_ref; h.swap_mask = a.swap_mask; h.qparams = a.qparams;
  h.planes = a.planes; h.num_planes = a.num_planes; h.suns = a.suns; h.num_suns = a.num_suns; h.bulbs = a.bulbs; h.num_bulbs = a.num_bulbs; h.shadow_anyhit = a.shadow_anyhit;
  h.stack_spill = a.stack_spill; h.lds_depth = a.lds_depth; h.refill_k = pl.refill_k; h.batch_k = a.batch_k; h.drain_lanes = a.drain_lanes;
  h.reach_check = a.reach_check; h.leaf_k = pl.leaf_k; h.reps = pl.reps;
  return MIRT_OK;
}

// ---- step 6a, sched = 1: longest-first CHUNK order (single-kernel path, one-slab calls), per context ---------------------
// The newest finished frame with the same sample count (and chunk size) that MEASURED its chunks provides the order; a frame
// that is still running does not.  The scene is immutable and samples are seeded by pixel and sample index only, so a frame's
// chunk costs are the same every time: once an order exists for this frame size it is reused, and the frame neither stamps
// costs nor sorts them again (the sort took 0.34 ms of a 24 ms frame, on the stream's critical path).
// Returns the order in *order, or null: this frame measures one (chunk_order_finish).
static int chunk_order_find(MirtScene* sc, RenderCtx& cx, size_t nchunks, long long okey, const uint32_t** order)
{
  // (the four are freed together before the first is made, and the last one made stands for all: if any fails, it is empty)
  if (cx.order_out[RenderCtx::ORDER_BUFS - 1].cap() < nchunks) {
    MIRT_HIP(hipDeviceSynchronize());   // (not grow(): a frame on another stream may still be reading one of these orders)
    cx.order_key = -1;
    cx.chunk_cost.reset();
    for (DevBuf<uint32_t>& o : cx.order_out) o.reset();
    MIRT_TRY(cx.chunk_cost.alloc(nchunks, "chunk_cost"));
    for (DevBuf<uint32_t>& o : cx.order_out) MIRT_TRY(o.alloc(nchunks, "order_out"));
  }
  unsigned long long best = 0;
  *order = nullptr;
  for (int i = 0; i < MIRT_MAX_FRAMES; ++i) {
    RenderCtx& c = sc->ctx[i];
    if (&c == &cx || !c.used || c.order_key != okey || c.order_frame <= best) continue;
    if (hipEventQuery(c.order_ev) != hipSuccess) continue;
    best = c.order_frame; *order = c.order_out[(c.order_writes - 1) % RenderCtx::ORDER_BUFS];
  }
  if (!*order && cx.used && cx.order_key == okey) *order = cx.order_out[(cx.order_writes - 1) % RenderCtx::ORDER_BUFS];   // cx's own earlier frame (finished: take_context waited)
  return MIRT_OK;
}

// The order for later frames.  It overwrites the buffer this context wrote three orders ago; every frame that could have read
// that one has finished -- the host waited for each of them when it reused their contexts.
static int chunk_order_finish(RenderCtx& cx, size_t nchunks, long long okey, hipStream_t stream)
{
  uint32_t* out = cx.order_out[cx.order_writes % RenderCtx::ORDER_BUFS];
  hipLaunchKernelGGL(order_kernel, dim3(1), dim3(SORT_BINS), 0, stream, cx.chunk_cost, (uint32_t)nchunks, out);
  MIRT_HIP(hipGetLastError());
  MIRT_HIP(hipEventRecord(cx.order_ev, stream));
  cx.order_key = okey;
  cx.order_frame = cx.frame_id;
  ++cx.order_writes;
  return MIRT_OK;
}

// ---- step 6b, sched = 2 (default): the same idea by SAMPLE -- the samples of every launch in order of decreasing cost class,
// positions within a class kept (a stable one-byte radix pass: neighbours in the frame stay neighbours in the hand-out, and the
// lanes of a wave work on samples of one kind).  One table per scene (4 B per sample of the call, at most 12 GiB), for the call
// shape rendered last; measured by the first call of that shape (counting kernels + one sort per launch), reused afterwards.
// Against the chunk order: a 1/8 stripe share of the headline frame 4.16 -> 3.22 ms alone (its last expensive samples no longer
// start late), redchair.txt 1080p16 23.8 -> 20.5 ms, tenthousand.txt 22.5 -> 21.7.
// *ordered: the table serves this call.  *measure: this call measures it (sample_table_finish).  Neither: frame order.
static int sample_table_find(MirtScene* sc, const CallPlan& pl, long long okey, bool* ordered, bool* measure)
{
  const size_t total = (size_t)pl.total_samples, slab = (size_t)pl.slab_samples_max;
  *ordered = *measure = false;
  MIRT_TRY(sample_order_landed(sc));      // (the measurement in flight has landed?)
  if (sc->so_busy) return MIRT_OK;
  // (the table is a permutation of every launch's sample range: valid for exactly this total and this slab size)
  if (sc->so_key == okey && sc->so_total == pl.total_samples) { *ordered = true; return MIRT_OK; }
  // (no frame in flight reads the old table once every context's frame has finished: wait for them before rewriting it)
  for (int i = 0; i < MIRT_MAX_FRAMES; ++i) if (sc->ctx[i].used) MIRT_HIP(hipEventSynchronize(sc->ctx[i].ev3));
  if (sc->so_order.cap() < total || sc->so_keys.cap() < slab) {
    sc->so_order.reset(); sc->so_keys.reset(); sc->so_keys2.reset(); sc->so_ws.reset(); sc->so_key = -1;
    // (the table is an optimisation: without the memory for it the call is rendered in frame order)
    const bool got = sc->so_order.alloc_raw(total) == hipSuccess && sc->so_keys.alloc_raw(slab) == hipSuccess &&
                     sc->so_keys2.alloc_raw(slab) == hipSuccess && sc->so_ws.alloc_raw(sort_low_byte_ws_words(pl.slab_samples_max)) == hipSuccess;
    if (!got) {
      (void)hipGetLastError();
      sc->so_order.reset(); sc->so_keys.reset(); sc->so_keys2.reset(); sc->so_ws.reset();
      return MIRT_OK;
    }
  }
  // (the counts behind the scene's ratio of primitive tests to node visits travel with the order: without the two small
  // buffers for them the order is measured alone)
  if (!sc->so_counters.get() && sc->so_counters.alloc_raw(12) != hipSuccess) { (void)hipGetLastError(); sc->so_counters.reset(); }
  if (!sc->so_counts_host.get() && sc->so_counts_host.alloc_raw(3) != hipSuccess) { (void)hipGetLastError(); sc->so_counts_host.reset(); }
  *measure = true;
  sc->so_key = -1; sc->so_ratio = -1.0f;      // (another shape: the old order goes, and the ratio with it)
  sc->so_pending_key = okey; sc->so_total = pl.total_samples;
  return MIRT_OK;
}

static int sample_table_finish(MirtScene* sc, hipStream_t stream)
{
  MIRT_HIP(hipEventRecord(sc->so_ev, stream));
  sc->so_key = sc->so_pending_key; sc->so_busy = true;
  return MIRT_OK;
}

// mirt_get_sample_order: the table as the next call of its shape would read it, and the keys of the last launch measured.  A
// measurement in flight is waited for.  (The table outlives camera, geometry and shading updates, as the hand-out does.)
int get_sample_order(MirtScene* sc, MirtSampleOrderInfo* info, uint32_t* order, uint32_t* keys, uint32_t* sorted_keys)
{
  MIRT_TRY(sample_order_landed(sc, true));
  if (sc->so_key < 0 || !sc->so_order.get()) {
    set_error("mirt_get_sample_order: the scene has no sample order (the first call of a shape measures one under sched = 2)");
    return MIRT_ERR_STATE;
  }
  if (info) { info->total_samples = sc->so_total; info->last_launch_samples = sc->so_last; }
  if (order) MIRT_HIP(hipMemcpy(order, sc->so_order, 4 * (size_t)sc->so_total, hipMemcpyDeviceToHost));
  if (keys) MIRT_HIP(hipMemcpy(keys, sc->so_keys, 4 * (size_t)sc->so_last, hipMemcpyDeviceToHost));
  if (sorted_keys) MIRT_HIP(hipMemcpy(sorted_keys, sc->so_keys2, 4 * (size_t)sc->so_last, hipMemcpyDeviceToHost));
  return MIRT_OK;
}

// one instantiation per form of the random-number tables (device_common.h, xw_init), per node format and per specialisation:
// 2 (counting) x 2 (tables) x 8 = 32 kernels, and the LDS-only stack (SPEC_LDS_STACK) for the five of the eight that walk a
// binary tree: 20 more; the form with the ray-start block (SPEC_START_LDS) of the sphere-only one among those: 4 more
using TraceKernel = void (*)(const RenderArgs*, HotArgs);
template <bool C, bool Q, int P>
static TraceKernel trace_kernel_tables(bool t8) { return t8 ? trace_kernel<C, 8, Q, P> : trace_kernel<C, 4, Q, P>; }
template <bool C>
static TraceKernel trace_kernel_spec(bool t8, const CallPlan& pl)
{
  const bool both = pl.nobulb && pl.nopend;
  if (pl.start_lds) return trace_kernel_tables<C, true, SPEC_START_LDS | SPEC_LDS_STACK | SPEC_NOTRI | SPEC_NOBULB | SPEC_NOPEND>(t8);      // (the plan: qn, notri, nobulb, nopend)
  if (pl.lds_only) {
    constexpr int L = SPEC_LDS_STACK;
    if (pl.qn) return both ? trace_kernel_tables<C, true, L | SPEC_NOTRI | SPEC_NOBULB | SPEC_NOPEND>(t8) : trace_kernel_tables<C, true, L | SPEC_NOTRI>(t8);      // (the plan: notri)
    return both ? trace_kernel_tables<C, false, L | SPEC_NOBULB | SPEC_NOPEND>(t8) : pl.nobulb ? trace_kernel_tables<C, false, L | SPEC_NOBULB>(t8) : trace_kernel_tables<C, false, L>(t8);
  }
  if (pl.qn && pl.notri) return both ? trace_kernel_tables<C, true, SPEC_NOTRI | SPEC_NOBULB | SPEC_NOPEND>(t8) : trace_kernel_tables<C, true, SPEC_NOTRI>(t8);
  if (pl.qn) return both ? trace_kernel_tables<C, true, SPEC_NOBULB | SPEC_NOPEND>(t8) : pl.nobulb ? trace_kernel_tables<C, true, SPEC_NOBULB>(t8) : trace_kernel_tables<C, true, 0>(t8);
  return both ? trace_kernel_tables<C, false, SPEC_NOBULB | SPEC_NOPEND>(t8) : pl.nobulb ? trace_kernel_tables<C, false, SPEC_NOBULB>(t8) : trace_kernel_tables<C, false, 0>(t8);
}
static TraceKernel trace_kernel_for(bool count, bool t8, const CallPlan& pl) { return count ? trace_kernel_spec<true>(t8, pl) : trace_kernel_spec<false>(t8, pl); }

// step 7: the trace launch of one slab, pixels [p0, p0 + pn) of the part.  `a` holds the slab's arguments already.
// (the work counter, counters[8], and the count of waves that ran past its end, counters[12], are left at zero by the launch
// itself; counters[9], the overflow events, is only reset by mirt_get_stats)
static int launch_slab(const RenderCall& c, RenderCtx& cx, const CallPlan& pl, RenderArgs& a, const HotArgs& h, int slab, long long p0, long long pn,
                       int blocks, TraceKernel kernel)
{
  const hipStream_t stream = c.stream;
  if (c.sc->opt.wavefront != 0) {
    float tms = 0.0f;
    int rc = wavefront_trace(c.sc, cx, a, c.count(), stream, &tms);
    if (rc != MIRT_OK) return rc;
    cx.wf_trace_ms = (cx.wf_trace_ms < 0.0f ? 0.0f : cx.wf_trace_ms) + tms;
    MIRT_HIP(hipGetLastError());
    return MIRT_OK;
  }
  // this slab's arguments: the kernel reads them from device memory; a ring of copies, so that the copy for slab k + 1
  // does not wait for the kernel of slab k (the stream orders a copy after the kernel that used the same slot)
  // (a frame like the one before it finds its arguments in place: nothing is copied)
  const int slot = slab % MAX_SLAB_ARGS;
  RenderArgs* adev = cx.args_dev + slot;
  if (!cx.args_valid[slot] || memcmp(&cx.args_host[slot], &a, sizeof(RenderArgs)) != 0) {
    MIRT_HIP(hipMemcpyAsync(adev, &a, sizeof(RenderArgs), hipMemcpyHostToDevice, stream));
    cx.args_host[slot] = a; cx.args_valid[slot] = true;
  }
  if (c.sparse()) {
    // this slab's listed pixels -> the hand-out table and, in the device copy of the arguments, the number of samples
    cx.args_valid[slot] = false;      // (the device copy no longer equals the host's)
    int rc = sparse_expand(cx, c.ax->list, c.ax->num_listed, p0, pn, c.sample_count, &adev->num_samples, stream);
    if (rc != MIRT_OK) return rc;
  }
  MIRT_HIP(hipEventRecord(cx.slab_ev[2 * slab], stream));
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(TRACE_BLOCK), 0, stream, adev, h);
  MIRT_HIP(hipGetLastError());
  MIRT_HIP(hipEventRecord(cx.slab_ev[2 * slab + 1], stream));
  return MIRT_OK;
}

// step 8: the slab's samples -> pixels (mirt_render) or sums (mirt_render_accumulate*)
static int resolve_slab(const RenderCall& c, RenderCtx& cx, long long p0, long long pn)
{
  const hipStream_t stream = c.stream;
  if (c.d_accum) {
    const AdaptiveArgs mx = c.ax ? *c.ax : AdaptiveArgs();      // (mirt_render_accumulate: every pixel, the sums only)
    return resolve_moments(cx, cx.samples, mx, (float4*)c.d_accum, p0, pn, mx.num_listed, c.sample_count, stream);
  }
  ResolveArgs ra;
  ra.samples = cx.samples; ra.rgba8 = (unsigned char*)c.d_rgba8; ra.rgba_f32 = (float4*)c.d_rgba_f32;
  ra.num_local_pixels = pn; ra.pixel_base = p0; ra.spp = c.p->spp; ra.count = c.sample_count;
  int P = 1, lg = 0;
  while (P < c.sample_count) { P <<= 1; ++lg; }
  if (c.sample_count > 1 && P <= 64) {
    const long long ppb = TBLOCK >> lg;
    hipLaunchKernelGGL(resolve_tree_kernel, dim3((unsigned)((pn + ppb - 1) / ppb)), dim3(TBLOCK), 0, stream, ra, P, lg);
  } else {
    hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)((pn + RBLOCK - 1) / RBLOCK)), dim3(RBLOCK), 0, stream, ra);
  }
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

static int render_impl(MirtScene* sc, const MirtRenderParams* p, void* d_rgba8, void* d_rgba_f32, void* d_accum, int sample_first,
                       int sample_count, hipStream_t stream, const AdaptiveArgs* ax = nullptr)
{
  const RenderCall c{sc, p, d_rgba8, d_rgba_f32, d_accum, ax, sample_first, sample_count, stream};
  int64_t npix = 0;
  int rc = check_call(c, &npix);
  if (rc != MIRT_OK || npix == 0) return rc;
  const bool count = c.count();
  CallShape shape;
  shape.npix = npix; shape.sample_first = sample_first; shape.sample_count = sample_count; shape.spp = p->spp;
  shape.accumulate = d_accum != nullptr; shape.num_listed = c.sparse() ? ax->num_listed : -1; shape.counters = count;
  SceneFacts facts;
  rc = scene_facts(sc, &facts);
  if (rc != MIRT_OK) return rc;
  const CallPlan pl = plan_call(facts, sc->opt, shape);
  const int blocks = size_grid(sc, pl, count, stream);
  const int chunk_shift = plan_chunk_shift(pl.launch_samples_max, blocks, sc->opt.chunk_shift);
  const size_t nchunks = (size_t)((pl.slab_samples_max + (1ll << chunk_shift) - 1) >> chunk_shift);
  const long long okey = pl.slab_samples_max * 16 + chunk_shift;      // names the shape a measured order belongs to

  RenderCtx* cxp = nullptr;
  rc = take_context(sc, &cxp);
  if (rc != MIRT_OK) return rc;
  RenderCtx& cx = *cxp;
  rc = ensure_workspace(c, cx, pl, blocks);
  if (rc != MIRT_OK) return rc;
  RenderArgs a;
  HotArgs h;
  rc = fill_args(c, cx, pl, chunk_shift, a, h);
  if (rc != MIRT_OK) return rc;

  // the hand-out order: found, or measured by this call for the calls after it
  bool measure_chunks = false, measure_samples = false, ordered_samples = false;
  if (pl.hand_out == HAND_BY_CHUNK) {
    rc = chunk_order_find(sc, cx, nchunks, okey, &a.chunk_order);
    measure_chunks = !a.chunk_order;
    if (measure_chunks) a.chunk_cost = cx.chunk_cost;
  } else if (pl.hand_out == HAND_BY_SAMPLE) {
    rc = sample_table_find(sc, pl, okey, &ordered_samples, &measure_samples);
  }
  if (rc != MIRT_OK) return rc;
  // The call that measures the sample order runs the counting kernels: its node visits and primitive tests are kept as well,
  // in the scene's own counters where the caller asked for none (RenderArgs::counters; zeroed below, copied out after the last slab).
  unsigned long long* ratio_counts = nullptr;
  if (measure_samples && sc->so_counts_host.get()) ratio_counts = count ? cx.counters.get() : sc->so_counters.get();
  if (ratio_counts && !count) a.counters = ratio_counts;
  const TraceKernel kernel = trace_kernel_for(count || measure_chunks || measure_samples,      // (measure: cost stamps need the step counter)
                                              a.needs_rng && a.rng.mode == 0 && a.rng.chunk_bits == 8, pl);

  cx.frame_id = ++sc->frame_seq;
  MIRT_HIP(hipEventRecord(cx.ev0, stream));
  if (measure_chunks) MIRT_HIP(hipMemsetAsync(cx.chunk_cost, 0, 4 * nchunks, stream));
  if (count) { MIRT_HIP(hipMemsetAsync(cx.counters, 0, 8 * sizeof(unsigned long long), stream)); MIRT_HIP(hipMemsetAsync(cx.counters + 11, 0, sizeof(unsigned long long), stream)); }
  else if (ratio_counts) MIRT_HIP(hipMemsetAsync(ratio_counts, 0, 12 * sizeof(unsigned long long), stream));
  cx.wf_trace_ms = -1.0f;
  cx.launches = pl.nslabs;
  cx.node_bytes = pl.node_bytes;
  sc->last_lds_only = pl.lds_only;
  sc->last_stack_slots = pl.start_lds ? START_LDS_SLOTS : STACK_LDS;
  MIRT_HIP(hipEventRecord(cx.ev1, stream));
  for (int slab = 0; slab < pl.nslabs; ++slab) {
    const long long p0 = (long long)slab * pl.slab_pixels;
    const long long pn = (p0 + pl.slab_pixels < npix ? p0 + pl.slab_pixels : npix) - p0;
    a.pixel_base = p0; a.num_local_pixels = pn; a.num_samples = pn * sample_count;
    a.sample_order = ordered_samples ? sc->so_order + (size_t)p0 * sample_count : nullptr;      // (this launch's part of the table)
    a.sample_key = measure_samples ? sc->so_keys : nullptr;
    if (c.sparse()) {
      a.sample_order = cx.sp_table;
      a.num_samples = (pn < pl.listed_max ? pn : pl.listed_max) * sample_count;      // (an upper bound: sparse_expand writes the launch's own number over it)
    }
    rc = launch_slab(c, cx, pl, a, h, slab, p0, pn, blocks, kernel);
    if (rc != MIRT_OK) return rc;
    if (slab == pl.nslabs - 1) MIRT_HIP(hipEventRecord(cx.ev2, stream));
    rc = resolve_slab(c, cx, p0, pn);
    // this launch's part of the cost-ordered sample table, for later calls of this shape (the key buffer is reused by the next slab)
    if (rc == MIRT_OK && measure_samples) {
      rc = sort_low_byte(sc->so_keys, sc->so_keys2, sc->so_order + (size_t)p0 * sample_count, pn * sample_count, sc->so_ws, stream);
      sc->so_last = pn * sample_count;      // (what so_keys / so_keys2 hold from here on: mirt_get_sample_order)
    }
    if (rc != MIRT_OK) return rc;
  }
  if (measure_samples) {
    // (words 3..5 of the counters: internal visits, sphere tests, triangle tests -- flush_counters, shade_common.h)
    if (ratio_counts) MIRT_HIP(hipMemcpyAsync(sc->so_counts_host.get(), ratio_counts + 3, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    sc->so_ratio_stale = !ratio_counts;
    rc = sample_table_finish(sc, stream);
  }
  else if (measure_chunks) rc = chunk_order_finish(cx, nchunks, okey, stream);
  if (rc != MIRT_OK) return rc;
  ++cx.uses;
  ++sc->frame_no;
  MIRT_HIP(hipEventRecord(cx.ev3, stream));
  cx.used = true; cx.counted = count; cx.timed = false; cx.stream = stream; sc->last = &cx;
  return MIRT_OK;
}

// trace-kernel time of the context's last (finished) call: the sum over its launches
int trace_ms_of(RenderCtx& cx, float* ms)
{
  *ms = 0.0f;
  if (cx.wf_trace_ms >= 0.0f) { *ms = cx.wf_trace_ms; return MIRT_OK; }
  for (int k = 0; k < cx.launches && 2 * k + 1 < (int)cx.slab_ev.size(); ++k) {
    float t = 0.0f;
    MIRT_HIP(hipEventElapsedTime(&t, cx.slab_ev[2 * k], cx.slab_ev[2 * k + 1]));
    *ms += t;
  }
  return MIRT_OK;
}

int render(MirtScene* sc, const MirtRenderParams* p, void* d_rgba8, void* d_rgba_f32, hipStream_t stream)
{
  if (p->spp > MAX_SPP) { set_error("mirt_render: more than 4096 samples per pixel in one call (use mirt_render_accumulate + mirt_finalize)"); return MIRT_ERR_ARG; }
  if (!d_rgba8) { set_error("mirt_render: bad parameters"); return MIRT_ERR_ARG; }
  return render_impl(sc, p, d_rgba8, d_rgba_f32, nullptr, 0, p->spp > 1 ? p->spp : 1, stream);
}

// render_kernel_atomic_aa, draw.cu:49-92: adds the samples [sample_first, sample_first + sample_count) of every pixel of the
// part to d_accum (float4 per pixel of the compact part buffer).  The reference adds sample by sample with atomicAdd, i.e. in
// no particular order; here a call adds one value per pixel, the sum of its samples in the xor-butterfly order of draw.cu:181-189.
int render_accumulate(MirtScene* sc, const MirtRenderParams* p, void* d_accum, int sample_first, int sample_count, hipStream_t stream)
{
  if (!d_accum) { set_error("mirt_render_accumulate: bad parameters"); return MIRT_ERR_ARG; }
  return render_impl(sc, p, nullptr, nullptr, d_accum, sample_first, sample_count, stream);
}

// mirt_render_accumulate_pixels: the list is device memory, so its entries are bounded on the device (adaptive.hip, RangePred)
int render_accumulate_pixels(MirtScene* sc, const MirtRenderParams* p, const AdaptiveArgs& ax, void* d_accum, int sample_first, int sample_count, hipStream_t stream)
{
  if (!d_accum || ax.num_listed < 0 || sample_count < 0) { set_error("mirt_render_accumulate_pixels: bad parameters"); return MIRT_ERR_ARG; }
  if (ax.list && ax.num_listed > 0 && ((uintptr_t)ax.list & 3u) != 0) { set_error("mirt_render_accumulate_pixels: the pixel list must be 4-byte aligned"); return MIRT_ERR_ARG; }
  if (!sc->built) { set_error("mirt_render_accumulate_pixels: call mirt_build_lbvh first"); return MIRT_ERR_STATE; }
  if (ax.list && ax.num_listed == 0) return MIRT_OK;
  return render_impl(sc, p, nullptr, nullptr, d_accum, sample_first, sample_count, stream, &ax);
}

int scatter_part(const MirtRenderParams* p, const void* d_part, void* d_frame, hipStream_t stream)
{
  const int64_t n = local_pixels(p);
  if (n < 0 || !d_part || !d_frame) { set_error("mirt_scatter_part: bad parameters"); return MIRT_ERR_ARG; }
  if (n == 0) return MIRT_OK;
  hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)((n + RBLOCK - 1) / RBLOCK)), dim3(RBLOCK), 0, stream, (const uchar4*)d_part,
                     (uchar4*)d_frame, (long long)n, p->width, p->height, p->stripe_rows, p->num_parts, p->part);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

int64_t render_num_pixels(const MirtRenderParams* p) { return local_pixels(p); }

int part_pixel(const MirtRenderParams* p, int64_t local, int32_t* x, int32_t* y)
{
  const int64_t n = local_pixels(p);
  if (n < 0 || local < 0 || local >= n || !x || !y) { set_error("mirt_part_pixel_xy: bad argument"); return MIRT_ERR_ARG; }
  long long xx, yy;
  part_pixel_xy(local, p->width, p->stripe_rows, p->num_parts, p->part, xx, yy);
  *x = (int32_t)xx; *y = (int32_t)yy;
  return MIRT_OK;
}

int probe_math(int device, int which, int n, const float* in, float* out)
{
  MIRT_HIP(hipSetDevice(device));
  DevBuf<float> di, dout;
  MIRT_TRY(di.alloc((size_t)n, "di")); MIRT_TRY(dout.alloc((size_t)n, "dout"));
  MIRT_HIP(hipMemcpy(di, in, 4 * (size_t)n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(probe_math_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, which, n, di, dout);
  MIRT_HIP(hipGetLastError());
  MIRT_HIP(hipMemcpy(out, dout, 4 * (size_t)n, hipMemcpyDeviceToHost));
  return MIRT_OK;
}

int probe_qbox(int device, int n, const float* in, uint32_t* out)
{
  MIRT_HIP(hipSetDevice(device));
  DevBuf<float> di;
  DevBuf<uint32_t> dout;
  MIRT_TRY(di.alloc(20 * (size_t)n, "di")); MIRT_TRY(dout.alloc(20 * (size_t)n, "dout"));
  MIRT_HIP(hipMemcpy(di, in, 4 * 20 * (size_t)n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(probe_qbox_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, di, dout);
  MIRT_HIP(hipGetLastError());
  MIRT_HIP(hipMemcpy(out, dout, 4 * 20 * (size_t)n, hipMemcpyDeviceToHost));
  return MIRT_OK;
}

// which = 0: cost_key of every element.  which = 1: order_kernel over n chunk costs, launched as chunk_order_finish launches it.
int probe_sched(int device, int which, int n, const uint32_t* in, uint32_t* out)
{
  MIRT_HIP(hipSetDevice(device));
  DevBuf<uint32_t> di, dout;
  MIRT_TRY(di.alloc((size_t)n, "di")); MIRT_TRY(dout.alloc((size_t)n, "dout"));
  MIRT_HIP(hipMemcpy(di, in, 4 * (size_t)n, hipMemcpyHostToDevice));
  MIRT_HIP(hipMemset(dout, 0xff, 4 * (size_t)n));      // (a position the kernel leaves out reads as no index)
  if (which == 0) hipLaunchKernelGGL(probe_cost_key_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, di, dout);
  else hipLaunchKernelGGL(order_kernel, dim3(1), dim3(SORT_BINS), 0, 0, di, (uint32_t)n, dout);
  MIRT_HIP(hipGetLastError());
  MIRT_HIP(hipMemcpy(out, dout, 4 * (size_t)n, hipMemcpyDeviceToHost));
  return MIRT_OK;
}

int probe_xorwow(int device, int spp, int nstreams, int draws, uint32_t* out)
{
  MIRT_HIP(hipSetDevice(device));
  RngCache cache;
  RngTablesDev t;
  int rc = ensure_rng_tables(&cache, spp > 1 ? spp : 0, nstreams, nullptr, &t, false);
  if (rc != MIRT_OK) return rc;
  DevBuf<uint32_t> d;
  MIRT_TRY(d.alloc((size_t)nstreams * draws, "draws"));
  hipLaunchKernelGGL(probe_xorwow_kernel, dim3((nstreams + 255) / 256), dim3(256), 0, 0, t, spp, nstreams, draws, d);
  MIRT_HIP(hipGetLastError());
  MIRT_HIP(hipMemcpy(out, d, 4 * (size_t)nstreams * draws, hipMemcpyDeviceToHost));
  return MIRT_OK;
}

} // namespace mirt
