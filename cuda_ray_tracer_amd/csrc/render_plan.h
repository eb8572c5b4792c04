// What one render call decides before it touches the device: a pure function from (scene facts, options, call shape) to a
// CallPlan.  No HIP in here -- this header compiles with a plain host compiler, and tests/plan_probe.cpp runs it against
// the tests' Python mirror of the same decisions (product_flags) without a GPU.  render.hip's render_impl carries the plan
// out step by step.
#ifndef MIRT_RENDER_PLAN_H
#define MIRT_RENDER_PLAN_H

#include <cstdint>

// The trace kernel's waves never talk to each other, so a workgroup is one wave: a finished wave frees its slot (and its
// 10 KB of LDS) at once instead of waiting for the slowest of four, which is what lets the next frame's waves move in
// while this frame drains.
#ifndef MIRT_TRACE_BLOCK
#define MIRT_TRACE_BLOCK 64
#endif
#ifndef MIRT_STACK_LDS
#define MIRT_STACK_LDS 24
#endif

namespace mirt {

constexpr int TRACE_BLOCK = MIRT_TRACE_BLOCK;
constexpr int STACK_LDS = MIRT_STACK_LDS;
// Entries the trace kernel's stack holds without the global spill area: the top entry in a register (Lane::tos) and entries
// 1 .. STACK_LDS - 1 in LDS slots of the same number.  Slot 0 never holds an entry (render.hip, MIRT_PUSH).
constexpr int STACK_LDS_CAPACITY = STACK_LDS;
// The kernel with the ray-start block (render.hip, SPEC_START_LDS).  The LDS-only kernel's walk never holds more than D entries
// (the argument at MIRT_PUSH), so a tree with D < STACK_LDS leaves the last slot of every lane untouched: this kernel moves its
// stack up by one slot and keeps, in the 256 bytes that frees per wave, what the loop header's ray start reads -- one 16-byte
// head (root reference, planes, suns, shadow-ray mode) and up to START_LDS_SUNS sun records of 24 bytes.
constexpr int START_LDS_SLOTS = STACK_LDS - 1;
constexpr int START_LDS_SUNS = 10;
static_assert(16 + START_LDS_SUNS * 24 <= TRACE_BLOCK * 4, "head and suns fit the bytes of one stack slot");
constexpr int MAX_CHUNK_SHIFT = 8, MIN_CHUNK_SHIFT = 6;   // a wave takes 64..256 consecutive samples from the frame per atomic
// node record word 14 (after the two child references): which descent orders the node allows
constexpr uint32_t NODE_SWAP_PURE = 1u;       // both subtrees hold spheres only: near-child-first cannot change the closest hit
constexpr uint32_t NODE_SWAP_ANY = 2u;        // always set (the mask of MIRT_TRAVERSAL_ORDERED_ALL)

// Mode switches and tuning values of a scene.  The defaults are the measured optima.  MIRT_<NAME> environment variables
// override them ONCE, when the scene is created (tools/ sweeps); mirt_scene_set_option changes them afterwards.  Nothing
// reads the environment during a render.
struct Options {
  int bounds_as_shipped = 0;   // build: 1 = scene bounds never stored, every Morton code 0 -- the tree of the shipped reference (parse.cpp:28)
  int traversal = 1;           // MIRT_TRAVERSAL_*: 0 reference (left first), 1 ordered where pixels cannot change, 2 ordered everywhere
  int wavefront = 0;           // 1: the trace / shade kernel pair instead of the single kernel
  int stack_lds_depth = -1;    // traversal-stack entries kept in LDS (-1: the compiled size); tests force the spill path with it
  int refill_k = 0;            // leave the traversal loop when this many lanes wait to shade; 0 = by kind of kernel (plan_call)
  int batch_k = 0;             // lanes whose batch ray finished start their next one once this many wait; 0 = by kind of kernel and scene (plan_call: 8)
  int drain_lanes = 16;
  int leaf_k = 0;              // primitive tests are held back until this many lanes have one pending; 0 = by kind of kernel (8; exact records 4)
  int reps = 0;                // traversal steps per pass through the loop header; 0 = by kind of kernel and scene (plan_call: 4; wide records 5)
  int init_k = 0;              // lanes without a sample are refilled once this many wait (1: at every shade phase); 0 = by kind of kernel (plan_call)
  int chunk_shift = 0;         // 0: by frame size
  int trace_waves = 0;         // 0: fill the device
  int shadow_anyhit = 1;       // 0: shadow rays are nearest-hit queries, as in diffuseLight (draw.cu:347-352, 365-370): the reference's walk, more node visits
  int skip_unlit = 1;          // 0: shadow rays towards lights the shading normal faces away from are traced as well (draw.cu:342-374 traces them all)
  int qnodes = 1;              // quantised node records in the single-kernel path: 0 never; 1 sphere-only scenes (traversal >= 1) and scenes with
                               // triangles of 65536 primitives or more (wide records, traversal = 1); 2 every scene
  int ray_start_lds = 1;       // 1: the sphere-only LDS-only kernel whose loop header starts rays from values kept in LDS, where the plan allows (plan_call)
  int specialise = 1;          // kernels compiled without what the scene does not have: point lights; transparency and gi (SPEC_*, shade_common.h)
  int sched = 2;               // longest-first hand-out measured on the first call of a shape: 2 by sample (stable within a cost class), 1 by chunk (one-slab calls), 0 off
  int slab_log2 = 28;          // a call is rendered in slabs of at most 2^slab_log2 samples (4 GiB of per-sample workspace; 2^26: +1.8 % on config 5)
  int wf_pool = 1 << 21, wf_refill_k = 16;
};

// the facts of a built scene that the decisions read
struct SceneFacts {
  int N = 0, Nt = 0;                       // primitives, triangles among them
  bool grid_ok = false;                    // the grid of the quantised records resolves the scene's coordinates (lbvh_build.hip)
  bool has_quantised = false, has_wide = false;   // the build made 32-byte quantised / 64-byte wide records
  bool colors_finite = true, any_trans = false, any_rough = false;
  int gi = 0, bounces = 0;
  int num_suns = 0, num_bulbs = 0;
  int tree_depth = -1;                     // D: the most internal nodes on a root-to-leaf path of the built tree (lbvh_build.hip); -1: not known
  // r: primitive tests per internal-node visit of the scene's rays, (sphere tests + triangle tests) / internal visits, as the
  // measuring call of the sample order counted them (render.hip, sample_table_find); negative: not known (yet)
  float prim_ratio = -1.0f;
};

// Pass length and batch threshold of the sphere-only quantised kernels by r (plan_call).  Primitives are tested in the first
// step of a pass only, so a lane that reached one waits out the pass: rays that test many primitives per node visit want short
// passes, rays that walk long chains of nodes between two primitives want the loop header amortised over more steps.  A monotone
// step function: the first row with r < below.  Two columns: the kernel that starts rays from LDS (start_lds: tenthousand.txt,
// spiral.txt) and the other sphere-only quantised kernels (deeper trees; measured on synthetic scenes of 1 M and 8 M spheres).
// Measured, 1920 x 1080 (profiles/r09_ab_runs.txt): r = 0.0013 nothing moves; 0.010 best at 6 / 8; 0.046 and
// 0.067 (deep trees) at 5 / 8; 0.065 (tenthousand.txt) at 6 / 12; 0.28 (spiral.txt) at 3 / 8.  Nothing was measured between 0.067
// and 0.28: from 0.1, half again above the largest r that wants long passes, to 0.2, the same margin below spiral.txt's, the
// values stay the ones from before the rule, as they do above 0.2 for the kernels spiral.txt does not run.
// What rests on no run: the 0.1 and 0.2 bounds themselves (placed by margin; no syntheticScene(n, 0) has r between 0.067 and
// 0.28), 5 / 8 below 0.03 in the deep-tree column (its two scenes have r = 0.046 and 0.067; taken over from the row above it), and
// every kernel but the first column's above 0.067.  A scene measured there moves the bound or the row, nothing else.
struct PassStep { float below; int reps, batch_k, reps_other, batch_k_other; };
constexpr int PASS_REPS_DEFAULT = 4, PASS_BATCH_K_DEFAULT = 8;
constexpr PassStep PASS_STEPS[] = {{0.03f, 6, 8, 5, 8}, {0.1f, 6, 12, 5, 8}, {0.2f, PASS_REPS_DEFAULT, PASS_BATCH_K_DEFAULT, PASS_REPS_DEFAULT, PASS_BATCH_K_DEFAULT},
                                   {3.0e38f, 3, 8, PASS_REPS_DEFAULT, PASS_BATCH_K_DEFAULT}};

struct CallShape {
  long long npix = 0;                      // pixels of the part (> 0)
  int sample_first = 0, sample_count = 1;  // each pixel's samples [sample_first, sample_first + sample_count)
  int spp = 0;                             // MirtRenderParams::spp
  bool accumulate = false;                 // sums are added to an accumulation buffer (else pixels are written)
  long long num_listed = -1;               // length of the pixel list; < 0: no list, every pixel
  bool counters = false;                   // MIRT_RENDER_COUNTERS
};

// who decides the order in which a launch's samples are handed to the waves
enum HandOut {
  HAND_FRAME = 0,     // frame order
  HAND_LIST,          // the listed pixels' samples, in list order (adaptive.hip)
  HAND_BY_CHUNK,      // sched = 1: chunks, longest first, per context
  HAND_BY_SAMPLE,     // sched = 2: samples by decreasing cost class, one table per scene
};

struct CallPlan {
  // slabs: whole pixels, at most 2^slab_log2 samples each
  long long slab_pixels = 0; int nslabs = 0;
  long long slab_samples_max = 0;          // per-sample workspace of a launch
  long long listed_max = 0;                // a sparse launch hands out at most this many pixels: the listed pixels of one slab
  long long launch_samples_max = 0;        // ... and any launch at most this many samples
  long long total_samples = 0;
  bool per_pixel_seed = false;             // curand_init(1234 + pixel, sample, 0) (draw.cu:74,162) vs curand_init(1234, pixel, 0) (draw.cu:105)
  int args_spp = 0;                        // RenderArgs::spp
  int rng_sample_tables = 0;               // ensure_rng_tables: tables of this many sample indices, 0 = the per-pixel tables
  bool shading_rng = false;                // rough normals or GI draw random numbers whatever the camera does
  // node records and walk order
  bool notri = false, qn = false;          // sphere-only scene; a quantised walk (notri: the 32-byte records, else the wide ones)
  uint32_t swap_mask = 0;
  int reach_check = 0;
  int node_bytes = 64;
  // specialisation, shading switches
  bool nobulb = false, nopend = false;
  bool need_pending = false; int pending_slots = 0;
  int skip_unlit = 0, shadow_anyhit = 0;
  // thresholds by kind of kernel
  int refill_k = 0, init_k = 0, leaf_k = 0, reps = 0, batch_k = 0, lds_depth = 0;
  bool lds_only = false;                   // the trace kernel compiled without the spill arm of push and pop (SPEC_LDS_STACK)
  bool start_lds = false;                  // ... and with the loop header's ray-start values in LDS, the stack one slot shorter (SPEC_START_LDS)
  HandOut hand_out = HAND_FRAME;
};

inline CallPlan plan_call(const SceneFacts& s, const Options& opt, const CallShape& c)
{
  CallPlan pl;
  const bool sparse = c.num_listed >= 0;
  const bool wavefront = opt.wavefront != 0;
  pl.slab_pixels = (1ll << opt.slab_log2) / c.sample_count;
  if (pl.slab_pixels < 1) pl.slab_pixels = 1;
  if (pl.slab_pixels > c.npix) pl.slab_pixels = c.npix;
  pl.nslabs = (int)((c.npix + pl.slab_pixels - 1) / pl.slab_pixels);
  pl.slab_samples_max = pl.slab_pixels * c.sample_count;
  pl.listed_max = sparse ? (c.num_listed < pl.slab_pixels ? c.num_listed : pl.slab_pixels) : 0;
  pl.launch_samples_max = sparse ? pl.listed_max * c.sample_count : pl.slab_samples_max;
  pl.total_samples = c.npix * c.sample_count;
  pl.per_pixel_seed = c.accumulate || c.spp > 1;
  pl.args_spp = c.accumulate ? (c.spp > 1 ? c.spp : 2) : c.spp;      // only "is it >= 1" matters to the kernel: jittered samples (draw.cu:78-84,110-118,165-171)
  pl.rng_sample_tables = pl.per_pixel_seed ? c.sample_first + c.sample_count : 0;
  pl.shading_rng = s.any_rough || s.gi != 0;

  // Quantised node records: single-kernel path, any order but the reference's own.  A sphere-only scene: the 32-byte records,
  // always.  A scene with triangles: the wide records -- the reference's order at every node, so traversal = 1 only -- when the
  // scene is large enough for memory to matter (qnodes = 1: N >= 65536, the exact records no longer fit an L2; redchair.txt's
  // 1.7 k primitives are 12 % faster on the exact records, the 2 M-primitive scene 25 % faster on the wide ones) or always (2).
  pl.notri = s.Nt == 0;
  const bool qwant = opt.qnodes != 0 && !wavefront;
  // (and only if the grid of the quantised records resolves the scene's coordinates: grid_ok, lbvh_build.hip -- a scene that
  // sits hundreds of its own extents away from the world origin walks the exact records, in the reference's order)
  pl.qn = s.grid_ok && (pl.notri ? (qwant && opt.traversal >= 1 && s.has_quantised)
                                 : (qwant && opt.traversal == 1 && s.has_wide && (opt.qnodes >= 2 || s.N >= 65536)));
  // traversal = 1: near child first on the quantised records of a sphere-only scene, nowhere else.  Over the exact boxes the
  // reordered walk can cull a box over a sphere whose hit distance rounds below that box's entry distance (one ulp is enough; the
  // reference, in its order, gets there first): 13 of 4 000 far-camera fuzz scenes differed by a pixel or a ray.  The quantised
  // boxes are rounded outwards by more than that rounding as long as the grid resolves it (grid_ok, a condition of qn) -- no differing byte
  // in 10 000 sphere scenes, 3 000 of them far-camera ones.  Everything else walks in the reference's order.
  pl.swap_mask = opt.traversal == 1 ? ((pl.qn && pl.notri) ? NODE_SWAP_PURE : 0u) : (opt.traversal == 2 ? NODE_SWAP_ANY : 0u);
  // (the quantised walks; the exact records are walked in the reference's own order, or -- traversal = 2 -- in one that promises nothing)
  pl.reach_check = (pl.qn && s.N > 1) ? 1 : 0;
  pl.node_bytes = (pl.qn && pl.notri) ? 32 : 64;

  pl.need_pending = s.any_trans || s.gi != 0;
  pl.pending_slots = pl.need_pending ? 2 * (s.bounces + (s.gi > 0 ? s.gi : 0) + 2) : 0;
  // kernels specialised for what the scene does not have (SPEC_*, shade_common.h)
  // (a scene with a non-finite colour gets the general kernels: only they carry the colour * 0 terms, gi_zero_term)
  const bool specialise = opt.specialise != 0 && s.colors_finite;
  pl.nobulb = specialise && s.num_bulbs == 0;
  pl.nopend = specialise && !pl.need_pending;
  pl.skip_unlit = (opt.skip_unlit != 0 && s.colors_finite && s.num_suns + s.num_bulbs <= 32) ? 1 : 0;
  pl.shadow_anyhit = opt.shadow_anyhit != 0 ? 1 : 0;

  pl.lds_depth = (opt.stack_lds_depth >= 0 && opt.stack_lds_depth <= STACK_LDS) ? opt.stack_lds_depth : STACK_LDS;   // tests force the spill path
  // The kernel without a spill arm: a binary walk (the sphere-only quantised records or the exact ones; the wide walk pushes up
  // to three entries a step) keeps at most one pending sibling per internal node above the current one, so never more than D
  // entries (render.hip, next to MIRT_PUSH).  Only with the option at its default: any explicit value, the compiled size
  // included, keeps the general kernel -- that is how the tests force the spill path and how the two kernels are compared.
  pl.lds_only = !wavefront && opt.stack_lds_depth < 0 && (!pl.qn || pl.notri) && s.tree_depth >= 0 && s.tree_depth <= STACK_LDS_CAPACITY;
  // The kernel with the ray-start block: the sphere-only quantised kernel without point lights, transparency or gi (the only
  // LDS-only kernel compiled in that form), a tree that leaves one stack slot free, no more suns than the block has room for.
  pl.start_lds = pl.lds_only && opt.ray_start_lds != 0 && pl.qn && pl.notri && pl.nobulb && pl.nopend && s.tree_depth <= START_LDS_SLOTS &&
                 s.num_suns <= START_LDS_SUNS;
  // Thresholds of the two expensive divergent pieces of work, measured per kind of kernel (round 3, tools/r03_i.sh, r03_x.sh): lanes
  // wait to shade until refill_k of them do, lanes without a sample until init_k of them do.  Sphere-only scenes 32 / 10; wide
  // records (2 M-primitive scene) 24 / 8; exact records (redchair.txt) 64 / 64 -- with the samples handed out by cost class
  // (sched = 2) the lanes of a wave run samples of one kind, and redchair.txt's short ray trees are fastest in lock step: the whole
  // wave traverses, the whole wave shades, the whole wave takes 64 new samples (1080p16: 20.6 ms at 52 / 48, 18.1 at 64 / 64;
  // tenthousand.txt's deep reflection chains want the opposite: 28.0 ms at 64 / 64 against 21.7).  Refilling finished lanes at
  // every shade phase (init_k = 1, rounds 1-2) cost redchair.txt 14 % of its frame, the sphere scenes 1.5 %.
  pl.refill_k = opt.refill_k > 0 ? opt.refill_k : (pl.qn ? (pl.notri ? 32 : 24) : 64);
  const int init_k = opt.init_k > 0 ? opt.init_k : (pl.qn ? (pl.notri ? 10 : 8) : 64);
  pl.init_k = init_k < pl.refill_k ? init_k : pl.refill_k;      // (<= refill_k: lanes waiting for a sample count as waiting in the loop header)
  pl.leaf_k = opt.leaf_k > 0 ? opt.leaf_k : (pl.qn ? 8 : 4);      // (exact records, redchair.txt: 4 is 1.3 % better than 8)
  // Pass length and batch threshold.  By kind of kernel: 4 steps a pass (wide records: 5 is 1 % better on the 2 M-primitive
  // scene, worse elsewhere), a batch transition once 8 lanes wait for one.  The sphere-only quantised kernels, once the scene's
  // rays have been counted (prim_ratio >= 0): by PASS_STEPS.  An explicit option wins, each on its own.
  int reps = (pl.qn && !pl.notri) ? 5 : PASS_REPS_DEFAULT, batch_k = PASS_BATCH_K_DEFAULT;
  if (pl.qn && pl.notri && s.prim_ratio >= 0.0f) {
    for (const PassStep& st : PASS_STEPS)
      if (s.prim_ratio < st.below) { reps = pl.start_lds ? st.reps : st.reps_other; batch_k = pl.start_lds ? st.batch_k : st.batch_k_other; break; }
  }
  pl.reps = opt.reps > 0 ? opt.reps : reps;
  pl.batch_k = opt.batch_k > 0 ? opt.batch_k : batch_k;

  // A sparse call is handed out in list order: it neither measures an order nor uses one, and leaves the chunk orders and the
  // scene's by-sample table -- which belong to the dense shape rendered last -- as they are.
  // sched = 1 (by chunk): one-slab calls only.
  // sched = 2 (default, by sample): any call whose launches fit a 32-bit sample index and whose table (4 B per sample of the
  // call) stays within 12 GiB; beyond that the call is rendered in frame order.
  if (sparse) pl.hand_out = HAND_LIST;
  else if (wavefront) pl.hand_out = HAND_FRAME;
  else if (opt.sched == 1 && pl.nslabs == 1) pl.hand_out = HAND_BY_CHUNK;
  else if (opt.sched == 2 && pl.slab_samples_max < 0x7fffffffll && pl.total_samples <= (3ll << 30)) pl.hand_out = HAND_BY_SAMPLE;
  return pl;
}

// Chunk size of the work counter: 256 samples, smaller for a small (part of a) frame so that every wave still gets a dozen
// chunks or more -- with four chunks per wave (1/8 of a 1080p frame) the waves finished up to a chunk apart.  `blocks` is
// the launch's grid, which depends on the device and on the frames in flight.
inline int plan_chunk_shift(long long launch_samples_max, int blocks, int option)
{
  int chunk_shift = MAX_CHUNK_SHIFT;
  while (chunk_shift > MIN_CHUNK_SHIFT && (launch_samples_max >> chunk_shift) < 16ll * blocks * (TRACE_BLOCK / 64)) --chunk_shift;
  return option >= 4 ? option : chunk_shift;
}

} // namespace mirt
#endif
