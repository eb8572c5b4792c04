// Device-resident scene (the reference's RawConfig, config.hpp:75-126) and kernel argument structs.
#ifndef MIRT_SCENE_DEV_H
#define MIRT_SCENE_DEV_H

#include <hip/hip_runtime.h>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mirt.h"
#include "build_plan.h"
#include "dev_mem.h"
#include "device_common.h"
#include "query_launch.h"
#include "render_plan.h"
#include "xorwow_tables.h"

namespace mirt {

// child reference inside a packed node / the root reference (REF_*, build_plan.h): names a record of the heap [nodes | primitives]
//   bit 31 = leaf (a primitive record); bit 30 = primitive type (0 sphere, 1 triangle);
//   bits 0..27 = the record's offset in the heap in 16-byte units (node i: 4 i; the primitive of sorted leaf j:
//   prim_base/16 + j + 2 * (triangles among leaves [0, j))), so that the traversal step gets a record's byte offset with
//   one shift.  Primitive records are stored in sorted (Morton) order: the offset of a leaf grows with its sorted index,
//   which is what breaks exact ties in the hit distance the way the reference's left-first walk does.
// Quantised node records (option "qnodes"): 32 bytes instead of 64, i.e. two 16-byte requests per node visit instead of four
// and half the bytes -- the address units bound the trace kernel on the bundled scenes, memory on the 2 M-primitive one.  Both
// child boxes as 12 x uint16 on the scene-bounds grid (65535 steps per axis, rounded outwards by one more step), then the two
// child references.  The boxes are supersets of the exact ones, so the walk visits a superset of the reference's nodes in the
// same order.  For spheres the closest hit cannot change (shade_common.h, sphere_leaf_box_admits restores the one clause of the
// reference's box test that a larger box weakens).  A triangle hit is accepted only if the reference's walk provably reaches
// that leaf (triangle_leaf_reached, render.hip); otherwise the ray is walked again over the 64-byte exact records.
//   words 0..2 child 0: (xmin | xmax << 16), (ymin | ymax << 16), (zmin | zmax << 16); words 3..5 child 1; 6, 7: references
//   (bit 29 of word 6, REF_QPURE: both subtrees of this node hold spheres only -- NODE_SWAP_PURE of the 64-byte record)
// Node i sits at heap offset qnode_base + 32 i: its reference is qnode_base / 16 + 2 i.
constexpr float QGRID = 65535.0f;
// a box plane on the scene-bounds grid, rounded outwards (the builder's pack kernels, lbvh_build.hip; mirt_probe_qbox, render.hip)
MIRT_DEV uint32_t qlo(float x, float smin, float step) { const float q = floorf((x - smin) / step) - 1.0f; return (uint32_t)fminf(fmaxf(q, 0.0f), QGRID); }
MIRT_DEV uint32_t qhi(float x, float smin, float step) { const float q = ceilf((x - smin) / step) + 1.0f; return (uint32_t)fminf(fmaxf(q, 0.0f), QGRID); }
constexpr uint32_t REF_QPURE = 0x20000000u;
// Wide quantised records (scenes with triangles, option "wide"): one 64-byte record per internal node P holding the boxes of P's
// GRANDchildren (a child of P that is a leaf stands for itself) in the reference's visiting order -- up to four boxes of
// 3 words each (words 0..11; an absent slot holds an inverted box, which no ray hits) -- and their four references (words
// 12..15).  A step tests four boxes and descends two levels: half as many dependent memory round trips per ray.  The walk
// visits a superset of the reference's leaves in the reference's order (render.hip), which is all that exactness needs.
// Node i sits at heap offset wnode_base + 64 i.
constexpr uint32_t QBOX_NONE = 0x0000ffffu;   // lo = 65535, hi = 0
constexpr int STACK_TOTAL_WIDE = 88;          // up to three pushes per two levels of a tree at most 58 levels deep
constexpr float QINV_STEPS = 1152921504606846976.0f;   // 2^60: |1 / d| is clamped to this many grid steps per unit of t (quantised_axis)
// (NODE_SWAP_*, the descent orders a node record allows: render_plan.h)

struct PlaneDev { float nx, ny, nz, px, py, pz; float mat[11]; float pad; };   // 72 B
// suns: direction; bulbs: position.  n* = normalize(direction) and i* = 1 / n* for suns, computed on the host with the same
// IEEE operations the kernels would use (vec3::normalize, bvh_traversal.cu:106), so shadow rays to suns need no sqrt/div.
struct LightDev { float x, y, z, r, g, b; float nx, ny, nz, ix, iy, iz; };

// Arguments of the trace kernel (passed by value in the kernarg segment: uniform, scalar loads)
struct RenderArgs {
  // frame / camera (RawConfig scalars)
  int width, height, bounces, spp, gi;
  int fisheye, panorama;
  float dof_focus, dof_lens, expose;
  f3 forward, right, up, eye;
  // partition (MirtRenderParams)
  int stripe_rows, num_parts, part;
  long long num_local_pixels;     // pixels of this launch (a slab of the call's part)
  long long num_samples;          // num_local_pixels * samples per pixel of this launch
  long long pixel_base;           // first local pixel of this launch within the call's compact part buffer
  int sample_first;               // index of a pixel's first sample in this launch (0 for mirt_render; mirt_render_accumulate: any)
  int sample_count;               // samples per pixel in this launch (max(spp, 1) for mirt_render)
  int seed_per_pixel;             // 1: curand_init(1234 + pixel, sample, 0) (draw.cu:74,162); 0: curand_init(1234, pixel, 0) (draw.cu:105)
  // geometry
  const float4* nodes;            // record heap: 4 x float4 per internal node, then the primitive records in sorted order:
                                  // sphere (cx,cy,cz,r); triangle 3 x float4: p0.xyz nor.x | nor.yz e1.xy | e1.z e2.xyz
  const uint32_t* unit_prim;      // per 16-byte unit of the primitive region: type << 31 | index in the scene's sphere / triangle array
  const float4* mats;             // 3 x float4 per primitive: spheres first, then triangles
  uint32_t root_ref;
  uint32_t prim_base16;           // offset of the primitive region in the heap, in 16-byte units
  uint32_t swap_mask;             // NODE_SWAP_* bits that allow near-child-first descent (0: the reference's left-first order)
  int reach_check;                // the walk is not the reference's own (order or boxes): sphere hits are vetted before they are shaded (hit_needs_literal_walk)
  float reach_slack;              // 2^-21 x the largest coordinate magnitude of the scene box
  int skip_unlit;                 // 1: shadow rays towards lights the shading normal faces away from are not traced (all colours finite)
  int shadow_anyhit;              // 1: a shadow ray ends at its first occluder; 0: nearest-hit query like every other ray (draw.cu:347-352)
  const float* qparams;           // quantised nodes in use: grid origin xyz, grid step xyz, 2^60 / grid step xyz (else null)
  const float4* tri_boxes;        // 2 x float4 per triangle (scene order): its exact leaf box (xmin, xmax, ymin, ymax) (zmin, zmax, -, -)
  int num_spheres;
  int num_prims;
  const PlaneDev* planes; int num_planes;
  int nonfinite_colours;          // 1: some colour of the scene (or its exposure) is inf or NaN: terms that are colour * 0 are not dropped (advance_core, gi_zero_term; general kernels only)
  const LightDev* suns; int num_suns;
  const LightDev* bulbs; int num_bulbs;
  // rng
  RngTablesDev rng;
  int needs_rng;
  // outputs / workspace
  float4* samples;                // one RGBA per sample
  uint32_t* stack_spill;          // [STACK_TOTAL - STACK_LDS][grid threads]
  float* pending;                 // [pending_slots][16 words][grid threads] or null
  int pending_slots;
  int refill_k;                   // leave the traversal loop when this many lanes wait to shade
  int lds_depth;                  // traversal-stack entries kept in LDS (<= the compiled STACK_LDS); deeper ones spill
  int drain_lanes;                // a wave with at most this many live lanes and nothing left to fetch stops batching
  int batch_k;                    // start the next rays of ray batches when this many lanes wait for one
  int init_k;                     // start new samples when this many lanes wait for one (or the wave has nothing else to do)
  unsigned long long* counters;   // MirtStats head (8 x u64) or null
  unsigned long long* overflow;   // never null: capacity overflows (traversal stack beyond 64, pending list), must stay 0
  unsigned long long* work_counter; // next unclaimed chunk of the frame (single-kernel path)
  const uint32_t* chunk_order;      // chunk k of the hand-out order is chunk chunk_order[k] of the frame (null: identity)
  int chunk_shift;                  // log2 of the number of consecutive samples a wave takes from the frame per atomic
  uint32_t* chunk_cost;             // per chunk: the largest number of traversal steps one of its samples took
  const uint32_t* sample_order;     // sched = 2: position k of the hand-out is sample sample_order[k] of the launch (null: identity)
  uint32_t* sample_key;             // sched = 2, measuring frame: per sample 255 - its cost class (sorted ascending: expensive first)
};

// What the traversal loop of the single-kernel path touches, passed by value (scalar registers).  Everything else is read
// through a pointer to the RenderArgs in device memory, and only inside the shade phase, so that it does not occupy
// scalar registers across the hot loop.
struct HotArgs {
  const float4* nodes;            // start of the record heap
  uint32_t root_ref;
  uint32_t swap_mask;
  const float* qparams;
  const PlaneDev* planes; int num_planes;
  const LightDev* suns; int num_suns;
  const LightDev* bulbs; int num_bulbs;
  int shadow_anyhit;
  uint32_t* stack_spill;
  int lds_depth, refill_k, batch_k, drain_lanes;
  int reps;                       // traversal steps per pass through the loop header
  int leaf_k;                     // primitive tests are held back until this many lanes of the wave have one pending
  int reach_check;                // RenderArgs::reach_check
};

struct ResolveArgs {
  const float4* samples;          // this launch's samples: [num_local_pixels][count]
  unsigned char* rgba8;           // the call's part buffer
  float4* rgba_f32;               // nullable
  long long num_local_pixels;     // pixels of this launch
  long long pixel_base;           // where they start in rgba8 / rgba_f32
  int spp;                        // the call's spp (quantiser choice: draw.cu:129-132 for spp <= 1, :9-11,202-205 otherwise)
  int count;                      // samples per pixel in `samples`
};

// device copies of the skip-ahead tables, keyed by spp (spp > 1) or by -(frame pixels) (spp <= 1)
struct RngCache {
  RngTables host;
  long long key = -1;
  DevBuf<uint4> A; DevBuf<uint32_t> B, K, R2;
};

// (Options, the mode switches and tuning values of a scene: render_plan.h)

constexpr int MIRT_MAX_FRAMES = 4;
// everything one frame in flight owns
struct RenderCtx {
  DevBuf<float4> samples;
  DevBuf<uint32_t> stack_spill;
  DevBuf<float> pending;
  DevBuf<unsigned long long> counters;     // device: [0..7] MirtStats counters, [8] work counter, [9] overflow events, [10] scratch (mirt_get_stats), [11] rays traversed, [12] waves past the end of the work
  hipStream_t stream = nullptr;            // the stream this context's latest frame was issued on
  DevBuf<RenderArgs> args_dev;             // this frame's RenderArgs in device memory (a ring of slots, one per slab in flight)
  RenderArgs args_host[4];                 // what each slot holds
  bool args_valid[4] = {false, false, false, false};
  Event ev0, ev1, ev2, ev3;                // render start / first trace start / last trace end / render end
  std::vector<Event> slab_ev;              // start / end of every trace launch of the last call beyond the first (ev1 / ev2 serve a one-slab call)
  int launches = 0;                        // trace launches of the last call
  int node_bytes = 64;                     // record size of the walk the last call used
  bool used = false, counted = false, timed = true;
  // longest-first scheduling: this frame's per-chunk cost, and the hand-out orders computed from it (two buffers used in
  // turn, so that a frame still reading an order never sees it rewritten)
  DevBuf<uint32_t> chunk_cost;
  // chunk orders this context produced, used round-robin.  Three of them: the one written at use u is next written at use
  // u + 3, i.e. 12 frames later, and by then the host has waited (on context reuse) for every frame that could read it --
  // so no frame ever needs a device-side wait on another frame's stream.
  static constexpr unsigned ORDER_BUFS = 3;
  DevBuf<uint32_t> order_out[ORDER_BUFS];
  unsigned uses = 0;
  unsigned long long frame_id = 0;         // sequence number of the frame that last used this context
  long long order_key = -1;                // frame size (and chunk size) the order in order_out[(order_writes - 1) % ORDER_BUFS] was measured on
  unsigned order_writes = 0;               // orders this context has produced
  unsigned long long order_frame = 0;      // frame_id of the frame that measured it
  Event order_ev;                          // ... and the end of its sort
  float wf_trace_ms = -1.0f;               // >= 0: the wavefront path ran; summed trace-kernel time
  // mirt_render_accumulate_pixels with a pixel list (adaptive.hip): the listed pixels of the current slab in list order, the
  // position -> launch-sample table made from them (RenderArgs::sample_order of that launch), and the per-block counts of the
  // compaction, whose last word is the number of pixels kept
  DevBuf<uint32_t> sp_list, sp_table, sp_blocks;
};

// What mirt_render_accumulate_pixels adds to mirt_render_accumulate (which renders with an empty one): the pixels to render
// (null: every pixel of the part) and the two optional outputs.
struct AdaptiveArgs {
  const uint32_t* list = nullptr;          // device: num_listed distinct local pixels of the part, any order
  long long num_listed = 0;
  float4* accum_sq = nullptr;              // nullable: per-pixel sums of the squared samples
  uint32_t* counts = nullptr;              // nullable: per-pixel sample counts
};

} // namespace mirt

struct MirtScene {
  int device = 0;
  MirtSceneDesc d{};
  int N = 0, Ns = 0, Nt = 0;
  mirt::Options opt;
  int grid_blocks = 0, wf_trace_blocks = 0;   // persistent-grid sizes for this scene's device (filled on first use)
  // uploaded geometry, file order (inputs of the build)
  mirt::DevBuf<float4> spheres;         // (cx, cy, cz, r)
  mirt::DevBuf<float4> tris;            // 3 x float4 per triangle: p0.xyz nor.x | nor.yz e1.xy | e1.z e2.xyz
  mirt::DevBuf<float4> mats;
  mirt::DevBuf<MirtPrimRef> refs_in;    // file order
  mirt::DevBuf<float4> tri_verts;       // 3 x float4 per triangle (p0,p1,p2) -- build only
  mirt::DevBuf<mirt::PlaneDev> planes;
  mirt::DevBuf<mirt::LightDev> suns;
  mirt::DevBuf<mirt::LightDev> bulbs;
  // build products
  mirt::DevBuf<uint32_t> codes;         // sorted Morton codes [N]
  mirt::DevBuf<uint32_t> order;         // sorted position -> file-order index [N]
  mirt::DevBuf<uint32_t> child_l;       // reference numbering [N-1]
  mirt::DevBuf<uint32_t> child_r;
  mirt::DevBuf<int> parent;             // [2N-1]
  mirt::DevBuf<float> boxes;            // [2N-1][6] xmin,xmax,ymin,ymax,zmin,zmax
  float4* nodes = nullptr;              // packed [N-1][4]; start of the record heap [nodes | primitive records, sorted order | pad] (not owning: points into heap)
  mirt::DevBuf<unsigned char> heap;
  uint32_t prim_base = 0;               // byte offset of the primitive region in the heap
  mirt::DevBuf<uint32_t> unit_prim;     // [Ns + 3 Nt]: per 16-byte unit of the primitive region, type << 31 | index (first unit of a record)
  mirt::DevBuf<uint32_t> tris_before;   // [N + 1]: triangles among sorted leaves [0, j)
  mirt::DevBuf<uint2> range;            // [N - 1]: sorted-leaf range (first, last) of every internal node
  uint32_t qnode_base = 0;              // byte offset of the quantised node records in the heap (0: none built)
  uint32_t wnode_base = 0;              // byte offset of the wide quantised records (scenes with triangles; 0: none built)
  uint32_t root_ref_w = mirt::REF_NONE; // root reference into the wide records
  uint32_t root_ref_q = mirt::REF_NONE; // root reference into the quantised records
  mirt::DevBuf<float> qparams;          // [9] device: grid origin, grid step, 2^60 / grid step
  mirt::DevBuf<float4> tri_boxes;       // [2 Nt]: exact leaf box of every triangle (scene order), for the quantised walk's triangle check
  mirt::DevBuf<uint32_t> build_ws;      // LBVH build workspace (sort buffers, histograms, arrival counters)
  mirt::DevBuf<uint32_t> bounds_keys;   // [6] ordered-uint min xyz, max xyz
  mirt::DevBuf<uint32_t> depth_dev;     // [1] the build's max reduction behind tree_depth
  uint32_t root_ref = mirt::REF_NONE;
  bool built = false;
  float build_ms = 0.0f;
  float coord_max = 0.0f;               // largest |coordinate| of the scene box (set by the build)
  bool grid_ok = false;                 // the grid of the quantised records resolves the scene's coordinates (set by the build): they may be walked
  int tree_depth = -1;                  // D: the most internal nodes on a root-to-leaf path (set by the build; -1: not built).  Bounds the binary walk's stack
  int last_stack_slots = 0;             // ... LDS slots of that kernel's traversal stack, "stack_lds_slots" (0: nothing rendered yet)
  bool last_lds_only = false;           // the most recent render's plan chose the trace kernel without a stack-spill arm (mirt_scene_get_option, "stack_lds_only")
  // render workspaces: MIRT_MAX_FRAMES contexts so that several frames can be in flight on different streams (the next frame's blocks fill the
  // CUs the draining frame frees); a context is reused only after its previous frame has finished
  mirt::RenderCtx ctx[mirt::MIRT_MAX_FRAMES];
  unsigned frame_no = 0;
  unsigned long long frame_seq = 0;
  mirt::RenderCtx* last = nullptr;        // context of the most recent render (mirt_get_stats)
  unsigned long long overflow_events = 0;  // capacity overflows seen since the last mirt_get_stats
  double trace_ms_sum = 0.0; int trace_frames = 0;   // trace-kernel time of the frames finished since the last mirt_get_stats
  // wavefront path workspace (wavefront.hip)
  mirt::DevBuf<uint32_t> wf_state;
  mirt::DevBuf<float4> wf_rays;
  mirt::DevBuf<unsigned long long> wf_ctr;
  mirt::PinnedBuf<unsigned long long> wf_ctr_host;
  std::vector<mirt::Event> wf_events;
  int wf_rounds = 0;
  // sched = 2: the frame's samples in order of decreasing cost class, measured once per frame size (shared by the contexts)
  mirt::DevBuf<uint32_t> so_order, so_keys, so_keys2, so_ws;      // [call's samples], [slab's samples] x 2, the sort's workspace
  long long so_key = -1, so_pending_key = -1, so_total = -1; mirt::Event so_ev; bool so_busy = false;
  long long so_last = 0;                   // samples of the last launch measured: what so_keys / so_keys2 hold (mirt_get_sample_order)
  // ... and what the measuring call's rays did: primitive tests per internal-node visit (SceneFacts::prim_ratio; negative: not
  // known).  The measuring call runs the counting kernels; its counters -- the scene's own so_counters where the caller asked for
  // none -- are copied to so_counts_host ahead of so_ev, and the first call to find so_ev passed takes the ratio (render.hip,
  // sample_order_landed).  Discarded with the order, and by a geometry update (update.hip, begin_update).
  float so_ratio = -1.0f;
  bool so_ratio_stale = false;             // the geometry changed while the measurement was in flight: its counts are not kept
  mirt::DevBuf<unsigned long long> so_counters;      // device: laid out as RenderCtx::counters, words [0..11]
  mirt::PinnedBuf<unsigned long long> so_counts_host; // pinned: internal visits, sphere tests, triangle tests of the measuring call
  // rng tables cache
  mirt::RngCache rng;
  // LBVH build timing
  mirt::Event ev0, ev1;
  bool colors_finite = true;               // every material colour and light colour is finite (0 * colour == 0)
  bool any_trans = false;                  // some material has transparency != 0
  bool any_rough = false;
  int query_blocks = 0;                    // grid size of the ray-query kernel on this scene's device (query.hip; filled on first use)
  int light_blocks = 0;                    // ... and of the direct-light kernel (light.hip)
  int vis_blocks = 0;                      // ... and of the hemisphere-visibility kernel (visibility.hip)
  int indirect_blocks = 0;                 // ... and of the indirect-light kernel (indirect.hip)
  int closest_blocks = 0;                  // ... and of the closest-point kernel (closest.hip)
  int multihit_blocks[4] = {0, 0, 0, 0};   // ... and of the multi-hit kernel's instances (multihit.hip: capacity 0, 1, 4, 8)
  int contacts_blocks[4] = {0, 0, 0, 0};   // ... and of the contact kernel's instances (closest_multi.hip: capacity 0, 1, 4, 8)
  int spherecast_blocks[2] = {0, 0};       // ... and of the sphere-cast kernel's instances (spherecast.hip: first contact, any contact)
  int overlap_blocks[5] = {0, 0, 0, 0, 0}; // ... and of the box-overlap kernel's instances (overlap.hip: count, any, capacity 1, 4, 8)
  int overlap_list_blocks = 0;             // ... and of the overlap-list fill kernel (overlap_list.hip)
  int overlap_tris_blocks[3] = {0, 0, 0};  // ... and of the triangle-overlap kernels (overlap_tris.hip: count, any, fill)
  int ray_list_blocks[2] = {0, 0};         // ... and of the ray-list fill kernel's instances (query_lists.hip: words, words and values)
  int ball_list_blocks[2] = {0, 0};        // ... and of the ball-list fill kernel's instances (query_lists.hip: words, words and values)
  int cast_list_blocks[3] = {0, 0, 0};     // ... and of the cast-list kernels (cast_lists.hip: count, words, words and values)
  bool updated = false;                    // geometry updated in place since the last build (update.hip): mirt_camera_rays waits for the build like every other call
  // Shading values updated in place (update_shading.hip).  The three facts above are prim_flags | host_flags (MAT_* bits,
  // material_flags.h), by source: the primitives' materials -- after a material update known only to the device, until
  // settle_facts has read the reduction's word -- and what the host holds: planes, lights, exposure.
  unsigned prim_flags = 0, host_flags = 0;
  std::vector<MirtLight> suns_host, bulbs_host;      // what mirt_scene_create / mirt_scene_set_lights were given
  std::vector<MirtPlane> planes_host;
  mirt::DevBuf<unsigned char> mat_flags;   // device: material_flags of every primitive (spheres, then triangles), padded with zeros to whole words; made by the first material update
  mirt::DevBuf<unsigned> flags_or;         // device: the OR over mat_flags, written by the reduction that ends a material update
  mirt::PinnedBuf<unsigned> flags_or_host; // pinned: its copy, valid once facts_ev has passed
  mirt::Event facts_ev;                    // end of the last material update's reduction and copy
  bool facts_pending = false;              // a material update was issued since prim_flags was read
  hipStream_t facts_stream = nullptr;      // ... on this stream
  mirt::PinnedBuf<unsigned char> stage;    // pinned staging of the light and plane records on their way to the device
  mirt::Event stage_ev; bool stage_used = false;          // ... and the end of the last copy out of it
};

namespace mirt {
// lbvh_build.hip (sort_low_byte_ws_words: build_plan.h)
int build_lbvh(MirtScene* sc, hipStream_t stream);
int sort_low_byte(const uint32_t* keys_in, uint32_t* keys_out, uint32_t* vals_out, long long n, uint32_t* ws, hipStream_t stream);
int probe_sort(int device, int mode, int n, const uint32_t* keys, uint32_t* keys_out, uint32_t* vals_out);
int get_tree(MirtScene* sc, MirtTreeNode* nodes, uint32_t* codes, MirtPrimRef* refs, float* bounds);
int get_records(MirtScene* sc, MirtRecordInfo* info, void* nodes, void* qnodes, void* wnodes, void* prims, uint32_t* unit_prim,
                uint32_t* tris_before, float* tri_boxes, float* qparams);
// render.hip
int render(MirtScene* sc, const MirtRenderParams* p, void* d_rgba8, void* d_rgba_f32, hipStream_t stream);
int scatter_part(const MirtRenderParams* p, const void* d_part, void* d_frame, hipStream_t stream);
int64_t render_num_pixels(const MirtRenderParams* p);
int part_pixel(const MirtRenderParams* p, int64_t local, int32_t* x, int32_t* y);
int trace_ms_of(RenderCtx& cx, float* ms);
int fold_trace_time(MirtScene* sc, RenderCtx& cx);
int probe_math(int device, int which, int n, const float* in, float* out);
int probe_xorwow(int device, int spp, int nstreams, int draws, uint32_t* out);
int probe_qbox(int device, int n, const float* in, uint32_t* out);
int probe_sched(int device, int which, int n, const uint32_t* in, uint32_t* out);
int get_sample_order(MirtScene* sc, MirtSampleOrderInfo* info, uint32_t* order, uint32_t* keys, uint32_t* sorted_keys);
int ensure_rng_tables(RngCache* rc, int sample_tables, long long frame_pixels, hipStream_t stream, RngTablesDev* out, bool allow_larger);
int render_accumulate(MirtScene* sc, const MirtRenderParams* p, void* d_accum, int sample_first, int sample_count, hipStream_t stream);
void rng_cache_free(RngCache* rc);
int render_accumulate_pixels(MirtScene* sc, const MirtRenderParams* p, const AdaptiveArgs& ax, void* d_accum, int sample_first, int sample_count, hipStream_t stream);
// adaptive.hip
size_t sparse_blocks_words(long long num_listed);
int sparse_expand(RenderCtx& cx, const uint32_t* list, long long num_listed, long long p0, long long pn, int count, long long* num_samples_dev, hipStream_t stream);
int resolve_moments(RenderCtx& cx, const float4* samples, const AdaptiveArgs& ax, float4* accum, long long p0, long long pn, long long num_listed,
                    int count, hipStream_t stream);
int select_pixels(const MirtRenderParams* p, const void* d_accum, const void* d_accum_sq, const uint32_t* d_counts, int min_samples, int max_samples,
                  float max_variance, uint32_t* d_pixels_out, uint32_t* d_num_out, hipStream_t stream);
int finalize(const MirtRenderParams* p, const void* d_accum, int total_samples, void* d_rgba8, hipStream_t stream);
int finalize_counts(const MirtRenderParams* p, const void* d_accum, const uint32_t* d_counts, void* d_rgba8, hipStream_t stream);
// query.hip
int trace_rays(MirtScene* sc, const void* d_rays, int64_t num_rays, void* d_hits, uint32_t flags, hipStream_t stream);
int camera_rays(MirtScene* sc, const MirtRenderParams* p, void* d_rays, hipStream_t stream);
// light.hip
int direct_light(MirtScene* sc, const void* d_features, int64_t n, void* d_out_f32, uint64_t* d_lit_mask, uint32_t flags, hipStream_t stream);
// visibility.hip
int hemisphere_visibility(MirtScene* sc, const void* d_features, int64_t n, const void* d_dirs, int num_dirs, const void* d_rot, float radius,
                          void* d_out_f32, uint64_t* d_vis_mask, uint32_t flags, hipStream_t stream);
// indirect.hip
int indirect_light(MirtScene* sc, const void* d_features, int64_t n, const void* d_dirs, int num_dirs, const void* d_rot, float radius,
                   void* d_out_f32, uint64_t* d_hit_mask, uint32_t flags, hipStream_t stream);
// closest.hip
int closest_points(MirtScene* sc, const void* d_points, int64_t n, void* d_hits, void* d_features, uint32_t flags, hipStream_t stream);
// closest_multi.hip
int closest_points_multi(MirtScene* sc, const void* d_points, int64_t n, int k, void* d_hits, uint32_t* d_counts, void* d_features, uint32_t flags,
                         hipStream_t stream);
// spherecast.hip
int cast_spheres(MirtScene* sc, const void* d_casts, int64_t n, void* d_hits, void* d_features, uint32_t flags, hipStream_t stream);
// overlap.hip
int overlap_boxes(MirtScene* sc, const void* d_boxes, int64_t n, int k, void* d_hits, uint32_t* d_counts, void* d_features, uint32_t flags,
                  hipStream_t stream);
// overlap_list.hip
int64_t list_offsets_work_bytes(int64_t n);
int list_offsets(MirtScene* sc, const uint32_t* d_counts, int64_t n, int64_t* d_offsets, void* d_work, hipStream_t stream);
int overlap_list(MirtScene* sc, const void* d_boxes, int64_t n, const int64_t* d_offsets, uint32_t* d_words, int64_t capacity, hipStream_t stream);
// overlap_tris.hip
int overlap_triangles(MirtScene* sc, const void* d_tris, int64_t n, uint32_t* d_counts, uint32_t flags, hipStream_t stream);
int triangle_list(MirtScene* sc, const void* d_tris, int64_t n, const int64_t* d_offsets, uint32_t* d_words, int64_t capacity, hipStream_t stream);
// query_lists.hip
int ray_list(MirtScene* sc, const void* d_rays, int64_t num_rays, const int64_t* d_offsets, uint32_t* d_words, float* d_t, int64_t capacity, uint32_t flags,
             hipStream_t stream);
int ball_list(MirtScene* sc, const void* d_points, int64_t n, const int64_t* d_offsets, uint32_t* d_words, float* d_dist, int64_t capacity, uint32_t flags,
              hipStream_t stream);
// cast_lists.hip
int cast_counts(MirtScene* sc, const void* d_casts, int64_t n, uint32_t* d_counts, uint32_t flags, hipStream_t stream);
int cast_list(MirtScene* sc, const void* d_casts, int64_t n, const int64_t* d_offsets, uint32_t* d_words, float* d_t, int64_t capacity, uint32_t flags,
              hipStream_t stream);
// multihit.hip
int trace_rays_multi(MirtScene* sc, const void* d_rays, int64_t num_rays, int k, void* d_hits, uint32_t* d_counts, uint32_t flags, hipStream_t stream);
// denoise.hip
int hit_features(MirtScene* sc, const void* d_rays, const void* d_hits, int64_t n, void* d_features, hipStream_t stream);
size_t denoise_work_bytes(const MirtRenderParams* p);
int denoise(const MirtRenderParams* p, const void* d_accum, const void* d_accum_sq, const uint32_t* d_counts, const void* d_features, int iterations,
            float sigma_c, float sigma_n, float sigma_p, void* d_work, void* d_out, hipStream_t stream);
// update.hip
int update_spheres(MirtScene* sc, const void* d_spheres, int first, int count, hipStream_t stream);
int update_triangles(MirtScene* sc, const void* d_verts, int first, int count, hipStream_t stream);
int wait_for_frames(MirtScene* sc);
// update_shading.hip
LightDev sun_dev(const MirtLight& l);
LightDev bulb_dev(const MirtLight& l);
PlaneDev plane_dev(const MirtPlane& p);
void pack_mat(const float m[11], float4* out);
void refresh_host_facts(MirtScene* sc);
int settle_facts(MirtScene* sc);
int set_lights(MirtScene* sc, const MirtLight* suns, const MirtLight* bulbs, hipStream_t stream);
int set_planes(MirtScene* sc, const MirtPlane* planes, int first, int count, hipStream_t stream);
int update_materials(MirtScene* sc, const char* who, const void* d_mats, int base, int total, int first, int count, hipStream_t stream);
int get_materials(MirtScene* sc, const char* who, int base, int total, int first, int count, void* d_mats_out, hipStream_t stream);
// temporal.hip
int get_spheres(MirtScene* sc, int first, int count, void* d_xyzr_out, hipStream_t stream);
int get_triangles(MirtScene* sc, int first, int count, void* d_verts_out, hipStream_t stream);
int prev_features(MirtScene* sc, const void* d_rays, const void* d_hits, int64_t n, const void* d_prev_xyzr, const void* d_prev_verts, void* d_features,
                  hipStream_t stream);
int temporal_accumulate(const MirtRenderParams* p, const MirtCamera* prev_camera, const void* d_accum, const void* d_accum_sq, const uint32_t* d_counts,
                        const void* d_prev_features, const void* d_hist_accum, const void* d_hist_accum_sq, const uint32_t* d_hist_counts,
                        const void* d_hist_features, int max_history, float sigma_n, float sigma_p, void* d_out_accum, void* d_out_accum_sq,
                        uint32_t* d_out_counts, hipStream_t stream);
// wavefront.hip
int wavefront_trace(MirtScene* sc, RenderCtx& cx, RenderArgs& a, bool count, hipStream_t stream, float* trace_ms);
}
// (MIRT_HIP, MIRT_TRY: dev_mem.h)

namespace mirt {

// Blocks of a persistent grid that fills the device: compute units x resident blocks of `kernel` per unit (per_cu_fallback
// if the occupancy query fails).  An error only if the device's properties cannot be read.
template <class K>
hipError_t persistent_grid_blocks(int device, K kernel, int block, int per_cu_fallback, int* blocks)
{
  hipDeviceProp_t prop;
  const hipError_t e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return e;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess || per_cu < 1) per_cu = per_cu_fallback;
  *blocks = prop.multiProcessorCount * per_cu;
  return hipSuccess;
}

// The query kernels' host side (query.hip, light.hip, visibility.hip, indirect.hip, closest.hip, closest_multi.hip, spherecast.hip,
// overlap.hip, overlap_list.hip, query_lists.hip, multihit.hip; launch arithmetic: query_launch.h; argument checks: host_scene.h).
// Stack entries their walk keeps in LDS: the compiled size, unless the option names a smaller one (tests force the spill path).
inline int query_lds_depth(const MirtScene* sc)
{
  const int opt = sc->opt.stack_lds_depth;
  return (opt >= 0 && opt < QUERY_STACK_LDS) ? opt : QUERY_STACK_LDS;
}

// The persistent grid of a query kernel compiled for waves_per_simd waves: *cache (one of MirtScene's *_blocks, since occupancy
// is per kernel), filled on first use -- per scene, i.e. per device.
template <class K>
int query_grid_blocks(const MirtScene* sc, K kernel, int waves_per_simd, int* cache)
{
  if (!*cache && persistent_grid_blocks(sc->device, kernel, QUERY_BLOCK, waves_per_simd * 4 * 64 / QUERY_BLOCK, cache) != hipSuccess) *cache = 1024;
  return *cache;
}

// One launch of a kernel with one lane per row: its persistent grid, as many blocks of it as n rows need (row_launch), the launch
// and its error.
template <class K, class A>
int launch_rows(const MirtScene* sc, K kernel, int waves_per_simd, int* cache, long long n, const A& args, hipStream_t stream)
{
  const int grid = query_grid_blocks(sc, kernel, waves_per_simd, cache);
  hipLaunchKernelGGL(kernel, dim3(row_launch(n, grid)), dim3(QUERY_BLOCK), 0, stream, args);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

// The scene fields of a row kernel's *Args struct: what every walk over the exact records reads ...
template <class A>
void fill_walk_args(A& q, const MirtScene* sc)
{
  q.nodes = sc->nodes; q.unit_prim = sc->unit_prim;
  q.planes = sc->planes; q.num_planes = sc->d.num_planes;
  q.root_ref = sc->root_ref; q.prim_base16 = sc->prim_base / 16u;
  q.lds_depth = query_lds_depth(sc);
}
// ... and what the point, cast and box queries read beside it
template <class A>
void fill_scene_args(A& q, const MirtScene* sc)
{
  fill_walk_args(q, sc);
  q.tri_verts = sc->tri_verts;
  q.coord_max = sc->coord_max;
}

// The list kernels' capacity ladder: f(the smallest of the capacities 0, 1, 4, 8 that holds k, as a std::integral_constant; its
// index 0..3 -- the slot of the instance's cached grid size, since occupancy is per kernel).
template <class F>
int with_capacity(int k, F f)
{
  if (k == 0) return f(std::integral_constant<int, 0>(), 0);
  if (k == 1) return f(std::integral_constant<int, 1>(), 1);
  if (k <= 4) return f(std::integral_constant<int, 4>(), 2);
  return f(std::integral_constant<int, 8>(), 3);
}

// the frame, camera and partition block of RenderArgs (what a primary ray is made from, apart from spp and the rng tables)
inline void fill_camera(RenderArgs& a, const MirtScene* sc, const MirtRenderParams* p)
{
  a.width = p->width; a.height = p->height; a.bounces = sc->d.bounces;
  a.fisheye = sc->d.fisheye; a.panorama = sc->d.panorama;
  a.dof_focus = sc->d.dof_focus; a.dof_lens = sc->d.dof_lens;
  a.forward.x = sc->d.forward.x; a.forward.y = sc->d.forward.y; a.forward.z = sc->d.forward.z;
  a.right.x = sc->d.right.x; a.right.y = sc->d.right.y; a.right.z = sc->d.right.z;
  a.up.x = sc->d.up.x; a.up.y = sc->d.up.y; a.up.z = sc->d.up.z;
  a.eye.x = sc->d.eye.x; a.eye.y = sc->d.eye.y; a.eye.z = sc->d.eye.z;
  a.stripe_rows = p->stripe_rows; a.num_parts = p->num_parts; a.part = p->part;
}

} // namespace mirt

#endif
