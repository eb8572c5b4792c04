/*
 * mirt.h -- C ABI of libmirt.so, the MI355X-native replacement for the hot path of
 * GJ0407790/cuda_ray_tracer (LBVH build + BVH-traversal render).
 *
 * Every entry point names the reference interface it replaces (paths relative to the reference
 * tree).  Plain C: opaque handles, POD structs, pointers and sizes; no C++ or torch types.
 * All functions return 0 on success and a non-zero MirtStatus otherwise; mirt_last_error() returns a
 * thread-local description.  The library never calls exit() (the reference's CUDA_CHECK does,
 * main.cu:14-23); the CLI maps a non-zero status to the reference's message + exit code.
 *
 * Device pointers are ordinary HIP device pointers (hipMalloc, or torch tensor data_ptr()).
 * `stream` is a hipStream_t passed as void* (NULL = the default stream).  A MirtScene is bound to the
 * HIP device it was created on and is not thread-safe; render calls are asynchronous on `stream`
 * unless stated otherwise.  There is no CPU fallback: without a HIP device scene creation fails.
 */
#ifndef MIRT_H
#define MIRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIRT_VERSION 3

typedef enum MirtStatus {
  MIRT_OK = 0,
  MIRT_ERR_IO = 1,          /* "Error opening file..."            parse.cpp:22-25 */
  MIRT_ERR_PARSE = 2,       /* "One of the lines are not valid."  parse.cpp:218-221 */
  MIRT_ERR_ARG = 3,
  MIRT_ERR_HIP = 4,         /* any HIP runtime failure (CUDA_CHECK, main.cu:14-23) */
  MIRT_ERR_NO_DEVICE = 5,
  MIRT_ERR_STATE = 6        /* e.g. render before build; a capacity overflow reported by mirt_get_stats */
} MirtStatus;

/* ---- POD scene structs: same field order and size as the reference's classes -------------------- */
typedef struct MirtVec3 { float x, y, z; } MirtVec3;                       /* vec3.cuh:21-92, 12 B */
typedef struct MirtRGB { float r, g, b; } MirtRGB;                         /* struct.cuh:11-34, 12 B */
typedef struct MirtMaterials {                                             /* object.cuh:17-38, 44 B */
  MirtRGB color, shininess, trans;
  float ior, roughness;
} MirtMaterials;
typedef struct MirtSphere { MirtVec3 c; float r; MirtMaterials mat; } MirtSphere;            /* object.cuh:95-119, 60 B */
typedef struct MirtTriangle { MirtVec3 p0, p1, p2, nor, e1, e2; MirtMaterials mat; } MirtTriangle; /* object.cuh:165-194, 116 B */
typedef struct MirtPlane { float a, b, c, d; MirtVec3 nor, point; MirtMaterials mat; } MirtPlane;  /* object.cuh:124-149, 84 B */
typedef struct MirtSun { MirtVec3 dir; MirtRGB color; } MirtSun;           /* object.cuh:232-248, 24 B */
typedef struct MirtBulb { MirtVec3 point; MirtRGB color; } MirtBulb;       /* object.cuh:250-266, 24 B */
typedef struct MirtPrimRef { uint32_t type; uint32_t id; } MirtPrimRef;    /* object.cuh:72-88, 8 B; 0 sphere, 1 triangle */

/* Scalars of StlConfig/RawConfig (config.hpp:24-73, 75-126) + host arrays in file order.
 * Pointers are borrowed for the duration of the call that takes the descriptor. */
typedef struct MirtSceneDesc {
  int32_t width, height, bounces, aa;
  float dof_focus, dof_lens;
  MirtVec3 forward, right, up, eye;
  float expose;                       /* +inf = exposure off (config.hpp:50) */
  int32_t fisheye, panorama, gi;
  int32_t num_spheres, num_triangles, num_prims, num_planes, num_suns, num_bulbs;
  const MirtSphere* spheres;
  const MirtTriangle* triangles;
  const MirtPrimRef* prim_refs;       /* host_primitive_references, config.hpp:64 */
  const MirtPlane* planes;
  const MirtSun* suns;
  const MirtBulb* bulbs;
} MirtSceneDesc;

typedef struct MirtHostScene MirtHostScene;   /* parsed scene on the host  (StlConfig, config.hpp:24-73) */
typedef struct MirtScene MirtScene;           /* device-resident scene     (RawConfig, config.hpp:75-126) */

const char* mirt_last_error(void);
int mirt_version(void);

/* ---- scene front end -------------------------------------------------------------------------- */
/* parseInput(argv, StlConfig&), parse.hpp:10 / parse.cpp:16-39.  Same grammar (parse.cpp:41-222). */
int mirt_parse_scene_file(const char* path, MirtHostScene** out);
int mirt_parse_scene_text(const char* text, size_t len, MirtHostScene** out);
/* Deterministic synthetic scene of BASELINE config 5; not in the reference. */
int mirt_synthetic_scene(uint64_t seed, int num_spheres, int num_triangles, MirtHostScene** out);
void mirt_host_scene_destroy(MirtHostScene* hs);
int mirt_host_scene_desc(const MirtHostScene* hs, MirtSceneDesc* out);   /* pointers stay owned by hs */
const char* mirt_host_scene_filename(const MirtHostScene* hs);           /* the `png W H name` name, parse.cpp:47-51 */

/* ---- device scene ----------------------------------------------------------------------------- */
/* initRawConfigFromStl + copyConfigDataToDevice, config_utils.cuh:11-17 / config_utils.cu:18-199.
 * Uploads the scene to HIP device `device` in the SoA layout of DESIGN.md. */
int mirt_scene_create(const MirtSceneDesc* desc, int device, MirtScene** out);
/* freeRawConfigDeviceMemory, config_utils.cuh:20 (frees everything; the reference leaks the SoA arrays). */
void mirt_scene_destroy(MirtScene* sc);

/* Mode switches and tuning values of a scene, by name.  Not in the reference (its knobs are compile-time constants).
 *   build (take effect at the next mirt_build_lbvh):
 *     "bounds_as_shipped" 0/1 (default 0): 1 reproduces the shipped reference's tree -- scene bounds never stored
 *                         (parse.cpp:28), every Morton code 0
 *   render:
 *     "traversal"         MIRT_TRAVERSAL_*: 0 the reference's left-first descent (bvh_traversal.cu:149-157); 1 (default)
 *                         near-child-first on the quantised records of a sphere-only scene (see qnodes) -- same pixels, fewer
 *                         visits; the reference's order wherever the exact records are walked (scenes with triangles below
 *                         65536 primitives, qnodes 0, wavefront) and over the wide records; 2 near-child-first everywhere (a
 *                         sample may differ where the reference's own result depends on its visiting order: triangle
 *                         silhouettes, sphere hits within an ulp of their box from a far camera)
 *     "qnodes"            0/1/2 (default 1): quantised node records in the single-kernel path.  1: sphere-only scenes walk 32-byte
 *                         records (two memory requests per node visit instead of four; traversal >= 1); scenes with triangles of
 *                         65536 primitives or more walk the wide records (the boxes of a node's four grandchildren per 64-byte
 *                         record, two levels per step, the reference's order: traversal 1 only; a triangle hit the reference's
 *                         walk may not reach sends its ray over the exact records again).  2: every scene.  0: never.  Same
 *                         pixels in every case; not with wavefront; and only where the records' grid resolves the scene's
 *                         coordinates (on every axis below 64 extents of the scene box: a scene that sits far from the world
 *                         origin compared with its size walks the exact records).  Over the quantised records the sphere hit
 *                         a nearest-hit walk ends with -- shadow rays to point lights included -- is checked against the
 *                         reference's own box test, and a ray whose hit the reference may never test is walked again its way
 *     "shadow_anyhit"     0/1 (default 1): a shadow ray ends at its first occluder; 0: a nearest-hit query like every other ray,
 *                         as diffuseLight does (draw.cu:347-352, 365-370) -- same boolean, more node visits
 *     "skip_unlit"        0/1 (default 1): shadow rays towards lights the shading normal faces away from are not traced (their
 *                         term is 0 either way, draw.cu:353-357); 0: every light's shadow ray is traced (draw.cu:342-374)
 *                         {traversal 0, shadow_anyhit 0, skip_unlit 0, qnodes 0} is the reference's walk, ray for ray
 *     "specialise"        0/1 (default 1): a scene without point lights (and, sphere-only scenes, without transparent materials
 *                         and gi) is rendered by the kernel compiled without those features (same pixels and counters;
 *                         0: the general kernel)
 *     "ray_start_lds"     0/1 (default 1): a sphere-only scene without point lights, transparent materials and gi, with at most
 *                         ten suns and a tree at most 23 internal nodes deep, is rendered by the kernel whose traversal loop
 *                         starts the next ray of a batch from values kept in LDS, in the bytes of a stack slot such a tree never
 *                         fills (same pixels and counters; 0: the kernel that loads them from memory)
 *     "wavefront"         0/1: the trace/shade kernel pair instead of the single kernel
 *     "slab_log2"         (default 28) a call is rendered in slabs of at most 2^slab_log2 samples: 16 B of workspace per
 *                         sample, i.e. at most 4 GiB per frame in flight, however large the frame
 *     "sched"             0/1/2 (default 2): longest-first hand-out of a call's samples, measured by the first call of a shape and reused
 *                         (the scene is immutable): 2 by sample (every sample in its cost class, expensive classes first, positions
 *                         within a class kept; 4 B per sample), 1 by chunk of 64..256 samples (one-slab calls), 0 frame order
 *     "stack_lds_depth", "refill_k", "init_k", "batch_k", "leaf_k", "reps", "drain_lanes", "chunk_shift", "trace_waves",
 *     "wf_pool", "wf_refill_k": tuning (defaults are the measured optima; "reps" and "batch_k" at 0, their default, are chosen per
 *     call: by kind of kernel, and on a sphere-only scene by what its rays did in the call that measured the sample order)
 * Environment variables MIRT_<NAME> override the defaults of the TUNING values once, when the scene is created (the mode
 * switches -- bounds_as_shipped, traversal, wavefront, qnodes, shadow_anyhit, skip_unlit -- only with MIRT_ALLOW_ENV=1); nothing
 * reads the environment during a render.
 * mirt_scene_get_option also reads four facts about the traversal stack of the single-kernel path (mirt_scene_set_option does
 * not know them):
 *     "tree_depth"         D, the most internal nodes on any root-to-leaf path of the built tree (-1 before a build); every
 *                          mirt_build_lbvh recomputes it.  A walk over two-child records keeps at most D entries pending
 *     "stack_lds_capacity" entries the kernel's stack holds before it spills to global memory
 *     "stack_lds_only"     1 if the most recent render call ran the kernel that has no spill path at all: chosen when
 *                          D <= stack_lds_capacity, the walk is over two-child records (not the wide ones) and "stack_lds_depth"
 *                          is at its default, -1 -- any explicit value, the compiled size included, keeps the general kernel
 *     "stack_lds_slots"    LDS slots of the traversal stack of the kernel the most recent render call ran (0 before a render):
 *                          stack_lds_capacity, or one fewer when "ray_start_lds" chose its kernel
 * ... and one about the scene's rays:
 *     "prim_ratio_bits"    the bits of a float: primitive tests per internal-node visit, counted by the call that measured the
 *                          sample order ("sched" = 2) and read by the calls after it; negative while not known -- until a render
 *                          call or mirt_get_sample_order has found that call finished (the option itself polls nothing and
 *                          changes nothing), after a geometry update, for a scene whose rays visit no node */
#define MIRT_TRAVERSAL_REFERENCE 0
#define MIRT_TRAVERSAL_ORDERED 1
#define MIRT_TRAVERSAL_ORDERED_ALL 2
int mirt_scene_set_option(MirtScene* sc, const char* name, int value);
int mirt_scene_get_option(const MirtScene* sc, const char* name, int* value);

/* build_lbvh_karas(RawConfig&, int morton_bits), lbvh_builder.cuh:14 / lbvh_builder.cu:401-521:
 * scene bounds -> 30-bit Morton codes -> stable radix sort -> Karras hierarchy -> AABB refit -> 64-byte
 * two-child node records, primitive records in sorted order (+ 32-byte quantised node records for sphere-only scenes).  Synchronous (like the reference, lbvh_builder.cu:475).  build_ms (nullable)
 * receives the device time measured with HIP events (the reference prints it, lbvh_builder.cu:489). */
int mirt_build_lbvh(MirtScene* sc, void* stream, float* build_ms);

/* ---- render ----------------------------------------------------------------------------------- */
#define MIRT_RENDER_COUNTERS 1u   /* also count rays / node visits / leaf tests (slower kernel variant) */

/* The frame is cut into horizontal stripes of `stripe_rows` rows; stripe i belongs to part
 * (i % num_parts).  A call renders the stripes of part `part` into a compact buffer (the part's stripes
 * in increasing order, each row-major).  num_parts = 1, part = 0 renders the whole frame row-major. */
typedef struct MirtRenderParams {
  int32_t width, height;     /* frame size (RawConfig::width/height) */
  int32_t spp;               /* the reference's `aa`: 0 = one un-jittered sample, 1 = one jittered, >1 = spp samples */
  int32_t stripe_rows, num_parts, part;
  uint32_t flags;
} MirtRenderParams;

/* number of pixels the call writes */
int64_t mirt_render_num_pixels(const MirtRenderParams* p);

/* render(pixel_t* d_image, w, h, aa, RawConfig*), draw.cuh:10 / draw.cu:215-239.
 * d_rgba8: num_pixels * 4 bytes, RGBA (pixel_t, libpng.h:23-27).  d_rgba_f32 (nullable): num_pixels * 4
 * floats, the linear RGBA sample mean before sRGB/quantisation (for parity checks). */
int mirt_render(MirtScene* sc, const MirtRenderParams* p, void* d_rgba8, void* d_rgba_f32, void* stream);

/* render_kernel_atomic_aa + finalize_kernel, draw.cu:13-92 (in the reference tree but not called by its render()): the
 * accumulate / finalise pair for progressive rendering and for any number of samples per pixel.
 * mirt_render_accumulate adds, for every pixel of the part, the samples [sample_first, sample_first + sample_count) to
 * d_accum_f32 (num_pixels * 4 floats, zeroed by the caller before the first call); sample s of pixel p is seeded
 * curand_init(1234 + p, s, 0) and jittered (draw.cu:74-84) whatever p->spp says.  The reference adds with atomicAdd, i.e. in
 * no particular order; here one call adds one value per pixel -- the sum of its samples in the xor-butterfly order of
 * draw.cu:181-189 -- so results do not depend on timing.  At most 4096 sample indices per call; any number over several calls.
 * mirt_finalize writes the 8-bit image: mean over total_samples, sRGB, clamp * 255 + 0.5 (draw.cu:22-46).
 * A single mirt_render_accumulate of samples [0, spp) followed by mirt_finalize gives the bytes of mirt_render (spp > 1). */
int mirt_render_accumulate(MirtScene* sc, const MirtRenderParams* p, void* d_accum_f32, int sample_first, int sample_count, void* stream);
int mirt_finalize(const MirtRenderParams* p, const void* d_accum_f32, int total_samples, void* d_rgba8, void* stream);

/* ---- adaptive sampling: more samples only where the image is noisy -------------------------------- */
/* Not in the reference (render_kernel_atomic_aa adds the same samples to every pixel).  Callers detect the feature by these
 * symbols (MIRT_VERSION stays 3).  The three calls are the pieces of one loop: a dense call with moments and counts, then rounds
 * of mirt_select_pixels -> mirt_render_accumulate_pixels on the selected pixels, then mirt_finalize_counts.
 *
 * mirt_render_accumulate_pixels: mirt_render_accumulate for the pixels of a list.  d_pixels: num_listed DISTINCT local pixel
 * indices into the part's compact buffer (the indexing of mirt_part_pixel_xy), uint32, device memory, 4-byte aligned, any order.
 * For every listed pixel lp:
 *   d_accum_f32[lp]    += the sum of its samples [sample_first, sample_first + sample_count): the float4, bit for bit, that
 *                         mirt_render_accumulate with the same p, sample_first and sample_count adds to that pixel
 *   d_accum_sq_f32[lp] += (nullable) the per-channel sum of the squares of the same samples (float4): each square one float32
 *                         multiply, summed in the same xor-butterfly order as the samples (absent samples 0, P the next power of two)
 *   d_counts[lp]       += (nullable, uint32) sample_count
 * One read-modify-write per pixel and buffer, no atomics.  A pixel that is not listed is neither traced nor written, in any of
 * the three buffers; neither is an entry >= mirt_render_num_pixels(p) (the list is bounded on the device).
 * d_pixels == NULL with num_listed == 0: every pixel of the part -- the dense call, its measured hand-out order included, plus the
 * two extra outputs.  d_pixels != NULL with num_listed == 0: MIRT_OK, nothing launched.
 * As mirt_render_accumulate: asynchronous on `stream`; sample_first + sample_count <= 4096; rendered in slabs of at most
 * 2^slab_log2 samples of workspace (a slab is a range of the part's pixels, and holds the listed pixels that fall into it);
 * MIRT_RENDER_COUNTERS counts (samples = num_listed x sample_count); render contexts, frames in flight and overflow reporting
 * as for every render call.  A call with a list is handed out in list order: it neither uses nor changes the measured hand-out
 * order ("sched") of the dense shape rendered last, so a full frame rendered afterwards is not measured again.
 * MIRT_ERR_STATE before mirt_build_lbvh.  MIRT_ERR_ARG: null scene, p or d_accum_f32; a negative count; a null list with
 * num_listed > 0, or a misaligned one; a list (d_pixels != NULL) on a scene with wavefront = 1 -- the trace / shade kernel pair
 * takes its samples in frame order only. */
int mirt_render_accumulate_pixels(MirtScene* sc, const MirtRenderParams* p, const uint32_t* d_pixels, int64_t num_listed, void* d_accum_f32,
                                  void* d_accum_sq_f32, uint32_t* d_counts, int sample_first, int sample_count, void* stream);
/* The pixels of the part that need more samples, in increasing order, to d_pixels_out (capacity mirt_render_num_pixels(p)
 * entries) and their number to d_num_out (one uint32); all device memory.  Pixel lp with n = d_counts[lp] is selected when
 *     n < max_samples && (n < min_samples || e > max_variance)
 * where e is the largest, over the channels r, g, b, of the estimated variance of the pixel mean, in float32 with one rounding
 * per operation and IEEE division; S = d_accum_f32[lp], Q = d_accum_sq_f32[lp]:
 *     nf = (float)n;  m = S_c / nf;  q = Q_c / nf;  v = q - m * m;  v = v > 0 ? v : 0;  e_c = v / (nf - 1);  e = fmaxf(e_r, fmaxf(e_g, e_b))
 * (v > 0 ? v : 0 also turns a NaN into 0: a non-finite pixel is not chased to max_samples).  The result is deterministic: wave
 * ballots, a block scan and a scan over the blocks in a second pass; no kernel waits for another block.
 * Asynchronous on `stream`, on the current device; no allocation beyond a workspace kept per device and stream (4 B per 1024
 * pixels).  MIRT_ERR_ARG: a null pointer, min_samples < 2, max_samples < min_samples. */
int mirt_select_pixels(const MirtRenderParams* p, const void* d_accum_f32, const void* d_accum_sq_f32, const uint32_t* d_counts, int min_samples,
                       int max_samples, float max_variance, uint32_t* d_pixels_out, uint32_t* d_num_out, void* stream);
/* mirt_finalize with a sample count per pixel: pixel lp gets exactly the bytes mirt_finalize(total_samples = d_counts[lp])
 * gives it (mean, sRGB, clamp * 255 + 0.5, draw.cu:22-46); a pixel with count 0 is written as 0, 0, 0, 0. */
int mirt_finalize_counts(const MirtRenderParams* p, const void* d_accum_f32, const uint32_t* d_counts, void* d_rgba8, void* stream);

/* Where local pixel `local` of a part's compact buffer lies in the frame (host arithmetic: the mapping mirt_render,
 * mirt_scatter_part and the multi-GPU gather use).  Returns MIRT_ERR_ARG when `local` is not a pixel of the part. */
int mirt_part_pixel_xy(const MirtRenderParams* p, int64_t local, int32_t* x, int32_t* y);
/* Scatter a compact part buffer back into a full row-major frame (device to device). */
int mirt_scatter_part(const MirtRenderParams* p, const void* d_part_rgba8, void* d_frame_rgba8, void* stream);

/* ---- ray queries on a built scene --------------------------------------------------------------- */
/* What a ray hits, for rays the caller makes: the reference's hitNearest (draw.cu:292-318) and the occlusion test of diffuseLight
 * (draw.cu:347-352, 365-370) as entry points, plus the primary rays of a frame.  Not in the reference (its rays never leave the
 * render kernel).  Callers detect the feature by these symbols (MIRT_VERSION stays 3).
 *
 * MirtRay: origin, tmax, direction (any non-zero length), pad; 32 B, read as two 16-byte loads (d_rays 16-byte aligned).
 * MirtHit: the primary-hit record: t (distance along the unit direction; -1 for a miss), kind (MIRT_HIT_*), id (index into the
 * scene's sphere, triangle or plane array as passed in MirtSceneDesc, i.e. file order) and the normal n; 24 B (d_hits 4-byte
 * aligned).  A miss is t = -1, kind 0, id 0, n = 0. */
typedef struct MirtRay { MirtVec3 o; float tmax; MirtVec3 d; float pad; } MirtRay;        /* 32 B */
typedef struct MirtHit { float t; uint32_t kind, id; MirtVec3 n; } MirtHit;              /* 24 B */
#define MIRT_HIT_NONE 0
#define MIRT_HIT_SPHERE 1
#define MIRT_HIT_TRIANGLE 2
#define MIRT_HIT_PLANE 3
#define MIRT_QUERY_ANY_HIT 1u
/* num_rays rays from d_rays -> num_rays records to d_hits (device pointers).
 * flags 0, closest hit: the ray is Ray(eye, dir, bounce) (object.cuh:69): d normalised by vec3::normalize (vec3.cuh:72-82).  The
 *   answer is hitNearest of that ray, bit for bit: traverse_lbvh (bvh_traversal.cu:92-183) -- from node 0, left child first, box
 *   test with tmin 1e-4 and te < best, a leaf accepted when 1e-6 < t < best, ties to the earlier sorted leaf -- then checkPlane
 *   (draw.cu:581-615), the BVH hit winning only when strictly nearer.  It is reported only if t < tmax (the test diffuseLight
 *   applies to a bulb, draw.cu:365-370), otherwise the record is a miss.  The normal is ObjectInfo.normal with p = t d + o:
 *   sphere normalize(inside ? c - p : p - c) (struct.cu:64-109), triangle denom < 0 ? nor : -nor (struct.cu:111-163), plane
 *   dot(n, d) < 0 ? n : -n (draw.cu:581-615).
 * MIRT_QUERY_ANY_HIT, occlusion: kind != 0 exactly when something is hit at t < tmax -- the same boolean as the closest-hit
 *   query with the same tmax (the render's shadow_anyhit relies on it).  The planes are asked first; the walk ends at the first
 *   leaf hit with t < tmax.  The record is the occluder found, not necessarily the nearest.
 * Both walk the exact 64-byte node records in the reference's order (never the quantised or wide ones): the reference's result
 * by construction.  A ray with tmax <= 0 or NaN, or with a direction that normalises to 0 or NaN, is a miss and is not walked.
 * Asynchronous on `stream`; reads the scene only (no render workspace, MirtStats counter or random-number table), so it may run
 * on another stream while a frame is in flight.  No allocation and no synchronisation: one launch.  num_rays 0: MIRT_OK, nothing
 * launched.  MIRT_ERR_ARG: null scene, num_rays < 0, a null or misaligned buffer with num_rays > 0, unknown flag bits;
 * MIRT_ERR_STATE before mirt_build_lbvh. */
int mirt_trace_rays(MirtScene* sc, const void* d_rays, int64_t num_rays, void* d_hits, uint32_t flags, void* stream);
/* The primary rays of a frame (or part, p as for mirt_render; p->flags ignored): mirt_render_num_pixels(p) rays in the part's
 * compact order.  Ray i is the one sample 0 of its pixel starts with in the render: curand_init(1234, pixel, 0) for spp <= 1
 * (draw.cu:105), curand_init(1234 + pixel, 0, 0) for spp > 1 (draw.cu:162), the pixel jittered for spp >= 1 (draw.cu:110-118,
 * 165-171), fisheye / panorama / depth of field as the scene sets them (Ray::Ray, struct.cu:16-62).  o is the ray's origin (the
 * lens point with depth of field), d its direction BEFORE the Ray constructor normalises it -- mirt_trace_rays normalises it
 * once, so camera rays followed by a closest-hit query give the render's primary hit bit for bit.  tmax = +inf, or 0 when the
 * scene's bounces is 0 (hitNearest answers a bounce-0 ray with nothing, draw.cu:294).  Uses the scene's random-number table
 * cache: with spp > 1 any cached sample table serves. */
int mirt_camera_rays(MirtScene* sc, const MirtRenderParams* p, void* d_rays, void* stream);

/* ---- denoising a frame: hit features and a variance-guided a-trous filter ------------------------- */
/* Not in the reference (it writes the sample mean as it is).  Callers detect the feature by these symbols (MIRT_VERSION stays
 * 3).  The inputs are what the calls above leave in device memory: the closest hits of a frame's camera rays, and the sums, the
 * sums of squares and the counts of mirt_render_accumulate_pixels.  Both calls are asynchronous on `stream`, take device pointers
 * only, allocate nothing, never synchronise, and touch no render context, MirtStats counter or hand-out table.  All arithmetic is
 * float32 with one IEEE rounding per operation (no fused multiply-add), IEEE division and square root; a + b + c means (a + b) + c;
 * dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z; length(u) = sqrtf(dot(u, u)); fmaxf / fminf return the operand that is not a NaN.
 *
 * mirt_hit_features: n MirtRay rows and the n MirtHit rows a closest-hit mirt_trace_rays answered for them -> n feature rows of
 * 32 B (d_features 16-byte aligned), each written with two 16-byte stores:
 *     (Px, Py, Pz, hit)  (nx, ny, nz, 0)
 * hit = 1.0f and P_c = o_c + t * normalize(d)_c (normalize as mirt_trace_rays normalises: vec3.cuh:72-82; the product rounded,
 * then the sum), n the record's normal as reported; a miss (kind == MIRT_HIT_NONE) writes eight zeros.  One lane per row.  The
 * scene is needed only for its device and the "built" check.  n == 0: MIRT_OK, nothing launched.  MIRT_ERR_ARG: null scene,
 * n < 0, a null or misaligned buffer with n > 0; MIRT_ERR_STATE before mirt_build_lbvh. */
int mirt_hit_features(MirtScene* sc, const void* d_rays, const void* d_hits, int64_t n, void* d_features, void* stream);
/* mirt_denoise: the frame p describes (width x height, row-major, N = width * height pixels; p->spp, stripe_rows and flags are
 * not used) from S = d_accum_f32, Q = d_accum_sq_f32 (float4 per pixel), k = d_counts (uint32 per pixel) and F = d_features
 * (mirt_hit_features rows of the pixels' rays) -> d_out_f32: N float4, the filtered MEAN (mirt_finalize with total_samples = 1
 * turns it into the 8-bit image).  d_work: mirt_denoise_work_bytes(p) = 40 N bytes of caller memory (two colour and two variance
 * buffers; host arithmetic; 0 for parameters mirt_denoise refuses), 16-byte aligned like the float buffers; calls that may overlap
 * in time need a d_work each.  On the current device.
 *
 * Prepare (one kernel), pixel p with k = k_p:
 *     k == 0: c = (0, 0, 0, 0), else nf = (float)k; c_ch = S_ch / nf for r, g, b, a
 *     k < 2:  v = 0, else v = mirt_select_pixels' e: m = S_ch / nf; q = Q_ch / nf; t = q - m * m; t = t > 0 ? t : 0 (a NaN gives
 *             0); e_ch = t / (nf - 1); v = fmaxf(e_r, fmaxf(e_g, e_b))
 * Iteration i = 0 .. iterations - 1 with step s = 2^i (one kernel each; colour and variance ping-pong between the buffers of
 * d_work, the last colour goes to d_out_f32; iterations == 0: d_out_f32 = c), pixel p = (x, y):
 *     c_p.rgb has a non-finite channel: c'_p = c_p, v'_p = v_p.  Otherwise
 *     g = k00 v(x-1, y-1) + k01 v(x, y-1) + k02 v(x+1, y-1) + k10 v(x-1, y) + ... + k22 v(x+1, y+1), summed left to right in this
 *         (row-major) order, coordinates clamped to the frame, k = (1/16 1/8 1/16; 1/8 1/4 1/8; 1/16 1/8 1/16)
 *     den = sigma_c * sqrtf(g) + 1e-10f
 *     sw = sv = 0, sc = (0, 0, 0, 0); for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = (x + s dx, y + s dy):
 *         skip the tap when q is outside the frame, or c_q.rgb has a non-finite channel
 *         h = K[|dx|] * K[|dy|], K = (3/8, 1/4, 1/16)
 *         dx == 0 and dy == 0: a = 0.  Otherwise, with hit_p = (F_p[3] != 0):
 *             skip the tap when hit_p != hit_q
 *             both hit:  a_n = fmaxf(0, 1 - dot(n_p, n_q)) / sigma_n;  D = P_q - P_p;  l = length(D);
 *                        a_p = l == 0 ? 0 : fabsf(dot(n_p, D)) / (sigma_p * l)      -- |cosine| between the centre's normal and
 *                        the displacement: no scene unit, about 0 inside a flat surface, large across a depth step
 *             both miss: a_n = a_p = 0
 *             a_c = fmaxf(fmaxf(|c_p.r - c_q.r|, |c_p.g - c_q.g|), |c_p.b - c_q.b|) / den
 *             t = a_n + a_p + a_c; skip the tap when t is a NaN; a = fminf(t, 87)
 *         w = h * expf(-a)      -- the library's own expf (mirt_probe_math which = 1), the same bits on every device
 *         sw = sw + w;  sc_ch = sc_ch + w * c_q.ch (r, g, b, a);  sv = sv + (w * w) * v_q
 *     c'_p.ch = sc_ch / sw;  v'_p = sv / (sw * sw)      -- the centre tap is never skipped, so sw >= 9/64
 * Every pixel depends on its inputs only (no atomics, no communication between lanes): the result does not depend on timing.
 * MIRT_ERR_ARG (all checked on the host, before any device work): a null pointer; p->num_parts != 1 (whole frames only: a
 * striped part has no neighbours across stripes); iterations outside [0, 8]; a sigma that is not finite and positive; a
 * misaligned buffer; d_out_f32 or d_work overlapping an input range (16 N, 16 N, 4 N, 32 N bytes) or each other. */
/* The scales the drivers (api.denoise_frame, `raytracer --denoise`) use; DESIGN.md section 6f has the table they were chosen from. */
#define MIRT_DENOISE_SIGMA_C 1.0f
#define MIRT_DENOISE_SIGMA_N 0.03f
#define MIRT_DENOISE_SIGMA_P 0.1f
size_t mirt_denoise_work_bytes(const MirtRenderParams* p);
int mirt_denoise(const MirtRenderParams* p, const void* d_accum_f32, const void* d_accum_sq_f32, const uint32_t* d_counts, const void* d_features,
                 int iterations, float sigma_c, float sigma_n, float sigma_p, void* d_work, void* d_out_f32, void* stream);

/* ---- updates of a built scene in place ---------------------------------------------------------- */
/* Move the camera, the spheres and the triangles of a scene without creating it again: the render workspaces, the
 * random-number tables and the measured hand-out order of the samples ("sched") stay.  Not in the reference (its RawConfig is
 * filled once, config_utils.cu:18-199).  Callers detect the feature by these symbols (MIRT_VERSION stays 3).
 *
 * MirtCamera: the camera fields of MirtSceneDesc, taken as given (the forward / up keyword rule of parse.cpp:60-72 is the
 * parser's business and is not applied); 64 B.  expose, bounces and gi are MirtShading's, lights and planes have setters of their
 * own (below: "shading values of a built scene in place"). */
typedef struct MirtCamera { MirtVec3 eye, forward, right, up; float dof_focus, dof_lens; int32_t fisheye, panorama; } MirtCamera;
int mirt_scene_get_camera(const MirtScene* sc, MirtCamera* out);
/* The new camera applies to every mirt_render, mirt_render_accumulate, mirt_camera_rays (and mirt_multi_submit) issued after
 * the call.  A frame already issued keeps the camera it was issued with, in every slab of a call of several slabs: each slab's
 * kernel arguments were copied when the call was issued.  Host state only: no device work, no synchronisation, the scene stays
 * built.  MIRT_ERR_ARG: null scene or camera. */
int mirt_scene_set_camera(MirtScene* sc, const MirtCamera* cam);
/* New geometry from device memory (hipMalloc, or a torch data_ptr(), on the scene's device), values taken as they are, as
 * mirt_scene_create takes them.  One kernel, one lane per primitive, asynchronous on `stream`.
 *   d_spheres: float [count][4] = cx, cy, cz, r of spheres first .. first+count-1 (file order); 16-byte aligned
 *   d_verts:   float [count][9] = p0, p1, p2 of triangles first .. first+count-1 (file order); 4-byte aligned.  nor, e1 and e2
 *              are computed as Triangle(Vertex, Vertex, Vertex, RGB) computes them (object.cuh:177-191): normalize(cross(p1 - p0,
 *              p2 - p0)), the two crosses with nor, 1 / dot, three multiplies -- one rounding per operation, the bits the parser
 *              produces on the host for the same vertices (a zero-area triangle gives NaN in both places)
 * Primitive counts and the order of the primitives do not change; materials, planes and lights are not touched (they have
 * update calls of their own, below, which need no build).
 * State: an update marks the scene NOT BUILT: until the next mirt_build_lbvh (issued on the same stream, or after the caller
 * has ordered it behind the update), mirt_render*, mirt_trace_rays, mirt_camera_rays, mirt_get_tree and mirt_get_records return MIRT_ERR_STATE.
 * Several updates may precede one build.  The build is the full one: the result is exactly the scene that mirt_scene_create +
 * mirt_build_lbvh give for the same values (the reference builds its tree from scratch; a refitted tree would be another tree).
 * count 0: MIRT_OK, nothing launched, the scene stays built.
 * Frames in flight: before it enqueues anything the call waits on the host for the last frame of every render context -- the
 * build that follows rewrites the records those frames read -- so a frame issued before the update finishes with the old
 * geometry.  Ray queries in flight on other streams use no render context: ordering them before an update is the caller's duty.
 * MIRT_ERR_ARG: null scene, negative first or count, a range beyond num_spheres / num_triangles, a null or misaligned pointer
 * with count > 0. */
int mirt_scene_update_spheres(MirtScene* sc, const void* d_spheres, int first, int count, void* stream);
int mirt_scene_update_triangles(MirtScene* sc, const void* d_verts, int first, int count, void* stream);
/* The inverse of the two update calls, device to device: spheres / triangles first .. first+count-1 of the scene's file-order
 * arrays into d_xyzr_out (float [count][4] = cx, cy, cz, r; 16-byte aligned) / d_verts_out (float [count][9] = p0, p1, p2; 4-byte
 * aligned), as mirt_scene_create or the last update left them.  One kernel, one lane per primitive, asynchronous on `stream`
 * (ordering it behind an update issued on another stream is the caller's duty).  Legal whether or not the scene is built, and
 * that state does not change; nothing but the arrays is read.  count 0: MIRT_OK, nothing launched.  MIRT_ERR_ARG as for the
 * updates: null scene, negative first or count, a range beyond num_spheres / num_triangles, a null or misaligned pointer with
 * count > 0. */
int mirt_scene_get_spheres(MirtScene* sc, int first, int count, void* d_xyzr_out, void* stream);
int mirt_scene_get_triangles(MirtScene* sc, int first, int count, void* d_verts_out, void* stream);

/* ---- shading values of a built scene in place: lights, planes, materials, bounces / gi / expose ------------- */
/* Every field of a scene file that the calls above leave fixed.  None of these values is in the record heap the tree is built
 * from, so no call here needs a mirt_build_lbvh: the scene STAYS BUILT (mirt_render*, mirt_trace_rays, mirt_camera_rays and
 * mirt_get_tree keep working, the tree keeps its bits), and the render workspaces, the random-number tables and the measured
 * hand-out order ("sched") stay, as across a camera change -- an order learned under other values can cost time, never a byte.
 * A scene changed in place renders, bit for bit and counter for counter, what a scene created afresh with the new values renders:
 * the facts the call plan is made from (is any material transparent or rough, is every colour finite) follow every call.
 * Not in the reference.  Callers detect the feature by these symbols (MIRT_VERSION stays 3).
 *
 * Common to mirt_scene_set_lights, mirt_scene_set_planes and the two material updates:
 *   Frames in flight read these device arrays: before it enqueues anything the call waits on the host for the last frame of
 *   every render context, so a frame issued before the call finishes with the old values.  (Ray queries read none of them.)
 *   The device writes are asynchronous on `stream`; host arrays passed in may be reused as soon as the call returns.  A render
 *   issued on ANOTHER stream must be ordered behind `stream` by the caller (a material update orders itself: see below).
 *   MIRT_ERR_ARG: null scene; negative first or count, or a range beyond the array; a null or misaligned pointer with count > 0.
 *
 * Lights.  MirtLight is MirtSun / MirtBulb under one name: v is a sun's direction or a bulb's position.  The COUNTS are those the
 * scene was created with and do not change; a light is switched off by a zero colour.  set: suns / bulbs are arrays of num_suns /
 * num_bulbs records, NULL = leave that kind as it is.  A sun's device record carries vec3::normalize of its direction and the
 * reciprocals, computed by the code mirt_scene_create uses.  get: what was set (or created), either pointer may be NULL. */
typedef struct MirtLight { MirtVec3 v; MirtRGB color; } MirtLight;         /* 24 B */
int mirt_scene_get_lights(const MirtScene* sc, MirtLight* suns_out, MirtLight* bulbs_out);
int mirt_scene_set_lights(MirtScene* sc, const MirtLight* suns, const MirtLight* bulbs, void* stream);
/* Planes first .. first+count-1, records taken as given, as mirt_scene_create takes them: nor and point are what is rendered (a, b,
 * c, d are carried along).  count 0: MIRT_OK, nothing done.  The number of planes does not change. */
int mirt_scene_get_planes(const MirtScene* sc, int first, int count, MirtPlane* out);
int mirt_scene_set_planes(MirtScene* sc, const MirtPlane* planes, int first, int count, void* stream);
/* The record the parser makes of a `plane a b c d` line (Plane(a, b, c, d, rgb), object.cuh:136-141) with material *mat: nor and
 * point by the parser's own routine, the same bits.  Host arithmetic, no device.  MIRT_ERR_ARG: a null pointer. */
int mirt_make_plane(const float abcd[4], const MirtMaterials* mat, MirtPlane* out);
/* bounces, gi, expose (+inf = exposure off), taken as given.  Exactly like the camera pair: host state only, no device work, no
 * synchronisation; applies to the calls issued afterwards, a frame already issued keeps the settings it was issued with.
 * MIRT_ERR_ARG: null scene or struct. */
typedef struct MirtShading { int32_t bounces, gi; float expose; } MirtShading;
int mirt_scene_get_shading(const MirtScene* sc, MirtShading* out);
int mirt_scene_set_shading(MirtScene* sc, const MirtShading* sh);
/* New materials from device memory (hipMalloc, or a torch data_ptr(), on the scene's device), like the geometry updates -- a scene
 * can hold millions.  d_mats: float [count][11] = colour rgb, shininess rgb, trans rgb, ior, roughness of spheres / triangles
 * first .. first+count-1 (file order): MirtMaterials' field order; 4-byte aligned; values taken as they are.  One kernel, one lane
 * per primitive, writes the three float4 the renderer reads (triangle i sits behind the spheres, at num_spheres + i) and one
 * byte of facts; a second kernel ORs the bytes of ALL primitives -- a partial update forgets no glass sphere outside its range,
 * and glass turned opaque takes the pending-children list away again -- into a word the host reads.  count 0: MIRT_OK, nothing
 * launched.  The first material update of a scene also allocates that byte per primitive and fills it from the device arrays.
 * ONE HOST WAIT per material update: the next mirt_render* on the scene (on any stream) waits, before it plans anything, for the
 * update's kernels to finish and reads the word; calls that do not render never wait.
 * The get calls are the device-to-device inverses (d_mats_out: float [count][11]); asynchronous on `stream`, they wait for
 * nothing. */
int mirt_scene_update_sphere_materials(MirtScene* sc, const void* d_mats, int first, int count, void* stream);
int mirt_scene_update_triangle_materials(MirtScene* sc, const void* d_mats, int first, int count, void* stream);
int mirt_scene_get_sphere_materials(MirtScene* sc, int first, int count, void* d_mats_out, void* stream);
int mirt_scene_get_triangle_materials(MirtScene* sc, int first, int count, void* d_mats_out, void* stream);

/* ---- temporal accumulation: the previous frame's samples, reused by reprojection --------------------- */
/* Not in the reference (every frame starts from nothing).  Callers detect the feature by these symbols (MIRT_VERSION stays 3).
 * Both calls are asynchronous on `stream`, take device pointers only, allocate nothing, never synchronise, use no atomics and
 * touch no render context, MirtStats counter or hand-out table.  Arithmetic as for mirt_denoise: float32, one IEEE rounding per
 * operation (no fused multiply-add), a + b + c = (a + b) + c, dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z, length(u) =
 * sqrtf(dot(u, u)), normalize as mirt_trace_rays normalises (vec3.cuh:72-82), cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z,
 * a.x b.y - a.y b.x) with each product rounded, then the difference; a vector times or divided by a scalar works per component.
 *
 * mirt_prev_features: where was the surface point each ray hits now, one frame ago?  n MirtRay rows, the n MirtHit rows a
 * closest-hit mirt_trace_rays answered for them on the scene as it is now (built: MIRT_ERR_STATE otherwise), and the geometry
 * before it moved: d_prev_xyzr (float [num_spheres][4], 16-byte aligned) and d_prev_verts (float [num_triangles][9], 4-byte
 * aligned), whole arrays in the update calls' format -- mirt_scene_get_spheres / mirt_scene_get_triangles taken before the
 * updates -- either may be NULL: that kind did not move.  -> n rows of mirt_hit_features' layout, (Px, Py, Pz, hit) (nx, ny, nz, 0),
 * two 16-byte stores each.  One lane per row.  With P = o + t * normalize(d) (the product rounded, then the sum) and n the record's
 * normal, exactly as mirt_hit_features computes them:
 *     kind == MIRT_HIT_NONE: eight zeros
 *     MIRT_HIT_SPHERE with d_prev_xyzr, MIRT_HIT_TRIANGLE with d_prev_verts: id >= the scene's count of that kind gives eight zeros
 *         (the hit tensor is the caller's memory); otherwise
 *       sphere id:   (c, r) = the scene's sphere, (c', r') = d_prev_xyzr[id]:  P' = c' + ((P - c) / r) * r';  n' = n
 *       triangle id: p0, nor, e1, e2 = the scene's 48-byte record (object.cuh:177-191), p0', p1', p2' = d_prev_verts[id]:
 *                    v = P - p0;  b1 = dot(e1, v);  b2 = dot(e2, v)   -- the reference's barycentrics, the coefficients of p1 - p0
 *                    and p2 - p0;  d1 = p1' - p0';  d2 = p2' - p0';  P' = (p0' + b1 * d1) + b2 * d2;
 *                    m = normalize(cross(d1, d2));  n' = dot(n, nor) < 0 ? -m : m   -- the query faces normals to the ray; the
 *                    previous normal keeps that choice
 *       row = (P', 1, n', 0)
 *     every other record (a plane, a kind whose previous array is NULL, an unknown kind): (P, 1, n, 0)
 * n == 0: MIRT_OK, nothing launched.  MIRT_ERR_ARG: null scene, n < 0, a null d_rays / d_hits / d_features with n > 0, a
 * misaligned buffer. */
int mirt_prev_features(MirtScene* sc, const void* d_rays, const void* d_hits, int64_t n, const void* d_prev_xyzr, const void* d_prev_verts,
                       void* d_features, void* stream);
/* mirt_temporal_accumulate: the frame p describes (width x height, row-major, N = width * height pixels; p->spp, stripe_rows and
 * flags are not used), on the current device.  This frame's moments S, Q (float4 per pixel), k (uint32 per pixel) as
 * mirt_render_accumulate_pixels leaves them; G = d_prev_features: mirt_prev_features of this frame's pixels' rays; the previous
 * merged frame S^h, Q^h, k^h = d_hist_*; F^h = d_hist_features: mirt_hit_features of that frame's rays; prev_camera: that frame's
 * camera.  -> d_out_*: moments of the same format holding this frame's samples plus the history that survives, so
 * mirt_denoise, mirt_select_pixels and mirt_finalize_counts take them as they are.  With eye, forward, right, up of prev_camera,
 * max_dim = fmaxf((float)width, (float)height), pixel p:
 *   1. No history -- out = (S_p, Q_p, k_p), bit for bit -- when G_p[3] == 0 (a miss), or f below is not finite or f <= 0, or no
 *      tap is valid.
 *   2. P' = G_p[0..2], n' = G_p[4..6];  v = P' - eye;  f = dot(v, forward) / dot(forward, forward);
 *      sx = dot(v, right) / dot(right, right) / f;  sy = dot(v, up) / dot(up, up) / f;
 *      x = (sx * max_dim + (float)width) / 2;  y = ((float)height - sy * max_dim) / 2
 *      -- the inverse of the pinhole ray forward + sx right + sy up with sx = (2 x - width) / max_dim, sy = (height - 2 y) /
 *      max_dim, in which integer coordinates are pixel centres -- exact for a mutually orthogonal forward / right / up;
 *      otherwise the position is approximate and step 4 rejects what lands wrong.
 *   3. Snap: |x - rintf(x)| <= 1/1024 gives x = rintf(x); y likewise.  x0 = floorf(x), tx = x - x0, y0, ty likewise.  Taps
 *      q = (x0 + i, y0 + j), j = 0, 1 (outer), i = 0, 1 (inner), weight w = wx_i * wy_j, wx = (1 - tx, tx), wy = (1 - ty, ty).
 *      A tap outside the frame or with w == 0 is dropped.
 *   4. A tap is valid when k^h_q > 0, S^h_q and Q^h_q are finite in r, g and b, F^h_q[3] != 0 (a hit), and a_n + a_p <= 1:
 *          c = 1 - dot(n', n_q);  a_n = (c < 0 ? 0 : c) / sigma_n
 *          D = P_q - P';  foot = length(v) * 2 / max_dim   -- one pixel's footprint at that distance
 *          a_p = fabsf(dot(n', D)) / (sigma_p * fmaxf(length(D), foot))
 *      -- mirt_denoise's a_n and a_p, but a displacement below a pixel's footprint is measured against the footprint: the
 *      rounding noise between a recomputed P' and a stored P_q is not a direction.  A NaN in either term makes the tap invalid.
 *   5. A valid tap with w == 1 (both axes snapped; the other taps had weight 0): S_h = S^h_q, Q_h = Q^h_q, k_h = k^h_q as they
 *      are.  Otherwise sw = the sum of w over the valid taps in tap order, and over the valid taps in tap order, from 0,
 *          m_ch = m_ch + (w / sw) * (S^h_q.ch / (float)k^h_q);  s_ch = s_ch + (w / sw) * (Q^h_q.ch / (float)k^h_q)   (r, g, b, a)
 *      k_h = the smallest k^h_q of the valid taps;  S_h = m * (float)k_h;  Q_h = s * (float)k_h.
 *   6. Cap: k_h > max_history:  c = (float)max_history / (float)k_h;  S_h = S_h * c;  Q_h = Q_h * c;  k_h = max_history.
 *   7. out = (S_p + S_h, Q_p + Q_h, k_p + k_h), all four channels.
 * A lane reads S_p, Q_p, k_p at its own pixel only and before it writes: each output may be EXACTLY its own current-frame buffer
 * (d_out_accum_f32 == d_accum_f32, ...).  Every pixel depends on its inputs only: the result does not depend on timing.
 * MIRT_ERR_ARG (all checked on the host, before any device work): a null pointer; p->num_parts != 1 (whole frames only);
 * prev_camera not a pinhole (fisheye, panorama or dof_focus not 0); max_history < 1; sigma_n or sigma_p not finite and
 * positive (the drivers use MIRT_DENOISE_SIGMA_N and MIRT_DENOISE_SIGMA_P: no new constant); a misaligned buffer (16 bytes;
 * counts 4); an output range (16 N, 16 N, 4 N bytes) overlapping another output, d_prev_features or a history buffer (32 N, 16 N,
 * 16 N, 4 N, 32 N), or a current-frame buffer in any way but the one allowed above. */
int mirt_temporal_accumulate(const MirtRenderParams* p, const MirtCamera* prev_camera, const void* d_accum_f32, const void* d_accum_sq_f32,
                             const uint32_t* d_counts, const void* d_prev_features, const void* d_hist_accum_f32, const void* d_hist_accum_sq_f32,
                             const uint32_t* d_hist_counts, const void* d_hist_features, int max_history, float sigma_n, float sigma_p,
                             void* d_out_accum_f32, void* d_out_accum_sq_f32, uint32_t* d_out_counts, void* stream);

/* ---- several GPUs in one process --------------------------------------------------------------- */
/* Not in the reference (single GPU, main.cu:25-94).  The scene is uploaded to every listed device and every device builds
 * the identical LBVH; a frame is cut into interleaved stripes of `stripe_rows` rows, device r renders part r (a
 * MirtRenderParams with num_parts = ngpu, part = r), the parts are gathered to the first device with one grouped RCCL
 * send/recv exchange over xGMI and re-interleaved there.  Any partition gives the bytes of the single-GPU frame (samples are
 * seeded by global pixel and sample index, draw.cu:162).  RCCL is loaded at run time, and only for ngpu > 1. */
#define MIRT_MULTI_MAX_GPUS 16
typedef struct MirtMulti MirtMulti;
typedef struct MirtMultiStats {
  int32_t num_gpus;
  float build_ms;                          /* slowest device's LBVH build */
  float render_ms[MIRT_MULTI_MAX_GPUS];    /* device time of each part's render (HIP events on its stream) */
  float gather_ms;                         /* end of device 0's render -> frame re-interleaved on device 0 (includes waiting for the slowest peer) */
  float frame_ms;                          /* host wall clock of the call, host copy included */
} MirtMultiStats;
/* devices: ngpu device indices, or NULL for 0..ngpu-1.  Uploads and builds synchronously, all devices at once (one host thread
 * each).  MIRT_MULTI_GATHER=copy in the environment: peer-to-peer copies instead of RCCL, and a device may be listed more than
 * once -- or, with devices == NULL, ngpu may exceed the GPUs present (part r on GPU r mod their number): parts time-sharing a
 * GPU, a rehearsal of the N > 1 path on a small box, never a scaling measurement. */
int mirt_multi_create(const MirtSceneDesc* desc, int ngpu, const int* devices, MirtMulti** out);
void mirt_multi_destroy(MirtMulti* mm);
int mirt_multi_num_parts(const MirtMulti* mm);
int mirt_multi_set_option(MirtMulti* mm, const char* name, int value);      /* mirt_scene_set_option on every device's scene */
int mirt_multi_set_camera(MirtMulti* mm, const MirtCamera* cam);            /* mirt_scene_set_camera on every device's scene: frames submitted afterwards */
/* mirt_scene_set_lights / set_planes / set_shading on every device's scene, for the frames submitted afterwards (frames in
 * flight keep their values; the call returns once every device holds the new records).  Material updates take device memory on
 * every device and are not offered for a MirtMulti. */
int mirt_multi_set_lights(MirtMulti* mm, const MirtLight* suns, const MirtLight* bulbs);
int mirt_multi_set_planes(MirtMulti* mm, const MirtPlane* planes, int first, int count);
int mirt_multi_set_shading(MirtMulti* mm, const MirtShading* sh);
/* Frames in flight: mirt_multi_submit issues one width x height frame at spp samples per pixel on every device and returns at
 * once with a ticket; mirt_multi_wait blocks until that frame is gathered (and copied to host_rgba, nullable, which must stay
 * valid until then).  Up to MIRT_MULTI_MAX_IN_FLIGHT frames may be in flight: consecutive frames overlap on every device (the
 * next frame's waves take the slots the draining frame frees), the gathers run in submission order.  mirt_multi_wait returns
 * MIRT_ERR_STATE when a capacity overflowed on any device (checked whenever no other frame is in flight; MirtStats.overflow_events). */
#define MIRT_MULTI_MAX_IN_FLIGHT 4
int mirt_multi_submit(MirtMulti* mm, int width, int height, int spp, int stripe_rows, uint8_t* host_rgba, uint64_t* ticket);
int mirt_multi_wait(MirtMulti* mm, uint64_t ticket, MirtMultiStats* stats);
/* One frame, synchronously (submit + wait). */
int mirt_render_frame_multi(MirtMulti* mm, int width, int height, int spp, int stripe_rows, uint8_t* host_rgba, MirtMultiStats* stats);
/* nframes frames back to back with `in_flight` of them in flight; host_rgba_last / last_stats (nullable) receive the last frame;
 * ms_per_frame: host wall clock of the call / nframes. */
int mirt_render_frames_multi(MirtMulti* mm, int width, int height, int spp, int stripe_rows, int nframes, int in_flight, uint8_t* host_rgba_last,
                             MirtMultiStats* last_stats, float* ms_per_frame);
/* mirt_get_stats of device `part`'s scene (waits for its frames in flight). */
struct MirtStats;
int mirt_multi_get_stats(MirtMulti* mm, int part, struct MirtStats* out);

typedef struct MirtStats {
  /* filled by a render with MIRT_RENDER_COUNTERS */
  uint64_t samples, rays, shadow_rays, internal_visits, sphere_tests, tri_tests, mat_fetches, max_stack;
  /* capacity overflows of the frames finished since the previous call: a full pending-ray list (refraction / GI children).
   * Always counted; when non-zero mirt_get_stats fills the struct and returns MIRT_ERR_STATE -- the image is not
   * trustworthy.  (The reference's other capacity, its 64-entry traversal stack -- bvh_traversal.cu:8,154-164 prints a
   * warning and drops the subtree -- cannot overflow: the tree is at most 58 levels deep) */
  uint64_t overflow_events;
  /* device time of the last render's trace kernel and of the whole render call, HIP events, ms */
  float trace_kernel_ms, render_ms;
  float build_ms;
  int32_t num_nodes;
  /* mean trace-kernel time over the frames finished since the previous mirt_get_stats call, and their number */
  float trace_kernel_ms_mean;
  int32_t frames_timed;
  /* (version 3) launches of the trace kernel in the last render call (one per slab of at most 2^slab_log2 samples);
   * trace_kernel_ms is the SUM of their durations (one HIP event pair per launch), not a bracket around them */
  int32_t trace_launches;
  /* bytes of one internal-node record of the walk the last render used: 64 (exact boxes, two children per record; also the wide
   * quantised records: four grandchildren per record) or 32 (quantised records of a sphere-only scene) */
  int32_t node_record_bytes;
  /* with MIRT_RENDER_COUNTERS: rays that entered the BVH walk (`rays` counts the reference's hitNearest calls: a shadow ray towards
   * a light the surface faces away from, or one an infinite plane already blocks, is answered without a walk) */
  uint64_t rays_traversed;
} MirtStats;
/* Waits for every frame in flight, then reports (and resets the running mean).  mirt_render / mirt_render_accumulate never
 * report a capacity overflow themselves (they are asynchronous): poll this call after a render, or before using its image.  Up to four frames may be in flight on
 * different streams: a scene keeps four sets of render workspaces and reuses one only when its frame has finished. */
int mirt_get_stats(MirtScene* sc, MirtStats* out);

/* ---- introspection for parity tests ----------------------------------------------------------- */
typedef struct MirtTreeNode {      /* the reference's LBVHNode (lbvh.cuh:6-28), flattened */
  float xmin, xmax, ymin, ymax, zmin, zmax;
  uint32_t left, right, prim_offset, count;
} MirtTreeNode;
/* Copies the tree back in the reference's numbering: internal nodes [0,N-2], leaves [N-1,2N-2].
 * nodes: 2N-1 entries; codes: N sorted Morton codes; refs: N sorted primitive references;
 * bounds: 6 floats (min xyz, max xyz).  Any pointer may be NULL. */
int mirt_get_tree(MirtScene* sc, MirtTreeNode* nodes, uint32_t* codes, MirtPrimRef* refs, float* bounds);

/* What the traversal kernels read from a built scene, copied back word for word (mirt_get_tree returns what they do NOT read).
 * The counts say how many elements of each region the scene has -- 0 for a region it was built without -- and the rest is what
 * decodes a child reference and what the host decided from the tree:
 *   num_nodes      64-byte exact records: both child boxes as (min, max) pairs per axis (12 floats), the two child references,
 *                  the descent-order bits, one unused word.  N - 1 of them.
 *   num_qnodes     32-byte quantised records of a sphere-only scene: words 0..2 child 0 (min | max << 16 per axis, in grid steps
 *                  from qparams[0..2]), words 3..5 child 1, words 6, 7 the child references.  N - 1, or 0.
 *   num_wnodes     64-byte wide records of a scene with triangles: up to four grandchild boxes of three such words (words 0..11)
 *                  and their references (words 12..15).  N - 1, or 0.
 *   prim_units     16-byte units of the primitive region, in sorted (Morton) order: a sphere is one unit (cx, cy, cz, r), a
 *                  triangle three (p0.xyz nor.x | nor.yz e1.xy | e1.z e2.xyz); unit_prim has one word per unit
 *                  (type << 31 | index in the scene's sphere / triangle array).  Ns + 3 Nt.
 *   num_tris_before  N + 1 (0 for an empty scene): triangles among the sorted leaves [0, j).
 *   num_tri_boxes  Nt records of 8 floats, scene order: (xmin, xmax, ymin, ymax) (zmin, zmax, 0, 0), a triangle's exact leaf box.
 *   num_qparams    9 when quantised or wide records were built (grid origin xyz, grid step xyz, 2^60 / grid step xyz), else 0.
 * A reference is bit 31 leaf | bit 30 triangle | bits 0..27 the record's offset in 16-byte units from the start of the exact
 * records: node i of the exact records is 4 i, of the quantised ones qnode_base16 + 2 i, of the wide ones wnode_base16 + 4 i, the
 * primitive of sorted leaf j prim_base16 + j + 2 tris_before[j].  0xf0000000 is "no record": root_ref_q / root_ref_w of a scene
 * without those records. */
typedef struct MirtRecordInfo {
  uint32_t num_nodes, num_qnodes, num_wnodes, prim_units, num_tris_before, num_tri_boxes, num_qparams;
  uint32_t prim_base16, qnode_base16, wnode_base16;
  uint32_t root_ref, root_ref_q, root_ref_w;
  int32_t grid_ok;       /* the grid resolves the scene's coordinates: the quantised / wide records may be walked */
  int32_t tree_depth;    /* the most internal nodes on a root-to-leaf path */
  float coord_max;       /* largest |coordinate| of the root's two child boxes */
} MirtRecordInfo;
/* Host-synchronous, like mirt_get_tree, and with its errors.  Every output pointer is a host array sized for the counts above
 * (which follow from the scene's N, Ns and Nt: size for N - 1 records of each kind); any of them may be NULL. */
int mirt_get_records(MirtScene* sc, MirtRecordInfo* info, void* nodes, void* qnodes, void* wnodes, void* prims, uint32_t* unit_prim,
                     uint32_t* tris_before, float* tri_boxes, float* qparams);

/* Device-side probes of the arithmetic the kernels use (which: 0 logf 1 expf 2 sinf 3 cosf 4 pow(x,1/2.4)
 * 5 RGBtosRGB 6 sqrtf 7 1/x), and of the XORWOW generator. */
int mirt_probe_math(int device, int which, int n, const float* host_in, float* host_out);
/* Stream i of num_streams is seeded exactly as the trace kernel seeds it: spp > 1: pixel i / spp, sample i % spp
 * (curand_init(1234 + pixel, sample, 0), draw.cu:162); spp <= 1: pixel i (curand_init(1234, pixel, 0), draw.cu:105).
 * host_out[i * draws + k] is the k-th raw 32-bit output. */
int mirt_probe_xorwow(int device, int spp, int num_streams, int draws, uint32_t* host_out);
/* The box test of the quantised walk, one device thread per case, through the functions the builder and the trace kernels call
 * (not a restatement of them).  host_in, 20 floats per case: scene bounds smin[3], smax[3]; a box lo[3], hi[3]; a ray origin o[3]
 * and direction d[3] (taken as given, not normalised); tbest; one unused float.  The thread computes the grid step and
 * 2^60 / step of the bounds and the box's six grid coordinates as the builder does, 1 / d and the ray's three grid axes as the start of a
 * ray does, and then tests the box with tmin = 1e-4 in four forms: the exact box in a 64-byte record, the packed box as the left
 * child of a 32-byte record, as its right child (the other child being some other box), and as one box of a wide record.
 * host_out, 20 words per case: [0..2] the grid coordinates of lo, [3..5] of hi (a record packs them min | max << 16 per axis); [6..9] 1 where the form reports
 * a hit, in the order above; [10..12] the entry parameter of the first three forms (float bits; the wide form returns none);
 * [13] zero; [14..16] the grid step, [17..19] 2^60 / step (float bits). */
int mirt_probe_qbox(int device, int n, const float* host_in, uint32_t* host_out);
/* The radix-sort kernels on n keys of the caller's choosing (callers detect this call and the two below by their symbols;
 * MIRT_VERSION stays 3).  mode 0: the sort of a build -- four stable passes over all 32 bits, the values being the positions
 * 0..n-1 -- through the function mirt_build_lbvh calls.  mode 1: the one stable pass over the low byte that orders a frame's samples
 * by cost class, as the render calls it.  host_keys_out receives the whole keys in sorted order, host_vals_out where each stood in
 * host_keys: the stable argsort of the keys (mode 0) or of their low bytes (mode 1).  Host-synchronous; n <= 0, another mode or
 * a NULL pointer is MIRT_ERR_ARG. */
int mirt_probe_sort(int device, int mode, int n, const uint32_t* host_keys, uint32_t* host_keys_out, uint32_t* host_vals_out);
/* What the hand-out orders are made from.  which 0: host_out[i] = the cost key of a sample that took host_in[i] traversal steps
 * (255 for none, else 255 - 4 floor(log2 s) - the two bits below the leading one), through the device function the trace kernels
 * call.  which 1: host_in holds n chunk costs, host_out receives the chunk order of scene option "sched" = 1 -- a permutation of 0..n-1
 * by cost bin, most expensive bin first (bin = 1023 - cost / 8, costs of 8192 and more in bin 0), made by the kernel and the launch
 * shape the render uses.  Host-synchronous; n <= 0, another `which` or a NULL pointer is MIRT_ERR_ARG. */
int mirt_probe_sched(int device, int which, int n, const uint32_t* host_in, uint32_t* host_out);
/* The by-sample hand-out table of scene option "sched" = 2, as the next call of the measured shape reads it.  total_samples: the samples
 * of the call that measured it, the length of `order`; every launch of that call owns a consecutive segment of `order`, a permutation
 * of the launch's own sample indices (position k of the hand-out -> sample), most expensive cost class first, frame order within a class.
 * last_launch_samples: the samples of that call's last launch, the length of `keys` (its samples' cost keys, by sample) and of
 * `sorted_keys` (the same keys in hand-out order).  Host-synchronous: a measurement in flight is waited for.  Any output pointer
 * may be NULL (ask for `info` first to size the others).  MIRT_ERR_STATE when no call has measured a table on this scene; the table
 * outlives camera, geometry and shading updates, like the hand-out itself. */
typedef struct MirtSampleOrderInfo { int64_t total_samples, last_launch_samples; } MirtSampleOrderInfo;
int mirt_get_sample_order(MirtScene* sc, MirtSampleOrderInfo* info, uint32_t* order, uint32_t* keys, uint32_t* sorted_keys);

/* ---- output ----------------------------------------------------------------------------------- */
/* Image::save, libpng.cpp:73-107: 8-bit RGBA, non-interlaced PNG (own encoder; zlib only). */
int mirt_write_png(const char* path, const uint8_t* rgba, int width, int height);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_H */
