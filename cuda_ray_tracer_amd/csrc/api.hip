// C ABI glue for the device side of libmirt.so (include/mirt.h): scene upload, build, render, stats.
#include "scene_dev.h"
#include "host_scene.h"
#include "material_flags.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

using namespace mirt;

int mirt::hip_fail(hipError_t e, const char* what, const char* file, int line)
{
  char buf[512];
  snprintf(buf, sizeof(buf), "HIP error in %s at line %d: %s (%s)", file, line, hipGetErrorString(e), what);
  set_error(buf);
  return MIRT_ERR_HIP;
}

namespace {

template <typename T>
int upload(DevBuf<T>& dst, const std::vector<T>& src)
{
  if (src.empty()) return MIRT_OK;
  const int rc = dst.alloc(src.size(), "upload");
  if (rc != MIRT_OK) return rc;
  MIRT_HIP(hipMemcpy(dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
  return MIRT_OK;
}

// a primitive's material: its three float4 on the device, its facts (material_flags.h) into the scene's
void take_mat(MirtScene* sc, const MirtMaterials& mat, float4* out)
{
  float m[11];
  static_assert(sizeof(MirtMaterials) == sizeof(m), "MirtMaterials is 11 floats");
  memcpy(m, &mat, sizeof(m));
  pack_mat(m, out);
  sc->prim_flags |= material_flags(m);
}

// mode: the option selects what is computed or visited (another tree, another walk, another render path) -- as opposed to a
// tuning value, which only moves time
struct OptionDesc { const char* name; int Options::*field; int lo, hi; bool mode; };
const OptionDesc OPTIONS[] = {
  {"bounds_as_shipped", &Options::bounds_as_shipped, 0, 1, true},
  {"traversal", &Options::traversal, 0, 2, true}, {"wavefront", &Options::wavefront, 0, 1, true},
  {"qnodes", &Options::qnodes, 0, 2, true}, {"shadow_anyhit", &Options::shadow_anyhit, 0, 1, true}, {"skip_unlit", &Options::skip_unlit, 0, 1, true},
  {"stack_lds_depth", &Options::stack_lds_depth, -1, 64, false}, {"refill_k", &Options::refill_k, 0, 64, false}, {"batch_k", &Options::batch_k, 0, 64, false},
  {"leaf_k", &Options::leaf_k, 0, 64, false}, {"init_k", &Options::init_k, 0, 64, false}, {"reps", &Options::reps, 0, 8, false}, {"drain_lanes", &Options::drain_lanes, 0, 64, false},
  {"chunk_shift", &Options::chunk_shift, 0, 12, false}, {"trace_waves", &Options::trace_waves, 0, 1 << 20, false}, {"sched", &Options::sched, 0, 2, false},
  {"specialise", &Options::specialise, 0, 1, false}, {"ray_start_lds", &Options::ray_start_lds, 0, 1, false}, {"slab_log2", &Options::slab_log2, 8, 30, false},
  {"wf_pool", &Options::wf_pool, 256, 1 << 24, false}, {"wf_refill_k", &Options::wf_refill_k, 1, 64, false},
};

// MIRT_<NAME> (upper case) overrides an option's default; read once per scene, here.  Only the tuning values: a mode switch
// (traversal = 2 changes pixels on triangle silhouettes) is set through mirt_scene_set_option, or from the environment when
// MIRT_ALLOW_ENV=1 says that is meant (tools/ sweeps) -- a variable left over in a shell must not change an image.
void options_from_env(Options& o)
{
  const char* allow = getenv("MIRT_ALLOW_ENV");
  const bool modes = allow && atoi(allow) != 0;
  for (const OptionDesc& d : OPTIONS) {
    if (d.mode && !modes) continue;
    std::string env = "MIRT_";
    for (const char* c = d.name; *c; ++c) env += (char)toupper(*c);
    if (const char* e = getenv(env.c_str())) { const long v = atol(e); if (v >= d.lo && v <= d.hi) o.*(d.field) = (int)v; }
  }
}

int scene_create(const MirtSceneDesc* d, int device, MirtScene** out);

// the prologue of an entry point that works on a scene's device: "<who>: null scene", then the device made current
int enter_scene(const MirtScene* sc, const char* who)
{
  if (!sc) { set_error(std::string(who) + ": null scene"); return MIRT_ERR_ARG; }
  MIRT_HIP(hipSetDevice(sc->device));
  return MIRT_OK;
}

// mirt_get_stats: take a context's overflow count and zero it in one atomic step (a frame issued meanwhile from another host
// thread keeps every increment: it lands either in this reading or in the next)
__global__ void take_overflow_kernel(unsigned long long* counters)
{
  counters[10] = atomicExch(&counters[9], 0ull);
}

} // namespace

extern "C" {

int mirt_scene_set_option(MirtScene* sc, const char* name, int value)
{
  if (!sc || !name) { set_error("mirt_scene_set_option: null argument"); return MIRT_ERR_ARG; }
  for (const OptionDesc& d : OPTIONS)
    if (strcmp(d.name, name) == 0) {
      if (value < d.lo || value > d.hi) { set_error(std::string("mirt_scene_set_option: value out of range for ") + name); return MIRT_ERR_ARG; }
      sc->opt.*(d.field) = value;
      return MIRT_OK;
    }
  set_error(std::string("mirt_scene_set_option: unknown option ") + name);
  return MIRT_ERR_ARG;
}

int mirt_scene_get_option(const MirtScene* sc, const char* name, int* value)
{
  if (!sc || !name || !value) { set_error("mirt_scene_get_option: null argument"); return MIRT_ERR_ARG; }
  for (const OptionDesc& d : OPTIONS)
    if (strcmp(d.name, name) == 0) { *value = sc->opt.*(d.field); return MIRT_OK; }
  // read-only facts about the traversal stack (mirt.h): the built tree's depth, and which kernel the last render's plan chose
  if (strcmp(name, "tree_depth") == 0) { *value = sc->built ? sc->tree_depth : -1; return MIRT_OK; }
  if (strcmp(name, "stack_lds_capacity") == 0) { *value = STACK_LDS_CAPACITY; return MIRT_OK; }
  if (strcmp(name, "stack_lds_only") == 0) { *value = sc->last_lds_only ? 1 : 0; return MIRT_OK; }
  if (strcmp(name, "stack_lds_slots") == 0) { *value = sc->last_stack_slots; return MIRT_OK; }
  // ... and about the scene's rays: primitive tests per internal-node visit as the plan of the next render would read it, the
  // bits of a float (negative: not known).  What the scene holds, nothing polled: a finished measurement is taken by the next
  // render call or by mirt_get_sample_order, not here
  if (strcmp(name, "prim_ratio_bits") == 0) { static_assert(sizeof(float) == sizeof(int), "float bits in an int"); memcpy(value, &sc->so_ratio, sizeof(float)); return MIRT_OK; }
  set_error(std::string("mirt_scene_get_option: unknown option ") + name);
  return MIRT_ERR_ARG;
}

int mirt_scene_create(const MirtSceneDesc* d, int device, MirtScene** out)
{
  // nothing may unwind across the C boundary (std::bad_alloc from the host-side staging vectors of a huge scene)
  try {
    return scene_create(d, device, out);
  } catch (const std::bad_alloc&) {
    set_error("mirt_scene_create: out of host memory");
    return MIRT_ERR_ARG;
  }
}

} // extern "C"

namespace {

int scene_create(const MirtSceneDesc* d, int device, MirtScene** out)
{
  if (!d || !out) { set_error("mirt_scene_create: null argument"); return MIRT_ERR_ARG; }
  *out = nullptr;
  if (d->num_spheres < 0 || d->num_triangles < 0 || d->num_prims < 0 || d->num_planes < 0 || d->num_suns < 0 || d->num_bulbs < 0) {
    set_error("mirt_scene_create: negative count"); return MIRT_ERR_ARG;
  }
  if ((d->num_spheres > 0 && !d->spheres) || (d->num_triangles > 0 && !d->triangles) || (d->num_prims > 0 && !d->prim_refs) ||
      (d->num_planes > 0 && !d->planes) || (d->num_suns > 0 && !d->suns) || (d->num_bulbs > 0 && !d->bulbs)) {
    set_error("mirt_scene_create: a count is positive but its array is null"); return MIRT_ERR_ARG;
  }
  if ((long long)d->num_spheres + d->num_triangles != d->num_prims) { set_error("mirt_scene_create: num_prims != num_spheres + num_triangles"); return MIRT_ERR_ARG; }
  if (d->num_suns + d->num_bulbs > 64) { set_error("mirt_scene_create: more than 64 lights are not supported"); return MIRT_ERR_ARG; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_error("mirt_scene_create: no HIP device available (libmirt has no CPU path)");
    return MIRT_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) { set_error("mirt_scene_create: bad device index"); return MIRT_ERR_ARG; }
  MIRT_HIP(hipSetDevice(device));

  std::unique_ptr<MirtScene> owner(new MirtScene());      // until the scene is handed out, a return gives back whatever it holds by then
  MirtScene* const sc = owner.get();
  sc->device = device;
  options_from_env(sc->opt);
  sc->d = *d;
  sc->N = d->num_prims; sc->Ns = d->num_spheres; sc->Nt = d->num_triangles;
  const int N = sc->N;

  // de-interleave the AoS inputs into the device layout (config_utils.cu:72-199 does the same job for the reference)
  std::vector<float4> spheres((size_t)sc->Ns), tris(3 * (size_t)sc->Nt), verts(3 * (size_t)sc->Nt), mats(3 * (size_t)N);
  for (int i = 0; i < sc->Ns; ++i) {
    const MirtSphere& s = d->spheres[i];
    spheres[i] = make_float4(s.c.x, s.c.y, s.c.z, s.r);
    take_mat(sc, s.mat, &mats[3 * (size_t)i]);
  }
  for (int i = 0; i < sc->Nt; ++i) {
    const MirtTriangle& t = d->triangles[i];
    tris[3 * (size_t)i + 0] = make_float4(t.p0.x, t.p0.y, t.p0.z, t.nor.x);
    tris[3 * (size_t)i + 1] = make_float4(t.nor.y, t.nor.z, t.e1.x, t.e1.y);
    tris[3 * (size_t)i + 2] = make_float4(t.e1.z, t.e2.x, t.e2.y, t.e2.z);
    verts[3 * (size_t)i + 0] = make_float4(t.p0.x, t.p0.y, t.p0.z, 0.0f);
    verts[3 * (size_t)i + 1] = make_float4(t.p1.x, t.p1.y, t.p1.z, 0.0f);
    verts[3 * (size_t)i + 2] = make_float4(t.p2.x, t.p2.y, t.p2.z, 0.0f);
    take_mat(sc, t.mat, &mats[3 * ((size_t)sc->Ns + i)]);
  }
  std::vector<MirtPrimRef> refs(d->prim_refs, d->prim_refs + N);
  for (int i = 0; i < N; ++i) {
    const MirtPrimRef& r = refs[i];
    if (r.type > 1 || (r.type == 0 && (int)r.id >= sc->Ns) || (r.type == 1 && (int)r.id >= sc->Nt)) {
      set_error("mirt_scene_create: primitive reference out of range"); return MIRT_ERR_ARG;
    }
  }
  // planes and lights: the host keeps what it was given (mirt_scene_get_planes / _get_lights, and the facts they contribute)
  sc->planes_host.assign(d->planes, d->planes + d->num_planes);
  sc->suns_host.resize((size_t)d->num_suns); sc->bulbs_host.resize((size_t)d->num_bulbs);
  for (int i = 0; i < d->num_suns; ++i) sc->suns_host[i] = {d->suns[i].dir, d->suns[i].color};
  for (int i = 0; i < d->num_bulbs; ++i) sc->bulbs_host[i] = {d->bulbs[i].point, d->bulbs[i].color};
  std::vector<PlaneDev> planes((size_t)d->num_planes);
  for (int i = 0; i < d->num_planes; ++i) planes[i] = plane_dev(d->planes[i]);
  std::vector<LightDev> suns((size_t)d->num_suns), bulbs((size_t)d->num_bulbs);
  for (int i = 0; i < d->num_suns; ++i) suns[i] = sun_dev(sc->suns_host[i]);
  for (int i = 0; i < d->num_bulbs; ++i) bulbs[i] = bulb_dev(sc->bulbs_host[i]);
  refresh_host_facts(sc);
  sc->d.spheres = nullptr; sc->d.triangles = nullptr; sc->d.prim_refs = nullptr; sc->d.planes = nullptr; sc->d.suns = nullptr; sc->d.bulbs = nullptr;

  // record heap: [internal nodes 64 B each | primitive records in sorted order: sphere 16 B, triangle 48 B | 64 B pad] -- the
  // traversal kernel addresses any record with one 32-bit byte offset.  The build fills it (lbvh_build.hip).
  {
    const size_t nodes_bytes = N > 1 ? 64 * (size_t)(N - 1) : 0;
    const size_t sph_bytes = 16 * (size_t)sc->Ns, tri_bytes = 48 * (size_t)sc->Nt;
    // (quantised node records behind the primitives, scene_dev.h: 32-byte ones for a sphere-only scene, else the wide ones)
    const size_t qnode_bytes = (sc->Nt == 0 && N > 1) ? 32 * (size_t)(N - 1) : 0;
    const size_t wnode_bytes = (sc->Nt > 0 && N > 1) ? 64 * (size_t)(N - 1) + 128 : 0;      // wide records (scene_dev.h), line-aligned
    const size_t total = nodes_bytes + sph_bytes + tri_bytes + 64 + qnode_bytes + wnode_bytes;
    if (total > 0xfffffff0ull) { set_error("mirt_scene_create: scene too large for 32-bit record offsets"); return MIRT_ERR_ARG; }
    MIRT_TRY(sc->heap.alloc(total, "heap"));
    MIRT_HIP(hipMemset(sc->heap, 0, total));
    sc->prim_base = (uint32_t)nodes_bytes;
    sc->qnode_base = qnode_bytes ? (uint32_t)(nodes_bytes + sph_bytes + tri_bytes + 64) : 0u;
    sc->wnode_base = wnode_bytes ? (uint32_t)((nodes_bytes + sph_bytes + tri_bytes + 64 + qnode_bytes + 127) / 128 * 128) : 0u;
    sc->nodes = reinterpret_cast<float4*>(sc->heap.get());
  }
  MIRT_TRY(upload(sc->spheres, spheres)); MIRT_TRY(upload(sc->tris, tris));
  MIRT_TRY(upload(sc->tri_verts, verts)); MIRT_TRY(upload(sc->mats, mats));
  MIRT_TRY(upload(sc->refs_in, refs)); MIRT_TRY(upload(sc->planes, planes)); MIRT_TRY(upload(sc->suns, suns)); MIRT_TRY(upload(sc->bulbs, bulbs));
  if (N > 0) {
    const size_t n = (size_t)N;
    MIRT_TRY(sc->codes.alloc(n, "codes")); MIRT_TRY(sc->order.alloc(n, "order"));
    MIRT_TRY(sc->parent.alloc(2 * n - 1, "parent")); MIRT_TRY(sc->boxes.alloc(6 * (2 * n - 1), "boxes"));
    if (N > 1) { MIRT_TRY(sc->child_l.alloc(n - 1, "child_l")); MIRT_TRY(sc->child_r.alloc(n - 1, "child_r")); MIRT_TRY(sc->range.alloc(n - 1, "range")); }
    MIRT_TRY(sc->unit_prim.alloc((size_t)sc->Ns + 3 * (size_t)sc->Nt, "unit_prim"));
    MIRT_TRY(sc->tris_before.alloc(n + 1, "tris_before"));
  }
  MIRT_TRY(sc->bounds_keys.alloc(6, "bounds_keys"));
  MIRT_TRY(sc->depth_dev.alloc(1, "depth_dev"));
  MIRT_TRY(sc->qparams.alloc(9, "qparams"));
  MIRT_TRY(sc->tri_boxes.alloc(2 * (size_t)sc->Nt, "tri_boxes"));
  for (RenderCtx& c : sc->ctx) {
    MIRT_TRY(c.counters.alloc(16, "counters"));
    MIRT_HIP(hipMemset(c.counters, 0, 16 * sizeof(unsigned long long)));
  }
  // (created here, not on first use: a context that has never rendered or sorted is still asked about its events)
  MIRT_TRY(sc->ev0.create()); MIRT_TRY(sc->ev1.create()); MIRT_TRY(sc->so_ev.create());
  for (RenderCtx& c : sc->ctx) {
    MIRT_TRY(c.ev0.create()); MIRT_TRY(c.ev1.create()); MIRT_TRY(c.ev2.create()); MIRT_TRY(c.ev3.create()); MIRT_TRY(c.order_ev.create());
  }
  *out = owner.release();
  return MIRT_OK;
}

} // namespace

extern "C" {

void mirt_scene_destroy(MirtScene* sc)
{
  if (!sc) return;
  hipSetDevice(sc->device);
  hipDeviceSynchronize();
  delete sc;
}

int mirt_build_lbvh(MirtScene* sc, void* stream, float* build_ms)
{
  MIRT_TRY(enter_scene(sc, "mirt_build_lbvh"));
  int rc = build_lbvh(sc, (hipStream_t)stream);
  if (rc == MIRT_OK) sc->updated = false;
  if (rc == MIRT_OK && build_ms) *build_ms = sc->build_ms;
  return rc;
}

int64_t mirt_render_num_pixels(const MirtRenderParams* p) { return p ? render_num_pixels(p) : -1; }

int mirt_part_pixel_xy(const MirtRenderParams* p, int64_t local, int32_t* x, int32_t* y)
{
  if (!p) { set_error("mirt_part_pixel_xy: null argument"); return MIRT_ERR_ARG; }
  return part_pixel(p, local, x, y);
}

int mirt_render(MirtScene* sc, const MirtRenderParams* p, void* d_rgba8, void* d_rgba_f32, void* stream)
{
  if (!sc || !p) { set_error("mirt_render: null argument"); return MIRT_ERR_ARG; }
  MIRT_HIP(hipSetDevice(sc->device));
  return render(sc, p, d_rgba8, d_rgba_f32, (hipStream_t)stream);
}

int mirt_render_accumulate(MirtScene* sc, const MirtRenderParams* p, void* d_accum_f32, int sample_first, int sample_count, void* stream)
{
  if (!sc || !p) { set_error("mirt_render_accumulate: null argument"); return MIRT_ERR_ARG; }
  MIRT_HIP(hipSetDevice(sc->device));
  return render_accumulate(sc, p, d_accum_f32, sample_first, sample_count, (hipStream_t)stream);
}

int mirt_finalize(const MirtRenderParams* p, const void* d_accum_f32, int total_samples, void* d_rgba8, void* stream)
{
  if (!p) { set_error("mirt_finalize: null argument"); return MIRT_ERR_ARG; }
  return finalize(p, d_accum_f32, total_samples, d_rgba8, (hipStream_t)stream);
}

int mirt_render_accumulate_pixels(MirtScene* sc, const MirtRenderParams* p, const uint32_t* d_pixels, int64_t num_listed, void* d_accum_f32,
                                  void* d_accum_sq_f32, uint32_t* d_counts, int sample_first, int sample_count, void* stream)
{
  if (!sc || !p) { set_error("mirt_render_accumulate_pixels: null argument"); return MIRT_ERR_ARG; }
  if (!d_pixels && num_listed > 0) { set_error("mirt_render_accumulate_pixels: null pixel list (every pixel of the part: d_pixels = NULL with num_listed = 0)"); return MIRT_ERR_ARG; }
  MIRT_HIP(hipSetDevice(sc->device));
  mirt::AdaptiveArgs ax;
  ax.list = d_pixels; ax.num_listed = num_listed; ax.accum_sq = (float4*)d_accum_sq_f32; ax.counts = d_counts;
  return render_accumulate_pixels(sc, p, ax, d_accum_f32, sample_first, sample_count, (hipStream_t)stream);
}

int mirt_select_pixels(const MirtRenderParams* p, const void* d_accum_f32, const void* d_accum_sq_f32, const uint32_t* d_counts, int min_samples,
                       int max_samples, float max_variance, uint32_t* d_pixels_out, uint32_t* d_num_out, void* stream)
{
  if (!p) { set_error("mirt_select_pixels: null argument"); return MIRT_ERR_ARG; }
  return select_pixels(p, d_accum_f32, d_accum_sq_f32, d_counts, min_samples, max_samples, max_variance, d_pixels_out, d_num_out, (hipStream_t)stream);
}

int mirt_finalize_counts(const MirtRenderParams* p, const void* d_accum_f32, const uint32_t* d_counts, void* d_rgba8, void* stream)
{
  if (!p) { set_error("mirt_finalize_counts: null argument"); return MIRT_ERR_ARG; }
  return finalize_counts(p, d_accum_f32, d_counts, d_rgba8, (hipStream_t)stream);
}

int mirt_scatter_part(const MirtRenderParams* p, const void* d_part_rgba8, void* d_frame_rgba8, void* stream)
{
  if (!p) { set_error("mirt_scatter_part: null argument"); return MIRT_ERR_ARG; }
  return scatter_part(p, d_part_rgba8, d_frame_rgba8, (hipStream_t)stream);
}

int mirt_trace_rays(MirtScene* sc, const void* d_rays, int64_t num_rays, void* d_hits, uint32_t flags, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_trace_rays"));
  return trace_rays(sc, d_rays, num_rays, d_hits, flags, (hipStream_t)stream);
}

int mirt_camera_rays(MirtScene* sc, const MirtRenderParams* p, void* d_rays, void* stream)
{
  if (!sc || !p) { set_error("mirt_camera_rays: null argument"); return MIRT_ERR_ARG; }
  // (the rays themselves need no tree -- a scene that was never built gives them, as before -- but between an update and its
  // build the scene answers nothing)
  if (sc->updated) { set_error("mirt_camera_rays: the scene was updated: call mirt_build_lbvh first"); return MIRT_ERR_STATE; }
  MIRT_HIP(hipSetDevice(sc->device));
  return camera_rays(sc, p, d_rays, (hipStream_t)stream);
}

int mirt_hit_features(MirtScene* sc, const void* d_rays, const void* d_hits, int64_t n, void* d_features, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_hit_features"));
  return hit_features(sc, d_rays, d_hits, n, d_features, (hipStream_t)stream);
}

// (include/mirt_light.h)
int mirt_direct_light(MirtScene* sc, const void* d_features, int64_t n, void* d_out_f32, uint64_t* d_lit_mask, uint32_t flags, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_direct_light"));
  return direct_light(sc, d_features, n, d_out_f32, d_lit_mask, flags, (hipStream_t)stream);
}

// (include/mirt_visibility.h)
int mirt_hemisphere_visibility(MirtScene* sc, const void* d_features, int64_t n, const void* d_dirs, int num_dirs, const void* d_rot, float radius,
                               void* d_out_f32, uint64_t* d_vis_mask, uint32_t flags, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_hemisphere_visibility"));
  return hemisphere_visibility(sc, d_features, n, d_dirs, num_dirs, d_rot, radius, d_out_f32, d_vis_mask, flags, (hipStream_t)stream);
}

// (include/mirt_indirect.h)
int mirt_indirect_light(MirtScene* sc, const void* d_features, int64_t n, const void* d_dirs, int num_dirs, const void* d_rot, float radius,
                        void* d_out_f32, uint64_t* d_hit_mask, uint32_t flags, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_indirect_light"));
  return indirect_light(sc, d_features, n, d_dirs, num_dirs, d_rot, radius, d_out_f32, d_hit_mask, flags, (hipStream_t)stream);
}

// (include/mirt_closest.h)
int mirt_closest_points(MirtScene* sc, const void* d_points, int64_t n, void* d_hits, void* d_features, uint32_t flags, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_closest_points"));
  return closest_points(sc, d_points, n, d_hits, d_features, flags, (hipStream_t)stream);
}

// (include/mirt_multihit.h)
int mirt_trace_rays_multi(MirtScene* sc, const void* d_rays, int64_t num_rays, int k, void* d_hits, uint32_t* d_counts, uint32_t flags, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_trace_rays_multi"));
  return trace_rays_multi(sc, d_rays, num_rays, k, d_hits, d_counts, flags, (hipStream_t)stream);
}

// (include_ext/mirt_contacts.h)
int mirt_closest_points_multi(MirtScene* sc, const void* d_points, int64_t n, int k, void* d_hits, uint32_t* d_counts, void* d_features, uint32_t flags,
                              void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_closest_points_multi"));
  return closest_points_multi(sc, d_points, n, k, d_hits, d_counts, d_features, flags, (hipStream_t)stream);
}

// (include_ext/mirt_spherecast.h)
int mirt_cast_spheres(MirtScene* sc, const void* d_casts, int64_t n, void* d_hits, void* d_features, uint32_t flags, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_cast_spheres"));
  return cast_spheres(sc, d_casts, n, d_hits, d_features, flags, (hipStream_t)stream);
}

// (include_ext/mirt_overlap.h)
int mirt_overlap_boxes(MirtScene* sc, const void* d_boxes, int64_t n, int k, void* d_hits, uint32_t* d_counts, void* d_features, uint32_t flags,
                       void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_overlap_boxes"));
  return overlap_boxes(sc, d_boxes, n, k, d_hits, d_counts, d_features, flags, (hipStream_t)stream);
}

// (include_ext/mirt_overlap_list.h)
int64_t mirt_list_offsets_work_bytes(int64_t n) { return list_offsets_work_bytes(n); }

int mirt_list_offsets(MirtScene* sc, const uint32_t* d_counts, int64_t n, int64_t* d_offsets, void* d_work, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_list_offsets"));
  return list_offsets(sc, d_counts, n, d_offsets, d_work, (hipStream_t)stream);
}

int mirt_overlap_list(MirtScene* sc, const void* d_boxes, int64_t n, const int64_t* d_offsets, uint32_t* d_words, int64_t capacity, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_overlap_list"));
  return overlap_list(sc, d_boxes, n, d_offsets, d_words, capacity, (hipStream_t)stream);
}

// (include_ext/mirt_query_lists.h)
int mirt_ray_list(MirtScene* sc, const void* d_rays, int64_t num_rays, const int64_t* d_offsets, uint32_t* d_words, float* d_t, int64_t capacity,
                  uint32_t flags, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_ray_list"));
  return ray_list(sc, d_rays, num_rays, d_offsets, d_words, d_t, capacity, flags, (hipStream_t)stream);
}

int mirt_ball_list(MirtScene* sc, const void* d_points, int64_t n, const int64_t* d_offsets, uint32_t* d_words, float* d_dist, int64_t capacity,
                   uint32_t flags, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_ball_list"));
  return ball_list(sc, d_points, n, d_offsets, d_words, d_dist, capacity, flags, (hipStream_t)stream);
}

// (include_ext2/mirt_overlap_tris.h)
int mirt_overlap_triangles(MirtScene* sc, const void* d_tris, int64_t n, uint32_t* d_counts, uint32_t flags, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_overlap_triangles"));
  return overlap_triangles(sc, d_tris, n, d_counts, flags, (hipStream_t)stream);
}

int mirt_triangle_list(MirtScene* sc, const void* d_tris, int64_t n, const int64_t* d_offsets, uint32_t* d_words, int64_t capacity, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_triangle_list"));
  return triangle_list(sc, d_tris, n, d_offsets, d_words, capacity, (hipStream_t)stream);
}

// (include_ext3/mirt_cast_lists.h)
int mirt_cast_counts(MirtScene* sc, const void* d_casts, int64_t n, uint32_t* d_counts, uint32_t flags, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_cast_counts"));
  return cast_counts(sc, d_casts, n, d_counts, flags, (hipStream_t)stream);
}

int mirt_cast_list(MirtScene* sc, const void* d_casts, int64_t n, const int64_t* d_offsets, uint32_t* d_words, float* d_t, int64_t capacity, uint32_t flags,
                   void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_cast_list"));
  return cast_list(sc, d_casts, n, d_offsets, d_words, d_t, capacity, flags, (hipStream_t)stream);
}

size_t mirt_denoise_work_bytes(const MirtRenderParams* p) { return denoise_work_bytes(p); }

int mirt_denoise(const MirtRenderParams* p, const void* d_accum_f32, const void* d_accum_sq_f32, const uint32_t* d_counts, const void* d_features,
                 int iterations, float sigma_c, float sigma_n, float sigma_p, void* d_work, void* d_out_f32, void* stream)
{
  if (!p) { set_error("mirt_denoise: null argument"); return MIRT_ERR_ARG; }
  return denoise(p, d_accum_f32, d_accum_sq_f32, d_counts, d_features, iterations, sigma_c, sigma_n, sigma_p, d_work, d_out_f32, (hipStream_t)stream);
}

int mirt_scene_get_camera(const MirtScene* sc, MirtCamera* out)
{
  if (!sc || !out) { set_error("mirt_scene_get_camera: null argument"); return MIRT_ERR_ARG; }
  const MirtSceneDesc& d = sc->d;
  out->eye = d.eye; out->forward = d.forward; out->right = d.right; out->up = d.up;
  out->dof_focus = d.dof_focus; out->dof_lens = d.dof_lens; out->fisheye = d.fisheye; out->panorama = d.panorama;
  return MIRT_OK;
}

// Host state only: render.hip and query.hip copy these fields into the RenderArgs of every call they issue, so a frame in
// flight -- each of its slabs -- keeps the camera it was issued with.
int mirt_scene_set_camera(MirtScene* sc, const MirtCamera* cam)
{
  if (!sc || !cam) { set_error("mirt_scene_set_camera: null argument"); return MIRT_ERR_ARG; }
  MirtSceneDesc& d = sc->d;
  d.eye = cam->eye; d.forward = cam->forward; d.right = cam->right; d.up = cam->up;
  d.dof_focus = cam->dof_focus; d.dof_lens = cam->dof_lens; d.fisheye = cam->fisheye; d.panorama = cam->panorama;
  return MIRT_OK;
}

int mirt_scene_update_spheres(MirtScene* sc, const void* d_spheres, int first, int count, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_scene_update_spheres"));
  return update_spheres(sc, d_spheres, first, count, (hipStream_t)stream);
}

int mirt_scene_update_triangles(MirtScene* sc, const void* d_verts, int first, int count, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_scene_update_triangles"));
  return update_triangles(sc, d_verts, first, count, (hipStream_t)stream);
}

int mirt_scene_get_spheres(MirtScene* sc, int first, int count, void* d_xyzr_out, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_scene_get_spheres"));
  return get_spheres(sc, first, count, d_xyzr_out, (hipStream_t)stream);
}

int mirt_scene_get_triangles(MirtScene* sc, int first, int count, void* d_verts_out, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_scene_get_triangles"));
  return get_triangles(sc, first, count, d_verts_out, (hipStream_t)stream);
}

int mirt_scene_get_lights(const MirtScene* sc, MirtLight* suns_out, MirtLight* bulbs_out)
{
  if (!sc) { set_error("mirt_scene_get_lights: null scene"); return MIRT_ERR_ARG; }
  if (suns_out && !sc->suns_host.empty()) memcpy(suns_out, sc->suns_host.data(), sizeof(MirtLight) * sc->suns_host.size());
  if (bulbs_out && !sc->bulbs_host.empty()) memcpy(bulbs_out, sc->bulbs_host.data(), sizeof(MirtLight) * sc->bulbs_host.size());
  return MIRT_OK;
}

int mirt_scene_set_lights(MirtScene* sc, const MirtLight* suns, const MirtLight* bulbs, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_scene_set_lights"));
  return set_lights(sc, suns, bulbs, (hipStream_t)stream);
}

int mirt_scene_get_planes(const MirtScene* sc, int first, int count, MirtPlane* out)
{
  if (!sc) { set_error("mirt_scene_get_planes: null scene"); return MIRT_ERR_ARG; }
  bool go = false;
  const int rc = check_range("mirt_scene_get_planes", out, first, count, sc->d.num_planes, alignof(MirtPlane), &go);
  if (rc != MIRT_OK || !go) return rc;
  memcpy(out, sc->planes_host.data() + first, sizeof(MirtPlane) * (size_t)count);
  return MIRT_OK;
}

int mirt_scene_set_planes(MirtScene* sc, const MirtPlane* planes, int first, int count, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_scene_set_planes"));
  return set_planes(sc, planes, first, count, (hipStream_t)stream);
}

int mirt_scene_get_shading(const MirtScene* sc, MirtShading* out)
{
  if (!sc || !out) { set_error(sc ? "mirt_scene_get_shading: null argument" : "mirt_scene_get_shading: null scene"); return MIRT_ERR_ARG; }
  out->bounces = sc->d.bounces; out->gi = sc->d.gi; out->expose = sc->d.expose;
  return MIRT_OK;
}

// Host state only, like the camera: render.hip copies these fields into the RenderArgs of every call it issues.
int mirt_scene_set_shading(MirtScene* sc, const MirtShading* sh)
{
  if (!sc || !sh) { set_error(sc ? "mirt_scene_set_shading: null argument" : "mirt_scene_set_shading: null scene"); return MIRT_ERR_ARG; }
  sc->d.bounces = sh->bounces; sc->d.gi = sh->gi; sc->d.expose = sh->expose;
  refresh_host_facts(sc);
  return MIRT_OK;
}

int mirt_scene_update_sphere_materials(MirtScene* sc, const void* d_mats, int first, int count, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_scene_update_sphere_materials"));
  return update_materials(sc, "mirt_scene_update_sphere_materials", d_mats, 0, sc->Ns, first, count, (hipStream_t)stream);
}

int mirt_scene_update_triangle_materials(MirtScene* sc, const void* d_mats, int first, int count, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_scene_update_triangle_materials"));
  return update_materials(sc, "mirt_scene_update_triangle_materials", d_mats, sc->Ns, sc->Nt, first, count, (hipStream_t)stream);
}

int mirt_scene_get_sphere_materials(MirtScene* sc, int first, int count, void* d_mats_out, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_scene_get_sphere_materials"));
  return get_materials(sc, "mirt_scene_get_sphere_materials", 0, sc->Ns, first, count, d_mats_out, (hipStream_t)stream);
}

int mirt_scene_get_triangle_materials(MirtScene* sc, int first, int count, void* d_mats_out, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_scene_get_triangle_materials"));
  return get_materials(sc, "mirt_scene_get_triangle_materials", sc->Ns, sc->Nt, first, count, d_mats_out, (hipStream_t)stream);
}

int mirt_prev_features(MirtScene* sc, const void* d_rays, const void* d_hits, int64_t n, const void* d_prev_xyzr, const void* d_prev_verts,
                       void* d_features, void* stream)
{
  MIRT_TRY(enter_scene(sc, "mirt_prev_features"));
  return prev_features(sc, d_rays, d_hits, n, d_prev_xyzr, d_prev_verts, d_features, (hipStream_t)stream);
}

int mirt_temporal_accumulate(const MirtRenderParams* p, const MirtCamera* prev_camera, const void* d_accum_f32, const void* d_accum_sq_f32,
                             const uint32_t* d_counts, const void* d_prev_features, const void* d_hist_accum_f32, const void* d_hist_accum_sq_f32,
                             const uint32_t* d_hist_counts, const void* d_hist_features, int max_history, float sigma_n, float sigma_p,
                             void* d_out_accum_f32, void* d_out_accum_sq_f32, uint32_t* d_out_counts, void* stream)
{
  if (!p || !prev_camera) { set_error("mirt_temporal_accumulate: null argument"); return MIRT_ERR_ARG; }
  return temporal_accumulate(p, prev_camera, d_accum_f32, d_accum_sq_f32, d_counts, d_prev_features, d_hist_accum_f32, d_hist_accum_sq_f32, d_hist_counts,
                             d_hist_features, max_history, sigma_n, sigma_p, d_out_accum_f32, d_out_accum_sq_f32, d_out_counts, (hipStream_t)stream);
}

int mirt_get_stats(MirtScene* sc, MirtStats* out)
{
  if (!sc || !out) { set_error("mirt_get_stats: null argument"); return MIRT_ERR_ARG; }
  memset(out, 0, sizeof(*out));
  MIRT_HIP(hipSetDevice(sc->device));
  out->build_ms = sc->build_ms;
  out->num_nodes = sc->N > 0 ? 2 * sc->N - 1 : 0;
  if (!sc->last) return MIRT_OK;
  for (int i = 0; i < mirt::MIRT_MAX_FRAMES; ++i) {   // finish and time every frame still in flight
    mirt::RenderCtx& c = sc->ctx[i];
    if (c.used) {     // capacity overflows of the frames this context rendered since the previous call
      MIRT_HIP(hipEventSynchronize(c.ev3));
      unsigned long long ov = 0;
      hipLaunchKernelGGL(take_overflow_kernel, dim3(1), dim3(1), 0, c.stream, c.counters);
      MIRT_HIP(hipGetLastError());
      MIRT_HIP(hipStreamSynchronize(c.stream));
      MIRT_HIP(hipMemcpy(&ov, c.counters + 10, sizeof(ov), hipMemcpyDeviceToHost));
      sc->overflow_events += ov;
    }
    if (c.used) { int rc = fold_trace_time(sc, c); if (rc != MIRT_OK) return rc; }      // (finished: waited for above)
  }
  out->frames_timed = sc->trace_frames;
  out->trace_kernel_ms_mean = sc->trace_frames ? (float)(sc->trace_ms_sum / sc->trace_frames) : 0.0f;
  sc->trace_ms_sum = 0.0; sc->trace_frames = 0;
  mirt::RenderCtx& cx = *sc->last;
  { int rc = trace_ms_of(cx, &out->trace_kernel_ms); if (rc != MIRT_OK) return rc; }
  out->trace_launches = cx.launches;
  out->node_record_bytes = cx.node_bytes;
  MIRT_HIP(hipEventElapsedTime(&out->render_ms, cx.ev0, cx.ev3));
  if (cx.counted) {
    unsigned long long c[8];
    MIRT_HIP(hipMemcpy(c, cx.counters, sizeof(c), hipMemcpyDeviceToHost));
    out->samples = c[0]; out->rays = c[1]; out->shadow_rays = c[2]; out->internal_visits = c[3];
    out->sphere_tests = c[4]; out->tri_tests = c[5]; out->mat_fetches = c[6]; out->max_stack = c[7];
    MIRT_HIP(hipMemcpy(&out->rays_traversed, cx.counters + 11, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  }
  out->overflow_events = sc->overflow_events;
  sc->overflow_events = 0;
  if (out->overflow_events) {
    set_error("mirt_get_stats: capacity overflow during a render (the pending-children list of refraction / gi rays was full): the image is missing contributions");
    return MIRT_ERR_STATE;
  }
  return MIRT_OK;
}

int mirt_get_tree(MirtScene* sc, MirtTreeNode* nodes, uint32_t* codes, MirtPrimRef* refs, float* bounds)
{
  MIRT_TRY(enter_scene(sc, "mirt_get_tree"));
  return get_tree(sc, nodes, codes, refs, bounds);
}

int mirt_get_records(MirtScene* sc, MirtRecordInfo* info, void* nodes, void* qnodes, void* wnodes, void* prims, uint32_t* unit_prim,
                     uint32_t* tris_before, float* tri_boxes, float* qparams)
{
  MIRT_TRY(enter_scene(sc, "mirt_get_records"));
  return get_records(sc, info, nodes, qnodes, wnodes, prims, unit_prim, tris_before, tri_boxes, qparams);
}

int mirt_probe_math(int device, int which, int n, const float* host_in, float* host_out)
{
  if (n <= 0 || !host_in || !host_out) { set_error("mirt_probe_math: bad argument"); return MIRT_ERR_ARG; }
  return probe_math(device, which, n, host_in, host_out);
}

int mirt_probe_xorwow(int device, int spp, int num_streams, int draws, uint32_t* host_out)
{
  if (num_streams <= 0 || draws <= 0 || !host_out) { set_error("mirt_probe_xorwow: bad argument"); return MIRT_ERR_ARG; }
  return probe_xorwow(device, spp, num_streams, draws, host_out);
}

int mirt_probe_qbox(int device, int n, const float* host_in, uint32_t* host_out)
{
  if (n <= 0 || !host_in || !host_out) { set_error("mirt_probe_qbox: bad argument"); return MIRT_ERR_ARG; }
  return probe_qbox(device, n, host_in, host_out);
}

int mirt_probe_sort(int device, int mode, int n, const uint32_t* host_keys, uint32_t* host_keys_out, uint32_t* host_vals_out)
{
  if (n <= 0 || (mode != 0 && mode != 1) || !host_keys || !host_keys_out || !host_vals_out) { set_error("mirt_probe_sort: bad argument"); return MIRT_ERR_ARG; }
  return probe_sort(device, mode, n, host_keys, host_keys_out, host_vals_out);
}

int mirt_probe_sched(int device, int which, int n, const uint32_t* host_in, uint32_t* host_out)
{
  if (n <= 0 || (which != 0 && which != 1) || !host_in || !host_out) { set_error("mirt_probe_sched: bad argument"); return MIRT_ERR_ARG; }
  return probe_sched(device, which, n, host_in, host_out);
}

int mirt_get_sample_order(MirtScene* sc, MirtSampleOrderInfo* info, uint32_t* order, uint32_t* keys, uint32_t* sorted_keys)
{
  MIRT_TRY(enter_scene(sc, "mirt_get_sample_order"));
  return get_sample_order(sc, info, order, keys, sorted_keys);
}

} // extern "C"
