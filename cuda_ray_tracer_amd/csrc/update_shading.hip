// Shading values of a built scene in place (include/mirt.h: mirt_scene_set_lights, mirt_scene_set_planes,
// mirt_scene_update_sphere_materials / _triangle_materials and their inverses).  None of these values is
// in the record heap, so the scene stays built.  What has to follow every update is the call plan's view of the scene
// (render_plan.h, SceneFacts: any_trans, any_rough, colors_finite): the facts are kept by source -- MirtScene::host_flags for
// planes, lights and exposure, recomputed on the host at every setter; MirtScene::prim_flags for the primitives' materials,
// which after a material update only the device knows: the update ends with an OR over one flag byte per primitive, and
// settle_facts, the first thing a render call does, waits for that word once.
//
// update_materials_kernel   one lane per primitive: 11 floats in (dword loads), three float4 and one flag byte out.
// material_flags_kernel     one lane per primitive: the flag bytes of a scene's materials as mirt_scene_create uploaded them.
// reduce_flags_kernel       grid-stride over the flag bytes, four per load; one LDS word per block, one atomicOr per block.
// get_materials_kernel      the inverse of update_materials_kernel.
#include "scene_dev.h"
#include "host_scene.h"
#include "material_flags.h"

#include <cmath>
#include <cstring>
#include <string>

namespace mirt {

namespace {

constexpr int SBLOCK = 256;
constexpr int REDUCE_BLOCKS_MAX = 256;

__device__ inline void unpack_mat(const float4* __restrict__ in, float m[11])
{
  const float4 a = in[0], b = in[1], c = in[2];
  m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w;
  m[4] = b.x; m[5] = b.y; m[6] = b.z; m[7] = b.w;
  m[8] = c.x; m[9] = c.y; m[10] = c.z;
}

__global__ __launch_bounds__(SBLOCK) void update_materials_kernel(const float* __restrict__ in, float4* __restrict__ mats, unsigned char* __restrict__ flags, int count)
{
  const int i = (int)(blockIdx.x * SBLOCK + threadIdx.x);
  if (i >= count) return;
  const float* v = in + 11 * (size_t)i;
  float m[11];
#pragma unroll
  for (int k = 0; k < 11; ++k) m[k] = v[k];
  float4* o = mats + 3 * (size_t)i;
  o[0] = make_float4(m[0], m[1], m[2], m[3]);
  o[1] = make_float4(m[4], m[5], m[6], m[7]);
  o[2] = make_float4(m[8], m[9], m[10], 0.0f);
  flags[i] = (unsigned char)material_flags(m);
}

__global__ __launch_bounds__(SBLOCK) void material_flags_kernel(const float4* __restrict__ mats, unsigned char* __restrict__ flags, int count)
{
  const int i = (int)(blockIdx.x * SBLOCK + threadIdx.x);
  if (i >= count) return;
  float m[11];
  unpack_mat(mats + 3 * (size_t)i, m);
  flags[i] = (unsigned char)material_flags(m);
}

__global__ __launch_bounds__(SBLOCK) void get_materials_kernel(const float4* __restrict__ mats, float* __restrict__ out, int count)
{
  const int i = (int)(blockIdx.x * SBLOCK + threadIdx.x);
  if (i >= count) return;
  float m[11];
  unpack_mat(mats + 3 * (size_t)i, m);
  float* o = out + 11 * (size_t)i;
#pragma unroll
  for (int k = 0; k < 11; ++k) o[k] = m[k];
}

// words: the flag bytes four at a time (the array is padded with zero bytes to a whole word)
__global__ __launch_bounds__(SBLOCK) void reduce_flags_kernel(const uint32_t* __restrict__ words, long long num_words, unsigned* __restrict__ out)
{
  __shared__ unsigned block_or;
  if (threadIdx.x == 0) block_or = 0u;
  __syncthreads();
  unsigned v = 0u;
  for (long long j = (long long)blockIdx.x * SBLOCK + threadIdx.x; j < num_words; j += (long long)gridDim.x * SBLOCK) v |= words[j];
  v |= v >> 16; v |= v >> 8; v &= 0xffu;
  if (v) atomicOr(&block_or, v);
  __syncthreads();
  if (threadIdx.x == 0 && block_or) atomicOr(out, block_or);
}

unsigned grid_of(long long n) { return (unsigned)((n + SBLOCK - 1) / SBLOCK); }

void recombine(MirtScene* sc)
{
  const unsigned f = sc->prim_flags | sc->host_flags;
  sc->any_trans = (f & MAT_TRANS) != 0; sc->any_rough = (f & MAT_ROUGH) != 0; sc->colors_finite = (f & MAT_NONFINITE) == 0;
}

// The pinned staging buffer, free for `bytes` of new records: the copy that used it last has finished.
int take_stage(MirtScene* sc, size_t bytes)
{
  if (sc->stage_used) { MIRT_HIP(hipEventSynchronize(sc->stage_ev)); sc->stage_used = false; }
  MIRT_TRY(sc->stage_ev.create(hipEventDisableTiming));
  if (sc->stage.cap() < bytes) MIRT_TRY(sc->stage.alloc(bytes, "stage"));
  return MIRT_OK;
}

// The flag byte per primitive and the reduction's word, on first use: the bytes of the materials as they are on the device.
int ensure_flags(MirtScene* sc, hipStream_t stream)
{
  if (sc->mat_flags) return MIRT_OK;
  const size_t bytes = ((size_t)sc->N + 3) / 4 * 4;
  if (!sc->flags_or) MIRT_TRY(sc->flags_or.alloc(1, "flags_or"));
  if (!sc->flags_or_host) MIRT_TRY(sc->flags_or_host.alloc(1, "flags_or_host"));
  MIRT_TRY(sc->facts_ev.create(hipEventDisableTiming));
  DevBuf<unsigned char> flags;      // (the scene's only once they are filled: mat_flags set means made)
  MIRT_TRY(flags.alloc(bytes, "mat_flags"));
  MIRT_HIP(hipMemsetAsync(flags, 0, bytes, stream));
  hipLaunchKernelGGL(material_flags_kernel, dim3(grid_of(sc->N)), dim3(SBLOCK), 0, stream, sc->mats, flags, sc->N);
  MIRT_HIP(hipGetLastError());
  sc->mat_flags = std::move(flags);
  return MIRT_OK;
}

} // namespace

void pack_mat(const float m[11], float4* out)
{
  out[0] = make_float4(m[0], m[1], m[2], m[3]);
  out[1] = make_float4(m[4], m[5], m[6], m[7]);
  out[2] = make_float4(m[8], m[9], m[10], 0.0f);
}

LightDev sun_dev(const MirtLight& l)
{
  const MirtVec3& v = l.v;
  // vec3::normalize (vec3.cuh:72-82) -- this translation unit is built with -ffp-contract=off
  const float mag = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  const float diff = fabsf(mag - 0.0f), largest = fmaxf(fabsf(mag), fabsf(0.0f));
  const bool zero = (largest < 1e-6f) ? (diff < 1e-6f) : (diff / largest < 1e-6f);
  if (!zero) { const float inv = 1.0f / mag; nx = v.x * inv; ny = v.y * inv; nz = v.z * inv; }
  return {v.x, v.y, v.z, l.color.r, l.color.g, l.color.b, nx, ny, nz, 1.0f / nx, 1.0f / ny, 1.0f / nz};
}

LightDev bulb_dev(const MirtLight& l) { return {l.v.x, l.v.y, l.v.z, l.color.r, l.color.g, l.color.b, 0, 0, 0, 0, 0, 0}; }

PlaneDev plane_dev(const MirtPlane& p)
{
  PlaneDev q;
  q.nx = p.nor.x; q.ny = p.nor.y; q.nz = p.nor.z; q.px = p.point.x; q.py = p.point.y; q.pz = p.point.z;
  static_assert(sizeof(MirtMaterials) == sizeof(q.mat), "MirtMaterials is 11 floats");
  memcpy(q.mat, &p.mat, sizeof(q.mat)); q.pad = 0.0f;
  return q;
}

// host_flags from the scene's host copies: the planes' materials, the lights' colours, the exposure (+inf: exposure off)
void refresh_host_facts(MirtScene* sc)
{
  unsigned f = 0u;
  for (const MirtPlane& p : sc->planes_host) {
    float m[11];
    memcpy(m, &p.mat, sizeof(m));
    f |= material_flags(m);
  }
  for (const MirtLight& l : sc->suns_host) if (!finite_rgb(l.color.r, l.color.g, l.color.b)) f |= MAT_NONFINITE;
  for (const MirtLight& l : sc->bulbs_host) if (!finite_rgb(l.color.r, l.color.g, l.color.b)) f |= MAT_NONFINITE;
  if (!finite_f32(sc->d.expose) && sc->d.expose != INFINITY) f |= MAT_NONFINITE;
  sc->host_flags = f;
  recombine(sc);
}

// The facts as of every update issued so far.  After a material update: one host wait for its reduction, then its word.
int settle_facts(MirtScene* sc)
{
  if (!sc->facts_pending) return MIRT_OK;
  MIRT_HIP(hipEventSynchronize(sc->facts_ev));
  sc->prim_flags = *sc->flags_or_host;
  sc->facts_pending = false;
  recombine(sc);
  return MIRT_OK;
}

int set_lights(MirtScene* sc, const MirtLight* suns, const MirtLight* bulbs, hipStream_t stream)
{
  const size_t ns = suns ? (size_t)sc->d.num_suns : 0, nb = bulbs ? (size_t)sc->d.num_bulbs : 0;
  if (ns + nb == 0) return MIRT_OK;
  int rc = wait_for_frames(sc);
  if (rc == MIRT_OK) rc = take_stage(sc, sizeof(LightDev) * (ns + nb));
  if (rc != MIRT_OK) return rc;
  LightDev* st = reinterpret_cast<LightDev*>(sc->stage.get());
  for (size_t i = 0; i < ns; ++i) st[i] = sun_dev(suns[i]);
  for (size_t i = 0; i < nb; ++i) st[ns + i] = bulb_dev(bulbs[i]);
  sc->stage_used = true;      // (from here on the buffer may be in use, whatever fails below)
  if (ns) MIRT_HIP(hipMemcpyAsync(sc->suns, st, sizeof(LightDev) * ns, hipMemcpyHostToDevice, stream));
  if (nb) MIRT_HIP(hipMemcpyAsync(sc->bulbs, st + ns, sizeof(LightDev) * nb, hipMemcpyHostToDevice, stream));
  MIRT_HIP(hipEventRecord(sc->stage_ev, stream));
  if (ns) sc->suns_host.assign(suns, suns + ns);
  if (nb) sc->bulbs_host.assign(bulbs, bulbs + nb);
  refresh_host_facts(sc);
  return MIRT_OK;
}

int set_planes(MirtScene* sc, const MirtPlane* planes, int first, int count, hipStream_t stream)
{
  bool go = false;
  int rc = check_range("mirt_scene_set_planes", planes, first, count, sc->d.num_planes, alignof(MirtPlane), &go);
  if (rc != MIRT_OK || !go) return rc;
  rc = wait_for_frames(sc);
  if (rc == MIRT_OK) rc = take_stage(sc, sizeof(PlaneDev) * (size_t)count);
  if (rc != MIRT_OK) return rc;
  PlaneDev* st = reinterpret_cast<PlaneDev*>(sc->stage.get());
  for (int i = 0; i < count; ++i) st[i] = plane_dev(planes[i]);
  sc->stage_used = true;
  MIRT_HIP(hipMemcpyAsync(sc->planes + first, st, sizeof(PlaneDev) * (size_t)count, hipMemcpyHostToDevice, stream));
  MIRT_HIP(hipEventRecord(sc->stage_ev, stream));
  for (int i = 0; i < count; ++i) sc->planes_host[(size_t)first + i] = planes[i];
  refresh_host_facts(sc);
  return MIRT_OK;
}

// materials [first, first + count) of the `total` primitives whose records start at `base` (spheres 0, triangles num_spheres)
int update_materials(MirtScene* sc, const char* who, const void* d_mats, int base, int total, int first, int count, hipStream_t stream)
{
  bool go = false;
  int rc = check_range(who, d_mats, first, count, total, 4, &go);
  if (rc != MIRT_OK || !go) return rc;
  rc = wait_for_frames(sc);
  // (an update pending on another stream: its flag bytes must be in place before this stream's reduction reads them)
  if (rc == MIRT_OK && sc->facts_pending && sc->facts_stream != stream) rc = settle_facts(sc);
  if (rc == MIRT_OK) rc = ensure_flags(sc, stream);
  if (rc != MIRT_OK) return rc;
  const size_t at = (size_t)base + (size_t)first;
  hipLaunchKernelGGL(update_materials_kernel, dim3(grid_of(count)), dim3(SBLOCK), 0, stream, static_cast<const float*>(d_mats), sc->mats + 3 * at,
                     sc->mat_flags + at, count);
  MIRT_HIP(hipGetLastError());
  // the OR over ALL primitives: a primitive outside the range keeps its say, one inside may have lost its own
  const long long words = ((long long)sc->N + 3) / 4;
  const unsigned blocks = grid_of(words) < (unsigned)REDUCE_BLOCKS_MAX ? grid_of(words) : (unsigned)REDUCE_BLOCKS_MAX;
  MIRT_HIP(hipMemsetAsync(sc->flags_or, 0, sizeof(unsigned), stream));
  hipLaunchKernelGGL(reduce_flags_kernel, dim3(blocks), dim3(SBLOCK), 0, stream, reinterpret_cast<const uint32_t*>(sc->mat_flags.get()), words, sc->flags_or);
  MIRT_HIP(hipGetLastError());
  MIRT_HIP(hipMemcpyAsync(sc->flags_or_host, sc->flags_or, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
  MIRT_HIP(hipEventRecord(sc->facts_ev, stream));
  sc->facts_pending = true; sc->facts_stream = stream;
  return MIRT_OK;
}

int get_materials(MirtScene* sc, const char* who, int base, int total, int first, int count, void* d_mats_out, hipStream_t stream)
{
  bool go = false;
  const int rc = check_range(who, d_mats_out, first, count, total, 4, &go);
  if (rc != MIRT_OK || !go) return rc;
  hipLaunchKernelGGL(get_materials_kernel, dim3(grid_of(count)), dim3(SBLOCK), 0, stream, sc->mats + 3 * ((size_t)base + (size_t)first),
                     static_cast<float*>(d_mats_out), count);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

} // namespace mirt
