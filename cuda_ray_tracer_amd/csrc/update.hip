// Updates of a built scene in place (include/mirt.h: mirt_scene_update_spheres, mirt_scene_update_triangles): new sphere
// and triangle values from device memory into the scene's file-order input arrays, which the next mirt_build_lbvh reads.
// The triangle kernel computes nor / e1 / e2 as the reference's Triangle(Vertex, Vertex, Vertex, RGB) does
// (object.cuh:177-191) -- the operations of make_triangle (host_scene.cpp) in the same order, one rounding each (this unit
// is built with -ffp-contract=off like every other), so the records are the bits a fresh mirt_scene_create would upload.
#include "scene_dev.h"
#include "host_scene.h"


namespace mirt {

namespace {

constexpr int UPDATE_BLOCK = 256;

// one lane per sphere: (cx, cy, cz, r) as given
__global__ __launch_bounds__(UPDATE_BLOCK) void update_spheres_kernel(const float4* __restrict__ in, float4* __restrict__ spheres, int count)
{
  const int i = (int)(blockIdx.x * UPDATE_BLOCK + threadIdx.x);
  if (i >= count) return;
  spheres[i] = in[i];
}

// one lane per triangle: 9 floats in (4-byte aligned: dword loads), the build's vertices and the 48-byte render record out
__global__ __launch_bounds__(UPDATE_BLOCK) void update_triangles_kernel(const float* __restrict__ in, float4* __restrict__ verts, float4* __restrict__ tris, int count)
{
  const int i = (int)(blockIdx.x * UPDATE_BLOCK + threadIdx.x);
  if (i >= count) return;
  const float* v = in + 9 * (size_t)i;
  const f3 p0 = mk3(v[0], v[1], v[2]), p1 = mk3(v[3], v[4], v[5]), p2 = mk3(v[6], v[7], v[8]);
  // object.cuh:177-191
  const f3 d1 = p1 - p0, d2 = p2 - p0;
  const f3 nor = normalize(cross(d1, d2));
  const f3 a1 = cross(d2, nor);
  const f3 a2 = cross(d1, nor);
  const float k1 = 1.0f / dot(a1, d1);
  const float k2 = 1.0f / dot(a2, d2);
  const f3 e1 = mk3(a1.x * k1, a1.y * k1, a1.z * k1);
  const f3 e2 = mk3(a2.x * k2, a2.y * k2, a2.z * k2);
  float4* vo = verts + 3 * (size_t)i;
  vo[0] = make_float4(p0.x, p0.y, p0.z, 0.0f);
  vo[1] = make_float4(p1.x, p1.y, p1.z, 0.0f);
  vo[2] = make_float4(p2.x, p2.y, p2.z, 0.0f);
  float4* to = tris + 3 * (size_t)i;
  to[0] = make_float4(p0.x, p0.y, p0.z, nor.x);
  to[1] = make_float4(nor.y, nor.z, e1.x, e1.y);
  to[2] = make_float4(e1.z, e2.x, e2.y, e2.z);
}

// Frames in flight read the record heap, which the build that follows an update rewrites: wait for every context's last
// frame before anything is enqueued.  From here on the scene is not built.
int begin_update(MirtScene* sc)
{
  const int rc = wait_for_frames(sc);
  if (rc != MIRT_OK) return rc;
  sc->built = false;
  sc->updated = true;
  // What the scene's rays did on the old geometry says nothing about the new one: the ratio behind the plan's pass length goes
  // (render_plan.h, prim_ratio), until a call measures a sample order again.  The order itself serves any content and stays.
  sc->so_ratio = -1.0f;
  sc->so_ratio_stale = sc->so_ratio_stale || sc->so_busy;      // (a measurement in flight counted the old geometry)
  return MIRT_OK;
}

} // namespace

// the last frame of every render context has finished (what an update in place waits for before it enqueues anything)
int wait_for_frames(MirtScene* sc)
{
  for (int i = 0; i < MIRT_MAX_FRAMES; ++i)
    if (sc->ctx[i].used) MIRT_HIP(hipEventSynchronize(sc->ctx[i].ev3));
  return MIRT_OK;
}

int update_spheres(MirtScene* sc, const void* d_spheres, int first, int count, hipStream_t stream)
{
  bool go = false;
  int rc = check_range("mirt_scene_update_spheres", d_spheres, first, count, sc->Ns, 16, &go);
  if (rc != MIRT_OK || !go) return rc;
  rc = begin_update(sc);
  if (rc != MIRT_OK) return rc;
  hipLaunchKernelGGL(update_spheres_kernel, dim3((unsigned)((count + UPDATE_BLOCK - 1) / UPDATE_BLOCK)), dim3(UPDATE_BLOCK), 0, stream,
                     static_cast<const float4*>(d_spheres), sc->spheres + first, count);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

int update_triangles(MirtScene* sc, const void* d_verts, int first, int count, hipStream_t stream)
{
  bool go = false;
  int rc = check_range("mirt_scene_update_triangles", d_verts, first, count, sc->Nt, 4, &go);
  if (rc != MIRT_OK || !go) return rc;
  rc = begin_update(sc);
  if (rc != MIRT_OK) return rc;
  hipLaunchKernelGGL(update_triangles_kernel, dim3((unsigned)((count + UPDATE_BLOCK - 1) / UPDATE_BLOCK)), dim3(UPDATE_BLOCK), 0, stream,
                     static_cast<const float*>(d_verts), sc->tri_verts + 3 * (size_t)first, sc->tris + 3 * (size_t)first, count);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

} // namespace mirt
