// Host-side scene container (the reference's StlConfig, config.hpp:24-73) and parser; the last-error string and the argument
// checks the C entry points share.
#ifndef MIRT_HOST_SCENE_H
#define MIRT_HOST_SCENE_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <istream>
#include <string>
#include <vector>

#include "../../include/mirt.h"

namespace mirt {

extern thread_local std::string g_last_error;
void set_error(const std::string& s);

// do the byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool overlaps(const void* a, size_t na, const void* b, size_t nb)
{
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}
inline bool positive_finite(float x) { return x > 0.0f && std::isfinite(x); }
// is every one of the pointers a multiple of n, a power of two (a null pointer is)
template <class... T>
bool is_aligned(size_t n, const T*... p) { return ((... | (uintptr_t)p) & (n - 1)) == 0; }
// A range [first, first + count) of a scene's `total` spheres or triangles and the device array that gives or receives it
// (mirt_scene_update_* / mirt_scene_get_*).  MIRT_OK with *go = false: nothing to do (count 0).
int check_range(const char* who, const void* d_array, int first, int count, int total, size_t align, bool* go);
// The frame and the part of it (npix pixels, render_num_pixels) that a call renders or makes rays for: both within the 32-bit
// pixel seed and sample index.  MIRT_OK with *go = false: nothing to do (an empty part).
int check_frame(const char* who, const MirtRenderParams* p, int64_t npix, bool* go);
// The arguments of a query that traces a caller's table of directions from every row of a feature buffer
// (mirt_hemisphere_visibility, mirt_indirect_light): mask_name is the mask parameter's own name, built whether the scene has its
// tree.  MIRT_OK with *go = false: nothing to do (n == 0).
int check_table_query(const char* who, const char* mask_name, const void* d_features, int64_t n, const void* d_dirs, int num_dirs, const void* d_rot,
                      float radius, const void* d_out_f32, const uint64_t* d_mask, uint32_t flags, bool built, bool* go);

// do any two of the byte ranges share a byte (a range of no bytes overlaps nothing)
struct ByteRange { const void* ptr; size_t bytes; };
bool any_overlap(const ByteRange* ranges, int count);

// The arguments of a query with one lane per row.  A buffer as its entry point describes it: the bytes the call reads or writes
// there (a null pointer's count as none), the alignment, and whether this call needs it.  A rule is an argument test of the entry
// point's own with its message.
struct QueryBuf { const void* ptr; size_t bytes; size_t align; bool required; };
struct ArgRule { bool bad; const char* msg; };
// The checks in the order every row query makes them -- unknown flag bits, a negative n (n_name: the parameter's own name), the
// rules, a required buffer that is null, alignment, overlap, the scene's tree (built) -- each with who + ": " in front of its
// message.  MIRT_OK with *go = false: nothing to do (n == 0).
int check_row_query(const char* who, uint32_t unknown_flags, int64_t n, const char* n_name, std::initializer_list<ArgRule> rules,
                    std::initializer_list<QueryBuf> bufs, const char* null_msg, const char* align_msg, const char* overlap_msg, bool built, bool* go);
// ... of the nine entry points (closest.hip, closest_multi.hip, spherecast.hip, overlap.hip, overlap_list.hip, query_lists.hip,
// multihit.hip)
int check_closest_points(const void* d_points, int64_t n, const void* d_hits, const void* d_features, uint32_t flags, bool built, bool* go);
int check_closest_points_multi(const void* d_points, int64_t n, int k, const void* d_hits, const void* d_counts, const void* d_features, uint32_t flags,
                               bool built, bool* go);
int check_cast_spheres(const void* d_casts, int64_t n, const void* d_hits, const void* d_features, uint32_t flags, bool built, bool* go);
int check_overlap_boxes(const void* d_boxes, int64_t n, int k, const void* d_hits, const void* d_counts, const void* d_features, uint32_t flags,
                        bool built, bool* go);
// (work_bytes: mirt_list_offsets_work_bytes(n); no scene is read, so there is no `built`)
int check_list_offsets(const void* d_counts, int64_t n, const void* d_offsets, const void* d_work, size_t work_bytes, bool* go);
int check_overlap_list(const void* d_boxes, int64_t n, const void* d_offsets, const void* d_words, int64_t capacity, bool built, bool* go);
// (d_values: the optional array of t or dist, null or `capacity` floats)
int check_ray_list(const void* d_rays, int64_t num_rays, const void* d_offsets, const void* d_words, const void* d_t, int64_t capacity, uint32_t flags,
                   bool built, bool* go);
int check_ball_list(const void* d_points, int64_t n, const void* d_offsets, const void* d_words, const void* d_dist, int64_t capacity, uint32_t flags,
                    bool built, bool* go);
int check_trace_rays_multi(const void* d_rays, int64_t num_rays, int k, const void* d_hits, const void* d_counts, uint32_t flags, bool built, bool* go);
// ... and of the two of include_ext2/mirt_overlap_tris.h (overlap_tris.hip): rows of 36 bytes, 4-byte aligned
int check_overlap_triangles(const void* d_tris, int64_t n, const void* d_counts, uint32_t flags, bool built, bool* go);
int check_triangle_list(const void* d_tris, int64_t n, const void* d_offsets, const void* d_words, int64_t capacity, bool built, bool* go);
// ... and of the two of include_ext3/mirt_cast_lists.h (cast_lists.hip): mirt_cast_spheres' rows
int check_cast_counts(const void* d_casts, int64_t n, const void* d_counts, uint32_t flags, bool built, bool* go);
int check_cast_list(const void* d_casts, int64_t n, const void* d_offsets, const void* d_words, const void* d_t, int64_t capacity, uint32_t flags, bool built,
                    bool* go);

class HostScene {
public:
  HostScene();
  int parse_stream(std::istream& in);                          // parseInput, parse.cpp:16-39
  int parse_line(const std::vector<std::string>& words);      // parseLine, parse.cpp:41-222
  void make_synthetic(uint64_t seed, int num_spheres, int num_triangles);
  void fill_desc(MirtSceneDesc* d) const;
  MirtMaterials current_material() const;

  int width, height;
  std::string filename;
  MirtRGB color;
  int bounces, aa;
  float dof_focus, dof_lens;
  MirtVec3 forward, right, up, eye, target_up;
  float expose;
  bool fisheye, panorama;
  float ior, rough;
  int gi;
  MirtRGB trans, shine;

  std::vector<MirtSphere> spheres;
  std::vector<MirtTriangle> triangles;
  std::vector<MirtPrimRef> refs;
  std::vector<MirtPlane> planes;
  std::vector<MirtSun> suns;
  std::vector<MirtBulb> bulbs;
  std::vector<MirtVec3> vertices;
};

} // namespace mirt
#endif
