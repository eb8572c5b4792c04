// Stand-alone probe of the triangle-overlap queries' argument checks (csrc/host_scene.h: check_overlap_triangles and
// check_triangle_list, through check_row_query) for tests/test_overlap_tris_checks.py: no HIP, no GPU, never loaded into python.
// Compiled together with csrc/host_scene.cpp.
// stdin, one case per line:
//   ENTRY flags n p0 p1 p2 capacity built     the addresses are numbers and never dereferenced; which argument each p is, per entry:
//       count   tris counts -  (capacity unused)            fill   tris offsets words
// stdout per case: "status go|message" (message: the last error after the call, cleared before it).
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../cuda_ray_tracer_amd/csrc/host_scene.h"

int main()
{
  using namespace mirt;
  char entry[32];
  while (scanf("%31s", entry) == 1) {
    uint32_t flags = 0;
    int64_t n = 0, capacity = 0;
    int built = 0;
    uint64_t a[3] = {0, 0, 0};
    if (scanf("%" SCNu32 " %" SCNd64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %d", &flags, &n, &a[0], &a[1], &a[2], &capacity, &built) != 7) return 1;
    const void* p[3];
    for (int i = 0; i < 3; ++i) p[i] = (const void*)(uintptr_t)a[i];
    bool go = false;
    int rc = -1;
    set_error("");
    if (!strcmp(entry, "count")) rc = check_overlap_triangles(p[0], n, p[1], flags, built != 0, &go);
    else if (!strcmp(entry, "fill")) rc = check_triangle_list(p[0], n, p[1], p[2], capacity, built != 0, &go);
    else return 1;
    printf("%d %d|%s\n", rc, go ? 1 : 0, g_last_error.c_str());
  }
  return 0;
}
