// Stand-alone probe of the row queries' argument checks (csrc/host_scene.h: check_row_query's seven callers and any_overlap) for
// tests/test_row_query_checks.py: no HIP, no GPU, never loaded into python.  Compiled together with csrc/host_scene.cpp.
// stdin, one case per line:
//   ENTRY flags n k p0 p1 p2 p3 extra built     the addresses are numbers and never dereferenced; which argument each p is, per entry:
//       closest   points hits features -            multi     points hits counts features      cast   casts hits features -
//       overlap   boxes hits counts features        offsets   counts offsets work - (extra: the work bytes; no built)
//       list      boxes offsets words - (extra: capacity)                                        multihit  rays hits counts -
//   ranges COUNT p bytes p bytes ...                 any_overlap of COUNT ranges
// stdout per case: "status go|message" (message: mirt_last_error after the call, cleared before it), or "overlap=0|1".
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../cuda_ray_tracer_amd/csrc/host_scene.h"

int main()
{
  using namespace mirt;
  char entry[32];
  while (scanf("%31s", entry) == 1) {
    if (!strcmp(entry, "ranges")) {
      int count = 0;
      if (scanf("%d", &count) != 1 || count < 0 || count > 8) return 1;
      ByteRange r[8];
      for (int i = 0; i < count; ++i) {
        uint64_t p = 0, b = 0;
        if (scanf("%" SCNu64 " %" SCNu64, &p, &b) != 2) return 1;
        r[i].ptr = (const void*)(uintptr_t)p;
        r[i].bytes = (size_t)b;
      }
      printf("overlap=%d\n", any_overlap(r, count) ? 1 : 0);
      continue;
    }
    uint32_t flags = 0;
    int64_t n = 0, extra = 0;
    int k = 0, built = 0;
    uint64_t a[4] = {0, 0, 0, 0};
    if (scanf("%" SCNu32 " %" SCNd64 " %d %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %d", &flags, &n, &k, &a[0], &a[1], &a[2], &a[3], &extra,
              &built) != 9) return 1;
    const void* p[4];
    for (int i = 0; i < 4; ++i) p[i] = (const void*)(uintptr_t)a[i];
    bool go = false;
    int rc = -1;
    set_error("");
    if (!strcmp(entry, "closest")) rc = check_closest_points(p[0], n, p[1], p[2], flags, built != 0, &go);
    else if (!strcmp(entry, "multi")) rc = check_closest_points_multi(p[0], n, k, p[1], p[2], p[3], flags, built != 0, &go);
    else if (!strcmp(entry, "cast")) rc = check_cast_spheres(p[0], n, p[1], p[2], flags, built != 0, &go);
    else if (!strcmp(entry, "overlap")) rc = check_overlap_boxes(p[0], n, k, p[1], p[2], p[3], flags, built != 0, &go);
    else if (!strcmp(entry, "offsets")) rc = check_list_offsets(p[0], n, p[1], p[2], (size_t)extra, &go);
    else if (!strcmp(entry, "list")) rc = check_overlap_list(p[0], n, p[1], p[2], extra, built != 0, &go);
    else if (!strcmp(entry, "multihit")) rc = check_trace_rays_multi(p[0], n, k, p[1], p[2], flags, built != 0, &go);
    else return 1;
    printf("%d %d|%s\n", rc, go ? 1 : 0, g_last_error.c_str());
  }
  return 0;
}
