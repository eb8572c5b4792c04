// Stand-alone probe of the cast lists' argument checks (csrc/host_scene.h: check_cast_counts, check_cast_list, both through
// check_row_query) for tests/test_cast_lists_checks.py: no HIP, no GPU, never loaded into python.  Compiled together with
// csrc/host_scene.cpp.
// stdin, one case per line:
//   ENTRY flags n p0 p1 p2 p3 capacity built     ENTRY: counts | list; the addresses are numbers and never dereferenced:
//       p0 d_casts, p1 d_counts (counts) or d_offsets (list), p2 d_words, p3 d_t (0: not given); counts reads p0, p1 only
// stdout per case: "status go|message" (message: mirt_last_error after the call, cleared before it).
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
    uint64_t a[4] = {0, 0, 0, 0};
    if (scanf("%" SCNu32 " %" SCNd64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %d", &flags, &n, &a[0], &a[1], &a[2], &a[3], &capacity,
              &built) != 8) return 1;
    const void* p[4];
    for (int i = 0; i < 4; ++i) p[i] = (const void*)(uintptr_t)a[i];
    bool go = false;
    int rc = -1;
    set_error("");
    if (!strcmp(entry, "counts")) rc = check_cast_counts(p[0], n, p[1], flags, built != 0, &go);
    else if (!strcmp(entry, "list")) rc = check_cast_list(p[0], n, p[1], p[2], p[3], capacity, flags, built != 0, &go);
    else return 1;
    printf("%d %d|%s\n", rc, go ? 1 : 0, g_last_error.c_str());
  }
  return 0;
}
