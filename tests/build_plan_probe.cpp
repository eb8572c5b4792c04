// Stand-alone probe of csrc/build_plan.h for tests/test_build_plan.py: no HIP, no GPU, never loaded into python.
// stdin: one case per line, a letter and its arguments (floats travel as their 32 bits in hex).  stdout: one line of name=value each.
//   L n                    the workspace layout and the grid counts of n primitives
//   K bits                 f2key of a float and key2f of that key
//   T                      the two tables of bounds keys, and what they are defined as
//   B bits x 12            scene_box_facts of a root record
//   R n triangle base16    tree_root_ref
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../cuda_ray_tracer_amd/csrc/build_plan.h"

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t as_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main()
{
  using namespace mirt;
  char what;
  while (scanf(" %c", &what) == 1) {
    if (what == 'L') {
      long long n;
      if (scanf("%lld", &n) != 1) return 1;
      const BuildLayout w = build_layout(n);
      printf("k0=%zu v0=%zu k1=%zu v1=%zu hist=%zu totals=%zu arrived=%zu block_sums=%zu total=%zu sort_ws=%zu item_blocks=%d inner_blocks=%d "
             "sort_blocks=%d scan_blocks=%d block=%d sort_tile=%d scan_tile=%d radix=%d\n",
             w.k0, w.v0, w.k1, w.v1, w.hist, w.totals, w.arrived, w.block_sums, w.total, sort_low_byte_ws_words(n), item_blocks(n), item_blocks(n - 1),
             sort_blocks(n), scan_blocks(n), BUILD_BLOCK, SORT_TILE, SCAN_TILE, RADIX);
    } else if (what == 'K') {
      uint32_t u;
      if (scanf("%" SCNx32, &u) != 1) return 1;
      const uint32_t k = f2key(as_float(u));
      printf("key=%" PRIu32 " back=%" PRIu32 "\n", k, as_bits(key2f(k)));
    } else if (what == 'T') {
      const uint32_t lo = f2key(as_float(0x7f800000u)), hi = f2key(as_float(0xff800000u));      // +inf, -inf
      for (int i = 0; i < 6; ++i) printf("empty%d=%" PRIu32 " shipped%d=%" PRIu32 " ", i, BOUNDS_KEYS_EMPTY[i], i, BOUNDS_KEYS_SHIPPED[i]);
      printf("key_pos_inf=%" PRIu32 " key_neg_inf=%" PRIu32 "\n", lo, hi);
    } else if (what == 'B') {
      float rec[12];
      for (float& v : rec) { uint32_t u; if (scanf("%" SCNx32, &u) != 1) return 1; v = as_float(u); }
      const SceneBoxFacts f = scene_box_facts(rec);
      printf("coord_max=%" PRIu32 " grid_ok=%d\n", as_bits(f.coord_max), (int)f.grid_ok);
    } else if (what == 'R') {
      int n, tri; uint32_t base16;
      if (scanf("%d %d %" SCNu32, &n, &tri, &base16) != 3) return 1;
      printf("root_ref=%" PRIu32 "\n", tree_root_ref(n, tri != 0, base16));
    } else {
      return 1;
    }
  }
  return 0;
}
