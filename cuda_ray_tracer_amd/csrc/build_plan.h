// What the LBVH build (lbvh_build.hip) decides without the device: grid counts, the layout of its workspace, the ordered-key
// map of the scene bounds, and what the host concludes from the root record it reads back.  No HIP in here -- this header
// compiles with a plain host compiler, and tests/build_plan_probe.cpp runs it without a GPU (as plan_probe.cpp runs render_plan.h).
#ifndef MIRT_BUILD_PLAN_H
#define MIRT_BUILD_PLAN_H

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace mirt {

// child reference inside a packed node / the root reference (what the bits mean: scene_dev.h)
constexpr uint32_t REF_LEAF = 0x80000000u;
constexpr uint32_t REF_TRI = 0x40000000u;
constexpr uint32_t REF_OFFMASK = 0x0fffffffu;  // the record's offset in the heap, in 16-byte units: `ref << 4` is its byte offset (the shift drops the flags)
constexpr uint32_t REF_NONE = 0xf0000000u;   // no record (bits 29..28 are set in no real reference; offset bits 0)
// root: node 0, unless the whole scene is a single primitive (then its record, the first of the primitive region)
inline uint32_t tree_root_ref(int n, bool triangle, uint32_t prim_base16) { return n == 1 ? (REF_LEAF | (triangle ? REF_TRI : 0u) | prim_base16) : 0u; }

// ---- grids: blocks of 256 threads; the sort and the placement scan give a block a tile of 8 items per thread ----
constexpr int BUILD_BLOCK = 256;
constexpr int SORT_ITEMS = 8, SORT_TILE = BUILD_BLOCK * SORT_ITEMS;   // 2048 keys per workgroup; each wave owns 512 consecutive keys
constexpr int SCAN_ITEMS = 8, SCAN_TILE = BUILD_BLOCK * SCAN_ITEMS;
constexpr int RADIX = 256;                                            // digits of a sort pass
inline int blocks_of(long long items, int per_block) { return (int)((items + per_block - 1) / per_block); }
inline int item_blocks(long long items) { return blocks_of(items, BUILD_BLOCK); }   // kernels with one item per thread
inline int sort_blocks(long long n) { return blocks_of(n, SORT_TILE); }
inline int scan_blocks(long long n) { return blocks_of(n, SCAN_TILE); }

// ---- the workspace, in 32-bit words from its start ----
// The build of n >= 1 primitives: two key / value buffer pairs the sort passes alternate between, one pass's histogram
// [RADIX digits][sort_blocks] and RADIX row totals, and the refit's arrival counters (one per internal node).  block_sums
// (scan_blocks words, the placement scan's carries) is k1 again: the sort is over when the scan runs, and an even number of
// passes leaves its result in k0 / v0.  sort_pass_only: what sort_low_byte needs, a pass's histogram and totals alone.
struct BuildLayout { size_t k0, v0, k1, v1, hist, totals, arrived, block_sums, total; };
static_assert(SCAN_TILE >= 1, "block_sums fits in k1: ceil(n / SCAN_TILE) words never outnumber n");
inline BuildLayout build_layout(long long n, bool sort_pass_only = false)
{
  const size_t N = sort_pass_only ? 0 : (size_t)n;
  BuildLayout w;
  w.k0 = 0; w.v0 = N; w.k1 = 2 * N; w.v1 = 3 * N;
  w.hist = 4 * N;
  w.totals = w.hist + RADIX * (size_t)sort_blocks(n);
  w.arrived = w.totals + RADIX;
  w.total = w.arrived + (N > 1 ? N - 1 : 0);
  w.block_sums = w.k1;
  return w;
}
inline size_t sort_low_byte_ws_words(long long n) { return build_layout(n, true).total; }

// ---- ordered keys: an order-preserving float <-> uint map, so that atomicMin / atomicMax on uints realise float min / max ----
// (constexpr: host and device code both call them)
constexpr uint32_t f2key(float f) { const uint32_t u = __builtin_bit_cast(uint32_t, f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
constexpr float key2f(uint32_t k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// The six bounds keys (min xyz, max xyz) before prim_bounds_kernel folds the primitives in: the identities of atomicMin and
// atomicMax.  And as the shipped reference leaves them, which never stores the bounds it accumulates (parse.cpp:28):
// min = +inf, max = -inf, every Morton code 0.
constexpr uint32_t BOUNDS_KEYS_EMPTY[6] = {UINT32_MAX, UINT32_MAX, UINT32_MAX, 0u, 0u, 0u};
constexpr uint32_t BOUNDS_KEYS_SHIPPED[6] = {f2key(INFINITY), f2key(INFINITY), f2key(INFINITY), f2key(-INFINITY), f2key(-INFINITY), f2key(-INFINITY)};
static_assert(f2key(INFINITY) == 0xff800000u && f2key(-INFINITY) == 0x007fffffu && key2f(0x007fffffu) == -INFINITY, "the map orders and inverts");

// ---- the scene box, from the root record's two child boxes: left x, y | left z, right x | right y, z  (min, max pairs) ----
// coord_max: its largest coordinate magnitude (RenderArgs::reach_slack).  grid_ok: the grid of the quantised records resolves
// the scene's coordinates -- on every axis they stay below 64 extents, i.e. ulp(coordinate) below a quarter of a grid step.
// Only then do the outward-rounded quantised boxes cover what float rounding does to a primitive's own box planes and to a
// sphere's hit distance against them; a scene that fails the test -- one that sits far from the world
// origin compared with its size, or has a NaN in its box -- is walked over the exact records.
struct SceneBoxFacts { float coord_max; bool grid_ok; };
inline SceneBoxFacts scene_box_facts(const float rec[12])
{
  SceneBoxFacts f{0.0f, true};
  for (int i = 0; i < 12; ++i) f.coord_max = fmaxf(f.coord_max, fabsf(rec[i]));
  for (int k = 0; k < 3; ++k) {
    const float lo = fminf(rec[2 * k], rec[6 + 2 * k]), hi = fmaxf(rec[2 * k + 1], rec[6 + 2 * k + 1]);
    if (!(fmaxf(fabsf(lo), fabsf(hi)) <= 64.0f * (hi - lo))) f.grid_ok = false;
  }
  return f;
}

} // namespace mirt
#endif
