// Launch arithmetic of the query kernels (query.hip, light.hip, visibility.hip, indirect.hip, closest.hip, closest_multi.hip,
// spherecast.hip, overlap.hip, overlap_list.hip, query_lists.hip, multihit.hip): no HIP and no scene, so that a stand-alone host program can include
// it (tests/group_launch_probe.cpp, as tests/plan_probe.cpp includes render_plan.h).
#ifndef MIRT_QUERY_LAUNCH_H
#define MIRT_QUERY_LAUNCH_H

namespace mirt {

constexpr int QUERY_BLOCK = 256;
// the walk's stack entries kept in LDS ([entry][lane]): QUERY_STACK_LDS x 4 B x 64 lanes = 5 KiB per wave, 160 KiB per CU at 8
// waves per SIMD; deeper entries go to a per-lane private array (query_walk.h)
constexpr int QUERY_STACK_LDS = 20;

// A grouped kernel (one lane = one (row, item) pair; light.hip, visibility.hip, indirect.hip) gives each row G = 1 << gshift
// lanes of a wave, G the least power of two >= lanes_per_row (no item at all: G = 1).  A block then serves
// (QUERY_BLOCK / 64) * (64 / G) rows at a time, and the grid is as many blocks as n rows need, at most cached_blocks (the
// persistent grid that fills the device; the kernels stride over the rest).
struct GroupLaunch { int gshift; int blocks; };

inline GroupLaunch group_launch(long long n, int lanes_per_row, int cached_blocks)
{
  GroupLaunch g;
  g.gshift = 0;
  while ((1 << g.gshift) < lanes_per_row) ++g.gshift;
  const long long rows_per_block = (long long)(QUERY_BLOCK / 64) * (64 >> g.gshift);
  const long long want = (n + rows_per_block - 1) / rows_per_block;
  g.blocks = (int)(want < cached_blocks ? want : cached_blocks);
  return g;
}

// A kernel with one lane per row (query.hip, closest.hip, closest_multi.hip, spherecast.hip, overlap.hip, overlap_list.hip,
// query_lists.hip, multihit.hip, through scene_dev.h's launch_rows): as many blocks as n rows need, at most cached_blocks.
inline int row_launch(long long n, int cached_blocks)
{
  const long long want = (n + QUERY_BLOCK - 1) / QUERY_BLOCK;
  return (int)(want < cached_blocks ? want : cached_blocks);
}

} // namespace mirt

#endif
