// LBVH build on the device: replaces build_lbvh_karas (lbvh_builder.cu:401-521) and
// build_morton_codes_and_sort_primitives (lbvh_utils.cu:77-129).
//
// The kernels by step of build_lbvh (the steps: bottom of the file; grids, workspace layout, host decisions: build_plan.h):
//   scene_bounds         prim_bounds_kernel: union of the primitive boxes (what parse.cpp:147-155,193-200 computes on the
//                        host and then drops -- reference bug #1; here the bounds are real)
//   sort_by_morton       morton_kernel: 30-bit codes (lbvh_utils.cu:10-75); radix_sort_pass x 4 = radix_pass_kernel<false> (count),
//                        row_scan_kernel, radix_pass_kernel<true> (scatter): stable LSD radix sort, 8 bits a pass, wave64 ballot
//                        ranking (replaces thrust::sort_by_key).  sort_low_byte is one such pass, for render.hip
//   hierarchy_and_depth  karras_kernel: Karras 2012 hierarchy with the reference's index tie-break (lbvh_builder.cu:76-322);
//                        tree_depth_kernel: the most internal nodes on a root-to-leaf path
//   place_primitives     tri_scan_kernel<false>, scan_sums_kernel, tri_scan_kernel<true>: exclusive scan of the triangle flags in
//                        sorted order (where each sorted leaf's record goes in the heap, which subtrees hold spheres only;
//                        the block scan itself: block_scan.h, shared with overlap_list.hip);
//                        scatter_prims_kernel: the records into the heap in that order (neighbours in space, neighbours in memory)
//   refit_and_pack       refit_pack_kernel: bottom-up boxes (lbvh_builder.cu:324-387, with the missing release/acquire added)
//                        and 64-byte two-child node records for the traversal kernel
//   pack_quantised       pack_qnodes_kernel, pack_wnodes_kernel: the 32-byte and the wide records on the scene-bounds grid
#include "scene_dev.h"
#include "block_scan.h"

#include <algorithm>
#include <utility>

namespace mirt {

namespace {

constexpr int BLOCK = BUILD_BLOCK;

// One-dimensional launches of BLOCK threads: `blocks` of them, or as many as `items` need at one item per thread.
template <class... P, class... A>
void launch_blocks(void (*kernel)(P...), int blocks, hipStream_t stream, A&&... args)
{
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(BLOCK), 0, stream, static_cast<P>(args)...);
}
template <class K, class... A>
void launch_items(K kernel, long long items, hipStream_t stream, A&&... args) { launch_blocks(kernel, item_blocks(items), stream, args...); }

struct Box { float xmin, xmax, ymin, ymax, zmin, zmax; };

// get_primitive_aabb_device, lbvh_builder.cu:33-57 with AABB ctors interval.cuh:55-81
MIRT_DEV Box prim_box(uint32_t type, uint32_t id, const float4* __restrict__ spheres, const float4* __restrict__ tri_verts)
{
  Box b;
  if (type == 0) {
    const float4 s = spheres[id];
    const float ax = s.x - s.w, bx = s.x + s.w;
    const float ay = s.y - s.w, by = s.y + s.w;
    const float az = s.z - s.w, bz = s.z + s.w;
    if (ax <= bx) { b.xmin = ax; b.xmax = bx; } else { b.xmin = bx; b.xmax = ax; }
    if (ay <= by) { b.ymin = ay; b.ymax = by; } else { b.ymin = by; b.ymax = ay; }
    if (az <= bz) { b.zmin = az; b.zmax = bz; } else { b.zmin = bz; b.zmax = az; }
  } else {
    const float4 p0 = tri_verts[3 * (size_t)id + 0], p1 = tri_verts[3 * (size_t)id + 1], p2 = tri_verts[3 * (size_t)id + 2];
    b.xmin = fminf(fminf(p0.x, p1.x), p2.x); b.xmax = fmaxf(fmaxf(p0.x, p1.x), p2.x);
    b.ymin = fminf(fminf(p0.y, p1.y), p2.y); b.ymax = fmaxf(fmaxf(p0.y, p1.y), p2.y);
    b.zmin = fminf(fminf(p0.z, p1.z), p2.z); b.zmax = fmaxf(fmaxf(p0.z, p1.z), p2.z);
    if (b.xmax - b.xmin < 0.01f) { b.xmin = b.xmin - 0.01f; b.xmax = b.xmax + 0.01f; }
    if (b.ymax - b.ymin < 0.01f) { b.ymin = b.ymin - 0.01f; b.ymax = b.ymax + 0.01f; }
    if (b.zmax - b.zmin < 0.01f) { b.zmin = b.zmin - 0.01f; b.zmax = b.zmax + 0.01f; }
  }
  return b;
}

__global__ void __launch_bounds__(BLOCK) prim_bounds_kernel(const MirtPrimRef* __restrict__ refs, const float4* __restrict__ spheres,
                                                            const float4* __restrict__ tri_verts, int n, uint32_t* __restrict__ keys)
{
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
    const MirtPrimRef r = refs[i];
    const Box b = prim_box(r.type, r.id, spheres, tri_verts);
    mn[0] = fminf(mn[0], b.xmin); mx[0] = fmaxf(mx[0], b.xmax);
    mn[1] = fminf(mn[1], b.ymin); mx[1] = fmaxf(mx[1], b.ymax);
    mn[2] = fminf(mn[2], b.zmin); mx[2] = fmaxf(mx[2], b.zmax);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      mn[k] = fminf(mn[k], __shfl_xor(mn[k], off));
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off));
    }
  // one set of atomics per block (the six words are hot: every block of the grid hits them)
  __shared__ float red[BLOCK / 64][6];
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { red[wv][k] = mn[k]; red[wv][3 + k] = mx[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = red[0][threadIdx.x];
    for (int i = 1; i < BLOCK / 64; ++i) v = (threadIdx.x < 3) ? fminf(v, red[i][threadIdx.x]) : fmaxf(v, red[i][threadIdx.x]);
    if (threadIdx.x < 3) atomicMin(&keys[threadIdx.x], f2key(v));
    else atomicMax(&keys[threadIdx.x], f2key(v));
  }
}

// lbvh_utils.cu:10-30
MIRT_DEV uint32_t expand_bits(uint32_t v)
{
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}
MIRT_DEV uint32_t quantize_coordinate(float coord, float smin, float range)
{
  if (range <= 1e-6f) return 0;
  float normalized = (coord - smin) / range;
  normalized = fmaxf(0.0f, fminf(1.0f, normalized));
  return (uint32_t)(normalized * 1023);
}

// generate_morton_codes_kernel, lbvh_utils.cu:32-75
__global__ void __launch_bounds__(BLOCK) morton_kernel(const MirtPrimRef* __restrict__ refs, const float4* __restrict__ spheres,
                                                       const float4* __restrict__ tri_verts, int n, const uint32_t* __restrict__ bkeys,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const float mnx = key2f(bkeys[0]), mny = key2f(bkeys[1]), mnz = key2f(bkeys[2]);
  const float mxx = key2f(bkeys[3]), mxy = key2f(bkeys[4]), mxz = key2f(bkeys[5]);
  const MirtPrimRef r = refs[i];
  float cx, cy, cz;
  if (r.type == 0) {
    const float4 s = spheres[r.id];
    cx = s.x; cy = s.y; cz = s.z;
  } else {
    const float4 p0 = tri_verts[3 * (size_t)r.id + 0], p1 = tri_verts[3 * (size_t)r.id + 1], p2 = tri_verts[3 * (size_t)r.id + 2];
    cx = ((p0.x + p1.x) + p2.x) / 3.0f;
    cy = ((p0.y + p1.y) + p2.y) / 3.0f;
    cz = ((p0.z + p1.z) + p2.z) / 3.0f;
  }
  const uint32_t qx = quantize_coordinate(cx, mnx, mxx - mnx);
  const uint32_t qy = quantize_coordinate(cy, mny, mxy - mny);
  const uint32_t qz = quantize_coordinate(cz, mnz, mxz - mnz);
  keys[i] = expand_bits(qx) | (expand_bits(qy) << 1) | (expand_bits(qz) << 2);
  vals[i] = (uint32_t)i;
}

// ---- stable LSD radix sort (SORT_TILE keys per workgroup, build_plan.h) ------------------------------
static_assert(RADIX == BLOCK, "one thread per digit");
template <bool SCATTER>
__global__ void __launch_bounds__(BLOCK) radix_pass_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                                                           uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out,
                                                           uint32_t* __restrict__ hist, const uint32_t* __restrict__ offsets,
                                                           const uint32_t* __restrict__ totals, int n, int shift, int nblocks)
{
  __shared__ uint32_t wcnt[4][256];
  __shared__ uint32_t dbase[256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < 4 * 256; i += BLOCK) (&wcnt[0][0])[i] = 0;
  __syncthreads();

  const int base = blockIdx.x * SORT_TILE + wave * (SORT_ITEMS * 64);
  uint32_t key[SORT_ITEMS], rank[SORT_ITEMS];
  const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int it = 0; it < SORT_ITEMS; ++it) {
    const int idx = base + it * 64 + lane;
    const bool valid = idx < n;
    key[it] = valid ? keys_in[idx] : 0xffffffffu;
    const uint32_t digit = (key[it] >> shift) & 255u;
    unsigned long long mask = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (digit >> b) & 1u;
      const unsigned long long bal = __ballot(valid && bit);
      mask &= bit ? bal : ~bal;
    }
    const uint32_t r = (uint32_t)__popcll(mask & lt);
    const uint32_t c = (uint32_t)__popcll(mask);
    uint32_t prev = 0;
    if (valid) prev = wcnt[wave][digit];
    rank[it] = prev + r;
    __builtin_amdgcn_wave_barrier();
    if (valid && r == 0) wcnt[wave][digit] = prev + c;
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  const uint32_t c0 = wcnt[0][tid], c1 = wcnt[1][tid], c2 = wcnt[2][tid], c3 = wcnt[3][tid];
  if (!SCATTER) {
    hist[(size_t)tid * nblocks + blockIdx.x] = c0 + c1 + c2 + c3;
    return;
  }
  // exclusive scan of the 256 digit totals (every block repeats it: 256 values)
  const uint32_t off = block_exclusive_scan<BLOCK>(totals[tid], dbase, nullptr) + offsets[(size_t)tid * nblocks + blockIdx.x];
  wcnt[0][tid] = off; wcnt[1][tid] = off + c0; wcnt[2][tid] = off + c0 + c1; wcnt[3][tid] = off + c0 + c1 + c2;
  __syncthreads();
#pragma unroll
  for (int it = 0; it < SORT_ITEMS; ++it) {
    const int idx = base + it * 64 + lane;
    if (idx < n) {
      const uint32_t digit = (key[it] >> shift) & 255u;
      const uint32_t pos = wcnt[wave][digit] + rank[it];
      keys_out[pos] = key[it];
      vals_out[pos] = vals_in ? vals_in[idx] : (uint32_t)idx;      // (no values: the position itself)
    }
  }
}

// hist is [256 digits][nblocks].  Block d scans row d in place (exclusive) and writes the row total to totals[d]; the
// scatter kernel adds the exclusive scan of the 256 totals (done per block in LDS).
__global__ void __launch_bounds__(BLOCK) row_scan_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ totals, int nblocks)
{
  __shared__ uint32_t sums[BLOCK];
  const int tid = threadIdx.x;
  uint32_t* row = hist + (size_t)blockIdx.x * nblocks;
  const int chunk = (nblocks + BLOCK - 1) / BLOCK;
  const int lo = tid * chunk, hi = min(lo + chunk, nblocks);
  uint32_t s = 0;
  for (int i = lo; i < hi; ++i) s += row[i];
  uint32_t run = block_exclusive_scan<BLOCK>(s, sums, nullptr);
  if (tid == BLOCK - 1) totals[blockIdx.x] = run + s;
  for (int i = lo; i < hi; ++i) { const uint32_t v = row[i]; row[i] = run; run += v; }
}

// ---- Karras hierarchy ------------------------------------------------------------------------------
MIRT_DEV int clz32(uint32_t x) { return x ? __clz((int)x) : 32; }
// adapted_delta, lbvh_builder.cu:76-101
MIRT_DEV int delta(int a, int b, int n, const uint32_t* __restrict__ codes)
{
  if (a < 0 || a >= n || b < 0 || b >= n) return -1;
  const uint32_t ka = codes[a], kb = codes[b];
  if (ka == kb) return 32 + clz32((uint32_t)a ^ (uint32_t)b);
  return clz32(ka ^ kb);
}

// generate_internal_nodes_karas_kernel, lbvh_builder.cu:224-322 (+ determine_range_adapted :103-182,
// find_split_adapted :186-221).  Children use the reference numbering: internal i in [0,N-2], leaf j -> N-1+j.
__global__ void __launch_bounds__(BLOCK) karras_kernel(const uint32_t* __restrict__ codes, int n, uint32_t* __restrict__ child_l,
                                                       uint32_t* __restrict__ child_r, int* __restrict__ parent, uint2* __restrict__ range)
{
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n - 1) return;
  // range
  const int dl = delta(i, i - 1, n, codes), dr = delta(i, i + 1, n, codes);
  int d, dmin;
  if (dr > dl) { d = 1; dmin = dl; } else { d = -1; dmin = dr; }
  uint32_t lmax = 1;
  int nb = (int)((uint32_t)i + lmax * (uint32_t)d);
  int cur = delta(i, nb, n, codes);
  while (cur > dmin) {
    lmax <<= 1;
    nb = (int)((uint32_t)i + lmax * (uint32_t)d);
    if (nb < 0 || nb >= n) break;
    cur = delta(i, nb, n, codes);
  }
  uint32_t l = 0;
  for (uint32_t t = lmax >> 1; t > 0; t >>= 1) {
    const int nbb = (int)((uint32_t)i + (l + t) * (uint32_t)d);
    if (nbb >= 0 && nbb < n) {
      if (delta(i, nbb, n, codes) > dmin) l += t;
    }
  }
  const int j = (int)((uint32_t)i + l * (uint32_t)d);
  const int first = (i < j) ? i : j, last = (i < j) ? j : i;
  range[i] = make_uint2((uint32_t)first, (uint32_t)last);
  // split
  int split = first;
  if (first != last) {
    const int common = delta(first, last, n, codes);
    int step = last - first;
    do {
      step = (step + 1) >> 1;
      const int cand = split + step;
      if (cand < last) {
        if (delta(first, cand, n, codes) > common) split = cand;
      }
    } while (step > 1);
  }
  if (split < first || split >= last) {   // cannot happen for a valid range; mirror the reference's marker
    child_l[i] = 0xffffffffu; child_r[i] = 0xffffffffu;
    return;
  }
  const uint32_t leaf_base = (uint32_t)(n - 1);
  const int d_split = delta(split, split + 1, n, codes);
  uint32_t lc, rc;
  if (split == first) lc = leaf_base + (uint32_t)split;
  else lc = (delta(first, split, n, codes) > d_split) ? (uint32_t)split : leaf_base + (uint32_t)first;
  if (split + 1 == last) rc = leaf_base + (uint32_t)last;
  else rc = (delta(split + 1, last, n, codes) > d_split) ? (uint32_t)(split + 1) : leaf_base + (uint32_t)last;
  child_l[i] = lc; child_r[i] = rc;
  parent[lc] = i; parent[rc] = i;
  if (i == 0) parent[0] = -1;
}

// ---- where the primitive records go: exclusive scan of the triangle flags over the sorted leaves ------------------------
// Sorted leaf j's record starts at unit j + 2 * tris_before[j] of the primitive region (a sphere is one 16-byte unit, a
// triangle three), and leaves [f, l] hold spheres only iff tris_before[l + 1] == tris_before[f].  SCAN_TILE leaves per workgroup.
template <bool WRITE>
__global__ void __launch_bounds__(BLOCK) tri_scan_kernel(int n, const uint32_t* __restrict__ order, const MirtPrimRef* __restrict__ refs,
                                                         uint32_t* __restrict__ block_sums, uint32_t* __restrict__ tris_before)
{
  __shared__ uint32_t sh[BLOCK];
  const int base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  uint32_t f[SCAN_ITEMS], s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    const int j = base + k;
    f[k] = (j < n) ? (refs[order[j]].type != 0 ? 1u : 0u) : 0u;
    s += f[k];
  }
  uint32_t total;
  uint32_t run = block_exclusive_scan<BLOCK>(s, sh, &total);
  if (!WRITE) { if (threadIdx.x == 0) block_sums[blockIdx.x] = total; return; }
  run += block_sums[blockIdx.x];                // exclusive prefix of the blocks before this one
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    const int j = base + k;
    if (j < n) tris_before[j] = run;
    run += f[k];
    if (j == n - 1) tris_before[n] = run;
  }
}
// one block: block_sums -> exclusive prefix, in place
__global__ void __launch_bounds__(BLOCK) scan_sums_kernel(uint32_t* __restrict__ block_sums, int nb)
{
  __shared__ uint32_t sh[BLOCK];
  uint32_t carry = 0;
  for (int b0 = 0; b0 < nb; b0 += BLOCK) {
    const int i = b0 + threadIdx.x;
    const uint32_t v = (i < nb) ? block_sums[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan<BLOCK>(v, sh, &total);
    if (i < nb) block_sums[i] = carry + ex;
    carry += total;
  }
}

// reference to child `node` (reference numbering: internal [0, N-2], leaf j -> N-1+j) as the traversal kernels want it
MIRT_DEV uint32_t make_ref(uint32_t node, uint32_t leaf_base, const uint32_t* __restrict__ order, const MirtPrimRef* __restrict__ refs,
                           const uint32_t* __restrict__ tris_before, const uint2* __restrict__ range, uint32_t prim_base16, bool* pure)
{
  if (node >= leaf_base) {
    const uint32_t j = node - leaf_base;
    const bool tri = refs[order[j]].type != 0;
    *pure = !tri;
    return REF_LEAF | (tri ? REF_TRI : 0u) | (prim_base16 + j + 2u * tris_before[j]);
  }
  const uint2 fl = range[node];
  *pure = tris_before[fl.y + 1] == tris_before[fl.x];
  return 4u * node;
}

// The grid of the quantised records: QGRID steps across the scene bounds on every axis (a flat axis: step 1).
struct QuantGrid { float smin[3], step[3]; };
MIRT_DEV QuantGrid quant_grid(const uint32_t* __restrict__ bkeys)
{
  QuantGrid g;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    g.smin[k] = key2f(bkeys[k]);
    const float range = key2f(bkeys[3 + k]) - g.smin[k];
    g.step[k] = range > 0.0f ? range / QGRID : 1.0f;
  }
  return g;
}
// what the walk needs of it (RenderArgs::qparams): origin, step, 2^60 / step
MIRT_DEV void write_qparams(float* __restrict__ qparams, const QuantGrid& g)
{
  for (int k = 0; k < 3; ++k) { qparams[k] = g.smin[k]; qparams[3 + k] = g.step[k]; qparams[6 + k] = QINV_STEPS / g.step[k]; }
}
// a box (xmin, xmax, ymin, ymax, zmin, zmax) as three words (lo | hi << 16), rounded outwards (qlo, qhi: scene_dev.h)
MIRT_DEV void pack_box_words(const float* __restrict__ box, const QuantGrid& g, uint32_t* w3)
{
#pragma unroll
  for (int k = 0; k < 3; ++k) w3[k] = qlo(box[2 * k], g.smin[k], g.step[k]) | (qhi(box[2 * k + 1], g.smin[k], g.step[k]) << 16);
}

// Quantised node records (scene_dev.h): both child boxes on the grid, then the two references.
__global__ void __launch_bounds__(BLOCK) pack_qnodes_kernel(int n, const uint32_t* __restrict__ bkeys, const uint32_t* __restrict__ child_l,
                                                            const uint32_t* __restrict__ child_r, const float* __restrict__ boxes,
                                                            const uint32_t* __restrict__ order, const MirtPrimRef* __restrict__ refs,
                                                            const uint32_t* __restrict__ tris_before, const uint2* __restrict__ range,
                                                            uint4* __restrict__ qnodes, float* __restrict__ qparams, uint32_t qbase16, uint32_t prim_base16)
{
  const int p = blockIdx.x * BLOCK + threadIdx.x;
  const QuantGrid g = quant_grid(bkeys);
  if (p == 0) write_qparams(qparams, g);
  if (p >= n - 1) return;
  const uint32_t leaf_base = (uint32_t)(n - 1);
  const uint32_t c[2] = {child_l[p], child_r[p]};
  uint32_t w[8];
  bool pure[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    pack_box_words(boxes + 6 * (size_t)c[s], g, w + 3 * s);
    const uint32_t r = make_ref(c[s], leaf_base, order, refs, tris_before, range, prim_base16, &pure[s]);
    w[6 + s] = c[s] >= leaf_base ? r : (qbase16 + 2u * c[s]);
  }
  if (pure[0] && pure[1]) w[6] |= REF_QPURE;
  qnodes[2 * (size_t)p + 0] = make_uint4(w[0], w[1], w[2], w[3]);
  qnodes[2 * (size_t)p + 1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// Wide quantised records (scene_dev.h): the grandchildren of every internal node, in the reference's visiting order.
__global__ void __launch_bounds__(BLOCK) pack_wnodes_kernel(int n, const uint32_t* __restrict__ bkeys, const uint32_t* __restrict__ child_l,
                                                            const uint32_t* __restrict__ child_r, const float* __restrict__ boxes,
                                                            const uint32_t* __restrict__ order, const MirtPrimRef* __restrict__ refs,
                                                            const uint32_t* __restrict__ tris_before, const uint2* __restrict__ range,
                                                            uint4* __restrict__ wnodes, float* __restrict__ qparams, uint32_t wbase16, uint32_t prim_base16)
{
  const int p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= n - 1) return;
  const QuantGrid g = quant_grid(bkeys);
  if (p == 0) write_qparams(qparams, g);
  const uint32_t leaf_base = (uint32_t)(n - 1);
  uint32_t kids[4];
  int nk = 0;
  const uint32_t two[2] = {child_l[p], child_r[p]};
  for (int s = 0; s < 2; ++s) {
    if (two[s] >= leaf_base) kids[nk++] = two[s];
    else { kids[nk++] = child_l[two[s]]; kids[nk++] = child_r[two[s]]; }
  }
  uint32_t w[16];
  for (int i = 0; i < 4; ++i) {
    if (i < nk) {
      pack_box_words(boxes + 6 * (size_t)kids[i], g, w + 3 * i);
      bool pure;
      const uint32_t r = make_ref(kids[i], leaf_base, order, refs, tris_before, range, prim_base16, &pure);
      w[12 + i] = kids[i] >= leaf_base ? r : (wbase16 + 4u * kids[i]);
    } else {
      w[3 * i + 0] = QBOX_NONE; w[3 * i + 1] = QBOX_NONE; w[3 * i + 2] = QBOX_NONE;
      w[12 + i] = REF_NONE;
    }
  }
  for (int i = 0; i < 4; ++i) wnodes[4 * (size_t)p + i] = make_uint4(w[4 * i + 0], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}

// primitive records in sorted order + the unit -> primitive map the shading code uses to find the material
__global__ void __launch_bounds__(BLOCK) scatter_prims_kernel(int n, const uint32_t* __restrict__ order, const MirtPrimRef* __restrict__ refs,
                                                              const uint32_t* __restrict__ tris_before, const float4* __restrict__ spheres,
                                                              const float4* __restrict__ tris, float4* __restrict__ prim_region,
                                                              uint32_t* __restrict__ unit_prim)
{
  const int j = blockIdx.x * BLOCK + threadIdx.x;
  if (j >= n) return;
  const MirtPrimRef r = refs[order[j]];
  const size_t unit = (size_t)j + 2 * (size_t)tris_before[j];
  if (r.type == 0) {
    prim_region[unit] = spheres[r.id];
    unit_prim[unit] = r.id;
  } else {
    prim_region[unit + 0] = tris[3 * (size_t)r.id + 0];
    prim_region[unit + 1] = tris[3 * (size_t)r.id + 1];
    prim_region[unit + 2] = tris[3 * (size_t)r.id + 2];
    unit_prim[unit + 0] = 0x80000000u | r.id; unit_prim[unit + 1] = 0x80000000u | r.id; unit_prim[unit + 2] = 0x80000000u | r.id;
  }
}

// D, the most internal nodes on a root-to-leaf path: one thread per leaf counts the parent links up to the root, one atomic
// per wave.  It bounds the stack of a binary walk (render.hip, MIRT_PUSH), so the render plan can pick a kernel whose stack
// never leaves LDS.  (A link that was never written is -1 like the root's: the count stops there.  The tree is at most 58
// levels deep; the cap only bounds the loop.)
__global__ void __launch_bounds__(BLOCK) tree_depth_kernel(int n, const int* __restrict__ parent, uint32_t* __restrict__ depth)
{
  const int j = blockIdx.x * BLOCK + threadIdx.x;
  uint32_t d = 0;
  if (j < n) {
    int p = parent[n - 1 + j];
    while (p >= 0 && p < n - 1 && d < 255u) { ++d; p = parent[p]; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) d = max(d, (uint32_t)__shfl_xor((int)d, off));
  if ((threadIdx.x & 63) == 0 && d > 0) atomicMax(depth, d);
}

// The refit hand-off's box traffic (refit_pack_kernel, below): every word of a box stored write-through -- a relaxed
// agent-scope atomic store -- and every word loaded past the L1 -- a relaxed agent-scope atomic load.
MIRT_DEV void store_wt(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
MIRT_DEV float load_bypass(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
MIRT_DEV void store_box_wt(float* p, const Box& b)
{
  store_wt(p + 0, b.xmin); store_wt(p + 1, b.xmax); store_wt(p + 2, b.ymin); store_wt(p + 3, b.ymax); store_wt(p + 4, b.zmin); store_wt(p + 5, b.zmax);
}
MIRT_DEV Box load_box_bypass(const float* p)
{
  return {load_bypass(p + 0), load_bypass(p + 1), load_bypass(p + 2), load_bypass(p + 3), load_bypass(p + 4), load_bypass(p + 5)};
}
// AABB(AABB, AABB), interval.cuh:83-88 (the left child's operand first)
MIRT_DEV Box box_union(const Box& a, const Box& c)
{
  return {fminf(a.xmin, c.xmin), fmaxf(a.xmax, c.xmax), fminf(a.ymin, c.ymin), fmaxf(a.ymax, c.ymax), fminf(a.zmin, c.zmin), fmaxf(a.zmax, c.zmax)};
}

// set_aabb_kernel_adapted, lbvh_builder.cu:324-387.  One thread per leaf; the second thread to arrive at a parent
// merges the children.  The box stores are published before the arrival counter is bumped, see below (the reference
// has no fence there).  The merging thread also writes the parent's packed traversal record.
__global__ void __launch_bounds__(BLOCK) refit_pack_kernel(int n, const uint32_t* __restrict__ order, const MirtPrimRef* __restrict__ refs,
                                                           const float4* __restrict__ spheres, const float4* __restrict__ tri_verts,
                                                           const uint32_t* __restrict__ child_l, const uint32_t* __restrict__ child_r,
                                                           const int* __restrict__ parent, uint32_t* __restrict__ arrived,
                                                           float* boxes, float4* __restrict__ nodes, const uint32_t* __restrict__ tris_before,
                                                           const uint2* __restrict__ range, uint32_t prim_base16, float4* __restrict__ tri_boxes)
{
  const int j = blockIdx.x * BLOCK + threadIdx.x;
  if (j >= n) return;
  const uint32_t leaf_base = (uint32_t)(n - 1);
  uint32_t cur = leaf_base + (uint32_t)j;
  const MirtPrimRef r = refs[order[j]];
  const Box b = prim_box(r.type, r.id, spheres, tri_verts);
  if (r.type != 0) {      // the triangle's exact leaf box, by scene index (the quantised walk's triangle check, render.hip)
    tri_boxes[2 * (size_t)r.id + 0] = make_float4(b.xmin, b.xmax, b.ymin, b.ymax);
    tri_boxes[2 * (size_t)r.id + 1] = make_float4(b.zmin, b.zmax, 0.0f, 0.0f);
  }
  // Hand-off protocol (MI355X guide, "sc1 stores and loads on both sides"): every box word is written with a write-through
  // (agent-scope atomic) store and drained with s_waitcnt vmcnt(0) before the arrival counter is bumped; the second arriver
  // learns from the value its own add returned that the sibling's box is out, and reads it with L1-bypassing loads.
  // No cache-wide release/acquire fences: they cost microseconds per tree level.
  store_box_wt(boxes + 6 * (size_t)cur, b);
  int p = parent[cur];
  while (p != -1 && p < n - 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t prev = __hip_atomic_fetch_add(&arrived[p], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == 0) break;
    const uint32_t lc = child_l[p], rc = child_r[p];
    const Box a = load_box_bypass(boxes + 6 * (size_t)lc), c = load_box_bypass(boxes + 6 * (size_t)rc);
    // traversal record: both child boxes as (min, max) pairs per axis (the slab test works on pairs) + child references
    float4* rec = nodes + 4 * (size_t)p;
    rec[0] = make_float4(a.xmin, a.xmax, a.ymin, a.ymax);
    rec[1] = make_float4(a.zmin, a.zmax, c.xmin, c.xmax);
    rec[2] = make_float4(c.ymin, c.ymax, c.zmin, c.zmax);
    bool pure_l, pure_r;
    const uint32_t ref_l = make_ref(lc, leaf_base, order, refs, tris_before, range, prim_base16, &pure_l);
    const uint32_t ref_r = make_ref(rc, leaf_base, order, refs, tris_before, range, prim_base16, &pure_r);
    rec[3] = make_float4(__uint_as_float(ref_l), __uint_as_float(ref_r),
                         __uint_as_float(NODE_SWAP_ANY | ((pure_l && pure_r) ? NODE_SWAP_PURE : 0u)), 0.0f);
    store_box_wt(boxes + 6 * (size_t)p, box_union(a, c));
    cur = (uint32_t)p;
    p = parent[cur];
  }
}

// One stable pass over the 8 key bits from `shift`: count per tile, scan every digit's row of counts, scatter.  vals_in == null:
// the values are the positions.  The pass's histogram and totals lie in ws where `at` says (BuildLayout, build_plan.h).
void radix_sort_pass(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out, uint32_t* ws, const BuildLayout& at,
                     int n, int shift, hipStream_t stream)
{
  const int sblocks = sort_blocks(n);
  uint32_t *hist = ws + at.hist, *totals = ws + at.totals;
  launch_blocks(radix_pass_kernel<false>, sblocks, stream, keys_in, vals_in, keys_out, vals_out, hist, hist, totals, n, shift, sblocks);
  launch_blocks(row_scan_kernel, RADIX, stream, hist, totals, sblocks);
  launch_blocks(radix_pass_kernel<true>, sblocks, stream, keys_in, vals_in, keys_out, vals_out, hist, hist, totals, n, shift, sblocks);
}

// The whole sort: four stable passes over the n keys in k0 with their values in v0 (BuildLayout) -- an even number, so keys and
// values end where they started, in k0 / v0
void radix_sort_keys(uint32_t* ws, const BuildLayout& at, int n, hipStream_t stream)
{
  uint32_t *ki = ws + at.k0, *vi = ws + at.v0, *ko = ws + at.k1, *vo = ws + at.v1;
  for (int pass = 0; pass < 4; ++pass) {
    radix_sort_pass(ki, vi, ko, vo, ws, at, n, 8 * pass, stream);
    std::swap(ki, ko); std::swap(vi, vo);
  }
}

} // namespace

// One stable radix pass over the low byte of the keys (render.hip orders a frame's samples by cost class with it): keys_out /
// vals_out receive the keys and their original positions in ascending key order.  ws: sort_low_byte_ws_words(n) words.
int sort_low_byte(const uint32_t* keys_in, uint32_t* keys_out, uint32_t* vals_out, long long n, uint32_t* ws, hipStream_t stream)
{
  radix_sort_pass(keys_in, nullptr, keys_out, vals_out, ws, build_layout(n, true), (int)n, 0, stream);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

// ---- the steps of a build of n >= 1 primitives, in stream order ---------------------------------------
namespace {

struct Build {
  MirtScene* sc; int n; hipStream_t stream;
  uint32_t* ws; BuildLayout at;      // sc->build_ws and what lies where in it
  int scene_bounds() const, sort_by_morton() const, hierarchy_and_depth() const, read_back_scene_facts() const;
  void place_primitives() const, refit_and_pack() const, pack_quantised() const;
};

int Build::scene_bounds() const
{
  const bool shipped = sc->opt.bounds_as_shipped != 0;
  MIRT_HIP(hipMemcpyAsync(sc->bounds_keys, shipped ? BOUNDS_KEYS_SHIPPED : BOUNDS_KEYS_EMPTY, sizeof(BOUNDS_KEYS_EMPTY), hipMemcpyHostToDevice, stream));
  // (a grid-stride kernel: one set of atomics per block, at most 512 of them)
  if (!shipped) launch_blocks(prim_bounds_kernel, std::min(item_blocks(n), 512), stream, sc->refs_in, sc->spheres, sc->tri_verts, n, sc->bounds_keys);
  return MIRT_OK;
}

// Morton codes and positions into k0 / v0, the sort, and its result out of k0 / v0
int Build::sort_by_morton() const
{
  uint32_t *codes = ws + at.k0, *order = ws + at.v0;
  launch_items(morton_kernel, n, stream, sc->refs_in, sc->spheres, sc->tri_verts, n, sc->bounds_keys, codes, order);
  radix_sort_keys(ws, at, n, stream);
  MIRT_HIP(hipMemcpyAsync(sc->codes, codes, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, stream));
  MIRT_HIP(hipMemcpyAsync(sc->order, order, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, stream));
  return MIRT_OK;
}

// the hierarchy, the refit's arrival counters zeroed, and the tree's depth for the render plan (every build: a rebuild changes the topology)
int Build::hierarchy_and_depth() const
{
  if (n == 1) { MIRT_HIP(hipMemsetAsync(sc->parent, 0xff, sizeof(int), stream)); return MIRT_OK; }
  MIRT_HIP(hipMemsetAsync(ws + at.arrived, 0, sizeof(uint32_t) * (n - 1), stream));
  MIRT_HIP(hipMemsetAsync(sc->parent, 0xff, sizeof(int) * (2 * (size_t)n - 1), stream));
  launch_items(karras_kernel, n - 1, stream, sc->codes, n, sc->child_l, sc->child_r, sc->parent, sc->range);
  MIRT_HIP(hipMemsetAsync(sc->depth_dev, 0, sizeof(uint32_t), stream));
  launch_items(tree_depth_kernel, n, stream, n, sc->parent, sc->depth_dev);
  return MIRT_OK;
}

// heap placement of the sorted leaves (the sort is over: the block sums live in its k1, BuildLayout)
void Build::place_primitives() const
{
  const int sblocks = scan_blocks(n);
  uint32_t* const block_sums = ws + at.block_sums;
  launch_blocks(tri_scan_kernel<false>, sblocks, stream, n, sc->order, sc->refs_in, block_sums, sc->tris_before);
  launch_blocks(scan_sums_kernel, 1, stream, block_sums, sblocks);
  launch_blocks(tri_scan_kernel<true>, sblocks, stream, n, sc->order, sc->refs_in, block_sums, sc->tris_before);
  launch_items(scatter_prims_kernel, n, stream, n, sc->order, sc->refs_in, sc->tris_before, sc->spheres, sc->tris,
               reinterpret_cast<float4*>(sc->heap + sc->prim_base), sc->unit_prim);
}

void Build::refit_and_pack() const
{
  launch_items(refit_pack_kernel, n, stream, n, sc->order, sc->refs_in, sc->spheres, sc->tri_verts, sc->child_l, sc->child_r, sc->parent,
               ws + at.arrived, sc->boxes, sc->nodes, sc->tris_before, sc->range, sc->prim_base / 16u, sc->tri_boxes);
}

// the quantised records the scene has room for (none for a single primitive, none on the shipped reference's empty bounds)
void Build::pack_quantised() const
{
  const bool offered = n > 1 && !sc->opt.bounds_as_shipped;
  sc->root_ref_q = sc->root_ref_w = REF_NONE;
  if (sc->qnode_base && offered) {
    launch_items(pack_qnodes_kernel, n - 1, stream, n, sc->bounds_keys, sc->child_l, sc->child_r, sc->boxes, sc->order, sc->refs_in, sc->tris_before,
                 sc->range, reinterpret_cast<uint4*>(sc->heap + sc->qnode_base), sc->qparams, sc->qnode_base / 16u, sc->prim_base / 16u);
    sc->root_ref_q = sc->qnode_base / 16u;
  }
  if (sc->wnode_base && offered) {
    launch_items(pack_wnodes_kernel, n - 1, stream, n, sc->bounds_keys, sc->child_l, sc->child_r, sc->boxes, sc->order, sc->refs_in, sc->tris_before,
                 sc->range, reinterpret_cast<uint4*>(sc->heap + sc->wnode_base), sc->qparams, sc->wnode_base / 16u, sc->prim_base / 16u);
    sc->root_ref_w = sc->wnode_base / 16u;
  }
}

// after the synchronise: the tree's depth, what the root record says about the scene box (scene_box_facts), the root reference
int Build::read_back_scene_facts() const
{
  sc->coord_max = 0.0f;
  sc->grid_ok = false;
  sc->tree_depth = 0;      // (a single primitive: no internal node)
  if (n > 1) {
    uint32_t depth = 0;
    MIRT_HIP(hipMemcpy(&depth, sc->depth_dev, sizeof(depth), hipMemcpyDeviceToHost));
    sc->tree_depth = (int)depth;
    float rec[12];
    MIRT_HIP(hipMemcpy(rec, sc->nodes, sizeof(rec), hipMemcpyDeviceToHost));
    const SceneBoxFacts f = scene_box_facts(rec);
    sc->coord_max = f.coord_max;
    sc->grid_ok = f.grid_ok;
  }
  sc->root_ref = tree_root_ref(n, sc->Nt != 0, sc->prim_base / 16u);
  return MIRT_OK;
}

} // namespace

// mirt_probe_sort: the sort kernels on keys of the caller's choosing, on the null stream.  Mode 0: the build's sort, through
// radix_sort_keys as sort_by_morton calls it, the values being the positions 0 .. n-1.  Mode 1: sort_low_byte as render.hip calls it.
int probe_sort(int device, int mode, int n, const uint32_t* keys, uint32_t* keys_out, uint32_t* vals_out)
{
  MIRT_HIP(hipSetDevice(device));
  const size_t bytes = sizeof(uint32_t) * (size_t)n;
  if (mode == 0) {
    const BuildLayout at = build_layout(n);
    DevBuf<uint32_t> ws;
    MIRT_TRY(ws.alloc(at.total, "ws"));
    std::vector<uint32_t> positions((size_t)n);
    for (int i = 0; i < n; ++i) positions[i] = (uint32_t)i;
    MIRT_HIP(hipMemcpy(ws + at.k0, keys, bytes, hipMemcpyHostToDevice));
    MIRT_HIP(hipMemcpy(ws + at.v0, positions.data(), bytes, hipMemcpyHostToDevice));
    radix_sort_keys(ws, at, n, nullptr);
    MIRT_HIP(hipGetLastError());
    MIRT_HIP(hipMemcpy(keys_out, ws + at.k0, bytes, hipMemcpyDeviceToHost));
    MIRT_HIP(hipMemcpy(vals_out, ws + at.v0, bytes, hipMemcpyDeviceToHost));
    return MIRT_OK;
  }
  DevBuf<uint32_t> ki, ko, vo, ws;
  MIRT_TRY(ki.alloc((size_t)n, "keys_in")); MIRT_TRY(ko.alloc((size_t)n, "keys_out")); MIRT_TRY(vo.alloc((size_t)n, "vals_out"));
  MIRT_TRY(ws.alloc(sort_low_byte_ws_words(n), "ws"));
  MIRT_HIP(hipMemcpy(ki, keys, bytes, hipMemcpyHostToDevice));
  MIRT_TRY(sort_low_byte(ki, ko, vo, n, ws, nullptr));
  MIRT_HIP(hipMemcpy(keys_out, ko, bytes, hipMemcpyDeviceToHost));
  MIRT_HIP(hipMemcpy(vals_out, vo, bytes, hipMemcpyDeviceToHost));
  return MIRT_OK;
}

int build_lbvh(MirtScene* sc, hipStream_t stream)
{
  const int n = sc->N;
  sc->built = false;
  sc->root_ref = REF_NONE;
  sc->tree_depth = -1;
  if (n == 0) { sc->built = true; sc->build_ms = 0.0f; sc->tree_depth = 0; return MIRT_OK; }   // main.cu:44: build skipped when there are no primitives

  // sort / refit workspace: one allocation, made before the timed region and kept with the scene (a rebuild reuses it)
  const BuildLayout at = build_layout(n);
  if (sc->build_ws.cap() < at.total) MIRT_TRY(sc->build_ws.alloc(at.total, "build_ws"));
  const Build b{sc, n, stream, sc->build_ws, at};
  MIRT_HIP(hipEventRecord(sc->ev0, stream));
  MIRT_TRY(b.scene_bounds());
  MIRT_TRY(b.sort_by_morton());
  MIRT_TRY(b.hierarchy_and_depth());
  b.place_primitives();
  b.refit_and_pack();
  b.pack_quantised();
  MIRT_HIP(hipGetLastError());
  MIRT_HIP(hipEventRecord(sc->ev1, stream));
  MIRT_HIP(hipStreamSynchronize(stream));   // lbvh_builder.cu:475
  MIRT_HIP(hipEventElapsedTime(&sc->build_ms, sc->ev0, sc->ev1));
  MIRT_TRY(b.read_back_scene_facts());
  sc->built = true;
  return MIRT_OK;
}

} // namespace mirt
