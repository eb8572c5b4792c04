// Accumulation buffers: what adds to them, selects from them and turns them into pixels (include/mirt.h, the resolve of
// mirt_render_accumulate and mirt_render_accumulate_pixels, mirt_select_pixels, mirt_finalize, mirt_finalize_counts; DESIGN.md
// section 6e).  The reference's progressive pair (draw.cu:13-92) adds the same samples to every pixel; the pixel lists, the second
// moment and the per-pixel counts are not in it.
//
// compact_*_kernel   ordered stream compaction in three launches -- per-block counts (wave ballot + popcount), one block's
//                    exclusive scan of the counts, scatter (ballot prefix inside a wave, wave offsets inside a block, the
//                    scanned count across blocks).  No block ever waits for another one inside a kernel.  Two predicates use
//                    it: "this pixel needs more samples" (mirt_select_pixels) and "this list entry lies in the slab being
//                    rendered" (the pixel list of a sparse call; an entry past the end of the part lies in no slab).
// sparse_table_kernel  the kept pixels -> RenderArgs::sample_order of the launch: position j * count + s of the hand-out is
//                    launch sample (pixel - slab base) * count + s.  The trace kernels are the dense call's, untouched.
// moments_tree_kernel / moments_kernel
//                    the accumulating resolve of mirt_render_accumulate and mirt_render_accumulate_pixels: per pixel the butterfly
//                    sum of its samples (draw.cu:181-189; one lane per sample when the butterfly fits a wave, one thread per pixel
//                    otherwise) and, SQUARE, the same butterfly over their squares, then one read-modify-write per pixel and
//                    buffer.  These are the only kernels that add to an accumulation buffer.
// finalize_kernel    finalize_kernel (draw.cu:13-47) with one sample count for the frame (mirt_finalize) or one per pixel
//                    (mirt_finalize_counts).
#include "scene_dev.h"
#include "host_scene.h"

#include <map>
#include <mutex>
#include <utility>

namespace mirt {
namespace {

constexpr int CBLOCK = 1024;          // compaction: items per block (one per thread)
constexpr int CWAVES = CBLOCK / 64;
constexpr int RBLOCK = 256;
constexpr int TBLOCK = 1024;          // moments_tree_kernel

// mirt_select_pixels: pixel i is kept when n < max && (n < min || e > max_variance), e the largest estimated variance of the
// mean over r, g, b -- float32, one rounding per operation (include/mirt.h spells the formula out)
struct SelectPred {
  const float4* sum; const float4* sq; const uint32_t* counts;
  uint32_t min_samples, max_samples; float max_variance;
  __device__ bool keep(long long i) const
  {
    const uint32_t n = counts[i];
    if (n >= max_samples) return false;
    if (n < min_samples) return true;
    const float4 S = sum[i], Q = sq[i];
    const float nf = (float)n;
    const float e = fmaxf(variance_of_mean(S.x, Q.x, nf), fmaxf(variance_of_mean(S.y, Q.y, nf), variance_of_mean(S.z, Q.z, nf)));
    return e > max_variance;
  }
  __device__ uint32_t value(long long i) const { return (uint32_t)i; }
};

// the pixel list of a sparse call: entry i is kept when it names a pixel of the slab [base, base + span)
struct RangePred {
  const uint32_t* list; uint32_t base, span;
  __device__ bool keep(long long i) const { return list[i] - base < span; }      // (unsigned: an entry below the base wraps past the span)
  __device__ uint32_t value(long long i) const { return list[i]; }
};

template <class Pred>
__global__ void __launch_bounds__(CBLOCK) compact_count_kernel(const Pred pr, long long n, uint32_t* __restrict__ block_counts)
{
  __shared__ uint32_t wave_n[CWAVES];
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * CBLOCK + tid;
  const bool keep = i < n && pr.keep(i);
  const unsigned long long m = __ballot(keep);
  if ((tid & 63) == 0) wave_n[tid >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < CWAVES; ++w) t += wave_n[w];
    block_counts[blockIdx.x] = t;
  }
}

// One block: counts[0 .. nblocks) -> their exclusive prefix sums, in place; counts[nblocks] and *total_out (nullable) receive
// the total, *scaled_out (nullable) the total times `scale` (the number of samples of a sparse launch).
__global__ void __launch_bounds__(CBLOCK) compact_scan_kernel(uint32_t* __restrict__ counts, uint32_t nblocks, uint32_t* __restrict__ total_out,
                                                              long long* __restrict__ scaled_out, int scale)
{
  __shared__ uint32_t buf[CBLOCK];
  __shared__ uint32_t carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (uint32_t tile = 0; tile < nblocks; tile += CBLOCK) {
    const uint32_t i = tile + (uint32_t)t;
    const uint32_t own = i < nblocks ? counts[i] : 0u;
    buf[t] = own;
    __syncthreads();
    for (int o = 1; o < CBLOCK; o <<= 1) {
      const uint32_t x = t >= o ? buf[t - o] : 0u;
      __syncthreads();
      buf[t] += x;
      __syncthreads();
    }
    const uint32_t base = carry;
    if (i < nblocks) counts[i] = base + buf[t] - own;
    __syncthreads();
    if (t == CBLOCK - 1) carry = base + buf[t];
    __syncthreads();
  }
  if (t == 0) {
    const uint32_t total = carry;
    counts[nblocks] = total;
    if (total_out) *total_out = total;
    if (scaled_out) *scaled_out = (long long)total * scale;
  }
}

template <class Pred>
__global__ void __launch_bounds__(CBLOCK) compact_scatter_kernel(const Pred pr, long long n, const uint32_t* __restrict__ block_offsets, uint32_t* __restrict__ out)
{
  __shared__ uint32_t wave_n[CWAVES];
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * CBLOCK + tid;
  const bool keep = i < n && pr.keep(i);
  const unsigned long long m = __ballot(keep);
  if ((tid & 63) == 0) wave_n[tid >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (!keep) return;
  uint32_t off = block_offsets[blockIdx.x];
  for (int w = 0; w < (tid >> 6); ++w) off += wave_n[w];
  const uint32_t rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
  out[off + rank] = pr.value(i);
}

template <class Pred>
int compact(const Pred& pr, long long n, uint32_t* blocks, uint32_t* out, uint32_t* total_out, long long* scaled_out, int scale, hipStream_t stream)
{
  const unsigned nblocks = (unsigned)((n + CBLOCK - 1) / CBLOCK);
  hipLaunchKernelGGL(compact_count_kernel<Pred>, dim3(nblocks), dim3(CBLOCK), 0, stream, pr, n, blocks);
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(CBLOCK), 0, stream, blocks, (uint32_t)nblocks, total_out, scaled_out, scale);
  hipLaunchKernelGGL((compact_scatter_kernel<Pred>), dim3(nblocks), dim3(CBLOCK), 0, stream, pr, n, (const uint32_t*)blocks, out);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

__global__ void __launch_bounds__(RBLOCK) sparse_table_kernel(const uint32_t* __restrict__ kept, const uint32_t* __restrict__ num_kept, uint32_t base,
                                                              uint32_t count, uint32_t* __restrict__ table)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * RBLOCK + threadIdx.x;
  if (t >= (unsigned long long)*num_kept * count) return;
  const uint32_t j = (uint32_t)(t / count);
  table[t] = (kept[j] - base) * count + (uint32_t)(t - (unsigned long long)j * count);
}

struct MomentArgs {
  const float4* samples;      // the launch's sample workspace: [pixel - pixel_base][count]
  float4* accum;              // the call's part buffers
  float4* accum_sq;           // nullable
  uint32_t* counts;           // nullable
  const uint32_t* kept;       // the launch's pixels (local pixels of the part); null: pixel_base + [0, num_pixels)
  const uint32_t* num_kept;   // with `kept`: how many
  long long num_pixels;
  long long pixel_base;
  int count;                  // samples per pixel in `samples`
};

MIRT_DEV long long moment_pixels(const MomentArgs& a) { return a.kept ? (long long)*a.num_kept : a.num_pixels; }

template <bool SQUARE>
MIRT_DEV void add_moments(const MomentArgs& a, long long lp, const float4 s, const float4 q)
{
  const float4 o = a.accum[lp];
  a.accum[lp] = make_float4(o.x + s.x, o.y + s.y, o.z + s.z, o.w + s.w);
  if (SQUARE) {
    const float4 r = a.accum_sq[lp];
    a.accum_sq[lp] = make_float4(r.x + q.x, r.y + q.y, r.z + q.z, r.w + q.w);
  }
  if (a.counts) a.counts[lp] += (uint32_t)a.count;
}

// P <= 64, one lane per sample: coalesced 16-byte loads, then literally the reference's butterfly `for (mask = P/2; mask > 0;
// mask /= 2) v += shfl_xor(v, mask)` (draw.cu:181-189) inside each group of P lanes, over the samples and (SQUARE: a.accum_sq is
// given) over their squares; the group's lane 0 parks its sums in LDS and the first threads of the block add the block's pixels
template <bool SQUARE>
__global__ void __launch_bounds__(TBLOCK) moments_tree_kernel(const MomentArgs a, int P, int lg)
{
  __shared__ float4 park[SQUARE ? 2 : 1][TBLOCK / 2];      // [0]: sums, [1]: sums of squares
  const int tid = threadIdx.x;
  const int ppb = TBLOCK >> lg;                       // pixels per block
  const int si = tid & (P - 1);
  const long long n = moment_pixels(a);
  const long long g = (long long)blockIdx.x * ppb + (tid >> lg);
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (g < n && si < a.count) {
    const long long lq = a.kept ? (long long)a.kept[g] - a.pixel_base : g;
    v = a.samples[lq * a.count + si];
  }
  float4 w = make_float4(v.x * v.x, v.y * v.y, v.z * v.z, v.w * v.w);
  for (int mask = P >> 1; mask > 0; mask >>= 1) {
    v.x += __shfl_xor(v.x, mask); v.y += __shfl_xor(v.y, mask); v.z += __shfl_xor(v.z, mask); v.w += __shfl_xor(v.w, mask);
    if (SQUARE) { w.x += __shfl_xor(w.x, mask); w.y += __shfl_xor(w.y, mask); w.z += __shfl_xor(w.z, mask); w.w += __shfl_xor(w.w, mask); }
  }
  if (si == 0) { park[0][tid >> lg] = v; if (SQUARE) park[1][tid >> lg] = w; }
  __syncthreads();
  const long long h = (long long)blockIdx.x * ppb + tid;
  if (tid < ppb && h < n) add_moments<SQUARE>(a, a.kept ? (long long)a.kept[h] : a.pixel_base + h, park[0][tid], park[SQUARE ? 1 : 0][tid]);
}

// one thread per pixel: count 1, and P > 64
template <bool SQUARE>
__global__ void __launch_bounds__(RBLOCK) moments_kernel(const MomentArgs a)
{
  const long long g = (long long)blockIdx.x * RBLOCK + threadIdx.x;
  if (g >= moment_pixels(a)) return;
  const long long lp = a.kept ? (long long)a.kept[g] : a.pixel_base + g;
  const float4* s = a.samples + (lp - a.pixel_base) * a.count;
  float4 m, q;
  if (a.count <= 1) {
    m = s[0];
    q = make_float4(m.x * m.x, m.y * m.y, m.z * m.z, m.w * m.w);
  } else {
    int P = 1, lg = 0;
    while (P < a.count) { P <<= 1; ++lg; }
    m = butterfly_sum<false>(s, a.count, P, lg);
    q = SQUARE ? butterfly_sum<true>(s, a.count, P, lg) : m;
  }
  add_moments<SQUARE>(a, lp, m, q);
}

// counts null: every pixel is the mean over `aa` samples; otherwise over its own count, and a count of 0 gives a zero pixel
__global__ void __launch_bounds__(RBLOCK) finalize_kernel(const float4* __restrict__ accum, const uint32_t* __restrict__ counts, uchar4* __restrict__ rgba8,
                                                          long long n, int aa)
{
  const long long i = (long long)blockIdx.x * RBLOCK + threadIdx.x;
  if (i >= n) return;
  const int c = counts ? (int)counts[i] : aa;
  // finalize_kernel, draw.cu:13-47
  rgba8[i] = c != 0 ? to_srgb8(mean_of(accum[i], c)) : make_uchar4(0, 0, 0, 0);
}

int launch_finalize(const void* d_accum, const uint32_t* d_counts, void* d_rgba8, int64_t n, int aa, hipStream_t stream)
{
  hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((n + RBLOCK - 1) / RBLOCK)), dim3(RBLOCK), 0, stream, (const float4*)d_accum, d_counts, (uchar4*)d_rgba8,
                     (long long)n, aa);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

// mirt_select_pixels has no scene to keep its block counts in: one buffer per (device, stream), grown on demand and kept, so
// that calls on different streams never share one
// (the map is made on first use and never destroyed: an owning buffer must not outlive the HIP runtime, dev_mem.h)
std::mutex select_mu;
using SelectWs = std::map<std::pair<int, hipStream_t>, DevBuf<uint32_t>>;
SelectWs& select_ws() { static SelectWs* const ws = new SelectWs(); return *ws; }

} // namespace

size_t sparse_blocks_words(long long num_listed) { return (size_t)((num_listed + CBLOCK - 1) / CBLOCK) + 1; }

// The pixels of `list` that lie in the slab [p0, p0 + pn) -> cx.sp_list (list order), their number -> the last word of
// cx.sp_blocks, the launch's hand-out table -> cx.sp_table, its number of samples -> *num_samples_dev (RenderArgs::num_samples of
// the launch's arguments in device memory: the host knows only the upper bound min(num_listed, pn) * count).
int sparse_expand(RenderCtx& cx, const uint32_t* list, long long num_listed, long long p0, long long pn, int count, long long* num_samples_dev, hipStream_t stream)
{
  RangePred pr;
  pr.list = list; pr.base = (uint32_t)p0; pr.span = (uint32_t)pn;
  int rc = compact(pr, num_listed, cx.sp_blocks, cx.sp_list, nullptr, num_samples_dev, count, stream);
  if (rc != MIRT_OK) return rc;
  const uint32_t* num_kept = cx.sp_blocks + (sparse_blocks_words(num_listed) - 1);
  const long long bound = (num_listed < pn ? num_listed : pn) * count;
  hipLaunchKernelGGL(sparse_table_kernel, dim3((unsigned)((bound + RBLOCK - 1) / RBLOCK)), dim3(RBLOCK), 0, stream, (const uint32_t*)cx.sp_list, num_kept,
                     (uint32_t)p0, (uint32_t)count, cx.sp_table);
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

// The resolve of one launch of mirt_render_accumulate (an empty ax) or mirt_render_accumulate_pixels: the pixels sparse_expand
// kept (ax.list given), or the slab's pixels [p0, p0 + pn).
int resolve_moments(RenderCtx& cx, const float4* samples, const AdaptiveArgs& ax, float4* accum, long long p0, long long pn, long long num_listed,
                    int count, hipStream_t stream)
{
  MomentArgs m;
  m.samples = samples; m.accum = accum; m.accum_sq = ax.accum_sq; m.counts = ax.counts;
  m.kept = ax.list ? cx.sp_list : nullptr;
  m.num_kept = ax.list ? cx.sp_blocks + (sparse_blocks_words(num_listed) - 1) : nullptr;
  m.num_pixels = pn; m.pixel_base = p0; m.count = count;
  const long long bound = ax.list ? (num_listed < pn ? num_listed : pn) : pn;
  int P = 1, lg = 0;
  while (P < count) { P <<= 1; ++lg; }
  if (count > 1 && P <= 64) {
    const long long ppb = TBLOCK >> lg;
    const dim3 grid((unsigned)((bound + ppb - 1) / ppb));
    if (m.accum_sq) hipLaunchKernelGGL(moments_tree_kernel<true>, grid, dim3(TBLOCK), 0, stream, m, P, lg);
    else hipLaunchKernelGGL(moments_tree_kernel<false>, grid, dim3(TBLOCK), 0, stream, m, P, lg);
  } else {
    const dim3 grid((unsigned)((bound + RBLOCK - 1) / RBLOCK));
    if (m.accum_sq) hipLaunchKernelGGL(moments_kernel<true>, grid, dim3(RBLOCK), 0, stream, m);
    else hipLaunchKernelGGL(moments_kernel<false>, grid, dim3(RBLOCK), 0, stream, m);
  }
  MIRT_HIP(hipGetLastError());
  return MIRT_OK;
}

int select_pixels(const MirtRenderParams* p, const void* d_accum, const void* d_accum_sq, const uint32_t* d_counts, int min_samples, int max_samples,
                  float max_variance, uint32_t* d_pixels_out, uint32_t* d_num_out, hipStream_t stream)
{
  const int64_t n = render_num_pixels(p);
  if (n < 0 || !d_accum || !d_accum_sq || !d_counts || !d_pixels_out || !d_num_out || min_samples < 2 || max_samples < min_samples) {
    set_error("mirt_select_pixels: bad parameters (a null pointer, min_samples < 2 or max_samples < min_samples)"); return MIRT_ERR_ARG;
  }
  if (n >= 0x7fffffffll) { set_error("mirt_select_pixels: part too large"); return MIRT_ERR_ARG; }
  if (n == 0) { MIRT_HIP(hipMemsetAsync(d_num_out, 0, 4, stream)); return MIRT_OK; }
  int device = 0;
  MIRT_HIP(hipGetDevice(&device));
  const size_t need = sparse_blocks_words(n);
  uint32_t* blocks = nullptr;
  {
    std::lock_guard<std::mutex> lock(select_mu);
    DevBuf<uint32_t>& ws = select_ws()[std::make_pair(device, stream)];
    MIRT_TRY(ws.grow(need, stream, "select blocks"));
    blocks = ws;
  }
  SelectPred pr;
  pr.sum = (const float4*)d_accum; pr.sq = (const float4*)d_accum_sq; pr.counts = d_counts;
  pr.min_samples = (uint32_t)min_samples; pr.max_samples = (uint32_t)max_samples; pr.max_variance = max_variance;
  return compact(pr, n, blocks, d_pixels_out, d_num_out, nullptr, 0, stream);
}

int finalize(const MirtRenderParams* p, const void* d_accum, int total_samples, void* d_rgba8, hipStream_t stream)
{
  const int64_t n = render_num_pixels(p);
  if (n < 0 || !d_accum || !d_rgba8 || total_samples < 1) { set_error("mirt_finalize: bad parameters"); return MIRT_ERR_ARG; }
  if (n == 0) return MIRT_OK;
  return launch_finalize(d_accum, nullptr, d_rgba8, n, total_samples, stream);
}

int finalize_counts(const MirtRenderParams* p, const void* d_accum, const uint32_t* d_counts, void* d_rgba8, hipStream_t stream)
{
  const int64_t n = render_num_pixels(p);
  if (n < 0 || !d_accum || !d_counts || !d_rgba8) { set_error("mirt_finalize_counts: bad parameters"); return MIRT_ERR_ARG; }
  if (n == 0) return MIRT_OK;
  return launch_finalize(d_accum, d_counts, d_rgba8, n, 0, stream);
}

} // namespace mirt
