// The block-wide exclusive scan the LBVH build's placement scan and radix passes use (lbvh_build.hip) and the list offsets are
// made from (overlap_list.hip): one copy, over the value type -- 32-bit in the build, 64-bit sums in the
// offsets.
#ifndef MIRT_BLOCK_SCAN_H
#define MIRT_BLOCK_SCAN_H

#include "device_common.h"

namespace mirt {

template <class T> struct scan_value { typedef T type; };      // (keeps `sh` and `total` out of the deduction: a nullptr total compiles)

// exclusive scan of one value per thread over a block of BLOCK threads; `total` (nullable) receives the sum
template <int BLOCK, class T>
MIRT_DEV T block_exclusive_scan(T v, typename scan_value<T>::type* sh /* [BLOCK] */, typename scan_value<T>::type* total)
{
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < BLOCK; o <<= 1) {
    const T x = (tid >= o) ? sh[tid - o] : 0;
    __syncthreads();
    sh[tid] += x;
    __syncthreads();
  }
  const T incl = sh[tid];
  if (total) *total = sh[BLOCK - 1];
  __syncthreads();
  return incl - v;
}

} // namespace mirt

#endif
