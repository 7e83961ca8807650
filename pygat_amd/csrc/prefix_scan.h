// The wave and work-group prefix count of the sampler family (k22_sample.hip: sample_emit, the radix select and count_long;
// k23_subgraph.hip: the long rows' count and fill): one copy.  Integer only, no atomics.  What else the family shares -- the row of
// an id that may be no node, the list of long rows, the launchers' preamble -- is in minibatch.h, which includes this file.
#pragma once
#include "common.h"

namespace pygat {

// exclusive prefix of v over the THREADS (64: the wave; 256: the work-group, wsum = 4 ints of LDS) threads, and the total
template <int THREADS>
__device__ __forceinline__ int sample_scan(int v, int* total, int* wsum) {
  const int lane = threadIdx.x & 63;
  int x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off);
    if (lane >= off) x += y;
  }
  if constexpr (THREADS == 64) {
    *total = __shfl(x, 63);
    return x - v;
  } else {
    const int w = threadIdx.x >> 6;
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < THREADS / 64; ++k) {
      if (k < w) pre += wsum[k];
      tot += wsum[k];
    }
    __syncthreads();
    *total = tot;
    return pre + x - v;
  }
}

}  // namespace pygat
