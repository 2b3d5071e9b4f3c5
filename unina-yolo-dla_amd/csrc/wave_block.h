// wave_block.h -- workgroup primitives on 64-lane waves, one copy each: the rank of a flag over the workgroup, the inclusive
// scan of a wave, one 64-bit word of a set held a word per lane. csrc/postprocess.hip and csrc/track.hip call them.
#ifndef UNINA_WAVE_BLOCK_H
#define UNINA_WAVE_BLOCK_H

#include <hip/hip_runtime.h>

namespace unina {

// inclusive prefix sum of v over the wave's lanes (six __shfl_up steps)
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  return v;
}

// reg holds word c of a set in lane c: the word as a wave-uniform value -- two v_readlane (c is wave-uniform), not a bpermute
__device__ __forceinline__ unsigned long long lane_word(unsigned long long reg, int c) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)reg, c);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(reg >> 32), c);
  return ((unsigned long long)hi << 32) | lo;
}

// Exclusive prefix of a 0/1 flag over a workgroup of WAVES waves, in thread order: returns this thread's offset, the number of
// set flags in *total. Every thread of the workgroup calls it. Barrier, write, barrier, read: the first barrier protects
// wave_cnt (LDS, WAVES ints) from the reads of a previous use, so calls may follow each other directly; a caller that writes
// wave_cnt itself puts a barrier between a call's reads and that write.
template <int WAVES>
__device__ __forceinline__ int block_rank(bool flag, int* wave_cnt, int* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  const int rank = __popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) wave_cnt[wid] = __popcll(b);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int c = wave_cnt[w];
    if (w < wid) off += c;
    tot += c;
  }
  *total = tot;
  return off + rank;
}

}  // namespace unina

#endif
