// wave_block.h -- workgroup primitives on 64-lane waves, one copy each: the rank of a flag over the workgroup, the inclusive
// scan of a wave, one 64-bit word of a set held a word per lane, the fold of a wave's lanes by key, and the shape of the
// one-workgroup scan. csrc/postprocess.hip, csrc/track.hip, csrc/lidar.hip, csrc/ground.hip and csrc/cluster.hip call them.
#ifndef UNINA_WAVE_BLOCK_H
#define UNINA_WAVE_BLOCK_H

#include <hip/hip_runtime.h>

namespace unina {

constexpr int kWave = 64;
// the one-workgroup exclusive scan of csrc/lidar.hip, csrc/ground.hip and csrc/cluster.hip: the kernels keep a copy each of the pass itself (a
// shared function is simplified before it is inlined, and lidar_scan_kernel then needs 52 VGPRs for 40)
constexpr int kScanBlock = 1024;
constexpr int kScanWaves = kScanBlock / kWave;
constexpr int kScanPer = 4;                    // words a thread scans in a pass

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

// The fold of a wave by key, one group of lanes at a time: of the lanes in `todo` (a ballot), the first is the group's leader, its key
// the group's, `lanes` the 64-bit mask of the lanes that hold the same key. The caller loops
//   unsigned long long todo = __ballot(key >= 0);
//   while (todo) { KeyGroup g; wave_first_group(todo, key, g); ...; todo &= ~g.lanes; }
// and does ONE atomic per group, from the lane == g.leader. The loop is wave-uniform: every lane of the wave enters it, none has
// returned before, because the group is found with a shuffle and a ballot. g is filled in place: returned by value, the same
// instructions come out with another address computation.
struct KeyGroup { int key; unsigned long long lanes; int leader; };
__device__ __forceinline__ void wave_first_group(unsigned long long todo, int key, KeyGroup& g) {
  g.leader = __ffsll((long long)todo) - 1;
  g.key = __shfl(key, g.leader, kWave);
  g.lanes = __ballot(key == g.key);
}

}  // namespace unina

#endif
