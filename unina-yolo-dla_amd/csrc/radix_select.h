// radix_select.h -- one step of the radix select that csrc/locate.hip and csrc/lidar.hip run over the bytes of a key, one copy:
// the per-wave 256-bin histograms of a pass are summed and scanned by one wave, which publishes the bin that holds the wanted
// rank and the rank inside that bin. Counting only: the selected key does not depend on the order in which keys were added.
#ifndef UNINA_RADIX_SELECT_H
#define UNINA_RADIX_SELECT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace unina {

constexpr int kRadixBins = 256;

// Called by ONE whole wave behind the barrier that ends a pass; `hist` = WAVES histograms of kRadixBins counts in LDS. The first
// pass of a select (`first`) counts every valid key: it wants the lower median, rank (total - 1) / 2, and leaves the total in
// sel[2]; a later pass wants rank k inside the bin the pass before it chose. sel[0] = the bin, sel[1] = the rank inside it; both
// stay untouched where the histograms are empty.
template <int WAVES>
__device__ __forceinline__ void radix_pick(const uint32_t (*hist)[kRadixBins], int lane, bool first, int k, int* sel) {
  // lane l owns bins 4 l .. 4 l + 3 of the summed histogram
  uint32_t c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] = 0u;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) c[j] += hist[v][4 * lane + j];
  }
  const uint32_t mine = c[0] + c[1] + c[2] + c[3];
  uint32_t incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  const uint32_t total = __shfl(incl, 63, 64);
  uint32_t want = (uint32_t)k;
  if (first) {
    want = total ? (total - 1u) / 2u : 0u;
    if (lane == 0) sel[2] = (int)total;
  }
  uint32_t excl = incl - mine;
  if (total != 0u && excl <= want && want < incl) {   // exactly one lane
    int bin = 4 * lane;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (bin == 4 * lane + j && want >= excl + c[j]) {
        excl += c[j];
        ++bin;
      }
    }
    sel[0] = bin;
    sel[1] = (int)(want - excl);
  }
}

}  // namespace unina
#endif  // UNINA_RADIX_SELECT_H
