// stereo_match.h -- the pure parts of unina_locate_stereo_async (include/unina_mi355.h "3-D localisation from a stereo pair"), as
// __host__ __device__ functions: the disparity range, the packed key of a cost, the acceptance test, the sub-pixel step and
// the point. csrc/stereo.hip calls them on the device (and the range on the host, once per call), tests/stereo_match_host.cpp
// sweeps them on the host, localize.locate_stereo_numpy is their numpy twin. Costs are integers; the floats are fp32, one
// rounding per operation: every translation unit that includes this header is compiled with -ffp-contract=off.
#ifndef UNINA_STEREO_MATCH_H
#define UNINA_STEREO_MATCH_H

#include "locate_window.h"

namespace unina {

constexpr int kStereoMaxDisparities = 1024;   // UNINA_STEREO_MAX_DISPARITIES: the index d - d_lo fits 10 bits
constexpr int kStereoMaxSide = 64;            // UNINA_STEREO_MAX_SIDE: n_samples <= 4096, cost <= 4096 * 255 < 2^20
constexpr int kStereoIndexBits = 10;
constexpr uint32_t kStereoNone = 0xFFFFFFFFu;   // "no such cost"; above every key and every cost

// The disparity range of one call. fx, baseline, min_depth, max_depth finite and positive, min_depth < max_depth, width in
// 1..kLocateMaxDim (the entry point has checked them). status: 0 = fine; 1 = fxB or fxB / min_depth is not finite; 2 = more
// than kStereoMaxDisparities disparities. Both bounds are clipped in float, so each converts to int exactly.
struct StereoRange {
  int status;
  float fxB;
  int d_lo, d_hi_all;   // d_hi_all < d_lo: nothing can be matched
};
UNINA_HD StereoRange stereo_range(float fx, float baseline, float min_depth, float max_depth, int width) {
  StereoRange r;
  r.status = 1;
  r.fxB = fx * baseline;
  r.d_lo = 1;
  r.d_hi_all = 0;
  const float nearest = r.fxB / min_depth, farthest = r.fxB / max_depth;
  if (!finite(r.fxB) || !finite(nearest)) return r;
  float lo = ceilf(farthest), hi = floorf(nearest);
  const float w = (float)width, last = (float)(width - 1);
  lo = lo < 1.0f ? 1.0f : lo;
  lo = lo > w ? w : lo;   // beyond d_hi_all already: no result depends on how far
  hi = hi > last ? last : hi;
  r.d_lo = (int)lo;
  r.d_hi_all = (int)hi;
  r.status = r.d_hi_all - r.d_lo + 1 > kStereoMaxDisparities ? 2 : 0;
  return r;
}

// the disparities of one record: d_lo .. min(d_hi_all, u0), so that no right column is negative
UNINA_HD int stereo_nd(int d_lo, int d_hi_all, int u0, int* d_hi) {
  *d_hi = d_hi_all < u0 ? d_hi_all : u0;
  const int nd = *d_hi - d_lo + 1;
  return nd > 0 ? nd : 0;
}

// (cost, d - d_lo) as one integer that orders as the pair does: cost < 2^20, index < 2^10
UNINA_HD uint32_t stereo_key(uint32_t cost, int index) { return (cost << kStereoIndexBits) | (uint32_t)index; }
UNINA_HD uint32_t stereo_key_cost(uint32_t key) { return key >> kStereoIndexBits; }
UNINA_HD int stereo_key_index(uint32_t key) { return (int)(key & ((1u << kStereoIndexBits) - 1u)); }

UNINA_HD int stereo_accept(int nd, uint32_t cost_best, uint32_t cost_second, int n_samples, int max_mean_sad, int uniqueness) {
  if (nd < 1) return 0;
  if ((uint64_t)cost_best > (uint64_t)max_mean_sad * (uint64_t)n_samples) return 0;
  if (cost_second == kStereoNone) return 1;
  return (uint64_t)cost_second * 100u > (uint64_t)cost_best * (uint64_t)(100 + uniqueness) ? 1 : 0;
}

// cm, cp: the costs beside the best one; read only where d_lo < d_best < d_hi
UNINA_HD float stereo_disparity(int d_best, int d_lo, int d_hi, uint32_t cm, uint32_t c0, uint32_t cp) {
  float delta = 0.0f;
  if (d_lo < d_best && d_best < d_hi) {
    const int den = (int)cm - 2 * (int)c0 + (int)cp;   // >= 0: c0 is the minimum
    if (den != 0) delta = (float)((int)cm - (int)cp) / (float)(2 * den);
  }
  return (float)d_best + delta;
}

// xyz[0..2] = the box centre back-projected at Z = fxB / disparity
UNINA_HD void stereo_point(float fxB, float disparity, float uc, float vc, float fx, float fy, float cx, float cy, float* xyz) {
  locate_point(uc, vc, fxB / disparity, fx, fy, cx, cy, xyz);
}

}  // namespace unina
#endif  // UNINA_STEREO_MATCH_H
