// stereo_match_host.cpp -- stand-alone host driver of csrc/stereo_match.h for tests/test_stereo_cpu.py: the disparity range, the
// packed key, the acceptance test, the sub-pixel step and the point that csrc/stereo.hip calls, built by a host compiler (no
// HIP, no GPU) and run on cases from a file.
//   stereo_match_host IN OUT
// IN : 3 int32 -- magic, mode, n -- then
//      mode 0: n cases of 4 float32 (fx, baseline, min_depth, max_depth) + 1 int32 (width)
//      mode 1: n cases of 11 int32 (n_samples, max_mean_sad, uniqueness, nd, d_lo, d_hi, d_best, cost_best, cost_second, cm, cp)
//              + 7 float32 (fxB, uc, vc, fx, fy, cx, cy)
// OUT: mode 0: per case 4 int32 -- status, bits of fxB, d_lo, d_hi_all (the last two 0 unless status is 0 or 2)
//      mode 1: per case 8 int32 -- key, cost and index unpacked from it, accepted, bits of disparity, bits of x, y, z
#include "../unina-yolo-dla_amd/csrc/stereo_match.h"

#include <cstdio>
#include <vector>

using namespace unina;

struct RangeCase {
  float fx, baseline, min_depth, max_depth;
  int32_t width;
};
struct MatchCase {
  int32_t n_samples, max_mean_sad, uniqueness, nd, d_lo, d_hi, d_best;
  uint32_t cost_best, cost_second, cm, cp;
  float fxB, uc, vc, fx, fy, cx, cy;
};

static int32_t bits(float f) {
  int32_t b;
  memcpy(&b, &f, 4);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[3];
  if (fread(h, sizeof h, 1, f) != 1 || h[0] != 0x53544d31 || h[2] < 0) return 4;
  const int mode = h[1], n = h[2];
  std::vector<int32_t> out;
  if (mode == 0) {
    std::vector<RangeCase> cases((size_t)n);
    if (n && fread(cases.data(), sizeof(RangeCase), (size_t)n, f) != (size_t)n) return 4;
    for (const RangeCase& c : cases) {
      if (c.width < 1 || c.width > kLocateMaxDim) return 4;
      const StereoRange r = stereo_range(c.fx, c.baseline, c.min_depth, c.max_depth, c.width);
      const bool formed = r.status != 1;
      // what the kernel relies on: a range it accepts has at most kStereoMaxDisparities entries, none below 1 or past the last column
      if (r.status == 0 && (r.d_lo < 1 || r.d_hi_all > c.width - 1 || r.d_hi_all - r.d_lo + 1 > kStereoMaxDisparities)) return 6;
      const int32_t rec[4] = {r.status, bits(r.fxB), formed ? r.d_lo : 0, formed ? r.d_hi_all : 0};
      out.insert(out.end(), rec, rec + 4);
    }
  } else if (mode == 1) {
    std::vector<MatchCase> cases((size_t)n);
    if (n && fread(cases.data(), sizeof(MatchCase), (size_t)n, f) != (size_t)n) return 4;
    for (const MatchCase& c : cases) {
      const int index = c.d_best - c.d_lo;
      if (index < 0 || index >= kStereoMaxDisparities || c.cost_best > 4096u * 255u) return 4;
      const uint32_t key = stereo_key(c.cost_best, index);
      const int ok = stereo_accept(c.nd, c.cost_best, c.cost_second, c.n_samples, c.max_mean_sad, c.uniqueness);
      const float disparity = stereo_disparity(c.d_best, c.d_lo, c.d_hi, c.cm, c.cost_best, c.cp);
      float xyz[3];
      stereo_point(c.fxB, disparity, c.uc, c.vc, c.fx, c.fy, c.cx, c.cy, xyz);
      const int32_t rec[8] = {(int32_t)key, (int32_t)stereo_key_cost(key), stereo_key_index(key), ok, bits(disparity), bits(xyz[0]), bits(xyz[1]),
                              bits(xyz[2])};
      out.insert(out.end(), rec, rec + 8);
    }
  } else {
    return 4;
  }
  fclose(f);
  f = fopen(argv[2], "wb");
  if (!f || (!out.empty() && fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size()) || fclose(f)) return 5;
  return 0;
}
