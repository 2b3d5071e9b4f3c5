// post_math.h -- the integer and bit-pattern arithmetic of the post-process (csrc/postprocess.hip) as __host__ __device__
// functions: the triangular tile layout, the confidence histogram's bins, the packed (class | enumeration index) field and the
// key ranges of the top-MAX_DETECTIONS cut. The kernels call exactly these; tests/post_math_host.cpp sweeps them on the host
// against cut_model of tests/test_post_cases_cpu.py. The two float operations (x 4096, / 4096) are exact scalings by a power
// of two in binary floating point.
#ifndef UNINA_POST_MATH_H
#define UNINA_POST_MATH_H

#include <stdint.h>
#include <string.h>

#include "hd.h"

namespace unina {

UNINA_HD uint32_t post_bits(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }
UNINA_HD float post_float(uint32_t b) { float v; memcpy(&v, &b, 4); return v; }

// ---- upper-triangular 64 x 64-bit tiles over nw chunks of 64 candidates: tile t <-> (row chunk c, column chunk w >= c), row-major
struct TileCW { int c, w; };
UNINA_HD TileCW tile_of(int t, int nw) {
  int c = 0, rem = t;
  while (rem >= nw - c) {
    rem -= nw - c;
    ++c;
  }
  return TileCW{c, c + rem};
}
// first 64-bit word of row chunk c's tiles (64 rows x (nw - c) words each) in the triangular mask
UNINA_HD int tri_off(int c, int nw) { return 64 * (c * nw - (c * (c - 1)) / 2); }

// ---- confidence -> bin of the decode launch's histogram: kBins linear bins, bin T = the confidences in [T / kBins, (T + 1) / kBins)
constexpr int kBins = 4096;
UNINA_HD int conf_bin(float c) {
  const int b = (int)(c * (float)kBins);
  return b > kBins - 1 ? kBins - 1 : b;
}

// ---- (class id | enumeration index << kClassBits) travels in the second float of a candidate's (confidence, class) pair. The
// enumeration index is below 2^18 (the candidate list's capacity), which leaves 14 bits for the class; the all-ones field is
// the padding dummy's class -1, so num_classes <= kClassMask (checked by unina_load_engine)
constexpr int kClassBits = 14;
constexpr int kClassMask = (1 << kClassBits) - 1;
UNINA_HD float pack_ce(int class_id, int eidx) { return post_float(((uint32_t)class_id & (uint32_t)kClassMask) | ((uint32_t)eidx << kClassBits)); }
UNINA_HD int ce_class(float y) {   // (not a sign extension: that would turn the ids from 8192 up into negative ones)
  const int f = (int)(post_bits(y) & (uint32_t)kClassMask);
  return f == kClassMask ? -1 : f;
}
UNINA_HD unsigned ce_eidx(float y) { return post_bits(y) >> kClassBits; }
UNINA_HD bool ce_same_class(float a, float b) { return ((post_bits(a) ^ post_bits(b)) & (uint32_t)kClassMask) == 0; }

// ---- the cut: key = bit pattern of a confidence (positive floats: the patterns order like the values)
struct KeyRange { uint32_t lo, hi; };   // [lo, hi)
UNINA_HD KeyRange bin_key_range(int T) {   // (a confidence is at most 1.0: the top bin ends just above its bit pattern)
  return KeyRange{post_bits((float)T / (float)kBins), T == kBins - 1 ? 0x3F800001u : post_bits((float)(T + 1) / (float)kBins)};
}
// a key range too crowded to rank is split into kBins sub-ranges of this width (the last ones may be empty)
UNINA_HD uint32_t split_width(uint32_t klo, uint32_t khi) { return (khi - klo + (uint32_t)kBins - 1u) / (uint32_t)kBins; }

}  // namespace unina

#endif
