// post_math_host.cpp -- stand-alone host driver of csrc/post_math.h for tests/test_post_math_cpu.py: the tile layout, the
// histogram bins, the packed (class | enumeration index) field and the cut's key ranges that csrc/postprocess.hip calls, built
// by a host compiler (no HIP, no GPU). No input; one line per evaluation on stdout, the test does the checking:
//   tile NW T C W TRI_OFF(C)          every nw in 1..16, every t of its triangle
//   bin K BIN(K/4096) BIN(nextafter(K/4096, 0))      K in 0..4096 (the third field is -1 for K = 0)
//   one BIN(1.0f)
//   ce CLASS EIDX CE_CLASS CE_EIDX    the round trip
//   same CLASS_A CLASS_B 0|1          the packed class-equality test (different enumeration indices on the two sides)
//   cut T KLO KHI WDT                 key range of bin T and the width of its first split
#include "../unina-yolo-dla_amd/csrc/post_math.h"

#include <cmath>
#include <cstdio>

using namespace unina;

int main() {
  for (int nw = 1; nw <= 16; ++nw)
    for (int t = 0; t < nw * (nw + 1) / 2; ++t) {
      const TileCW x = tile_of(t, nw);
      printf("tile %d %d %d %d %d\n", nw, t, x.c, x.w, tri_off(x.c, nw));
    }
  for (int k = 0; k <= kBins; ++k) {
    const float c = (float)k / (float)kBins;
    printf("bin %d %d %d\n", k, conf_bin(c), k ? conf_bin(std::nextafterf(c, 0.0f)) : -1);
  }
  printf("one %d\n", conf_bin(1.0f));
  const int classes[] = {-1, 0, 1, 16382};
  const int indices[] = {0, 1, (1 << 18) - 1};
  for (int cls : classes)
    for (int e : indices) {
      const float y = pack_ce(cls, e);
      printf("ce %d %d %d %u\n", cls, e, ce_class(y), ce_eidx(y));
    }
  for (int a : classes)
    for (int b : classes)
      for (int ea : indices)
        for (int eb : indices) printf("same %d %d %d\n", a, b, ce_same_class(pack_ce(a, ea), pack_ce(b, eb)) ? 1 : 0);
  for (int T = 0; T < kBins; ++T) {
    const KeyRange r = bin_key_range(T);
    printf("cut %d %u %u %u\n", T, r.lo, r.hi, split_width(r.lo, r.hi));
  }
  return 0;
}
