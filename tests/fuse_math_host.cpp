// fuse_math_host.cpp -- stand-alone host driver of csrc/fuse_math.h for tests/test_fuse_cpu.py: the LiDAR cone's point and pixel,
// the camera record's grown box, the gated pair with its key, and the output expressions csrc/fuse.hip calls, built by a host
// compiler (no HIP, no GPU) and run on cases from a file.
//   fuse_math_host IN OUT
// IN : 3 int32 -- magic, mode, n -- then n cases of 24 words each
//      mode 0: 12 float32 level_to_cam, 4 float32 fx, fy, cx, cy, 3 float32 lift, min_depth, max_depth, 3 float32 x, y, z, 1 int32 valid
//      mode 1: 8 float32 x1, y1, x2, y2, sx, sy, grow, pad
//      mode 2: 7 float32 u, v, zc, uc, vc, hw, hh, 1 int32 has_depth, 3 float32 cz, range_abs, range_rel, 1 uint32 index
//      mode 3: 2 float32 pixel, scale, 3 int32 n_camera, n_lidar_only, capacity
// OUT: 8 int32 per case
//      mode 0: bits of xc, yc, zc, u, v, usable, projected, 0       mode 1: bits of uc, vc, hw, hh, boxed, 0, 0, 0
//      mode 2: bits of d2, candidate, key low word, key high word, 0..  mode 3: bits of pixel / scale, records written, 0..
#include "../unina-yolo-dla_amd/csrc/fuse_math.h"

#include <cstdio>
#include <vector>

using namespace unina;

struct Case {
  union {
    float f[24];
    int32_t i[24];
    uint32_t u[24];
  };
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[3];
  if (fread(h, sizeof h, 1, f) != 1 || h[0] != 0x46555331 || h[2] < 0 || h[1] < 0 || h[1] > 3) return 4;
  const int mode = h[1], n = h[2];
  std::vector<Case> cases((size_t)n);
  if (n && fread(cases.data(), sizeof(Case), (size_t)n, f) != (size_t)n) return 4;
  fclose(f);
  std::vector<int32_t> out;
  out.reserve((size_t)n * 8);
  for (const Case& c : cases) {
    int32_t rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (mode == 0) {
      const FusePoint p = fuse_point(c.f, c.f[12], c.f[13], c.f[14], c.f[15], c.f[16], c.f[17], c.f[18], c.f[19], c.f[20], c.f[21], c.i[22]);
      rec[0] = (int32_t)float_bits(p.xc);
      rec[1] = (int32_t)float_bits(p.yc);
      rec[2] = (int32_t)float_bits(p.zc);
      rec[3] = (int32_t)float_bits(p.u);
      rec[4] = (int32_t)float_bits(p.v);
      rec[5] = p.usable;
      rec[6] = p.projected;
    } else if (mode == 1) {
      const FuseBox b = fuse_box(c.f[0], c.f[1], c.f[2], c.f[3], c.f[4], c.f[5], c.f[6], c.f[7]);
      rec[0] = (int32_t)float_bits(b.uc);
      rec[1] = (int32_t)float_bits(b.vc);
      rec[2] = (int32_t)float_bits(b.hw);
      rec[3] = (int32_t)float_bits(b.hh);
      rec[4] = b.boxed;
    } else if (mode == 2) {
      float d2;
      const bool cand = fuse_candidate(c.f[0], c.f[1], c.f[2], c.f[3], c.f[4], c.f[5], c.f[6], c.i[7], c.f[8], c.f[9], c.f[10], &d2);
      const uint64_t key = fuse_key(d2, c.u[11]);
      if (cand && key == kFuseNoKey) return 6;   // the empty key must stay above every candidate's key
      rec[0] = (int32_t)float_bits(d2);
      rec[1] = cand ? 1 : 0;
      rec[2] = (int32_t)(uint32_t)key;
      rec[3] = (int32_t)(uint32_t)(key >> 32);
    } else {
      if (c.i[2] < 0 || c.i[3] < 0 || c.i[4] < c.i[2]) return 4;
      rec[0] = (int32_t)float_bits(fuse_record_coord(c.f[0], c.f[1]));
      rec[1] = fuse_written(c.i[2], c.i[3], c.i[4]);
    }
    out.insert(out.end(), rec, rec + 8);
  }
  f = fopen(argv[2], "wb");
  if (!f || (!out.empty() && fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size()) || fclose(f)) return 5;
  return 0;
}
