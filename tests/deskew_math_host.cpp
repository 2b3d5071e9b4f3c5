// deskew_math_host.cpp -- stand-alone host driver of csrc/deskew_math.h for tests/test_deskew_cpu.py: the per-point half that
// csrc/deskew.hip calls (time, validity, segment, pose, point, shift) and the float64 table of unina_deskew_table, built by a host
// compiler (no HIP, no GPU) and run on cases from a file.
//   deskew_math_host IN OUT
// IN : 4 int32 -- magic, mode, n, n_keys
//      mode 0: 1 int32 format, 3 int32 padding, n_keys rows of 8 float32 (the table), then n points of 4 words: x, y, z, time
//      mode 1: n == 0; 2 float64 t_sweep, t_ref, then n_keys poses of 8 float64: t, qw, qx, qy, qz, px, py, pz
// OUT: mode 0: 8 int32 per point -- the words of x', y', z', the shift's word, invalid, before, after, 0
//      mode 1: 8 int32 -- the return code, 0.. -- then n_keys rows of 8 float32 (all-zero where the code is not 0)
#include "../unina-yolo-dla_amd/csrc/deskew_math.h"

#include <cstdio>
#include <vector>

using namespace unina;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[4];
  if (fread(h, sizeof h, 1, f) != 1 || h[0] != 0x44534b31 || h[1] < 0 || h[1] > 1 || h[2] < 0) return 4;
  const int mode = h[1], n = h[2], n_keys = h[3];
  std::vector<int32_t> out;
  if (mode == 0) {
    int32_t fmt[4];
    if (n_keys < 2 || n_keys > kDeskewMaxKeys || fread(fmt, sizeof fmt, 1, f) != 1) return 4;
    std::vector<float> keys((size_t)n_keys * 8), t((size_t)n_keys);
    if (fread(keys.data(), 32, (size_t)n_keys, f) != (size_t)n_keys) return 4;
    for (int k = 0; k < n_keys; ++k) t[(size_t)k] = keys[(size_t)k * 8 + 7];
    std::vector<uint32_t> pts((size_t)n * 4);
    if (n && fread(pts.data(), 16, (size_t)n, f) != (size_t)n) return 4;
    out.reserve((size_t)n * 8);
    for (int i = 0; i < n; ++i) {
      const uint32_t* w = pts.data() + (size_t)i * 4;
      const DeskewPoint p = deskew_point(t.data(), keys.data(), n_keys, fmt[0], w[0], w[1], w[2], w[3]);
      const int32_t rec[8] = {(int32_t)p.x, (int32_t)p.y, (int32_t)p.z, (int32_t)p.shift2, p.invalid, p.before, p.after, 0};
      out.insert(out.end(), rec, rec + 8);
    }
  } else {
    double stamps[2];
    if (n != 0 || n_keys < 0 || n_keys > 1000 || fread(stamps, sizeof stamps, 1, f) != 1) return 4;
    std::vector<unina_deskew_pose> poses((size_t)n_keys);
    if (n_keys && fread(poses.data(), sizeof(unina_deskew_pose), (size_t)n_keys, f) != (size_t)n_keys) return 4;
    std::vector<unina_deskew_key> rows((size_t)(n_keys > kDeskewMaxKeys ? n_keys : kDeskewMaxKeys), unina_deskew_key{0, 0, 0, 0, 0, 0, 0, 0});
    const int rc = deskew_table(poses.data(), n_keys, stamps[0], stamps[1], rows.data());
    out.assign(8, 0);
    out[0] = rc;
    for (int k = 0; k < n_keys; ++k) {
      int32_t r[8];
      memcpy(r, &rows[(size_t)k], sizeof r);
      out.insert(out.end(), r, r + 8);
    }
  }
  fclose(f);
  f = fopen(argv[2], "wb");
  if (!f || (!out.empty() && fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size()) || fclose(f)) return 5;
  return 0;
}
