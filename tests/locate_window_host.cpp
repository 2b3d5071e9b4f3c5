// locate_window_host.cpp -- stand-alone host driver of csrc/locate_window.h for tests/test_locate_cpu.py: the window, grid and
// sample-key and point functions csrc/locate.hip calls, built by a host compiler (no HIP, no GPU) and run on cases from a file.
//   locate_window_host IN OUT
// IN : 3 int32 -- magic, mode, n -- then
//      mode 0: n cases of 7 float32 (x1, y1, x2, y2, sx, sy, shrink) + 3 int32 (width, height, max_side)
//      mode 1: 1 int32 (format) + 3 float32 (unit, min_depth, max_depth), then n uint32 raw samples
//      mode 2: 4 float32 (fx, fy, cx, cy), then n triples of float32 (uc, vc, Z)
// OUT: mode 0: per case 12 int32 -- empty, u0, u1, v0, v1, stride_x, stride_y, cols, rows, n_samples, bits of uc, bits of vc;
//              every sampled index is also walked and checked against the map (exit 6 if one falls outside)
//      mode 1: n uint32 keys
//      mode 2: per triple 3 int32 -- the bits of x, y, z
#include "../unina-yolo-dla_amd/csrc/locate_window.h"

#include <cstdio>
#include <vector>

using namespace unina;

struct Case {
  float x1, y1, x2, y2, sx, sy, shrink;
  int32_t width, height, max_side;
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[3];
  if (fread(h, sizeof h, 1, f) != 1 || h[0] != 0x4c4f4331 || h[2] < 0) return 4;
  const int mode = h[1], n = h[2];
  std::vector<int32_t> out;
  if (mode == 0) {
    std::vector<Case> cases((size_t)n);
    if (n && fread(cases.data(), sizeof(Case), (size_t)n, f) != (size_t)n) return 4;
    out.reserve((size_t)n * 12);
    for (const Case& c : cases) {
      if (c.width < 1 || c.height < 1 || c.width > kLocateMaxDim || c.height > kLocateMaxDim || c.max_side < 1 || c.max_side > 256) return 4;
      const LocateWindow w = locate_window(c.x1, c.y1, c.x2, c.y2, c.sx, c.sy, c.shrink, c.width, c.height, c.max_side);
      if (!w.empty) {
        // what the kernel indexes: the first and last sample of each axis, and the grid's size
        const int last_u = w.u0 + (w.cols - 1) * w.stride_x, last_v = w.v0 + (w.rows - 1) * w.stride_y;
        if (w.u0 < 0 || w.u1 >= c.width || w.v0 < 0 || w.v1 >= c.height || last_u > w.u1 || last_v > w.v1 || last_u + w.stride_x <= w.u1 ||
            last_v + w.stride_y <= w.v1 || w.cols < 1 || w.rows < 1 || w.cols > c.max_side || w.rows > c.max_side ||
            w.n_samples != w.cols * w.rows)
          return 6;
      }
      int32_t ub, vb;
      memcpy(&ub, &w.uc, 4);
      memcpy(&vb, &w.vc, 4);
      const int32_t rec[12] = {w.empty, w.u0, w.u1, w.v0, w.v1, w.stride_x, w.stride_y, w.cols, w.rows, w.n_samples, ub, vb};
      out.insert(out.end(), rec, rec + 12);
    }
  } else if (mode == 1) {
    int32_t fmt;
    float p[3];
    if (fread(&fmt, sizeof fmt, 1, f) != 1 || fread(p, sizeof p, 1, f) != 1) return 4;
    std::vector<uint32_t> raw((size_t)n);
    if (n && fread(raw.data(), sizeof(uint32_t), (size_t)n, f) != (size_t)n) return 4;
    out.reserve((size_t)n);
    for (uint32_t r : raw) out.push_back((int32_t)(fmt == 0 ? locate_key_f32(r, p[0], p[1], p[2]) : locate_key_u16(r, p[0], p[1], p[2])));
  } else if (mode == 2) {
    float cam[4];
    if (fread(cam, sizeof cam, 1, f) != 1) return 4;
    std::vector<float> in((size_t)n * 3);
    if (n && fread(in.data(), 3 * sizeof(float), (size_t)n, f) != (size_t)n) return 4;
    out.resize((size_t)n * 3);
    for (size_t i = 0; i < (size_t)n; ++i) {
      float xyz[3];
      locate_point(in[3 * i], in[3 * i + 1], in[3 * i + 2], cam[0], cam[1], cam[2], cam[3], xyz);
      memcpy(&out[3 * i], xyz, sizeof xyz);
    }
  } else {
    return 4;
  }
  fclose(f);
  f = fopen(argv[2], "wb");
  if (!f || (!out.empty() && fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size()) || fclose(f)) return 5;
  return 0;
}
