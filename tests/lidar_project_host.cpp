// lidar_project_host.cpp -- stand-alone host driver of csrc/lidar_project.h for tests/test_lidar_cpu.py: the transform, the
// projection, the pixel, the key and the cell that csrc/lidar.hip computes per point, built by a host compiler (no HIP, no GPU)
// and run on points from a file.
//   lidar_project_host IN OUT
// IN : 2 int32 -- magic, n -- then the camera: 12 float32 (lidar_to_cam), 4 float32 (fx, fy, cx, cy), 2 int32 (width, height),
//      2 float32 (min_depth, max_depth); then n points of 3 float32
// OUT: per point 5 int32 -- u, v, key, projectable, and the point's cell (-1 where it is not projectable)
#include "../unina-yolo-dla_amd/csrc/lidar_project.h"

#include <cstdio>
#include <vector>

using namespace unina;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[2];
  LidarCamera cam;
  static_assert(sizeof(LidarCamera) == 80, "the camera block of the case file");
  if (fread(h, sizeof h, 1, f) != 1 || h[0] != 0x4c445231 || h[1] < 0 || fread(&cam, sizeof cam, 1, f) != 1) return 4;
  if (cam.width < 1 || cam.width > kLidarMaxDim || cam.height < 1 || cam.height > kLidarMaxDim) return 4;
  const int n = h[1];
  std::vector<float> xyz(3 * (size_t)n);
  if (n && fread(xyz.data(), 12, (size_t)n, f) != (size_t)n) return 4;
  fclose(f);
  const int cells_x = lidar_cells(cam.width), n_cells = cells_x * lidar_cells(cam.height);
  std::vector<int32_t> out;
  out.reserve(5 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    const LidarPixel p = lidar_project(cam, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    int cell = -1;
    if (p.projectable) {
      // what the kernels rely on: a projectable point's pixel is inside the image, so its cell has a counter
      if (p.u < 0 || p.u >= cam.width || p.v < 0 || p.v >= cam.height) return 6;
      cell = lidar_cell(p.u, p.v, cells_x);
      if (cell < 0 || cell >= n_cells) return 6;
    } else if (p.u != 0 || p.v != 0 || p.key != 0u) {
      return 6;
    }
    const int32_t rec[5] = {p.u, p.v, (int32_t)p.key, p.projectable, cell};
    out.insert(out.end(), rec, rec + 5);
  }
  f = fopen(argv[2], "wb");
  if (!f || (!out.empty() && fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size()) || fclose(f)) return 5;
  return 0;
}
