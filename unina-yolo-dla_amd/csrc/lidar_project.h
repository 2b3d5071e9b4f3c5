// lidar_project.h -- the per-point half of unina_locate_lidar_async (include/unina_mi355.h "3-D localisation from a LiDAR sweep"),
// as __host__ __device__ functions (csrc/hd.h): the LiDAR -> camera transform (csrc/cloud_io.h), the pinhole projection, the pixel, the key and
// the image cell of one point. csrc/lidar.hip calls them on the device, tests/lidar_project_host.cpp sweeps them on the host,
// localize.project_lidar_numpy is their numpy twin. fp32 throughout, one rounding per operation in the order written: every
// translation unit that includes this header is compiled with -ffp-contract=off.
#ifndef UNINA_LIDAR_PROJECT_H
#define UNINA_LIDAR_PROJECT_H

#include "cloud_io.h"

namespace unina {

constexpr int kLidarMaxDim = 16384;          // width / height limit: a pixel coordinate fits 14 bits, (float)width is exact
constexpr int kLidarCellShift = 5;           // image cells of 32 x 32 pixels
constexpr int kLidarMaxCells = (kLidarMaxDim >> kLidarCellShift) * (kLidarMaxDim >> kLidarCellShift);

struct LidarCamera {
  float m[12];   // row-major 3 x 4 [R|t]: LiDAR frame -> camera frame
  float fx, fy, cx, cy;
  int width, height;
  float min_depth, max_depth;
};

struct LidarPixel {   // unina_lidar_pixel
  int u, v;
  uint32_t key;
  int projectable;
};

UNINA_HD int lidar_cells(int pixels) { return (pixels + (1 << kLidarCellShift) - 1) >> kLidarCellShift; }
UNINA_HD int lidar_cell(int u, int v, int cells_x) { return (v >> kLidarCellShift) * cells_x + (u >> kLidarCellShift); }

// one point: all-zero where it is not projectable
UNINA_HD LidarPixel lidar_project(const LidarCamera& c, float x, float y, float z) {
  LidarPixel p;
  p.u = p.v = 0;
  p.key = 0u;
  p.projectable = 0;
  const float xc = cloud_transform_row(c.m, x, y, z);
  const float yc = cloud_transform_row(c.m + 4, x, y, z);
  const float zc = cloud_transform_row(c.m + 8, x, y, z);
  if (!finite(xc) || !finite(yc) || !finite(zc) || !(zc > 0.0f)) return p;
  const float u = (c.fx * xc) / zc + c.cx;
  const float v = (c.fy * yc) / zc + c.cy;
  if (!(u >= 0.0f && u < (float)c.width && v >= 0.0f && v < (float)c.height)) return p;   // a NaN fails
  p.u = (int)u;   // 0 <= u < width <= 16384: the conversion truncates inside the image; -0.0 is pixel 0
  p.v = (int)v;
  if (zc >= c.min_depth && zc <= c.max_depth) memcpy(&p.key, &zc, 4);   // min_depth > 0: the bits order as the depths do
  p.projectable = 1;
  return p;
}

}  // namespace unina
#endif  // UNINA_LIDAR_PROJECT_H
