// fuse_math.h -- the arithmetic of unina_fuse_async (include/unina_mi355.h "fusion of LiDAR cone candidates with camera records")
// as __host__ __device__ functions: the LiDAR cone's point and pixel, the camera record's grown box, the gated pair and its key,
// the point box of a LiDAR-only record and the slot count. csrc/fuse.hip calls them on the device, tests/fuse_math_host.cpp sweeps
// them on the host, fusion.fuse_numpy is their numpy twin. The transform is csrc/cloud_io.h's row, the projection csrc/lidar_project.h's
// expression, the box centre csrc/locate_window.h's. fp32 throughout, one rounding per operation in the order written: every
// translation unit that includes this header is compiled with -ffp-contract=off.
#ifndef UNINA_FUSE_MATH_H
#define UNINA_FUSE_MATH_H

#include <math.h>

#include "cloud_io.h"

namespace unina {

constexpr uint64_t kFuseNoKey = ~(uint64_t)0;   // above every pair key: d2's bits are at most +inf's

struct FusePoint {   // a LiDAR cone in the camera frame
  float xc, yc, zc;
  float u, v;        // 0, 0 where it is not projected
  int usable;        // 1: the cone is valid and the point is finite
  int projected;     // 1: usable and min_depth <= zc <= max_depth
};

struct FuseBox {     // a camera record's grown box in image pixels
  float uc, vc, hw, hh;
  int boxed;         // 1: the four scaled corners are finite and not inverted; 0: the floats are 0
};

// (x, y, z): the clusterer's position in the level frame; m: level frame -> camera optical frame
UNINA_HD FusePoint fuse_point(const float* m, float fx, float fy, float cx, float cy, float lift, float min_depth, float max_depth, float x,
                              float y, float z, int valid) {
  FusePoint p;
  const float zl = z + lift;
  p.xc = cloud_transform_row(m, x, y, zl);
  p.yc = cloud_transform_row(m + 4, x, y, zl);
  p.zc = cloud_transform_row(m + 8, x, y, zl);
  p.usable = (valid != 0 && finite(p.xc) && finite(p.yc) && finite(p.zc)) ? 1 : 0;
  p.projected = (p.usable && p.zc >= min_depth && p.zc <= max_depth) ? 1 : 0;
  p.u = p.v = 0.0f;
  if (p.projected) {   // zc >= min_depth > 0: the quotients are finite or infinite, never NaN
    p.u = (fx * p.xc) / p.zc + cx;
    p.v = (fy * p.yc) / p.zc + cy;
  }
  return p;
}

// (x1, y1, x2, y2): the record; sx, sy: record -> image pixels
UNINA_HD FuseBox fuse_box(float x1, float y1, float x2, float y2, float sx, float sy, float grow, float pad) {
  FuseBox b;
  b.uc = b.vc = b.hw = b.hh = 0.0f;
  b.boxed = 0;
  const float X1 = x1 * sx, X2 = x2 * sx, Y1 = y1 * sy, Y2 = y2 * sy;
  if (!finite(X1) || !finite(X2) || !finite(Y1) || !finite(Y2)) return b;
  if (!(X2 >= X1 && Y2 >= Y1)) return b;
  b.uc = 0.5f * (X1 + X2);
  b.vc = 0.5f * (Y1 + Y2);
  const float hg = 0.5f * grow;
  b.hw = hg * (X2 - X1) + pad;
  b.hh = hg * (Y2 - Y1) + pad;
  b.boxed = 1;
  return b;
}

// a projected LiDAR pixel (u, v, zc) against a boxed record; has_depth: cones[i].valid != 0, cz: cones[i].z. Every comparison fails
// on a NaN (a taken list entry carries u = NaN). *d2 is written in every case and read only where the pair is a candidate.
UNINA_HD bool fuse_candidate(float u, float v, float zc, float uc, float vc, float hw, float hh, int has_depth, float cz, float range_abs,
                             float range_rel, float* d2) {
  const float du = u - uc, dv = v - vc;
  *d2 = du * du + dv * dv;
  if (!(fabsf(du) <= hw && fabsf(dv) <= hh)) return false;
  return has_depth == 0 || fabsf(zc - cz) <= range_abs + range_rel * zc;
}

// (d2, index) as one unsigned key: ascending keys are ascending (d2, index); d2 is never negative
UNINA_HD uint64_t fuse_key(float d2, uint32_t index) { return ((uint64_t)float_bits(d2) << 32) | index; }

// one coordinate of a LiDAR-only record's point box, in record coordinates
UNINA_HD float fuse_record_coord(float pixel, float scale) { return pixel / scale; }

// how many records are written: the camera's, then the LiDAR-only ones while a slot is left
UNINA_HD int fuse_written(int n_camera, int n_lidar_only, int capacity) {
  const int room = capacity - n_camera;
  return n_camera + (n_lidar_only < room ? n_lidar_only : room);
}

}  // namespace unina
#endif  // UNINA_FUSE_MATH_H
