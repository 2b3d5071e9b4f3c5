// ground_cell.h -- the per-point and per-cell halves of unina_ground_filter_async (include/unina_mi355.h "ground removal from a
// LiDAR sweep"), as __host__ __device__ functions (csrc/hd.h): the LiDAR -> level transform (csrc/cloud_io.h),
// the grid cell of a point (also csrc/cluster_cell.h's), the ordered key of a height, one term of the envelope and the label. csrc/ground.hip calls them on
// the device, tests/ground_cell_host.cpp sweeps them on the host, ground.ground_numpy is their numpy twin. fp32 throughout, one
// rounding per operation in the order written: every translation unit that includes this header is compiled with
// -ffp-contract=off. Every decision after the transform and the two divides is a comparison of integers or of fp32 values
// that both sides compute alike.
#ifndef UNINA_GROUND_CELL_H
#define UNINA_GROUND_CELL_H

#include "cloud_io.h"

namespace unina {

constexpr int kGroundMaxSide = 1024;           // nx, ny: (float)nx is exact, a cell index fits 20 bits
constexpr int kGroundMaxReach = 4;
constexpr uint32_t kGroundEmpty = 0xffffffffu; // no finite float's key: a cell without a seed, a cell without an envelope
constexpr uint32_t kGroundNaN = 0x7fc00000u;   // the words of an entry behind the kept points, and h of a kept UNKNOWN point

enum GroundLabel { kGroundOutside = 0, kGroundUnknown = 1, kGroundGround = 2, kGroundObject = 3, kGroundAbove = 4, kGroundLabels = 5 };

struct GroundGrid {   // lidar_to_level, then unina_ground_params field for field
  float m[12];        // row-major 3 x 4 [R|t]: LiDAR frame -> level frame (z up)
  float x_min, y_min, cell;
  int nx, ny;
  float z_lo, z_hi, rise, band, max_height;
  int reach, keep_unknown;
};

struct GroundPoint {
  int cell;          // -1: not IN_GRID
  uint32_t z_bits;   // the bits of zl
  int seed;
};

// the casts of csrc/cloud_io.h under the names this header has always given them
UNINA_HD uint32_t ground_bits(float f) { return float_bits(f); }
UNINA_HD float ground_float(uint32_t b) { return bits_float(b); }

// unsigned order of keys = order of finite floats, -0.0 below +0.0
UNINA_HD uint32_t ground_key(float f) {
  const uint32_t b = ground_bits(f);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
UNINA_HD float ground_unkey(uint32_t k) { return ground_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }

// the grid cell of a point of the level frame, -1 where it is not IN_GRID; *fx, *fy: its position in cells (set whenever the
// three coordinates are finite). The one copy of the expression: ground_point and cluster_point (csrc/cluster_cell.h) call it.
UNINA_HD int grid_cell(float xl, float yl, float zl, float x_min, float y_min, float cell, int nx, int ny, float* fx, float* fy) {
  *fx = *fy = 0.0f;
  if (!finite(xl) || !finite(yl) || !finite(zl)) return -1;
  *fx = (xl - x_min) / cell;
  *fy = (yl - y_min) / cell;
  if (!(*fx >= 0.0f && *fx < (float)nx && *fy >= 0.0f && *fy < (float)ny)) return -1;   // a NaN fails
  return (int)*fy * nx + (int)*fx;   // 0 <= fx < nx <= 1024: the conversion truncates inside the grid; -0.0 is column 0
}

// one point: its cell, the bits of its height in the level frame, and whether it may found a ground height
UNINA_HD GroundPoint ground_point(const GroundGrid& g, float x, float y, float z) {
  GroundPoint p;
  const float xl = cloud_transform_row(g.m, x, y, z);
  const float yl = cloud_transform_row(g.m + 4, x, y, z);
  const float zl = cloud_transform_row(g.m + 8, x, y, z);
  float fx, fy;
  p.cell = grid_cell(xl, yl, zl, g.x_min, g.y_min, g.cell, g.nx, g.ny, &fx, &fy);
  p.z_bits = ground_bits(zl);
  p.seed = (p.cell >= 0 && zl >= g.z_lo && zl <= g.z_hi) ? 1 : 0;
  return p;
}

// the key a seeded cell at Chebyshev distance k offers to the envelope: its minimum raised by k rings
UNINA_HD uint32_t ground_term(uint32_t cellmin, int k, float rise) { return ground_key(ground_unkey(cellmin) + (float)k * rise); }

// the label of a point in `cell` (-1: not IN_GRID) at height zl over the envelope key g of that cell; *h_bits: the bits of zl - g,
// the NaN word where there is no envelope
UNINA_HD int ground_label(const GroundGrid& grid, int cell, float zl, uint32_t g, uint32_t* h_bits) {
  *h_bits = kGroundNaN;
  if (cell < 0) return kGroundOutside;
  if (g == kGroundEmpty) return kGroundUnknown;
  const float gf = ground_unkey(g);
  *h_bits = ground_bits(zl - gf);
  if (zl <= gf + grid.band) return kGroundGround;
  if (zl <= gf + grid.max_height) return kGroundObject;
  return kGroundAbove;
}

UNINA_HD bool ground_kept(int label, int keep_unknown) { return label == kGroundObject || (label == kGroundUnknown && keep_unknown != 0); }

}  // namespace unina
#endif  // UNINA_GROUND_CELL_H
