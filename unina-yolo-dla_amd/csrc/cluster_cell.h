// cluster_cell.h -- the per-point and per-component halves of unina_cluster_async (include/unina_mi355.h "cone candidates from a
// ground-free LiDAR sweep"), as __host__ __device__ functions (csrc/hd.h): a point's cell, keys and fixed-point offsets (the
// transform of csrc/cloud_io.h, the cell and the key of csrc/ground_cell.h), a component's sums, its table entry with the gate,
// and the two records a CONE component becomes. csrc/cluster.hip calls them on the device, tests/cluster_cell_host.cpp sweeps
// them on the host, cluster.cluster_numpy is their numpy twin. fp32 throughout, one rounding per operation in the order written:
// every translation unit that includes this header is compiled with -ffp-contract=off.
#ifndef UNINA_CLUSTER_CELL_H
#define UNINA_CLUSTER_CELL_H

#include "ground_cell.h"

namespace unina {

struct ClusterGrid {   // lidar_to_level, then unina_cluster_params field for field
  float m[12];         // row-major 3 x 4 [R|t]: LiDAR frame -> level frame (z up)
  float x_min, y_min, cell;
  int nx, ny;
  int min_points, max_points;
  float min_height, max_height, max_width, confidence;
  int class_id;
};

struct ClusterPoint {
  int cell;                // -1: not IN_GRID; the other fields are then not used
  uint32_t kx, ky, kz;     // ground_key of xl, yl, zl
  int qx, qy;              // (int)(fx * 256.0f), (int)(fy * 256.0f): 0 .. 2^18 - 1
};

// what a component accumulates: integer minima, maxima and sums only
struct ClusterSums {
  uint32_t kx_lo, kx_hi, ky_lo, ky_hi, kz_lo, kz_hi;
  int n_points, n_cells;
  unsigned long long sx, sy;
};

UNINA_HD ClusterPoint cluster_point(const ClusterGrid& g, float x, float y, float z) {
  ClusterPoint p;
  const float xl = cloud_transform_row(g.m, x, y, z);
  const float yl = cloud_transform_row(g.m + 4, x, y, z);
  const float zl = cloud_transform_row(g.m + 8, x, y, z);
  float fx, fy;
  p.cell = grid_cell(xl, yl, zl, g.x_min, g.y_min, g.cell, g.nx, g.ny, &fx, &fy);
  p.kx = p.ky = p.kz = 0u;
  p.qx = p.qy = 0;
  if (p.cell < 0) return p;
  p.kx = ground_key(xl);
  p.ky = ground_key(yl);
  p.kz = ground_key(zl);
  p.qx = (int)(fx * 256.0f);   // 0 <= fx < 1024: the product is exact and below 2^18, the conversion truncates
  p.qy = (int)(fy * 256.0f);
  return p;
}

UNINA_HD void cluster_sums_clear(ClusterSums& s) {
  s.kx_lo = s.ky_lo = s.kz_lo = 0xffffffffu;
  s.kx_hi = s.ky_hi = s.kz_hi = 0u;
  s.n_points = s.n_cells = 0;
  s.sx = s.sy = 0ull;
}

// one coordinate of a component's position: the mean offset in 1/256 cells (an integer division), back in metres
UNINA_HD float cluster_position(float origin, unsigned long long sum, int n_points, float cell) {
  const int mean = (int)(sum / (unsigned long long)n_points);   // < 2^18: its float is exact, and so is the product with 2^-8
  return origin + ((float)mean * 0.00390625f) * cell;
}

// the table entry of a component (n_points >= 1: a component has an occupied cell) and whether it passes the gate
UNINA_HD unina_cluster cluster_finish(const ClusterGrid& g, const ClusterSums& s, int root) {
  unina_cluster c;
  c.x = cluster_position(g.x_min, s.sx, s.n_points, g.cell);
  c.y = cluster_position(g.y_min, s.sy, s.n_points, g.cell);
  c.x_lo = ground_unkey(s.kx_lo); c.x_hi = ground_unkey(s.kx_hi);
  c.y_lo = ground_unkey(s.ky_lo); c.y_hi = ground_unkey(s.ky_hi);
  c.z_lo = ground_unkey(s.kz_lo); c.z_hi = ground_unkey(s.kz_hi);
  c.n_points = s.n_points;
  c.n_cells = s.n_cells;
  c.root = root;
  const float wx = c.x_hi - c.x_lo, wy = c.y_hi - c.y_lo, h = c.z_hi - c.z_lo;   // finite operands; an overflow to inf fails the gate
  c.cone = (s.n_points >= g.min_points && s.n_points <= g.max_points && wx <= g.max_width && wy <= g.max_width && h >= g.min_height &&
            h <= g.max_height) ? 1 : 0;
  return c;
}

// the records of a CONE component: a bird's-eye box in level-frame metres and its position
UNINA_HD void cluster_records(const ClusterGrid& g, const unina_cluster& c, GpuDetection* det, unina_cone3d* cone) {
  det->x1 = c.x_lo; det->y1 = c.y_lo; det->x2 = c.x_hi; det->y2 = c.y_hi;
  det->confidence = g.confidence;
  det->class_id = g.class_id;
  det->valid = 1;
  det->_pad = 0;
  cone->x = c.x; cone->y = c.y; cone->z = c.z_lo;
  cone->u = 0.0f; cone->v = 0.0f;
  cone->n_valid = c.n_points;
  cone->n_samples = c.n_points;
  cone->valid = 1;
}

}  // namespace unina
#endif  // UNINA_CLUSTER_CELL_H
