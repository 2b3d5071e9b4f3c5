// cluster_cell_host.cpp -- stand-alone host driver of csrc/cluster_cell.h for tests/test_cluster_cpu.py: the whole of
// unina_cluster_async computed with the functions csrc/cluster.hip calls per point and per component, built by a host compiler (no
// HIP, no GPU) and run on points from a file. The components come from a plain flood fill over the occupied cells.
//   cluster_cell_host IN OUT
// IN : 2 int32 -- magic, n -- then the ClusterGrid: 12 float32 (lidar_to_level) and the 48 bytes of unina_cluster_params; then n
//      points of 3 float32
// OUT: int32 words -- the header (8); per point 7 (cell or -1, kx, ky, kz, qx, qy, component or -1); the table (12 a component);
//      MAX_DETECTIONS GpuDetection (8 each); MAX_DETECTIONS unina_cone3d (8 each); the count (1); Sx and Sy of every component as
//      two words each (low, high)
#include "../unina-yolo-dla_amd/csrc/cluster_cell.h"

#include <cstdio>
#include <vector>

using namespace unina;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[2];
  ClusterGrid grid;
  static_assert(sizeof(ClusterGrid) == 96, "the grid block of the case file");
  static_assert(sizeof(unina_cluster) == 48 && sizeof(GpuDetection) == 32 && sizeof(unina_cone3d) == 32, "records as words");
  if (fread(h, sizeof h, 1, f) != 1 || h[0] != 0x434c5531 || h[1] < 0 || fread(&grid, sizeof grid, 1, f) != 1) return 4;
  if (grid.nx < 1 || grid.nx > kGroundMaxSide || grid.ny < 1 || grid.ny > kGroundMaxSide) return 4;
  const int n = h[1];
  std::vector<float> xyz(3 * (size_t)n);
  if (n && fread(xyz.data(), 12, (size_t)n, f) != (size_t)n) return 4;
  fclose(f);
  const int nx = grid.nx, ny = grid.ny, cells = nx * ny;

  std::vector<ClusterPoint> pts((size_t)n);
  std::vector<int> root((size_t)cells, -1), rank((size_t)cells, -1);
  std::vector<char> occupied((size_t)cells, 0);
  int n_in_grid = 0, n_cells = 0;
  for (int i = 0; i < n; ++i) {
    const ClusterPoint p = cluster_point(grid, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    // what the kernels rely on: a cell is -1 or has a word of the grid; an offset is below 2^18 and not negative
    if (p.cell < -1 || p.cell >= cells) return 6;
    if (p.cell >= 0 && (p.qx < 0 || p.qx >= (1 << 18) || p.qy < 0 || p.qy >= (1 << 18) || p.qx / 256 != p.cell % nx || p.qy / 256 != p.cell / nx)) return 6;
    if (p.cell >= 0 && (p.kx == kGroundEmpty || p.ky == kGroundEmpty || p.kz == kGroundEmpty)) return 6;   // finite: never the EMPTY key
    pts[i] = p;
    if (p.cell >= 0) {
      n_in_grid += 1;
      n_cells += !occupied[p.cell];
      occupied[p.cell] = 1;
    }
  }
  // components in ascending root: the first unvisited occupied cell in index order is the smallest of its component
  std::vector<ClusterSums> sums;
  std::vector<int> roots, stack;
  for (int c = 0; c < cells; ++c) {
    if (!occupied[c] || root[c] >= 0) continue;
    const int k = (int)roots.size();
    roots.push_back(c);
    ClusterSums s;
    cluster_sums_clear(s);
    sums.push_back(s);
    root[c] = c;
    stack.push_back(c);
    while (!stack.empty()) {
      const int v = stack.back();
      stack.pop_back();
      rank[v] = k;
      sums[k].n_cells += 1;
      for (int dj = -1; dj <= 1; ++dj) {
        for (int di = -1; di <= 1; ++di) {
          const int ox = v % nx + di, oy = v / nx + dj;
          if (ox < 0 || ox >= nx || oy < 0 || oy >= ny) continue;
          const int o = oy * nx + ox;
          if (occupied[o] && root[o] < 0) {
            root[o] = c;
            stack.push_back(o);
          }
        }
      }
    }
  }
  std::vector<int32_t> per_point;
  per_point.reserve(7 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    const ClusterPoint& p = pts[i];
    const int k = p.cell >= 0 ? rank[p.cell] : -1;
    const int32_t rec[7] = {p.cell, (int32_t)p.kx, (int32_t)p.ky, (int32_t)p.kz, p.qx, p.qy, k};
    per_point.insert(per_point.end(), rec, rec + 7);
    if (k < 0) continue;
    ClusterSums& s = sums[k];
    if (p.kx < s.kx_lo) s.kx_lo = p.kx;
    if (p.kx > s.kx_hi) s.kx_hi = p.kx;
    if (p.ky < s.ky_lo) s.ky_lo = p.ky;
    if (p.ky > s.ky_hi) s.ky_hi = p.ky;
    if (p.kz < s.kz_lo) s.kz_lo = p.kz;
    if (p.kz > s.kz_hi) s.kz_hi = p.kz;
    s.n_points += 1;
    s.sx += (unsigned long long)p.qx;
    s.sy += (unsigned long long)p.qy;
  }
  std::vector<unina_cluster> table(roots.size());
  std::vector<GpuDetection> dets(MAX_DETECTIONS);
  std::vector<unina_cone3d> cones(MAX_DETECTIONS);
  memset(dets.data(), 0, dets.size() * sizeof(GpuDetection));
  memset(cones.data(), 0, cones.size() * sizeof(unina_cone3d));
  int n_cones = 0, n_written = 0;
  std::vector<uint32_t> sum_words;
  for (size_t k = 0; k < roots.size(); ++k) {
    if (sums[k].n_points < 1) return 6;   // a component has an occupied cell, an occupied cell a point
    memset(&table[k], 0, sizeof(unina_cluster));
    table[k] = cluster_finish(grid, sums[k], roots[k]);
    if (table[k].cone != 0 && table[k].cone != 1) return 6;
    if (table[k].cone) {
      if (n_written < MAX_DETECTIONS) {
        cluster_records(grid, table[k], &dets[n_written], &cones[n_written]);
        n_written += 1;
      }
      n_cones += 1;
    }
    const uint32_t w[4] = {(uint32_t)sums[k].sx, (uint32_t)(sums[k].sx >> 32), (uint32_t)sums[k].sy, (uint32_t)(sums[k].sy >> 32)};
    sum_words.insert(sum_words.end(), w, w + 4);
  }
  int32_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (n) {
    const int32_t filled[8] = {n, n_in_grid, n_cells, (int32_t)roots.size(), n_cones, n_written, n_cones - n_written, 0};
    memcpy(head, filled, sizeof head);
  }
  const int32_t count = n_written;
  f = fopen(argv[2], "wb");
  if (!f) return 5;
  bool ok = fwrite(head, 4, 8, f) == 8;
  ok = ok && (per_point.empty() || fwrite(per_point.data(), 4, per_point.size(), f) == per_point.size());
  ok = ok && (table.empty() || fwrite(table.data(), sizeof(unina_cluster), table.size(), f) == table.size());
  ok = ok && fwrite(dets.data(), sizeof(GpuDetection), dets.size(), f) == dets.size();
  ok = ok && fwrite(cones.data(), sizeof(unina_cone3d), cones.size(), f) == cones.size();
  ok = ok && fwrite(&count, 4, 1, f) == 1;
  ok = ok && (sum_words.empty() || fwrite(sum_words.data(), 4, sum_words.size(), f) == sum_words.size());
  return (fclose(f) || !ok) ? 5 : 0;
}
