// ground_cell_host.cpp -- stand-alone host driver of csrc/ground_cell.h for tests/test_ground_cpu.py: the whole of
// unina_ground_filter_async computed with the functions csrc/ground.hip calls per point and per cell, built by a host compiler (no
// HIP, no GPU) and run on points from a file.
//   ground_cell_host IN OUT
// IN : 2 int32 -- magic, n -- then the GroundGrid: 12 float32 (lidar_to_level) and the 48 bytes of unina_ground_params; then n
//      points of 3 float32
// OUT: int32 words -- the header (8); per point 4 (cell or -1, bits of zl, label, bits of h); cellmin (nx * ny); ground (nx * ny);
//      the n entries of d_out (4 each)
#include "../unina-yolo-dla_amd/csrc/ground_cell.h"

#include <cstdio>
#include <vector>

using namespace unina;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[2];
  GroundGrid grid;
  static_assert(sizeof(GroundGrid) == 96, "the grid block of the case file");
  if (fread(h, sizeof h, 1, f) != 1 || h[0] != 0x47524e31 || h[1] < 0 || fread(&grid, sizeof grid, 1, f) != 1) return 4;
  if (grid.nx < 1 || grid.nx > kGroundMaxSide || grid.ny < 1 || grid.ny > kGroundMaxSide || grid.reach < 0 || grid.reach > kGroundMaxReach) return 4;
  const int n = h[1];
  std::vector<float> xyz(3 * (size_t)n);
  if (n && fread(xyz.data(), 12, (size_t)n, f) != (size_t)n) return 4;
  fclose(f);
  const int nx = grid.nx, ny = grid.ny, cells = nx * ny;

  std::vector<GroundPoint> pts((size_t)n);
  std::vector<uint32_t> cellmin((size_t)cells, kGroundEmpty), ground((size_t)cells, kGroundEmpty);
  for (int i = 0; i < n; ++i) {
    const GroundPoint p = ground_point(grid, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    // what the kernels rely on: a cell is -1 or has a word of the grid; only a point of the grid is a seed
    if (p.cell < -1 || p.cell >= cells || (p.seed && p.cell < 0)) return 6;
    pts[i] = p;
    if (p.seed) {
      const uint32_t k = ground_key(ground_float(p.z_bits));
      if (k == kGroundEmpty || ground_bits(ground_unkey(k)) != p.z_bits) return 6;   // a seed's key is never EMPTY and decodes to its height
      if (k < cellmin[p.cell]) cellmin[p.cell] = k;
    }
  }
  int seeded = 0;
  for (int cy = 0; cy < ny; ++cy) {
    for (int cx = 0; cx < nx; ++cx) {
      uint32_t best = kGroundEmpty;
      for (int dj = -grid.reach; dj <= grid.reach; ++dj) {
        for (int di = -grid.reach; di <= grid.reach; ++di) {
          const int gx = cx + di, gy = cy + dj;
          if (gx < 0 || gx >= nx || gy < 0 || gy >= ny) continue;
          const uint32_t v = cellmin[gy * nx + gx];
          if (v == kGroundEmpty) continue;
          const int aj = dj < 0 ? -dj : dj, ai = di < 0 ? -di : di;
          const uint32_t t = ground_term(v, aj > ai ? aj : ai, grid.rise);
          if (t == kGroundEmpty) return 6;   // finite + non-negative is never a NaN
          if (t < best) best = t;
        }
      }
      ground[cy * nx + cx] = best;
      seeded += cellmin[cy * nx + cx] != kGroundEmpty;
    }
  }
  std::vector<int32_t> head(8, 0), per_point, out_kept, out_rest;
  per_point.reserve(4 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    const GroundPoint& p = pts[i];
    uint32_t h_bits;
    const int label = ground_label(grid, p.cell, ground_float(p.z_bits), p.cell >= 0 ? ground[p.cell] : kGroundEmpty, &h_bits);
    if (label < 0 || label >= kGroundLabels) return 6;
    const int32_t rec[4] = {p.cell, (int32_t)p.z_bits, label, (int32_t)h_bits};
    per_point.insert(per_point.end(), rec, rec + 4);
    head[2 + label] += 1;
    if (ground_kept(label, grid.keep_unknown)) {
      const int32_t e[4] = {(int32_t)ground_bits(xyz[3 * i]), (int32_t)ground_bits(xyz[3 * i + 1]), (int32_t)ground_bits(xyz[3 * i + 2]), (int32_t)h_bits};
      out_kept.insert(out_kept.end(), e, e + 4);
    } else {
      out_rest.insert(out_rest.end(), 4, (int32_t)kGroundNaN);
    }
  }
  head[0] = n;
  head[1] = (int)(out_kept.size() / 4);
  head[7] = seeded;
  f = fopen(argv[2], "wb");
  if (!f) return 5;
  const std::vector<int32_t>* parts[] = {&head, &per_point, nullptr, nullptr, &out_kept, &out_rest};
  for (int k = 0; k < 6; ++k) {
    const void* data;
    size_t words;
    if (k == 2 || k == 3) {
      data = (k == 2 ? cellmin : ground).data();
      words = (size_t)cells;
    } else {
      data = parts[k]->data();
      words = parts[k]->size();
    }
    if (words && fwrite(data, 4, words, f) != words) return 5;
  }
  return fclose(f) ? 5 : 0;
}
