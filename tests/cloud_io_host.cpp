// cloud_io_host.cpp -- stand-alone host driver of csrc/cloud_io.h for tests/test_cloud_io_cpu.py: the checks of a cloud and an
// extrinsic that unina_locate_lidar_async and unina_ground_filter_async make before they touch HIP, and the choice of the 16-byte
// loads, built by a host compiler (no HIP, no GPU) and run on cases from a file. The addresses are never dereferenced.
//   cloud_io_host IN OUT
// IN : 2 int32 -- magic, n -- then n cases of 2 int32 (n_points, stride), 1 int64 (points), 2 int32 (max_points, 0), 12 float32
// prints per case one line: cloud_ok extrinsic_ok cloud_vec16, as 0 or 1; OUT is not written
#include "../unina-yolo-dla_amd/csrc/cloud_io.h"

#include <cstdio>
#include <vector>

using namespace unina;

struct Case {
  int32_t n_points, stride;
  int64_t points;
  int32_t max_points, pad;
  float m[12];
};
static_assert(sizeof(Case) == 72, "a case of the case file");

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[2];
  if (fread(h, sizeof h, 1, f) != 1 || h[0] != 0x434c4431 || h[1] < 0) return 4;
  std::vector<Case> cases((size_t)h[1]);
  if (h[1] && fread(cases.data(), sizeof(Case), cases.size(), f) != cases.size()) return 4;
  fclose(f);
  for (const Case& c : cases) {
    const unina_cloud cloud = {c.n_points, c.stride, reinterpret_cast<const void*>((uintptr_t)c.points)};
    printf("%d %d %d\n", cloud_ok(&cloud, c.max_points) ? 1 : 0, extrinsic_ok(c.m) ? 1 : 0, cloud_vec16(&cloud) ? 1 : 0);
  }
  printf("%d %d\n", cloud_ok(nullptr, 1) ? 1 : 0, extrinsic_ok(nullptr) ? 1 : 0);   // a missing cloud, a missing extrinsic
  return 0;
}
