// stem_sources_host.cpp -- stand-alone host driver of csrc/camera_source.h for tests/test_stem_sources_cpu.py: frame_kind, the
// function every camera call chooses its CameraKind with, on a list of (frame, destination, letterbox) geometries. Built by a host
// compiler (no HIP, no GPU).
//   stem_sources_host IN OUT
// IN : int32 n, then n records of 10 int32 -- format, region w, h, dst_w, dst_h, boxed, new_w, new_h, left, top.
// OUT: n int32 -- the CameraKind of each record.
#define UNINA_NO_HIP_HEADERS
#include "../unina-yolo-dla_amd/csrc/camera_source.h"

#include <cstdio>
#include <vector>

using namespace unina;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t n = 0;
  if (fread(&n, sizeof n, 1, f) != 1 || n < 0 || n > 100000) return 4;
  std::vector<int32_t> in((size_t)n * 10), out((size_t)n);
  if (n && fread(in.data(), sizeof(int32_t), in.size(), f) != in.size()) return 4;
  fclose(f);
  for (int i = 0; i < n; ++i) {
    const int32_t* r = &in[(size_t)i * 10];
    const unina_letterbox lb = {r[6], r[7], r[8], r[9]};   // new_w, new_h, left, top
    out[i] = frame_kind(r[0], r[1], r[2], r[3], r[4], r[5] ? &lb : nullptr);
  }
  f = fopen(argv[2], "wb");
  if (!f || (n && fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size()) || fclose(f)) return 5;
  return 0;
}
