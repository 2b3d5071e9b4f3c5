// rectify_map_host.cpp -- stand-alone host driver of csrc/rectify_map.h for tests/test_rectify_cpu.py: the functions that
// csrc/rectify.hip calls for every output pixel, built by a host compiler (no HIP, no GPU) and run over one whole small image.
//   rectify_map_host IN OUT
// IN : one or more cases, each 7 int32 -- magic, src_w, src_h, channels, dst_w, dst_h, border -- then 22 float32 (unina_rectify_cam,
//      field for field), then the raw image, src_h * src_w * channels bytes without padding
// OUT: per case the rectified image, dst_h * dst_w * channels bytes without padding
// Both images of a case live in heap blocks of exactly their size, so a tap or a store one byte outside either is an error under
// -fsanitize=address.
#include "../unina-yolo-dla_amd/csrc/rectify_map.h"

#include <cstdio>
#include <cstdlib>

using namespace unina;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 5;
  int32_t h[7];
  RectifyCam cam;
  static_assert(sizeof(RectifyCam) == 22 * sizeof(float), "unina_rectify_cam is 22 floats");
  int n_cases = 0;
  while (fread(h, sizeof h, 1, f) == 1) {
    if (h[0] != 0x52454331 || fread(&cam, sizeof cam, 1, f) != 1) return 4;
    const int src_w = h[1], src_h = h[2], channels = h[3], dst_w = h[4], dst_h = h[5], border = h[6];
    if (src_w < 1 || src_w > 1024 || src_h < 1 || src_h > 1024 || dst_w < 1 || dst_w > 1024 || dst_h < 1 || dst_h > 1024) return 4;
    if ((channels != 1 && channels != 3 && channels != 4) || border < 0 || border > 255) return 4;
    const size_t src_bytes = (size_t)src_h * src_w * channels, dst_bytes = (size_t)dst_h * dst_w * channels;
    uint8_t* src = (uint8_t*)malloc(src_bytes);
    uint8_t* dst = (uint8_t*)malloc(dst_bytes);
    if (!src || !dst || fread(src, 1, src_bytes, f) != src_bytes) return 4;
    for (int v = 0; v < dst_h; ++v)
      for (int u = 0; u < dst_w; ++u)
        rectify_pixel(cam, u, v, src, src_w, src_h, src_w * channels, channels, border, dst + ((size_t)v * dst_w + u) * channels);
    if (fwrite(dst, 1, dst_bytes, out) != dst_bytes) return 5;
    free(src);
    free(dst);
    ++n_cases;
  }
  if (!feof(f) || n_cases == 0) return 4;
  fclose(f);
  if (fclose(out)) return 5;
  return 0;
}
