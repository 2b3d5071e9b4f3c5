// camera_pixel_host.cpp -- stand-alone host driver of csrc/camera_source.h for tests/test_camera_pixel_cpu.py: the functions the
// stem and the pre-process kernels call, built by a host compiler (no HIP, no GPU) and run on a frame from a file.
//   camera_pixel_host IN OUT
// IN : 24 int32 -- magic, mode, kind, w, h, pitch, uv_pitch, x0, y0, dst_w, dst_h, in_x0, in_y0, in_w, in_h, plane_bytes, uv_bytes,
//      plane_skew, uv_skew, wide_y, wide_c, x_even, 2 reserved -- then 7 float32 (pad, mean r g b, std r g b), then the plane
//      bytes and the chroma bytes. The planes are copied to 16-byte aligned buffers + skew, so a case chooses their alignment.
// OUT: float32 [3][dst_h][dst_w].
// mode 0: camera_pixel(kind) at every destination pixel. mode 1: nv12_quad over the region (kind kSrcNv12Tap, dst == region), four
// pixels at a time with the row tails as n < 4; wide_y / wide_c: 0 bytes, 1 dwords where nv12_quad_alignment allows them (its answer
// is printed); x_even as given (the caller answers for it).
#define UNINA_NO_HIP_HEADERS
#include "../unina-yolo-dla_amd/csrc/camera_source.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace unina;

static const uint8_t* aligned_copy(std::vector<uint8_t>* store, const uint8_t* src, size_t n, int skew) {
  store->assign(n + 32, 0);
  uint8_t* base = store->data();
  base += (16 - ((uintptr_t)base & 15)) & 15;
  memcpy(base + skew, src, n);
  return base + skew;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[24];
  float fl[7];
  if (fread(h, sizeof h, 1, f) != 1 || fread(fl, sizeof fl, 1, f) != 1 || h[0] != 0x43414d31) return 4;
  const int mode = h[1], plane_bytes = h[15], uv_bytes = h[16];
  if (plane_bytes < 0 || uv_bytes < 0) return 4;
  std::vector<uint8_t> raw((size_t)plane_bytes + uv_bytes), plane_store, uv_store;
  if (!raw.empty() && fread(raw.data(), raw.size(), 1, f) != 1) return 4;
  fclose(f);
  CameraSource s = {};
  s.plane = aligned_copy(&plane_store, raw.data(), plane_bytes, h[17]);
  s.uv = uv_bytes ? aligned_copy(&uv_store, raw.data() + plane_bytes, uv_bytes, h[18]) : nullptr;
  s.kind = h[2];
  s.w = h[3]; s.h = h[4]; s.pitch = h[5]; s.uv_pitch = h[6]; s.x0 = h[7]; s.y0 = h[8];
  s.dst_w = h[9]; s.dst_h = h[10];
  s.in_x0 = h[11]; s.in_y0 = h[12]; s.in_w = h[13]; s.in_h = h[14];
  s.pad = fl[0];
  s.norm = NormParams{fl[1], fl[2], fl[3], fl[4], fl[5], fl[6]};
  const int dw = s.dst_w, dh = s.dst_h;
  if (dw <= 0 || dh <= 0) return 4;
  std::vector<float> out((size_t)3 * dw * dh);
  const size_t plane = (size_t)dw * dh;
  if (mode == 0) {
    for (int y = 0; y < dh; ++y)
      for (int x = 0; x < dw; ++x) {
        float rgb[3];
        camera_pixel(s, s.kind, x, y, rgb);
        for (int c = 0; c < 3; ++c) out[c * plane + (size_t)y * dw + x] = rgb[c];
      }
  } else if (mode == 1) {
    if (s.kind != kSrcNv12Tap || dw != s.w || dh != s.h) return 4;
    bool wide_y, wide_c;
    nv12_quad_alignment(s, wide_y, wide_c);
    printf("%d %d\n", (int)wide_y, (int)wide_c);   // (what the frame allows; the case may still ask for bytes)
    wide_y = wide_y && h[19];
    wide_c = wide_c && h[20];
    for (int y = 0; y < dh; ++y)
      for (int x = 0; x < dw; x += 4) {
        const int n = dw - x < 4 ? dw - x : 4;
        float o[4][3];
        nv12_quad(s, s.x0 + x, s.y0 + y, n, h[21] != 0, wide_y && n == 4, wide_c && n == 4, o);
        for (int i = 0; i < n; ++i)
          for (int c = 0; c < 3; ++c) out[c * plane + (size_t)y * dw + x + i] = o[i][c];
      }
  } else {
    return 4;
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size() || fclose(f)) return 5;
  return 0;
}
