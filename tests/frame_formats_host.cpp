// frame_formats_host.cpp -- stand-alone host driver of csrc/camera_source.h for tests/test_frame_formats_cpu.py: the frame
// descriptor's formats (RGB, RGBA, YUYV, UYVY, Bayer) through the functions the stem and the pre-process kernels call, and the host
// helpers the entry points build a CameraSource with (frame_defect, frame_source, frame_region, frame_kind), built by a host compiler
// (no HIP, no GPU) and run on a frame from a file.
//   frame_formats_host IN OUT
// IN : 24 int32 -- magic, mode, format, frame_w, frame_h, pitch, region x, y, w, h, dst_w, dst_h, boxed, in_x0, in_y0, in_w, in_h,
//      plane_bytes, plane_skew, wide, 4 reserved -- then 7 float32 (pad, mean r g b, std r g b), then the plane bytes. The plane is
//      copied to a 16-byte aligned buffer + skew that ends with it, so a case chooses its alignment.
// OUT: float32 [3][dst_h][dst_w] (modes 0 and 1).
// mode 0: camera_pixel at every destination pixel, the kind from frame_kind (boxed: letterboxed into the inner rectangle given).
// mode 1: yuv422_quad / bayer_quad over the region (tap only: dst == region), four pixels at a time with the row tails as n < 4;
//         wide: 0 bytes, 1 the wide loads where the format's alignment predicate allows them (its answer is printed).
// mode 2: frame_defect of the frame (plane_bytes == 0: a null plane); prints "ok" or what is wrong. No OUT.
#define UNINA_NO_HIP_HEADERS
#include "../unina-yolo-dla_amd/csrc/camera_source.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

using namespace unina;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[24];
  float fl[7];
  if (fread(h, sizeof h, 1, f) != 1 || fread(fl, sizeof fl, 1, f) != 1 || h[0] != 0x43414d32) return 4;
  const int mode = h[1], plane_bytes = h[17], skew = h[18];
  if (plane_bytes < 0 || skew < 0 || skew > 15) return 4;
  // exactly skew + plane_bytes bytes from a 16-byte aligned address: the sanitised build sees any read beyond the plane's last byte
  void* mem = nullptr;
  const size_t total = (size_t)plane_bytes + skew;
  if (posix_memalign(&mem, 16, total ? total : 1) != 0) return 4;
  const std::unique_ptr<void, decltype(&free)> owner(mem, free);
  uint8_t* base = static_cast<uint8_t*>(mem) + skew;
  if (plane_bytes && fread(base, plane_bytes, 1, f) != 1) return 4;
  fclose(f);
  unina_frame fr = {};
  fr.format = h[2];
  fr.width = h[3];
  fr.height = h[4];
  fr.plane[0] = plane_bytes ? base : nullptr;
  fr.pitch[0] = h[5];
  const char* why = frame_defect(&fr);
  if (mode == 2) {
    printf("%s\n", why ? why : "ok");
    return 0;
  }
  if (why) return 6;
  // (what the frame's geometry lets a kernel read must lie inside the bytes given: the sanitised build checks the rest)
  const NormParams norm = {fl[1], fl[2], fl[3], fl[4], fl[5], fl[6]};
  CameraSource s = frame_region(frame_source(fr, norm), h[6], h[7], h[8], h[9]);
  const int dw = h[10], dh = h[11];
  if (dw <= 0 || dh <= 0 || h[6] < 0 || h[7] < 0 || h[8] <= 0 || h[9] <= 0 || h[6] + h[8] > fr.width || h[7] + h[9] > fr.height) return 4;
  s.dst_w = dw;
  s.dst_h = dh;
  const unina_letterbox lb = {h[15], h[16], h[13], h[14]};   // new_w, new_h, left, top
  s.kind = frame_kind(fr.format, s.w, s.h, dw, dh, h[12] ? &lb : nullptr);
  if (h[12]) {
    s.in_x0 = lb.left;
    s.in_y0 = lb.top;
    s.in_w = lb.new_w;
    s.in_h = lb.new_h;
    s.pad = fl[0];
  }
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
    const bool yuv = cam_is_yuv422(s.format);
    if (s.kind != kSrcFrameTap || !(yuv || cam_is_bayer(s.format))) return 4;
    bool wide = yuv ? yuv422_quad_alignment(s) : bayer_quad_alignment(s);
    printf("%d\n", (int)wide);   // (what the frame allows; the case may still ask for bytes)
    wide = wide && h[19];
    for (int y = 0; y < dh; ++y)
      for (int x = 0; x < dw; x += 4) {
        const int n = dw - x < 4 ? dw - x : 4;
        float o[4][3];
        if (yuv) yuv422_quad(s, s.format, s.x0 + x, s.y0 + y, n, wide && n == 4, o);
        else bayer_quad(s, s.format, s.x0 + x, s.y0 + y, n, wide && n == 4, o);
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
