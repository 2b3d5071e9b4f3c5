// rectify_map.h -- the pure parts of unina_rectify_async (include/unina_mi355.h "Rectification"), as __host__ __device__
// functions (csrc/hd.h): the source position of one output pixel, the inside test, the fixed-point split, the four-tap blend
// and one whole output pixel. csrc/rectify.hip calls them on the device, tests/rectify_map_host.cpp runs them over whole small
// images on the host, rectify.rectify_source_numpy / rectify.rectify_numpy are their numpy twins. fp32 throughout, one rounding
// per operation in the order written: every translation unit that includes this header is compiled with -ffp-contract=off.
// Everything behind the inside test is integer arithmetic.
#ifndef UNINA_RECTIFY_MAP_H
#define UNINA_RECTIFY_MAP_H

#include <math.h>
#include <stdint.h>

#include "hd.h"

namespace unina {

constexpr int kRectifyMaxImages = 4;     // UNINA_RECTIFY_MAX_IMAGES
constexpr int kRectifyMaxDim = 16384;    // UNINA_RECTIFY_MAX_DIM: (float)(32 * size) is exact
constexpr int kRectifyFracBits = 5;      // 1/32 pixel, as OpenCV's fixed-point remap
constexpr int kRectifyOne = 1 << kRectifyFracBits;

struct RectifyPinhole {   // unina_pinhole
  float fx, fy, cx, cy;
};
struct RectifyCam {   // unina_rectify_cam, field for field
  RectifyPinhole src;
  float k1, k2, p1, p2, k3;
  float r[9];
  RectifyPinhole dst;
};

struct RectifySource {
  float us, vs;   // raw-image position of the output pixel's centre
  float tx, ty;   // the same in 1/32 pixels, plus the half that rounds
  float W;        // depth of the ray in the raw camera's frame: the pixel is behind that camera where W <= 0
};

// output pixel (u, v) -> where it comes from
UNINA_HD RectifySource rectify_source(const RectifyCam& c, int u, int v) {
  RectifySource s;
  const float x = ((float)u - c.dst.cx) / c.dst.fx;
  const float y = ((float)v - c.dst.cy) / c.dst.fy;
  const float X = (c.r[0] * x + c.r[3] * y) + c.r[6];   // R^T * (x, y, 1)
  const float Y = (c.r[1] * x + c.r[4] * y) + c.r[7];
  s.W = (c.r[2] * x + c.r[5] * y) + c.r[8];
  const float xn = X / s.W;
  const float yn = Y / s.W;
  const float r2 = xn * xn + yn * yn;
  const float rad = ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2 + 1.0f;
  const float xy2 = (2.0f * xn) * yn;
  const float xd = (xn * rad + c.p1 * xy2) + c.p2 * (r2 + 2.0f * (xn * xn));
  const float yd = (yn * rad + c.p1 * (r2 + 2.0f * (yn * yn))) + c.p2 * xy2;
  s.us = c.src.fx * xd + c.src.cx;
  s.vs = c.src.fy * yd + c.src.cy;
  s.tx = s.us * 32.0f + 0.5f;
  s.ty = s.vs * 32.0f + 0.5f;
  return s;
}

// a NaN fails; src_w, src_h <= kRectifyMaxDim, so both float bounds are exact and floorf(tx), floorf(ty) convert to int exactly
UNINA_HD bool rectify_inside(const RectifySource& s, int src_w, int src_h) {
  return s.W > 0.0f && -32.0f <= s.tx && s.tx < (float)(32 * src_w) && -32.0f <= s.ty && s.ty < (float)(32 * src_h);
}

// t in [-32, 32 * size): *p0 = the first tap in -1 .. size - 1, the return value = the weight of the second tap in 0 .. 31
UNINA_HD int rectify_split(float t, int* p0) {
  const int q = (int)floorf(t);
  *p0 = q >> kRectifyFracBits;   // arithmetic: -32 .. -1 is tap -1
  return q & (kRectifyOne - 1);
}

UNINA_HD int rectify_blend(int ax, int ay, int t00, int t10, int t01, int t11) {
  return ((kRectifyOne - ax) * (kRectifyOne - ay) * t00 + ax * (kRectifyOne - ay) * t10 + (kRectifyOne - ax) * ay * t01 + ax * ay * t11 + 512) >> 10;
}

// One tap of an interleaved image of `channels` bytes per pixel; a tap outside the image is `border`, and its address is never formed.
UNINA_HD int rectify_tap(const uint8_t* src, int src_w, int src_h, int pitch, int channels, int x, int y, int ch, int border) {
  if (x < 0 || y < 0 || x >= src_w || y >= src_h) return border;
  return src[(size_t)y * (size_t)pitch + (size_t)x * (size_t)channels + (size_t)ch];
}

// One whole output pixel, the plain way: out[0 .. channels - 1]
UNINA_HD void rectify_pixel(const RectifyCam& c, int u, int v, const uint8_t* src, int src_w, int src_h, int pitch, int channels, int border,
                            uint8_t* out) {
  const RectifySource s = rectify_source(c, u, v);
  if (!rectify_inside(s, src_w, src_h)) {
    for (int ch = 0; ch < channels; ++ch) out[ch] = (uint8_t)border;
    return;
  }
  int x0, y0;
  const int ax = rectify_split(s.tx, &x0), ay = rectify_split(s.ty, &y0);
  for (int ch = 0; ch < channels; ++ch) {
    const int t00 = rectify_tap(src, src_w, src_h, pitch, channels, x0, y0, ch, border);
    const int t10 = rectify_tap(src, src_w, src_h, pitch, channels, x0 + 1, y0, ch, border);
    const int t01 = rectify_tap(src, src_w, src_h, pitch, channels, x0, y0 + 1, ch, border);
    const int t11 = rectify_tap(src, src_w, src_h, pitch, channels, x0 + 1, y0 + 1, ch, border);
    out[ch] = (uint8_t)rectify_blend(ax, ay, t00, t10, t01, t11);
  }
}

}  // namespace unina
#endif  // UNINA_RECTIFY_MAP_H
