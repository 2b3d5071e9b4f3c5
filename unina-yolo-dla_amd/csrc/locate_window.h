// locate_window.h -- the window, the sampling grid, the sample key and the back-projected point of unina_locate_async
// (include/unina_mi355.h "3-D localisation"), as __host__ __device__ functions (csrc/hd.h): csrc/locate.hip and csrc/stereo.hip
// call them on the device, tests/locate_window_host.cpp sweeps them on the host, localize.window_numpy and localize.point_numpy
// are their numpy twins. fp32 throughout, one rounding per operation: every translation unit that includes this header is
// compiled with -ffp-contract=off.
#ifndef UNINA_LOCATE_WINDOW_H
#define UNINA_LOCATE_WINDOW_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "hd.h"

namespace unina {

constexpr int kLocateMaxDim = 1 << 24;   // width / height limit: (float)(W - 1) is exact, every clipped bound converts to int

struct LocateWindow {
  int empty;        // 1: no pixel of the map is covered (or a coordinate is not finite, or the box is inverted)
  int u0, u1;       // first / last covered column, clipped to the map (u0 <= u1)
  int v0, v1;       // first / last covered row
  int stride_x, stride_y;
  int cols, rows;   // sampled columns u0 + i * stride_x <= u1, rows likewise
  int n_samples;    // cols * rows <= max_side^2
  float uc, vc;     // centre of the box in depth-map pixels
};

// one axis: the covered pixels floorf(c - h) .. floorf(c + h) against 0 .. n - 1, decided in float, converted after the clip
UNINA_HD bool locate_axis(float c, float h, int n, int max_side, int* lo, int* hi, int* stride, int* count) {
  const float flo = floorf(c - h), fhi = floorf(c + h);
  const float last = (float)(n - 1);
  if (!finite(flo) || !finite(fhi)) return false;
  if (fhi < 0.0f || flo > last) return false;           // wholly off the map
  const int a = flo < 0.0f ? 0 : (int)flo;              // 0 <= flo <= last here
  const int b = fhi > last ? n - 1 : (int)fhi;
  const int span = b - a + 1;
  const int s = (span + max_side - 1) / max_side;
  *lo = a;
  *hi = b;
  *stride = s;
  *count = (span - 1) / s + 1;                          // the i with a + i * s <= b
  return true;
}

// (x1, y1, x2, y2): the record; sx, sy: record -> depth-map pixels; width, height in 1..kLocateMaxDim; max_side in 1..256
UNINA_HD LocateWindow locate_window(float x1, float y1, float x2, float y2, float sx, float sy, float shrink, int width, int height,
                                    int max_side) {
  LocateWindow w;
  memset(&w, 0, sizeof(w));
  w.empty = 1;
  const float X1 = x1 * sx, X2 = x2 * sx, Y1 = y1 * sy, Y2 = y2 * sy;
  if (!finite(X1) || !finite(X2) || !finite(Y1) || !finite(Y2)) return w;
  if (X2 < X1 || Y2 < Y1) return w;
  const float uc = 0.5f * (X1 + X2), vc = 0.5f * (Y1 + Y2);
  const float hs = 0.5f * shrink;
  const float hw = hs * (X2 - X1), hh = hs * (Y2 - Y1);
  int u0, u1, v0, v1, stx, sty, cols, rows;
  if (!locate_axis(uc, hw, width, max_side, &u0, &u1, &stx, &cols)) return w;
  if (!locate_axis(vc, hh, height, max_side, &v0, &v1, &sty, &rows)) return w;
  w.empty = 0;
  w.u0 = u0; w.u1 = u1; w.v0 = v0; w.v1 = v1;
  w.stride_x = stx; w.stride_y = sty;
  w.cols = cols; w.rows = rows;
  w.n_samples = cols * rows;
  w.uc = uc; w.vc = vc;
  return w;
}

// The key of a raw sample: 0 = rejected; otherwise the raw bits, which order as unsigned integers exactly as the depths do
// (every accepted float is positive: min_depth > 0 and unit > 0).
UNINA_HD uint32_t locate_key_f32(uint32_t bits, float unit, float min_depth, float max_depth) {
  float f;
  memcpy(&f, &bits, 4);
  if (!finite(f)) return 0u;
  const float z = f * unit;
  return (z >= min_depth && z <= max_depth) ? bits : 0u;
}
UNINA_HD uint32_t locate_key_u16(uint32_t raw, float unit, float min_depth, float max_depth) {
  if (raw == 0u) return 0u;
  const float z = (float)raw * unit;
  return (z >= min_depth && z <= max_depth) ? raw : 0u;
}

// xyz[0..2] = the pixel (uc, vc) back-projected through the pinhole at depth Z
UNINA_HD void locate_point(float uc, float vc, float Z, float fx, float fy, float cx, float cy, float* xyz) {
  xyz[0] = ((uc - cx) * Z) / fx;
  xyz[1] = ((vc - cy) * Z) / fy;
  xyz[2] = Z;
}

}  // namespace unina
#endif  // UNINA_LOCATE_WINDOW_H
