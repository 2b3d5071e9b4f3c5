// camera_source.h -- THE definition of a network-input pixel computed from a camera frame. The stem kernels (stem_pool.hip, the
// in-stem form behind unina_infer_bgra / _nv12 / _letterbox_* / _tiled_*) and the pre-process kernels (preprocess.hip, the two-step
// form that writes an fp32 tensor) both call camera_pixel / nv12_quad below, so the two forms agree bit for bit by construction.
// The arithmetic per pixel is that of ros2_ws/src/perception/src/cuda_preprocess.cu, expression trees rounded exactly as written:
//   plain BGRA   :99-128   u8 BGRA (pitched) -> RGB, ((v/255) - mean)/std
//   BGRA resize  :144-204  half-pixel-centre bilinear, clamp to [0, src-1], same normalise
//   NV12         :212-253  BT.601 (1.402 / 0.344136 / 0.714136 / 1.772), clamp, normalise
//   NV12 resize  (ours: the reference has none) the BGRA resize's coordinates, clamps and weights; the four taps are the clamped
//                FLOAT r, g, b of the NV12 conversion (never rounded to u8), blended w00*t00 + w01*t01 + w10*t10 + w11*t11 left to
//                right, then normalised
//   letterbox    (include/unina_mi355.h at unina_letterbox_geometry) inside the inner rectangle the pixel of the forms above for a
//                destination of in_w x in_h at (x - in_x0, y - in_y0), outside it r = g = b = pad, one normalise for both
// Every function carries `#pragma clang fp contract(off)` in its body: stem_pool.hip is built with contraction on (its FMA chain
// wants it), and a file-scope pragma here would leak into the includer.
// The header is plain C++17 as well: no HIP type is used, so a host compiler builds the same expressions (define
// UNINA_NO_HIP_HEADERS first) and tests/camera_pixel_host.cpp checks them against the oracle and the numpy twins without a GPU.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/unina_mi355.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define UNINA_CAM_FN __host__ __device__ __forceinline__
#else
#define UNINA_CAM_FN inline
#endif

namespace unina {

// What the stem reads. kSrcTensor: the fp32 planar tensor (StemParams::src). The others compute the pre-process on the fly instead of
// reading a tensor it would have written. *Tap: a region of the destination's size, one sample per pixel; *Resize: a region of any
// other size, bilinear; *Letterbox: the frame resized (or, where the inner rectangle has the region's size, tapped) into the inner
// rectangle, the pad value around it. camera_kind() (engine.hip) chooses.
enum CameraKind : int {
  kSrcTensor = 0,
  kSrcBgraTap = 1,
  kSrcBgraResize = 2,
  kSrcNv12Tap = 3,
  kSrcNv12Resize = 4,
  kSrcBgraLetterbox = 5,
  kSrcNv12Letterbox = 6
};

struct CameraSource {
  const uint8_t* plane;  // BGRA: the region's first pixel (a tile is a pointer offset). NV12: the luma plane of the WHOLE frame
  const uint8_t* uv;     // NV12: the interleaved chroma plane of the whole frame
  int w, h;              // size of the region that is read
  int pitch, uv_pitch;   // bytes per row of `plane` / `uv`
  int dst_w, dst_h;      // the destination (network input / output tensor): what the resize kinds are evaluated for
  NormParams norm;
  int in_x0, in_y0, in_w, in_h;   // letterbox kinds: the inner rectangle of the destination (unina_letterbox: left, top, new_w, new_h)
  float pad;             // letterbox kinds: r = g = b of every pixel outside it, before the normalisation
  int kind;              // CameraKind
  int x0, y0;            // NV12: the region's origin in the frame. It enters the chroma index ((y0 + y) / 2, (x0 + x) / 2), so an
                         // NV12 tile cannot be a pointer offset the way a BGRA tile is; may be odd
};

// an aligned dword of the frame (BGRA pixel, four luma bytes, two chroma pairs)
UNINA_CAM_FN uint32_t cam_load32(const uint8_t* p) {
  uint32_t v;
  memcpy(&v, __builtin_assume_aligned(p, 4), 4);
  return v;
}

UNINA_CAM_FN void cam_normalise(const NormParams& n, float r, float g, float b, float (&rgb)[3]) {
#pragma clang fp contract(off)
  rgb[0] = ((r / 255.0f) - n.mean_r) / n.std_r;
  rgb[1] = ((g / 255.0f) - n.mean_g) / n.std_g;
  rgb[2] = ((b / 255.0f) - n.mean_b) / n.std_b;
}

// BT.601 of one NV12 sample (cuda_preprocess.cu:229-241): the clamped values stay floats, they are never rounded to u8
UNINA_CAM_FN void nv12_rgb(float Y, float U, float V, float& r, float& g, float& b) {
#pragma clang fp contract(off)
  r = Y + 1.402f * V;
  g = Y - 0.344136f * U - 0.714136f * V;
  b = Y + 1.772f * U;
  r = fmaxf(0.0f, fminf(255.0f, r));
  g = fmaxf(0.0f, fminf(255.0f, g));
  b = fmaxf(0.0f, fminf(255.0f, b));
}

// The NV12 tap at pixel (xs, ys) of the region: frame pixel (x0 + xs, y0 + ys), whose chroma pair lies at row (y0 + ys) / 2, bytes
// 2 * ((x0 + xs) / 2) and + 1 of the chroma plane (cuda_preprocess.cu:224-227)
UNINA_CAM_FN void nv12_tap(const CameraSource& s, int xs, int ys, float& r, float& g, float& b) {
#pragma clang fp contract(off)
  const int X = s.x0 + xs, Y = s.y0 + ys;
  const float Yv = s.plane[(size_t)Y * s.pitch + X];
  const uint8_t* c = s.uv + (size_t)(Y / 2) * s.uv_pitch + (size_t)(X / 2) * 2;
  nv12_rgb(Yv, c[0] - 128.0f, c[1] - 128.0f, r, g, b);
}

// One BGRA pixel of the region: four bytes, B,G,R,A in memory, read as one aligned dword. (Returned by reference: by value the
// ABI turns the struct into an integer, and the device compiler then spends two more registers on the resize. The frame's
// bytes are read through a struct of char-typed members only, which may alias any storage.)
struct alignas(4) BgraPixel { uint8_t b, g, r, a; };
UNINA_CAM_FN const BgraPixel& bgra_tap(const CameraSource& s, int xs, int ys) {
  return *reinterpret_cast<const BgraPixel*>(s.plane + (size_t)ys * s.pitch + (size_t)xs * 4);
}

// the bilinear blend of four taps, left to right (cuda_preprocess.cu:186-198)
UNINA_CAM_FN float cam_blend(float w00, float w01, float w10, float w11, float t00, float t01, float t10, float t11) {
#pragma clang fp contract(off)
  return w00 * t00 + w01 * t01 + w10 * t10 + w11 * t11;
}

// Pixel (x, y) of the destination. `kind` is s.kind, passed apart so that a kernel built for one kind hands in a constant and the
// other branches fold; the stem hands in the kernel argument, where the branches are wave-uniform and only the letterbox's inside
// test is per pixel (lanes outside skip the taps).
UNINA_CAM_FN void camera_pixel(const CameraSource& s, int kind, int x, int y, float (&rgb)[3]) {
#pragma clang fp contract(off)
  float r, g, b;
  int dw = s.dst_w, dh = s.dst_h;
  bool inside = true;
  if (kind == kSrcBgraLetterbox || kind == kSrcNv12Letterbox) {
    dw = s.in_w;
    dh = s.in_h;
    x -= s.in_x0;
    y -= s.in_y0;
    inside = (unsigned)x < (unsigned)dw && (unsigned)y < (unsigned)dh;
    const bool tap = dw == s.w && dh == s.h;
    kind = kind == kSrcBgraLetterbox ? (tap ? kSrcBgraTap : kSrcBgraResize) : (tap ? kSrcNv12Tap : kSrcNv12Resize);
  }
  if (!inside) {
    r = g = b = s.pad;
  } else if (kind == kSrcBgraTap) {
    const BgraPixel px = bgra_tap(s, x, y);
    r = (float)px.r;
    g = (float)px.g;
    b = (float)px.b;
  } else if (kind == kSrcNv12Tap) {
    nv12_tap(s, x, y, r, g, b);
  } else {
    const int sw = s.w, sh = s.h;
    const float scale_x = (float)sw / dw, scale_y = (float)sh / dh;
    float sx = (x + 0.5f) * scale_x - 0.5f, sy = (y + 0.5f) * scale_y - 0.5f;
    sx = fmaxf(0.0f, fminf(sx, sw - 1.0f));
    sy = fmaxf(0.0f, fminf(sy, sh - 1.0f));
    const int xa = (int)sx, ya = (int)sy;
    const int xb = xa + 1 < sw - 1 ? xa + 1 : sw - 1, yb = ya + 1 < sh - 1 ? ya + 1 : sh - 1;
    const float fx = sx - xa, fy = sy - ya;
    const float w00 = (1.0f - fx) * (1.0f - fy), w01 = fx * (1.0f - fy), w10 = (1.0f - fx) * fy, w11 = fx * fy;
    if (kind == kSrcBgraResize) {
      const BgraPixel p00 = bgra_tap(s, xa, ya), p01 = bgra_tap(s, xb, ya), p10 = bgra_tap(s, xa, yb), p11 = bgra_tap(s, xb, yb);
      r = cam_blend(w00, w01, w10, w11, p00.r, p01.r, p10.r, p11.r);
      g = cam_blend(w00, w01, w10, w11, p00.g, p01.g, p10.g, p11.g);
      b = cam_blend(w00, w01, w10, w11, p00.b, p01.b, p10.b, p11.b);
    } else {
      float r00, g00, b00, r01, g01, b01, r10, g10, b10, r11, g11, b11;
      nv12_tap(s, xa, ya, r00, g00, b00);
      nv12_tap(s, xb, ya, r01, g01, b01);
      nv12_tap(s, xa, yb, r10, g10, b10);
      nv12_tap(s, xb, yb, r11, g11, b11);
      r = cam_blend(w00, w01, w10, w11, r00, r01, r10, r11);
      g = cam_blend(w00, w01, w10, w11, g00, g01, g10, g11);
      b = cam_blend(w00, w01, w10, w11, b00, b01, b10, b11);
    }
  }
  cam_normalise(s.norm, r, g, b, rgb);
}

// Whether nv12_quad may take the four luma bytes / the two chroma pairs of a quad as one dword: the same answer for every quad of
// the frame whose column within the region is a multiple of 4, it depends on the pitches, the plane addresses and the origin only
UNINA_CAM_FN void nv12_quad_alignment(const CameraSource& s, bool& wide_y, bool& wide_c) {
  wide_y = (s.pitch & 3) == 0 && (((uintptr_t)s.plane + (unsigned)s.x0) & 3) == 0;
  wide_c = (s.uv_pitch & 3) == 0 && (s.x0 & 1) == 0 && (((uintptr_t)s.uv + (unsigned)s.x0) & 3) == 0;
}

// Four consecutive kSrcNv12Tap pixels of a row, frame pixels (X .. X + 3, Y) with the origin already added, of which the first n lie
// inside the row (the others come out as the conversion of zero bytes and are not to be stored). A luma byte is read when its
// pixel is inside, a chroma pair when its first pixel is. wide_y / wide_c (nv12_quad_alignment; both need n == 4) take the luma /
// the chroma (X even: the pairs of pixels X, X + 1 | X + 2, X + 3) as one dword instead of bytes. x_even, a constant at the call
// site: the caller knows X to be even, so the byte form reads each of the two pairs once instead of once per pixel.
UNINA_CAM_FN void nv12_quad(const CameraSource& s, int X, int Y, int n, bool x_even, bool wide_y, bool wide_c, float (&o)[4][3]) {
#pragma clang fp contract(off)
  const uint8_t* yrow = s.plane + (size_t)Y * s.pitch + X;
  const uint8_t* crow = s.uv + (size_t)(Y / 2) * s.uv_pitch;
  uint8_t yy[4], uu[4], vv[4];
  if (wide_y) {
    const uint32_t yw = cam_load32(yrow);
#pragma unroll
    for (int i = 0; i < 4; ++i) yy[i] = (uint8_t)(yw >> (8 * i));
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) yy[i] = i < n ? yrow[i] : 0;
  }
  if (wide_c) {
    const uint32_t cw = cam_load32(crow + X);
    uu[0] = uu[1] = (uint8_t)cw;
    vv[0] = vv[1] = (uint8_t)(cw >> 8);
    uu[2] = uu[3] = (uint8_t)(cw >> 16);
    vv[2] = vv[3] = (uint8_t)(cw >> 24);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (x_even && (i & 1)) {
        uu[i] = uu[i - 1];
        vv[i] = vv[i - 1];
      } else {
        const int P = (X + i) & ~1;                     // the pair's first pixel (X >= 0)
        const bool in = P < X + n;
        uu[i] = in ? crow[P] : 0;
        vv[i] = in ? crow[P + 1] : 0;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float r, g, b;
    nv12_rgb((float)yy[i], uu[i] - 128.0f, vv[i] - 128.0f, r, g, b);
    cam_normalise(s.norm, r, g, b, o[i]);
  }
}

}  // namespace unina
