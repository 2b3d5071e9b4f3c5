// camera_source.h -- THE definition of a network-input pixel computed from a camera frame. The stem kernels (stem_pool.hip, the
// in-stem form behind unina_infer_bgra / _nv12 / _letterbox_* / _tiled_*) and the pre-process kernels (preprocess.hip, the two-step
// form that writes an fp32 tensor) both call camera_pixel / nv12_quad / yuv422_quad / bayer_quad below, so the two forms agree bit for bit by construction.
// The arithmetic per pixel is that of ros2_ws/src/perception/src/cuda_preprocess.cu, expression trees rounded exactly as written:
//   plain BGRA   :99-128   u8 BGRA (pitched) -> RGB, ((v/255) - mean)/std
//   BGRA resize  :144-204  half-pixel-centre bilinear, clamp to [0, src-1], same normalise
//   NV12         :212-253  BT.601 (1.402 / 0.344136 / 0.714136 / 1.772), clamp, normalise
//   NV12 resize  (ours: the reference has none) the BGRA resize's coordinates, clamps and weights; the four taps are the clamped
//                FLOAT r, g, b of the NV12 conversion (never rounded to u8), blended w00*t00 + w01*t01 + w10*t10 + w11*t11 left to
//                right, then normalised
//   RGB / RGBA   (GpuBufferPtr.msg formats 2 / 3) r, g, b are bytes 0, 1, 2 of the 3- / 4-byte pixel; everything else as for BGRA
//   YUYV / UYVY  packed 4:2:2: the pair of pixels (X & ~1, X | 1) is four bytes, Y0 U Y1 V / U Y0 V Y1; BT.601 as for NV12
//   Bayer        (ours) bilinear demosaic of an 8-bit mosaic, neighbours read from the FRAME with reflect-101 at its borders
//                (include/unina_mi355.h at unina_pixel_format); for these formats the tap / resize / letterbox geometry is the one
//                above on the float r, g, b of camera_tap
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
// rectangle, the pad value around it. frame_kind() (below) chooses.
enum CameraKind : int {
  kSrcTensor = 0,
  kSrcBgraTap = 1,
  kSrcBgraResize = 2,
  kSrcNv12Tap = 3,
  kSrcNv12Resize = 4,
  kSrcBgraLetterbox = 5,
  kSrcNv12Letterbox = 6,
  // every other unina_pixel_format (CameraSource::format says which; wave-uniform): the same three geometries on camera_tap
  kSrcFrameTap = 7,
  kSrcFrameResize = 8,
  kSrcFrameLetterbox = 9
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
                         // NV12 tile cannot be a pointer offset the way a BGRA tile is; may be odd. 4:2:2 (the pair index) and
                         // Bayer (the colour phase and the frame's borders) likewise; RGB / RGBA tiles are pointer offsets
  int format;            // the unina_pixel_format. The kSrcFrame* kinds (formats 2..9) dispatch on it; the kinds above name theirs
  int frame_w, frame_h;  // Bayer: the size of the WHOLE frame `plane` points at (a tile reads its neighbours from the frame)
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

// ---- the formats behind the kSrcFrame* kinds ----
UNINA_CAM_FN bool cam_is_yuv422(int format) { return format == UNINA_FMT_YUYV || format == UNINA_FMT_UYVY; }
UNINA_CAM_FN bool cam_is_bayer(int format) { return format >= UNINA_FMT_BAYER_RGGB && format <= UNINA_FMT_BAYER_GBRG; }

// Packed 4:2:2 at frame pixel (X, Y): the pair of pixels X & ~1, X | 1 is the four bytes at 4 * (X / 2) of the row, Y0 U Y1 V
// (YUYV) or U Y0 V Y1 (UYVY); then nv12_rgb unchanged
UNINA_CAM_FN void yuv422_tap(const CameraSource& s, int format, int X, int Y, float& r, float& g, float& b) {
#pragma clang fp contract(off)
  const uint8_t* pair = s.plane + (size_t)Y * s.pitch + (size_t)(X / 2) * 4;
  const int o = format == UNINA_FMT_UYVY ? 1 : 0;
  const float Yv = pair[o + 2 * (X & 1)];
  nv12_rgb(Yv, pair[1 - o] - 128.0f, pair[3 - o] - 128.0f, r, g, b);
}

// reflect-101 at a border of the frame (-1 -> 1, n -> n - 2): the neighbour keeps its colour phase. Only one step outside occurs.
UNINA_CAM_FN int cam_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// Where the pattern has its RED site: (X & 1, Y & 1) == (rx, ry). Blue is diagonal to it, green the other two.
UNINA_CAM_FN void bayer_red_site(int format, int& rx, int& ry) {
  rx = (format == UNINA_FMT_BAYER_BGGR || format == UNINA_FMT_BAYER_GRBG) ? 1 : 0;
  ry = (format == UNINA_FMT_BAYER_BGGR || format == UNINA_FMT_BAYER_GBRG) ? 1 : 0;
}

// The bilinear demosaic at a site from its 3 x 3 neighbourhood n[row][column] (n[1][1] the site itself), px / py the site's
// parities. Sums of at most four bytes times a power of two: exact in fp32.
UNINA_CAM_FN void bayer_rgb(const float (&n)[3][3], int px, int py, int rx, int ry, float& r, float& g, float& b) {
#pragma clang fp contract(off)
  const float cross = (n[0][1] + n[1][0] + n[1][2] + n[2][1]) * 0.25f;
  const float diag = (n[0][0] + n[0][2] + n[2][0] + n[2][2]) * 0.25f;
  const float horz = (n[1][0] + n[1][2]) * 0.5f, vert = (n[0][1] + n[2][1]) * 0.5f;
  const bool red_row = py == ry, red_col = px == rx;
  if (red_row == red_col) {                 // an R or a B site: green from the cross, the opposite colour from the diagonals
    g = cross;
    r = red_row ? n[1][1] : diag;
    b = red_row ? diag : n[1][1];
  } else {                                  // a G site: one colour on its row, the other on its column
    g = n[1][1];
    r = red_row ? horz : vert;
    b = red_row ? vert : horz;
  }
}

UNINA_CAM_FN void bayer_tap(const CameraSource& s, int format, int X, int Y, float& r, float& g, float& b) {
  int rx, ry;
  bayer_red_site(format, rx, ry);
  float n[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    // (a 32-bit byte offset from the uniform base: one address register per load instead of two. frame_defect refuses a Bayer
    // frame of 4 GiB or more.)
    const uint32_t row = (uint32_t)cam_reflect(Y + j - 1, s.frame_h) * (uint32_t)s.pitch;
#pragma unroll
    for (int i = 0; i < 3; ++i) n[j][i] = (float)s.plane[row + (uint32_t)cam_reflect(X + i - 1, s.frame_w)];
  }
  bayer_rgb(n, X & 1, Y & 1, rx, ry, r, g, b);
}

// The float r, g, b of pixel (xs, ys) of the region for the kSrcFrame* kinds. `format` is s.format, passed apart as `kind` is.
UNINA_CAM_FN void camera_tap(const CameraSource& s, int format, int xs, int ys, float& r, float& g, float& b) {
  if (format == UNINA_FMT_RGB || format == UNINA_FMT_RGBA) {
    const uint8_t* p = s.plane + (size_t)ys * s.pitch + (size_t)xs * (format == UNINA_FMT_RGB ? 3 : 4);
    r = (float)p[0];
    g = (float)p[1];
    b = (float)p[2];
  } else if (cam_is_yuv422(format)) {
    yuv422_tap(s, format, s.x0 + xs, s.y0 + ys, r, g, b);
  } else {
    bayer_tap(s, format, s.x0 + xs, s.y0 + ys, r, g, b);
  }
}

// Pixel (x, y) of the destination for the kSrcFrame* kinds (frame_rgb: before the normalisation): the geometry of camera_pixel_classic below (the same coordinates, clamps,
// weights, blend, inside test and normalise) on camera_tap. Kept apart from it so that the BGRA / NV12 kinds compile to what they
// compiled to before these formats existed; the stems call the two from separate loops. kRolled: the resize takes its four taps
// one after the other in a loop that is not unrolled -- the same sum (0 + w00 * t00 is w00 * t00: no product is negative), a
// quarter of the loads in flight, for a caller short of registers (the one-thread-per-pixel stem).
template <bool kRolled = false>
UNINA_CAM_FN void frame_rgb(const CameraSource& s, int kind, int x, int y, float& r, float& g, float& b) {
#pragma clang fp contract(off)
  const int format = s.format;
  int dw = s.dst_w, dh = s.dst_h;
  bool inside = true;
  if (kind == kSrcFrameLetterbox) {
    dw = s.in_w;
    dh = s.in_h;
    x -= s.in_x0;
    y -= s.in_y0;
    inside = (unsigned)x < (unsigned)dw && (unsigned)y < (unsigned)dh;
    kind = (dw == s.w && dh == s.h) ? kSrcFrameTap : kSrcFrameResize;
  }
  if (!inside) {
    r = g = b = s.pad;
  } else if (kind == kSrcFrameTap) {
    camera_tap(s, format, x, y, r, g, b);
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
    if (kRolled) {
      r = g = b = 0.0f;
#pragma unroll 1
      for (int t = 0; t < 4; ++t) {
        const float w = t == 0 ? w00 : t == 1 ? w01 : t == 2 ? w10 : w11;
        float tr, tg, tb;
        camera_tap(s, format, (t & 1) ? xb : xa, (t & 2) ? yb : ya, tr, tg, tb);
        r = r + w * tr;
        g = g + w * tg;
        b = b + w * tb;
      }
    } else {
      float r00, g00, b00, r01, g01, b01, r10, g10, b10, r11, g11, b11;
      camera_tap(s, format, xa, ya, r00, g00, b00);
      camera_tap(s, format, xb, ya, r01, g01, b01);
      camera_tap(s, format, xa, yb, r10, g10, b10);
      camera_tap(s, format, xb, yb, r11, g11, b11);
      r = cam_blend(w00, w01, w10, w11, r00, r01, r10, r11);
      g = cam_blend(w00, w01, w10, w11, g00, g01, g10, g11);
      b = cam_blend(w00, w01, w10, w11, b00, b01, b10, b11);
    }
  }
}

template <bool kRolled = false>
UNINA_CAM_FN void frame_pixel(const CameraSource& s, int kind, int x, int y, float (&rgb)[3]) {
  float r, g, b;
  frame_rgb<kRolled>(s, kind, x, y, r, g, b);
  cam_normalise(s.norm, r, g, b, rgb);
}

// Pixel (x, y) of the destination for the BGRA / NV12 kinds. `kind` is s.kind, passed apart so that a kernel built for one kind
// hands in a constant and the other branches fold; the stem hands in the kernel argument, where the branches are wave-uniform and
// only the letterbox's inside test is per pixel (lanes outside skip the taps).
UNINA_CAM_FN void camera_pixel_classic(const CameraSource& s, int kind, int x, int y, float (&rgb)[3]) {
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

// Pixel (x, y) of the destination, any kind but kSrcTensor
UNINA_CAM_FN void camera_pixel(const CameraSource& s, int kind, int x, int y, float (&rgb)[3]) {
  if (kind >= kSrcFrameTap) frame_pixel(s, kind, x, y, rgb);
  else camera_pixel_classic(s, kind, x, y, rgb);
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

// ---- packed 4:2:2 and Bayer, four pixels at a time ----
// Whether yuv422_quad may take the two pairs of a quad as one 8-byte load: the same answer for every quad whose column within the
// region is a multiple of 4 (frame pixel x0 + 4 k lies at byte 2 * x0 + 8 k of its row)
UNINA_CAM_FN bool yuv422_quad_alignment(const CameraSource& s) {
  return (s.pitch & 7) == 0 && (s.x0 & 1) == 0 && (((uintptr_t)s.plane + 2 * (unsigned)s.x0) & 7) == 0;
}

// Four consecutive kSrcFrameTap pixels of a 4:2:2 row, frame pixels (X .. X + 3, Y) with the origin already added, of which the
// first n lie inside the row (the others are not to be stored). A pair is read when
// one of its pixels is inside -- whole, as yuv422_tap reads it. X even: two pairs, each read and split once -- as one 8-byte load
// where `wide` (yuv422_quad_alignment; needs n == 4), as bytes otherwise. X odd (an odd origin): the quad straddles three pairs and
// goes pixel by pixel.
UNINA_CAM_FN void yuv422_quad(const CameraSource& s, int format, int X, int Y, int n, bool wide, float (&o)[4][3]) {
#pragma clang fp contract(off)
  const uint8_t* row = s.plane + (size_t)Y * s.pitch;
  const int yo = format == UNINA_FMT_UYVY ? 1 : 0;
  uint8_t yy[4], uu[4], vv[4];
  if ((X & 1) == 0) {
    uint8_t q[8];
    const uint8_t* p = row + (size_t)X * 2;
    if (wide) {
      memcpy(q, __builtin_assume_aligned(p, 8), 8);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) q[i] = (i / 4) * 2 < n ? p[i] : 0;          // (pair i / 4 starts at pixel 2 * (i / 4))
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint8_t* pair = q + 4 * (i / 2);
      yy[i] = pair[yo + 2 * (i & 1)];
      uu[i] = pair[1 - yo];
      vv[i] = pair[3 - yo];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint8_t* pair = row + (size_t)((X + i) / 2) * 4;
      const bool in = i < n;
      yy[i] = in ? pair[yo + 2 * ((X + i) & 1)] : 0;
      uu[i] = in ? pair[1 - yo] : 0;
      vv[i] = in ? pair[3 - yo] : 0;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float r, g, b;
    nv12_rgb((float)yy[i], uu[i] - 128.0f, vv[i] - 128.0f, r, g, b);
    cam_normalise(s.norm, r, g, b, o[i]);
  }
}

// Whether bayer_quad may take the four own bytes of each of its three rows as one dword: as above, one answer per region
UNINA_CAM_FN bool bayer_quad_alignment(const CameraSource& s) {
  return (s.pitch & 3) == 0 && (((uintptr_t)s.plane + (unsigned)s.x0) & 3) == 0;
}

// Four consecutive kSrcFrameTap pixels of a Bayer row, frame pixels (X .. X + 3, Y), the first n inside the row. Three rows
// (Y - 1, Y, Y + 1, reflected at the frame's borders) of six bytes (columns X - 1 .. X + 4, reflected likewise) serve the four
// 3 x 3 neighbourhoods, where bayer_tap reads nine bytes per pixel. `wide` (bayer_quad_alignment; needs n == 4): columns
// X .. X + 3 of a row as one dword, the two outer columns as bytes. A column is read when a pixel inside the row needs it
// (X + n <= frame_w, so it lies in the frame or one step outside, where it is reflected).
UNINA_CAM_FN void bayer_quad(const CameraSource& s, int format, int X, int Y, int n, bool wide, float (&o)[4][3]) {
#pragma clang fp contract(off)
  int rx, ry;
  bayer_red_site(format, rx, ry);
  float v[3][6];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const uint8_t* row = s.plane + (size_t)cam_reflect(Y + j - 1, s.frame_h) * s.pitch;
    if (wide) {
      const uint32_t w4 = cam_load32(row + X);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[j][1 + i] = (float)(uint8_t)(w4 >> (8 * i));
      v[j][0] = (float)row[cam_reflect(X - 1, s.frame_w)];
      v[j][5] = (float)row[cam_reflect(X + 4, s.frame_w)];
    } else {
#pragma unroll
      for (int i = 0; i < 6; ++i) v[j][i] = i <= n + 1 ? (float)row[cam_reflect(X + i - 1, s.frame_w)] : 0.0f;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float nb[3][3] = {{v[0][i], v[0][i + 1], v[0][i + 2]}, {v[1][i], v[1][i + 1], v[1][i + 2]}, {v[2][i], v[2][i + 1], v[2][i + 2]}};
    float r, g, b;
    bayer_rgb(nb, (X + i) & 1, Y & 1, rx, ry, r, g, b);
    cam_normalise(s.norm, r, g, b, o[i]);
  }
}

// ---- a unina_frame as the entry points take it (host side; engine.hip and preprocess.hip) ----
// The frame geometry each format accepts (include/unina_mi355.h at unina_pixel_format): nullptr, or what is wrong
inline const char* frame_defect(const unina_frame* f) {
  if (!f) return "null frame";
  if (f->format < UNINA_FMT_BGRA || f->format > UNINA_FMT_BAYER_GBRG) return "unknown pixel format";
  if (!f->plane[0]) return "null plane";
  const int w = f->width, h = f->height, pitch = f->pitch[0];
  if (w <= 0 || h <= 0) return "bad frame size";
  switch (f->format) {
    case UNINA_FMT_BGRA:
    case UNINA_FMT_RGBA:
      return (pitch < 4 * (long long)w || (pitch & 3) || ((uintptr_t)f->plane[0] & 3)) ? "bad frame geometry" : nullptr;
    case UNINA_FMT_NV12:
      if (!f->plane[1]) return "null chroma plane";
      return (pitch < w || f->pitch[1] < w || f->pitch[1] < 2 * ((w + 1) / 2)) ? "pitch too small for the width" : nullptr;
    case UNINA_FMT_RGB:
      return pitch < 3 * (long long)w ? "pitch too small for the width" : nullptr;
    case UNINA_FMT_YUYV:
    case UNINA_FMT_UYVY:
      return pitch < 4 * (((long long)w + 1) / 2) ? "pitch too small for the width" : nullptr;
    default:
      if (w < 2 || h < 2) return "a Bayer frame is at least 2 x 2";
      if ((long long)pitch * h > 0xffffffffLL) return "a Bayer frame is smaller than 4 GiB";   // (bayer_tap's 32-bit byte offsets)
      return pitch < w ? "pitch too small for the width" : nullptr;
  }
}

// The whole frame as a CameraSource; kind, destination and inner rectangle are the caller's to fill
inline CameraSource frame_source(const unina_frame& f, const NormParams& norm) {
  CameraSource c = {};
  c.plane = f.plane[0];
  c.w = f.width;
  c.h = f.height;
  c.pitch = f.pitch[0];
  if (f.format == UNINA_FMT_NV12) {
    c.uv = f.plane[1];
    c.uv_pitch = f.pitch[1];
  }
  c.norm = norm;
  c.format = f.format;
  c.frame_w = f.width;
  c.frame_h = f.height;
  return c;
}

// Region (x, y, w, h) of a frame (a CameraSource with origin 0): BGRA, RGB and RGBA as a pointer offset, the other formats by the
// origin, which their taps need
inline CameraSource frame_region(const CameraSource& frame, int x, int y, int w, int h) {
  CameraSource c = frame;
  c.w = w;
  c.h = h;
  const int bpp = frame.format == UNINA_FMT_RGB ? 3 : (frame.format == UNINA_FMT_BGRA || frame.format == UNINA_FMT_RGBA) ? 4 : 0;
  if (bpp) {
    c.plane = frame.plane + (size_t)y * frame.pitch + (size_t)x * bpp;
  } else {
    c.x0 = x;
    c.y0 = y;
  }
  return c;
}

// The kind of source a region of w x h is for a destination of dst_w x dst_h, stretched (lb == nullptr) or letterboxed into *lb.
// An inner rectangle that is the whole destination is the plain resize (or tap): the unboxed kinds and their fast paths.
inline int frame_kind(int format, int w, int h, int dst_w, int dst_h, const unina_letterbox* lb) {
  const int base = format == UNINA_FMT_BGRA ? kSrcBgraTap : format == UNINA_FMT_NV12 ? kSrcNv12Tap : kSrcFrameTap;
  const int boxed = format == UNINA_FMT_BGRA ? kSrcBgraLetterbox : format == UNINA_FMT_NV12 ? kSrcNv12Letterbox : kSrcFrameLetterbox;
  if (lb && !(lb->new_w == dst_w && lb->new_h == dst_h)) return boxed;
  return (w == dst_w && h == dst_h) ? base : base + 1;     // (each Resize kind follows its Tap kind)
}

// What one launch reads: `region` as `kind` (frame_kind's answer, or the kind an entry point is defined as) for a destination of
// dst_w x dst_h. The letterbox kinds get the inner rectangle *lb and the pad value; the others leave them zero.
inline CameraSource launch_source(CameraSource c, int kind, int dst_w, int dst_h, const unina_letterbox* lb, float pad) {
  c.kind = kind;
  c.dst_w = dst_w;
  c.dst_h = dst_h;
  if (kind == kSrcBgraLetterbox || kind == kSrcNv12Letterbox || kind == kSrcFrameLetterbox) {
    c.in_x0 = lb->left;
    c.in_y0 = lb->top;
    c.in_w = lb->new_w;
    c.in_h = lb->new_h;
    c.pad = pad;
  }
  return c;
}

}  // namespace unina
