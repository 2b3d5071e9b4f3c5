// colour_math.h -- the window, the silhouette, the pixel fetch, the pixel's class and hue, the row letters with the stripe count
// and the decision of unina_colour_async (include/unina_mi355.h "class from pixels"), as __host__ __device__ functions
// (csrc/hd.h): csrc/colour.hip calls them on the device, tests/colour_math_host.cpp on the host, colour.colour_numpy is their
// numpy twin. The window's floats are fp32, one rounding per operation: every translation unit that includes this header is
// compiled with -ffp-contract=off. Everything behind the window is integer arithmetic.
#ifndef UNINA_COLOUR_MATH_H
#define UNINA_COLOUR_MATH_H

#include <stdint.h>

#if !defined(__HIPCC__) && !defined(UNINA_NO_HIP_HEADERS)
#define UNINA_NO_HIP_HEADERS   // a host compiler: the public header without HIP's
#endif
#include "../../include/unina_mi355.h"
#include "locate_window.h"

namespace unina {

constexpr int kColourBins = 6;        // per row: yellow, blue, orange, white, black, mask
constexpr int kColourWhite = 3, kColourBlack = 4, kColourMask = 5;
constexpr int kColourOther = -1;      // a pixel in the silhouette that counts for the mask only
constexpr int kColourMaxDim = 16384;  // width / height limit of the image

struct ColourWindow {
  LocateWindow w;   // w.empty: the record has no window
  int size;         // 1: the SIZE window, from the cone's pixel and depth
};

// The BOX window of the record, or else the SIZE window of its cone (has_cone: d_cones != NULL), or else none.
UNINA_HD ColourWindow colour_window(float x1, float y1, float x2, float y2, int has_cone, int cone_valid, float u, float v, float z,
                                    float fx, float fy, const unina_colour_params& p, int width, int height) {
  ColourWindow o;
  o.size = 0;
  const float X1 = x1 * p.sx, X2 = x2 * p.sx, Y1 = y1 * p.sy, Y2 = y2 * p.sy;
  if (finite(X1) && finite(X2) && finite(Y1) && finite(Y2) && X2 > X1 && Y2 > Y1) {
    o.w = locate_window(x1, y1, x2, y2, p.sx, p.sy, p.shrink, width, height, p.max_side);
    return o;
  }
  if (has_cone && cone_valid != 0 && finite(u) && finite(v) && finite(z) && z > 0.0f) {
    const float hw = (fx * p.half_width) / z, up = (fy * p.above) / z, down = (fy * p.below) / z;
    o.w = locate_window(u - hw, v - up, u + hw, v + down, 1.0f, 1.0f, p.shrink, width, height, p.max_side);
    o.size = o.w.empty ? 0 : 1;
    return o;
  }
  memset(&o.w, 0, sizeof(o.w));
  o.w.empty = 1;
  return o;
}

// sample (c, k) of a cols x rows grid lies in the trapezoid whose top is taper / 256 of its base
UNINA_HD bool colour_inside(int c, int k, int cols, int rows, int taper) {
  int off = 2 * c - (cols - 1);
  off = off < 0 ? -off : off;
  return off * 256 * rows <= cols * (taper * rows + (256 - taper) * (k + 1));
}

// bytes 0..2 of a pixel as b0 | b1 << 8 | b2 << 16. A 4-channel pixel is one dword load where its address allows; a 3-channel
// pixel is three byte loads: no byte behind the pixel's last one is read.
UNINA_HD uint32_t colour_fetch(const uint8_t* px, int channels) {
  if (channels == 4 && (reinterpret_cast<uintptr_t>(px) & 3) == 0) return *reinterpret_cast<const uint32_t*>(px) & 0x00ffffffu;
  return (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
}

UNINA_HD bool colour_in_range(int h, int lo, int hi) { return lo <= hi ? (h >= lo && h <= hi) : (h >= lo || h <= hi); }

// hue of a pixel with d = max - min > 0: 0..1535, 256 per sextant
UNINA_HD int colour_hue(int R, int G, int B) {
  const int mx = R > G ? (R > B ? R : B) : (G > B ? G : B), mn = R < G ? (R < B ? R : B) : (G < B ? G : B), d = mx - mn;
  if (mx == R) return G >= B ? 256 * (G - B) / d : (1536 - 256 * (B - G) / d) % 1536;
  if (mx == G) return B >= R ? 512 + 256 * (B - R) / d : 512 - 256 * (R - B) / d;
  return R >= G ? 1024 + 256 * (R - G) / d : 1024 - 256 * (G - R) / d;
}

// the bin of a fetched pixel: 0..2 a colour, kColourWhite, kColourBlack, or kColourOther
UNINA_HD int colour_pixel(uint32_t px, const unina_colour_params& p) {
  const int b0 = (int)(px & 255u), G = (int)((px >> 8) & 255u), b2 = (int)((px >> 16) & 255u);
  const int R = p.order == UNINA_COLOUR_BGR ? b2 : b0, B = p.order == UNINA_COLOUR_BGR ? b0 : b2;
  const int mx = R > G ? (R > B ? R : B) : (G > B ? G : B), mn = R < G ? (R < B ? R : B) : (G < B ? G : B), d = mx - mn;
  if (mx <= p.black_max) return kColourBlack;
  if (d * 256 >= p.sat_min * mx && mx >= p.val_min) {
    const int h = colour_hue(R, G, B);
    for (int c = 0; c < 3; ++c)
      if (colour_in_range(h, p.hue_lo[c], p.hue_hi[c])) return c;
    return kColourOther;
  }
  return mx >= p.white_min ? kColourWhite : kColourOther;
}

// best = the colour with the most votes, second = the one with the most of the other two; ties go to the earlier colour
UNINA_HD void colour_rank(const int votes[3], int* best, int* second) {
  int b = 0;
  if (votes[1] > votes[b]) b = 1;
  if (votes[2] > votes[b]) b = 2;
  const int x = b == 0 ? 1 : 0, y = b == 2 ? 1 : 2;   // the other two, x < y
  *best = b;
  *second = votes[y] > votes[x] ? y : x;
}

// v[i] of a three-element array without an indexed access (a register array stays in registers)
UNINA_HD int colour_pick(const int v[3], int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : v[2]); }

// the letter of a row from its counts -- mask_k, votes_k[best], and black_k where best is yellow, else white_k:
// 1 = B (body), 2 = S (stripe), 0 = dropped
UNINA_HD int colour_row_letter(int mask, int body, int stripe) {
  if (mask <= 0) return 0;
  if (2 * body >= mask) return 1;
  return 2 * stripe >= mask ? 2 : 0;
}

// body / stripe: bit k set = row k is B / S. Row k starts a counted run iff it is S, the nearest remaining row above it (lower k)
// is a B, and a B lies somewhere below it: every maximal run of S with a B before and a B after it has exactly one such row.
UNINA_HD bool colour_run_start(uint64_t body, uint64_t stripe, int k) {
  const uint64_t bit = 1ull << k, below = bit - 1ull;
  if (!(stripe & bit)) return false;
  const uint64_t before = (body | stripe) & below;
  if (!before) return false;
  uint64_t top = before;                       // the highest set bit of `before`
  top |= top >> 1; top |= top >> 2; top |= top >> 4; top |= top >> 8; top |= top >> 16; top |= top >> 32;
  top ^= top >> 1;
  return (body & top) != 0 && (body & ~(below | bit)) != 0;
}

UNINA_HD int colour_stripes(uint64_t body, uint64_t stripe) {
  int n = 0;
  for (int k = 0; k < 64; ++k) n += colour_run_start(body, stripe, k) ? 1 : 0;
  return n;
}

struct ColourDecision {
  int decided, large, index;   // index: the colour index, 0..3
  int class_id;                // where decided
};

UNINA_HD ColourDecision colour_decide(const int votes[3], int best, int second, int n_mask, int n_stripes, const unina_colour_params& p) {
  ColourDecision o;
  o.large = (best == UNINA_COLOUR_ORANGE && n_stripes >= 2 && p.class_of[UNINA_COLOUR_LARGE_ORANGE] >= 0) ? 1 : 0;
  o.index = o.large ? UNINA_COLOUR_LARGE_ORANGE : best;
  o.class_id = p.class_of[o.index];
  const int vb = colour_pick(votes, best), vs = colour_pick(votes, second);
  o.decided = (n_mask >= p.min_pixels && vb * 256 >= p.min_share * n_mask && vs * 256 <= p.max_rival * vb && vb > 0 && (p.require_stripe == 0 || n_stripes >= 1) && o.class_id >= 0)
                  ? 1
                  : 0;
  if (!o.decided) o.large = 0;
  return o;
}

UNINA_HD int colour_status(int size_window, int best, const ColourDecision& d) {
  return UNINA_COLOUR_WINDOW | UNINA_COLOUR_SELECTED | (d.decided ? UNINA_COLOUR_DECIDED : 0) | (d.large ? UNINA_COLOUR_LARGE : 0) |
         (size_window ? UNINA_COLOUR_SIZE_WINDOW : 0) | (best << 8);
}

}  // namespace unina
#endif  // UNINA_COLOUR_MATH_H
