// regq_s2.h -- LDS image and request order of the STRIDE-2 register-queue 3x3 tiles (conv3x3_regq, S = 2, fp16 / int8), as plain
// constexpr functions (no HIP types: a host program can include this header; tests/regq_s2_layout_host.cpp does, and
// enumerates every lane address of every fragment read of every instantiated tile).
//
// A B fragment of v_mfma_*_16x16x* is 16 pixels (lane & 15) x 4 16-byte k-chunks (lane >> 4), read by ONE ds_read_b128. The LDS
// serves that instruction in four groups of 16 lanes; a group is conflict-free when its 16 addresses fall on 16 different 16-byte
// slots of the 256-byte bank row. In lane terms every group is
//     the pixels {0-3, 12-15} with chunk c   together with   the pixels {4-11} with chunk c ^ 1,
// c = 4 * (channel block) + (lane >> 4) for one group of a lane pair and the same with the roles of c and c ^ 1 swapped for the other.
//
// At stride 2 the 16 pixels of a fragment lie TWO patch pixels apart, and with the stride-1 image (pixel r at slot r * nch,
// chunk c at slot c ^ key(r) of the pixel) that halves the slots they reach:
//   * 256-byte pixels (fp16 Cin 128): slot = c ^ (r & 15), r = r0 + 2x (+ 34 = 2 mod 16 for an 8-wide tile's next output row): the
//     16 pixels have 8 different keys, every one twice -- pixel x of the first row and pixel x - 1 of the second -- and one such
//     pair falls into each half of every group: 2-way in all four groups, 4 extra LDS cycles on the instruction's 4.
//   * 128-byte pixels (fp16 Cin 64, int8 Cin 128): bit 3 of the slot is the PARITY of r, the same for all 16 pixels: 16 lanes on 8
//     slots, 2-way at best (16-wide tiles: 4 extra cycles) and 3-way where the keys of two output rows meet (8-wide: 8 extra).
//   * 64-byte pixels (fp16 Cin 32, int8 Cin 64): bits 3:2 of the slot are r & 3, two values at stride 2: again 8 slots (4 / 8 extra).
// (The host program prints these figures next to the new image's zeros.)
//
// The stride-2 image therefore
//   (1) stores a patch row with its even columns first and its odd columns behind them (column rx at rx / 2 + (rx & 1) * half):
//       the 16 pixels of a fragment -- one tap, so one column parity -- are CONSECUTIVE image pixels, v = v0 + (lane & 15) mod 16
//       (8-wide tiles: the row pitch P = 4 mod 8 pixels puts the second output row 2 P = 8 mod 16 behind the first);
//   (2) places chunk c of image pixel v (nch chunks a pixel, 16 / nch pixels a bank row) at slot
//           (nch / 2) * (c & 1)  +  ((c >> 1) + (v >> log2(16 / nch))) mod (nch / 2)
//       of the pixel: c and c ^ 1 never share a slot, whatever the pixels, and pixels less than 8 apart never share one under
//       the same chunk -- which is all a group asks, for every v0. No xor key, no dependence on the tap.
#pragma once

#if defined(__HIPCC__)
#define UNINA_S2_HD __host__ __device__
#else
#define UNINA_S2_HD
#endif

namespace unina {
namespace s2 {

constexpr int half_w(int r0w) { return (r0w + 1) / 2; }   // image pixels the even columns of a patch row take
// image pixels per patch row: both column halves; 8-wide tiles: the next value that is 4 mod 8
constexpr int pitch(int tw, int r0w) {
  int p = 2 * half_w(r0w);
  if (tw % 16 != 0)
    while (p % 8 != 4) ++p;
  return p;
}
// image pixel of patch pixel (ry, rx)
UNINA_S2_HD constexpr int pixel(int ry, int rx, int pitch_px, int half_px) { return ry * pitch_px + (rx & 1) * half_px + (rx >> 1); }
// 16-byte slot (index into the image) of chunk c of image pixel v; nch = 4, 8 or 16 chunks a pixel
UNINA_S2_HD constexpr int slot(int v, int c, int nch) {
  const int h = nch >> 1, sh = nch == 16 ? 0 : (nch == 8 ? 1 : 2);
  return v * nch + h * (c & 1) + (((c >> 1) + (v >> sh)) & (h - 1));
}
constexpr bool nch_ok(int nch) { return nch == 4 || nch == 8 || nch == 16; }
constexpr int image_bytes(int r0h, int pitch_px, int nch) { return r0h * pitch_px * nch * 16; }

// Request order: request s of the patch is (row ry, column rx, chunk c), chunks fastest: the lanes of a wave read consecutive
// 16-byte pieces of consecutive pixels, whatever the image does with them.
constexpr int requests(int r0h, int r0w, int nch) { return r0h * r0w * nch; }
constexpr int loads(int r0h, int r0w, int nch, int nthreads) { return (requests(r0h, r0w, nch) + nthreads - 1) / nthreads; }   // per wave
struct Request {
  int ry, rx, chunk;
};
UNINA_S2_HD constexpr Request request(int s, int r0w, int nch) {
  const int ry = s / (r0w * nch), rem = s - ry * (r0w * nch), rx = rem / nch;
  return Request{ry, rx, rem - rx * nch};
}

}  // namespace s2
}  // namespace unina
