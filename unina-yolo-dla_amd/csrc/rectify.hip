// Raw camera images rectified on the device: lens undistortion and the stereo rotation in one remap, 1 to 4 images per launch
// (include/unina_mi355.h "Rectification"; rectify.rectify_numpy is the definition, byte for byte). The position of every output
// pixel in the raw image, the inside test, the 1/32-pixel split and the four-tap integer blend are csrc/rectify_map.h, the same
// functions the host program of the tests runs; this file only decides which thread computes which pixel and how bytes travel.
//
// Work split. One workgroup of 4 waves per output tile of 4 rows, a wave per row: the taps of one output row lie along a gently
// curved line of the raw image, so a wave reads a few source rows densely, and the four rows of a tile (and the tiles beside and
// below it) share those source rows through the vector cache and L2. A tile of a 1-channel image is 256 pixels wide, each lane
// computing 4 adjacent pixels and storing them as ONE dword where its address is a multiple of 4 and all four lie in the row,
// else byte by byte; a tile of a 3- or 4-channel image is 64 pixels wide, a pixel per lane, and a 4-channel pixel -- tap or result
// -- travels as one dword where its address is a multiple of 4. Neither pointer nor pitch needs an alignment: the test is on the
// address. The jobs are in the kernel arguments by value, each with the index of its first workgroup; a workgroup finds its job
// by comparing its index with at most three of those. Taps are plain global loads (direct gathers: staging a tile's source
// footprint in LDS is not done here); a tap outside the raw image is the border value and no address is formed for it. No
// atomics, no LDS, no scratch; every output byte is written by exactly one thread, so two runs give the same bytes.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/unina_mi355.h"
#include "rectify_map.h"

namespace unina {
namespace {

constexpr int kRcWave = 64;
constexpr int kRcRows = 4;                          // rows of a tile: one per wave
constexpr int kRcBlock = kRcRows * kRcWave;
constexpr int kRcGroup = 4;                         // adjacent pixels per lane of a 1-channel image: one dword
constexpr int kRcTileW1 = kRcWave * kRcGroup;       // 256
constexpr int kRcTileWN = kRcWave;                  // 64

static_assert(kRectifyMaxImages == UNINA_RECTIFY_MAX_IMAGES && kRectifyMaxDim == UNINA_RECTIFY_MAX_DIM, "header limits");
static_assert(sizeof(RectifyCam) == sizeof(unina_rectify_cam) && sizeof(unina_rectify_cam) == 88, "the calibration is 22 floats");
static_assert(sizeof(unina_image) == 24 && sizeof(unina_rectify_job) == 144, "job layout");

struct RectifyJob {
  RectifyCam cam;
  const uint8_t* src;
  uint8_t* dst;
  int src_w, src_h, src_pitch;
  int dst_w, dst_h, dst_pitch;
  int channels, border;
  int tiles_x, first_block;
};
struct RectifyArgs {
  RectifyJob job[kRectifyMaxImages];
  int n_jobs;
};

// one tap of C bytes; outside the raw image it is the border and no address is formed
template <int C>
__device__ __forceinline__ void load_tap(const RectifyJob& j, int x, int y, int (&t)[C]) {
  if (x < 0 || y < 0 || x >= j.src_w || y >= j.src_h) {
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = j.border;
    return;
  }
  const uint8_t* p = j.src + ((size_t)y * (size_t)j.src_pitch + (size_t)x * C);
  if (C == 4 && ((uintptr_t)p & 3) == 0) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = (int)((w >> (8 * c)) & 255u);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = p[c];
  }
}

// output pixel (u, v), u < dst_w, v < dst_h -> its C bytes, each in 0..255
template <int C>
__device__ __forceinline__ void sample(const RectifyJob& j, int u, int v, int (&out)[C]) {
  const RectifySource s = rectify_source(j.cam, u, v);
  if (!rectify_inside(s, j.src_w, j.src_h)) {
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = j.border;
    return;
  }
  int x0, y0;
  const int ax = rectify_split(s.tx, &x0), ay = rectify_split(s.ty, &y0);
  int t00[C], t10[C], t01[C], t11[C];
  load_tap<C>(j, x0, y0, t00);
  load_tap<C>(j, x0 + 1, y0, t10);
  load_tap<C>(j, x0, y0 + 1, t01);
  load_tap<C>(j, x0 + 1, y0 + 1, t11);
#pragma unroll
  for (int c = 0; c < C; ++c) out[c] = rectify_blend(ax, ay, t00[c], t10[c], t01[c], t11[c]);
}

// a lane's four pixels of a 1-channel row
__device__ __forceinline__ void rectify_group(const RectifyJob& j, int u0, int v) {
  if (u0 >= j.dst_w) return;
  uint8_t* p = j.dst + ((size_t)v * (size_t)j.dst_pitch + (size_t)u0);
  const int n = j.dst_w - u0 < kRcGroup ? j.dst_w - u0 : kRcGroup;
  int px[kRcGroup];
#pragma unroll
  for (int i = 0; i < kRcGroup; ++i) {
    int one[1] = {0};
    if (i < n) sample<1>(j, u0 + i, v, one);
    px[i] = one[0];
  }
  if (n == kRcGroup && ((uintptr_t)p & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | ((uint32_t)px[3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < kRcGroup; ++i)
      if (i < n) p[i] = (uint8_t)px[i];
  }
}

// a lane's one pixel of a 3- or 4-channel row
template <int C>
__device__ __forceinline__ void rectify_one(const RectifyJob& j, int u, int v) {
  if (u >= j.dst_w) return;
  int px[C];
  sample<C>(j, u, v, px);
  uint8_t* p = j.dst + ((size_t)v * (size_t)j.dst_pitch + (size_t)u * C);
  if (C == 4 && ((uintptr_t)p & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | ((uint32_t)px[3] << 24);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = (uint8_t)px[c];
  }
}

__global__ void __launch_bounds__(kRcBlock) rectify_kernel(const RectifyArgs a) {
  const int block = (int)blockIdx.x;
  int k = 0;
#pragma unroll
  for (int i = 1; i < kRectifyMaxImages; ++i)
    if (i < a.n_jobs && block >= a.job[i].first_block) k = i;   // first_block ascends
  const RectifyJob& j = a.job[k];
  const int local = block - j.first_block;
  const int tile_y = local / j.tiles_x, tile_x = local - tile_y * j.tiles_x;
  const int lane = (int)threadIdx.x & (kRcWave - 1), wave = (int)threadIdx.x / kRcWave;
  const int v = tile_y * kRcRows + wave;
  if (v >= j.dst_h) return;
  const int col = tile_x * kRcWave + lane;
  if (j.channels == 1) {
    rectify_group(j, col * kRcGroup, v);
  } else if (j.channels == 4) {
    rectify_one<4>(j, col, v);
  } else {
    rectify_one<3>(j, col, v);
  }
}

bool image_ok(const unina_image& im) {
  if (!im.data) return false;
  if (im.width < 1 || im.width > kRectifyMaxDim || im.height < 1 || im.height > kRectifyMaxDim) return false;
  if (im.channels != 1 && im.channels != 3 && im.channels != 4) return false;
  return im.pitch >= im.width * im.channels;   // <= 65 536: no overflow
}

bool cam_ok(const unina_rectify_cam& c) {
  const float dist[5] = {c.k1, c.k2, c.p1, c.p2, c.k3};
  for (float v : dist)
    if (!finite(v)) return false;
  for (float v : c.r)
    if (!finite(v)) return false;
  for (const unina_pinhole* p : {&c.src, &c.dst})
    if (!finite_pos(p->fx) || !finite_pos(p->fy) || !finite(p->cx) || !finite(p->cy)) return false;
  return true;
}

}  // namespace
}  // namespace unina

extern "C" int unina_rectify_async(const unina_rectify_job* jobs, int n_jobs, hipStream_t stream) {
  using namespace unina;
  if (!jobs || n_jobs < 1 || n_jobs > kRectifyMaxImages) return UNINA_ERR_ARG;
  RectifyArgs a;
  memset(&a, 0, sizeof a);
  a.n_jobs = n_jobs;
  int blocks = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const unina_rectify_job& in = jobs[i];
    if (!image_ok(in.src) || !image_ok(in.dst) || in.src.channels != in.dst.channels || in.src.data == in.dst.data) return UNINA_ERR_ARG;
    if (in.border < 0 || in.border > 255 || !cam_ok(in.cam)) return UNINA_ERR_ARG;
    RectifyJob& j = a.job[i];
    j.cam.src = {in.cam.src.fx, in.cam.src.fy, in.cam.src.cx, in.cam.src.cy};
    j.cam.k1 = in.cam.k1; j.cam.k2 = in.cam.k2; j.cam.p1 = in.cam.p1; j.cam.p2 = in.cam.p2; j.cam.k3 = in.cam.k3;
    for (int e = 0; e < 9; ++e) j.cam.r[e] = in.cam.r[e];
    j.cam.dst = {in.cam.dst.fx, in.cam.dst.fy, in.cam.dst.cx, in.cam.dst.cy};
    j.src = in.src.data;
    j.dst = const_cast<uint8_t*>(in.dst.data);
    j.src_w = in.src.width; j.src_h = in.src.height; j.src_pitch = in.src.pitch;
    j.dst_w = in.dst.width; j.dst_h = in.dst.height; j.dst_pitch = in.dst.pitch;
    j.channels = in.dst.channels;
    j.border = in.border;
    const int tile_w = j.channels == 1 ? kRcTileW1 : kRcTileWN;
    j.tiles_x = (j.dst_w + tile_w - 1) / tile_w;
    j.first_block = blocks;
    blocks += j.tiles_x * ((j.dst_h + kRcRows - 1) / kRcRows);   // <= 4 * 256 * 4096
  }
  hipLaunchKernelGGL(rectify_kernel, dim3((unsigned)blocks), dim3(kRcBlock), 0, stream, a);
  return hipGetLastError() == hipSuccess ? UNINA_OK : UNINA_ERR_HIP;
}
