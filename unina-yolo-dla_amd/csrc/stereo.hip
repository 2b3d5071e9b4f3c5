// Detections lifted to 3-D cone positions from a rectified stereo pair on the device: one launch per frame behind the call that
// produced the records (include/unina_mi355.h "3-D localisation from a stereo pair"; localize.locate_stereo_numpy is the
// definition, bit for bit).
//
// Per kept record: the box's central window on the LEFT plane (csrc/locate_window.h, the locator's own), its sampling grid of at
// most 64 x 64 pixels, and one sum of absolute differences per integer disparity d_lo .. d_hi against the same rows of the RIGHT
// plane. The best and the second-best cost, the acceptance test, the sub-pixel step and the point are csrc/stereo_match.h. Costs
// are integers and every minimum is taken on packed integers (cost << 10 | d - d_lo), so no result depends on the order in which
// lanes arrive: two runs give the same bytes, and they are numpy's.
//
// Work split. One workgroup of 4 waves per record slot; the grid covers all MAX_DETECTIONS slots, so the slots at and beyond the
// count are zeroed by the same launch (one 48-byte store and the workgroup is gone). The work of a record is n_samples x nd and
// it is the DISPARITIES that are spread over the lanes, not the samples: lane t owns d_lo + t, d_lo + t + 256, ... (at most four)
// and walks all samples, so its costs stay in registers, nothing is reduced across lanes but the two minima at the end, and
// a distant cone (a few dozen samples, a few hundred disparities) fills the workgroup as well as the worst case (4096 x 1024)
// does. A frame of 60 records therefore occupies 60 CUs for the time of one record; sharing a workgroup between four small
// records (as csrc/locate.hip does, where the samples are the parallel axis and a small window cannot fill a workgroup) would
// put the same frame on 15 CUs, each four times as long.
//
// LDS. The template's sampled bytes (4 KB, a grid row per 64 bytes), the costs (4 KB) and the strip of the right plane: the sampled
// rows x the columns u0 - d_hi .. (last sampled column) - d_lo, i.e. (cols - 1) * stride_x + nd bytes per row. Consecutive lanes
// read consecutive descending bytes of one strip row -- four lanes per dword, which the LDS broadcasts, and 16 distinct banks per
// wave access -- and every lane reads the same template word, so neither read conflicts. kStripBytes = 64 x (63 + 1024) rounded
// up holds the strip of EVERY window with stride_x == 1 (a box up to 64 px wide after the shrink); the whole allocation is 76 KB,
// so two workgroups share a CU's 160 KB. The strip of a wider, column-strided window can pass 100 KB: such a window (a cone
// filling the frame) reads the right plane through L2 instead, with the same indexing -- it is rare, and sizing the allocation
// for it would halve the occupancy of every other record.
//
// Inner loop. Where the strip is on chip and stride_x == 1 (every cone-sized box), four samples go through one v_sad_u8: one
// aligned dword of the template, two aligned dwords of the strip joined by v_alignbyte_b32 at the lane's byte offset, the second
// of them kept for the next group -- two LDS reads and two VALU instructions per four samples and disparity. Column-strided
// windows, on chip or through L2, walk the samples a byte at a time.
// Image bytes are loaded from memory as bytes: neither plane nor the pitch has an alignment.
#include <hip/hip_runtime.h>

#include <atomic>

#include "locate_checks.h"
#include "stereo_match.h"
#include "wave_block.h"

namespace unina {
namespace {

constexpr int kStWaves = 4;
constexpr int kStBlock = kStWaves * kWave;
constexpr int kOwned = kStereoMaxDisparities / kStBlock;   // disparities a lane can own
constexpr int kTemplateBytes = kStereoMaxSide * kStereoMaxSide;
constexpr int kStripBytes = 68 * 1024;
constexpr int kStripPad = 16;                              // the packed path reads whole dwords: up to 7 bytes past the strip's last
constexpr int kStereoLds = kStripBytes + kStripPad + kTemplateBytes + kStereoMaxDisparities * 4 + kStWaves * 4;

static_assert(kStereoMaxDisparities == UNINA_STEREO_MAX_DISPARITIES && kStereoMaxSide == UNINA_STEREO_MAX_SIDE, "header limits");
static_assert(kOwned * kStBlock == kStereoMaxDisparities, "every disparity has an owner");
static_assert(kStereoMaxSide * (kStereoMaxSide - 1 + kStereoMaxDisparities) <= kStripBytes, "every unstrided strip stays on chip");
static_assert(2 * kStereoLds <= 160 * 1024, "two workgroups per CU");
static_assert(sizeof(unina_cone3d) == 32 && sizeof(GpuDetection) == 32 && sizeof(unina_stereo_match) == 16, "record layouts");

struct StereoArgs {
  const unsigned char *left, *right;
  int width, height, pitch;
  float fx, fy, cx, cy, fxB;
  int d_lo, d_hi_all;
  float sx, sy, shrink;
  int max_side, max_mean_sad, uniqueness;
};

// d_match may be NULL
__device__ __forceinline__ void store_records(unina_cone3d* __restrict__ out, unina_stereo_match* __restrict__ match, int slot,
                                              const RecordWords<unina_cone3d>& c, const RecordWords<unina_stereo_match>& m) {
  store_record(out + slot, c);
  if (match) store_record(match + slot, m);
}

__device__ __forceinline__ void store_zero(unina_cone3d* __restrict__ out, unina_stereo_match* __restrict__ match, int slot) {
  store_zero_record(out + slot);
  if (match) store_zero_record(match + slot);
}

// minimum over the workgroup; every thread calls it. The leading barrier also publishes what was written to LDS before the call.
__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t* s_red, int lane, int wave) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)v, o, kWave);
    v = other < v ? other : v;
  }
  __syncthreads();   // s_red is free again
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  uint32_t m = s_red[0];
#pragma unroll
  for (int i = 1; i < kStWaves; ++i) m = s_red[i] < m ? s_red[i] : m;
  return m;
}

// acc[j] = cost of the disparity whose strip offset is base[j] (j < NJ), over all samples. `rows_base` + r * row_pitch is the byte
// of sampled row r at the strip's first column; LDS for the strip, global for the plane (the address space follows the template
// argument after inlining).
template <int NJ, typename RowPtr>
__device__ __forceinline__ void accumulate(const unsigned char* __restrict__ s_tmpl, RowPtr rows_base, size_t row_pitch, int rows, int cols,
                                           int stride_x, const int (&base)[kOwned], uint32_t (&acc)[kOwned]) {
  for (int r = 0; r < rows; ++r) {
    const unsigned char* t = s_tmpl + r * kStereoMaxSide;
    RowPtr row = rows_base + (size_t)r * row_pitch;
#pragma unroll 4
    for (int c = 0; c < cols; ++c) {
      const int tv = t[c];
      RowPtr p = row + c * stride_x;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int d = tv - (int)p[base[j]];
        acc[j] += (uint32_t)(d < 0 ? -d : d);
      }
    }
  }
}

// The same sums for a strip in LDS with stride_x == 1, four samples per instruction: the template's row is read a dword at a time
// (its rows start on dwords), a lane's four strip bytes come out of two aligned dwords (the second one is the next group's first)
// through a byte alignment, and one packed sum of absolute differences adds the four. The bytes of the last group that lie
// beyond the row are masked to zero on both sides.
template <int NJ>
__device__ __forceinline__ void accumulate_packed(const unsigned char* __restrict__ s_tmpl, const unsigned char* s_strip, int strip_w, int rows,
                                                  int cols, const int (&base)[kOwned], uint32_t (&acc)[kOwned]) {
  const uint32_t* strip4 = reinterpret_cast<const uint32_t*>(s_strip);   // 16-byte aligned
  const int groups = cols >> 2, tail = cols & 3;
  const uint32_t tail_mask = (1u << (8 * tail)) - 1u;
  for (int r = 0; r < rows; ++r) {
    const uint32_t* t4 = reinterpret_cast<const uint32_t*>(s_tmpl + r * kStereoMaxSide);
    int word[NJ];
    uint32_t shift[NJ], lo[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int b = r * strip_w + base[j];
      word[j] = b >> 2;
      shift[j] = (uint32_t)(b & 3);
      lo[j] = strip4[word[j]];
    }
#pragma unroll 4
    for (int g = 0; g < groups; ++g) {
      const uint32_t t = t4[g];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const uint32_t hi = strip4[word[j] + g + 1];
        acc[j] = __builtin_amdgcn_sad_u8(t, __builtin_amdgcn_alignbyte(hi, lo[j], shift[j]), acc[j]);
        lo[j] = hi;
      }
    }
    if (tail) {
      const uint32_t t = t4[groups] & tail_mask;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const uint32_t hi = strip4[word[j] + groups + 1];
        acc[j] = __builtin_amdgcn_sad_u8(t, __builtin_amdgcn_alignbyte(hi, lo[j], shift[j]) & tail_mask, acc[j]);
      }
    }
  }
}

template <typename RowPtr>
__device__ __forceinline__ void accumulate_n(int nj, const unsigned char* __restrict__ s_tmpl, RowPtr rows_base, size_t row_pitch, int rows,
                                             int cols, int stride_x, const int (&base)[kOwned], uint32_t (&acc)[kOwned]) {
  switch (nj) {   // workgroup-uniform
    case 1: accumulate<1>(s_tmpl, rows_base, row_pitch, rows, cols, stride_x, base, acc); break;
    case 2: accumulate<2>(s_tmpl, rows_base, row_pitch, rows, cols, stride_x, base, acc); break;
    case 3: accumulate<3>(s_tmpl, rows_base, row_pitch, rows, cols, stride_x, base, acc); break;
    default: accumulate<4>(s_tmpl, rows_base, row_pitch, rows, cols, stride_x, base, acc); break;
  }
}
__device__ __forceinline__ void accumulate_packed_n(int nj, const unsigned char* __restrict__ s_tmpl, const unsigned char* s_strip, int strip_w,
                                                    int rows, int cols, const int (&base)[kOwned], uint32_t (&acc)[kOwned]) {
  switch (nj) {   // workgroup-uniform
    case 1: accumulate_packed<1>(s_tmpl, s_strip, strip_w, rows, cols, base, acc); break;
    case 2: accumulate_packed<2>(s_tmpl, s_strip, strip_w, rows, cols, base, acc); break;
    case 3: accumulate_packed<3>(s_tmpl, s_strip, strip_w, rows, cols, base, acc); break;
    default: accumulate_packed<4>(s_tmpl, s_strip, strip_w, rows, cols, base, acc); break;
  }
}
static_assert(kOwned == 4, "accumulate_n's and accumulate_packed_n's cases");

__global__ void __launch_bounds__(kStBlock) stereo_kernel(const GpuDetection* __restrict__ dets, const int* __restrict__ d_count,
                                                          StereoArgs a, unina_cone3d* __restrict__ out,
                                                          unina_stereo_match* __restrict__ match) {
  extern __shared__ __align__(16) unsigned char stereo_smem[];
  unsigned char* s_strip = stereo_smem;
  unsigned char* s_tmpl = stereo_smem + kStripBytes + kStripPad;   // row r of the grid at r * kStereoMaxSide: rows start on dwords
  uint32_t* s_cost = reinterpret_cast<uint32_t*>(s_tmpl + kTemplateBytes);
  uint32_t* s_red = s_cost + kStereoMaxDisparities;

  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int slot = (int)blockIdx.x;   // < MAX_DETECTIONS: the grid's size
  const int n = record_count(d_count);

  // ---- everything up to the first barrier is the same in every thread: each return is the whole workgroup's
  if (slot >= n) {
    if (tid == 0) store_zero(out, match, slot);
    return;
  }
  const float4 b = *reinterpret_cast<const float4*>(dets + slot);   // x1, y1, x2, y2
  const LocateWindow w = locate_window(b.x, b.y, b.z, b.w, a.sx, a.sy, a.shrink, a.width, a.height, a.max_side);
  if (w.empty) {
    if (tid == 0) store_zero(out, match, slot);
    return;
  }
  RecordWords<unina_cone3d> rec;
  RecordWords<unina_stereo_match> mw;
  rec.r.x = rec.r.y = rec.r.z = 0.0f;
  rec.r.u = w.uc;
  rec.r.v = w.vc;
  rec.r.n_samples = w.n_samples;
  rec.r.valid = 0;
  int d_hi;
  const int nd = stereo_nd(a.d_lo, a.d_hi_all, w.u0, &d_hi);   // <= kStereoMaxDisparities: the entry point refuses a longer range
  rec.r.n_valid = nd;
  if (nd == 0) {
    mw.r.disparity = 0.0f;
    mw.r.d_best = 0;
    mw.r.cost_best = mw.r.cost_second = kStereoNone;
    if (tid == 0) store_records(out, match, slot, rec, mw);
    return;
  }

  // ---- the template and the strip
  for (int s = tid; s < w.n_samples; s += kStBlock) {
    const int r = s / w.cols, c = s - r * w.cols;
    s_tmpl[r * kStereoMaxSide + c] = a.left[(size_t)(w.v0 + r * w.stride_y) * (size_t)a.pitch + (size_t)(w.u0 + c * w.stride_x)];
  }
  const int x0 = w.u0 - d_hi;                                  // >= 0: d_hi <= u0
  const int strip_w = (w.cols - 1) * w.stride_x + nd;          // columns x0 .. last sampled column - d_lo, all < width
  const bool on_chip = (long long)strip_w * w.rows <= (long long)kStripBytes;
  const unsigned char* right0 = a.right + (size_t)w.v0 * (size_t)a.pitch + (size_t)x0;
  const size_t right_pitch = (size_t)w.stride_y * (size_t)a.pitch;
  if (on_chip) {
    // a wave per row, a lane per byte; four loads are in flight before the first is stored
    for (int r = wave; r < w.rows; r += kStWaves) {
      const unsigned char* src = right0 + (size_t)r * right_pitch;
      unsigned char* dst = s_strip + r * strip_w;
      for (int x = lane; x < strip_w; x += 4 * kWave) {
        unsigned char v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = x + i * kWave < strip_w ? src[x + i * kWave] : (unsigned char)0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (x + i * kWave < strip_w) dst[x + i * kWave] = v[i];
      }
    }
  }
  __syncthreads();

  // ---- the costs: the sample at grid column c and the disparity of index k = d - d_lo meet at strip column
  //      (u0 + c * stride_x - d) - x0 = c * stride_x + (nd - 1 - k)
  int base[kOwned];
  uint32_t acc[kOwned];
#pragma unroll
  for (int j = 0; j < kOwned; ++j) {
    const int k = tid + j * kStBlock;
    base[j] = k < nd ? nd - 1 - k : 0;   // a lane without a disparity reads a valid column and drops the sum
    acc[j] = 0u;
  }
  const int nj = (nd + kStBlock - 1) / kStBlock;
  if (on_chip && w.stride_x == 1) {
    accumulate_packed_n(nj, s_tmpl, s_strip, strip_w, w.rows, w.cols, base, acc);
  } else if (on_chip) {
    accumulate_n<const unsigned char*>(nj, s_tmpl, s_strip, (size_t)strip_w, w.rows, w.cols, w.stride_x, base, acc);
  } else {
    accumulate_n<const unsigned char*>(nj, s_tmpl, right0, right_pitch, w.rows, w.cols, w.stride_x, base, acc);
  }

  // ---- the best (cost, d), then the best cost at least two disparities away from it
  uint32_t key = kStereoNone;
#pragma unroll
  for (int j = 0; j < kOwned; ++j) {
    const int k = tid + j * kStBlock;
    if (k < nd) {
      s_cost[k] = acc[j];
      const uint32_t kj = stereo_key(acc[j], k);
      key = kj < key ? kj : key;
    }
  }
  const uint32_t best = block_min(key, s_red, lane, wave);
  const int k_best = stereo_key_index(best);
  uint32_t second = kStereoNone;
#pragma unroll
  for (int j = 0; j < kOwned; ++j) {
    const int k = tid + j * kStBlock;
    if (k < nd && (k > k_best + 1 || k < k_best - 1)) second = acc[j] < second ? acc[j] : second;
  }
  second = block_min(second, s_red, lane, wave);
  if (tid != 0) return;

  const uint32_t cost_best = stereo_key_cost(best);
  const int d_best = a.d_lo + k_best;
  mw.r.d_best = d_best;
  mw.r.cost_best = cost_best;
  mw.r.cost_second = second;
  mw.r.disparity = 0.0f;
  if (stereo_accept(nd, cost_best, second, w.n_samples, a.max_mean_sad, a.uniqueness)) {
    const bool inner = k_best > 0 && k_best < nd - 1;
    const float disparity = stereo_disparity(d_best, a.d_lo, d_hi, inner ? s_cost[k_best - 1] : 0u, cost_best, inner ? s_cost[k_best + 1] : 0u);
    float xyz[3];
    stereo_point(a.fxB, disparity, w.uc, w.vc, a.fx, a.fy, a.cx, a.cy, xyz);
    rec.r.x = xyz[0];
    rec.r.y = xyz[1];
    rec.r.z = xyz[2];
    rec.r.valid = 1;
    mw.r.disparity = disparity;
  }
  store_records(out, match, slot, rec, mw);
}

// The kernel asks for more dynamic LDS than a launch gets by default: the limit is raised once per device (hipFuncSetAttribute
// applies to the current one).
constexpr int kMaxDevices = 64;
std::atomic<int> g_ready[kMaxDevices];
hipError_t stereo_prepare() {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
  if (g_ready[dev].load(std::memory_order_acquire)) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(stereo_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kStereoLds);
  if (e == hipSuccess) g_ready[dev].store(1, std::memory_order_release);
  return e;
}

}  // namespace
}  // namespace unina

extern "C" int unina_locate_stereo_async(const GpuDetection* d_dets, const int* d_count, const unina_stereo_pair* pair,
                                         const unina_pinhole* cam, float baseline, const unina_stereo_params* p, unina_cone3d* d_out,
                                         unina_stereo_match* d_match, hipStream_t stream) {
  using namespace unina;
  if (!record_io_ok(d_dets, d_count, d_out) || !pair || !p || !pair->left || !pair->right) return UNINA_ERR_ARG;
  if (!plane_dims_ok(pair->width, pair->height) || !pinhole_ok(cam)) return UNINA_ERR_ARG;
  if (!window_params_ok(p->sx, p->sy, p->shrink, p->min_depth, p->max_depth)) return UNINA_ERR_ARG;
  if (((uintptr_t)d_match & 15) || pair->pitch < pair->width || !finite_pos(baseline)) return UNINA_ERR_ARG;
  if (p->max_side < 1 || p->max_side > kStereoMaxSide) return UNINA_ERR_ARG;
  if (p->max_mean_sad < 0 || p->max_mean_sad > 255 || p->uniqueness < 0 || p->uniqueness > 1000) return UNINA_ERR_ARG;
  const StereoRange range = stereo_range(cam->fx, baseline, p->min_depth, p->max_depth, pair->width);
  if (range.status != 0) return UNINA_ERR_ARG;
  if (stereo_prepare() != hipSuccess) return UNINA_ERR_HIP;
  StereoArgs a;
  a.left = pair->left;
  a.right = pair->right;
  a.width = pair->width;
  a.height = pair->height;
  a.pitch = pair->pitch;
  a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
  a.fxB = range.fxB;
  a.d_lo = range.d_lo;
  a.d_hi_all = range.d_hi_all;
  a.sx = p->sx; a.sy = p->sy; a.shrink = p->shrink;
  a.max_side = p->max_side;
  a.max_mean_sad = p->max_mean_sad;
  a.uniqueness = p->uniqueness;
  hipLaunchKernelGGL(stereo_kernel, dim3(MAX_DETECTIONS), dim3(kStBlock), kStereoLds, stream, d_dets, d_count, a, d_out, d_match);
  return launch_status();
}
