// Detections lifted to 3-D cone positions from a depth map on the device: one launch per frame behind the call that produced
// the records (include/unina_mi355.h "3-D localisation"; localize.locate_numpy is the definition, bit for bit).
//
// Per kept record: the box's central window on the depth map (csrc/locate_window.h), an integer sampling grid of at most
// max_side x max_side pixels, the LOWER MEDIAN of the valid samples in raw order, and the pinhole back-projection of the box
// centre at that depth. The median is found by counting, never by comparing floats: a valid sample's raw bits order as
// unsigned integers, so the sample of rank (n_valid - 1) / 2 is selected on those bits. All counters are integers and every
// fp32 operation has one fixed place in one fixed order (the unit is compiled with -ffp-contract=off): two runs give the same
// bytes, and they are numpy's.
//
// Work split. A workgroup is 4 waves and owns 4 consecutive record slots; the grid covers all MAX_DETECTIONS slots, so the
// slots at and beyond the count are zeroed by the same launch.
//   phase 1, a WAVE per slot: a window of at most 64 samples (a cone beyond a few metres: under 15 px across) puts one sample
//            in each lane and ranks them with 64 broadcasts -- no LDS, no barrier, four slots in flight per workgroup.
//   phase 2, the WORKGROUP per remaining slot, one after another: radix select over the key's bytes from the top, 256-bin
//            histograms in LDS (four passes for f32, two for u16). Each wave adds into a histogram of its own (ds_add_u32
//            without return; a flat region of the map sends every lane of a wave to one bin, and that serialisation is then
//            not multiplied by four); wave 0 sums the four, scans the 256 bins with shuffles and publishes the bin that
//            holds the rank (csrc/radix_select.h). The first pass keeps the keys in LDS when the window has at most kCache
//            samples; the later passes read them there, and re-read the map (L2) for larger windows.
// 256 workgroups of 256 threads: one per CU, 36 KB of LDS each, so occupancy is no concern; a frame with ~500 records
// costs one small launch.
#include <hip/hip_runtime.h>

#include "locate_checks.h"
#include "radix_select.h"
#include "wave_block.h"

namespace unina {
namespace {

constexpr int kLocWaves = 4;
constexpr int kLocBlock = kLocWaves * kWave;
constexpr int kBins = kRadixBins;
constexpr int kCache = 8192;   // keys of one window kept in LDS between the passes (32 KB)

static_assert(MAX_DETECTIONS % kLocWaves == 0, "slots per workgroup");
static_assert(sizeof(unina_cone3d) == 32 && sizeof(GpuDetection) == 32, "record layouts");

struct LocateArgs {
  const unsigned char* plane;
  int format, width, height, pitch;
  float unit;
  float fx, fy, cx, cy;
  float sx, sy, shrink, min_depth, max_depth;
  int max_side, min_valid;
};

__device__ __forceinline__ LocateWindow slot_window(const GpuDetection* __restrict__ dets, int slot, const LocateArgs& a) {
  const float4 b = *reinterpret_cast<const float4*>(dets + slot);   // x1, y1, x2, y2
  return locate_window(b.x, b.y, b.z, b.w, a.sx, a.sy, a.shrink, a.width, a.height, a.max_side);
}

// key of sample s (row-major over the sampling grid); every index is inside the map by construction of the window
__device__ __forceinline__ uint32_t sample_key(const LocateArgs& a, const LocateWindow& w, int s) {
  const int r = s / w.cols, c = s - r * w.cols;
  const size_t row = (size_t)(w.v0 + r * w.stride_y) * (size_t)a.pitch;
  const int u = w.u0 + c * w.stride_x;
  if (a.format == UNINA_DEPTH_F32) {
    const uint32_t bits = *reinterpret_cast<const uint32_t*>(a.plane + row + 4 * (size_t)u);
    return locate_key_f32(bits, a.unit, a.min_depth, a.max_depth);
  }
  const uint32_t raw = *reinterpret_cast<const unsigned short*>(a.plane + row + 2 * (size_t)u);
  return locate_key_u16(raw, a.unit, a.min_depth, a.max_depth);
}

// the record of a non-empty window: the point where enough samples are valid, zeros in x, y, z otherwise
__device__ __forceinline__ void store_result(unina_cone3d* __restrict__ out, int slot, const LocateArgs& a, const LocateWindow& w,
                                             int n_valid, uint32_t median_key) {
  RecordWords<unina_cone3d> c;
  c.r.x = c.r.y = c.r.z = 0.0f;
  c.r.u = w.uc;
  c.r.v = w.vc;
  c.r.n_valid = n_valid;
  c.r.n_samples = w.n_samples;
  const int need = a.min_valid > 1 ? a.min_valid : 1;
  c.r.valid = n_valid >= need ? 1 : 0;
  if (c.r.valid) {
    const float raw = a.format == UNINA_DEPTH_F32 ? __uint_as_float(median_key) : (float)median_key;
    float xyz[3];
    locate_point(w.uc, w.vc, raw * a.unit, a.fx, a.fy, a.cx, a.cy, xyz);
    c.r.x = xyz[0];
    c.r.y = xyz[1];
    c.r.z = xyz[2];
  }
  store_record(out + slot, c);
}

__global__ void __launch_bounds__(kLocBlock) locate_kernel(const GpuDetection* __restrict__ dets, const int* __restrict__ d_count,
                                                           LocateArgs a, unina_cone3d* __restrict__ out) {
  __shared__ uint32_t s_cache[kCache];
  __shared__ uint32_t s_hist[kLocWaves][kBins];
  __shared__ int s_big[kLocWaves];
  __shared__ int s_sel[3];   // bin, rank inside the bin, n_valid

  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int n = record_count(d_count);
  const int slot0 = (int)blockIdx.x * kLocWaves;

  // ---- phase 1: a wave per slot
  {
    const int slot = slot0 + wave;
    int big = 0;
    if (slot >= n) {
      if (lane == 0) store_zero_record(out + slot);
    } else {
      const LocateWindow w = slot_window(dets, slot, a);
      if (w.empty) {
        if (lane == 0) store_zero_record(out + slot);
      } else if (w.n_samples > kWave) {
        big = 1;
      } else {
        const uint32_t key = lane < w.n_samples ? sample_key(a, w, lane) : 0u;
        const int n_valid = __popcll(__ballot(key != 0u));
        const int k = (n_valid - 1) / 2;
        // rank among the valid samples in (key, lane) order: a permutation of 0 .. n_valid - 1, so one lane holds rank k
        int rank = 0;
        for (int j = 0; j < w.n_samples; ++j) {
          const uint32_t kj = __shfl(key, j, kWave);
          rank += (kj != 0u && (kj < key || (kj == key && j < lane))) ? 1 : 0;
        }
        const unsigned long long hit = __ballot(key != 0u && rank == k);
        const int src = hit ? __ffsll((long long)hit) - 1 : 0;
        const uint32_t median = __shfl(key, src, kWave);
        if (lane == 0) store_result(out, slot, a, w, n_valid, median);
      }
    }
    if (lane == 0) s_big[wave] = big;
  }
  __syncthreads();

  // ---- phase 2: the workgroup per slot whose window holds more than 64 samples
  const int top = a.format == UNINA_DEPTH_F32 ? 24 : 8;   // shift of the key's highest byte
  for (int q = 0; q < kLocWaves; ++q) {
    if (!s_big[q]) continue;   // workgroup-uniform
    const int slot = slot0 + q;
    const LocateWindow w = slot_window(dets, slot, a);
    const bool cached = w.n_samples <= kCache;
    uint32_t prefix = 0u, himask = 0u;   // the bytes above the current one: fixed by the earlier passes
    int k = 0, n_valid = 0;
    for (int shift = top; shift >= 0; shift -= 8) {
      for (int i = tid; i < kLocWaves * kBins; i += kLocBlock) (&s_hist[0][0])[i] = 0u;
      __syncthreads();
      const bool first = shift == top;
      for (int s = tid; s < w.n_samples; s += kLocBlock) {
        uint32_t key;
        if (first || !cached) {
          key = sample_key(a, w, s);
          if (first && cached) s_cache[s] = key;
        } else {
          key = s_cache[s];
        }
        if (key != 0u && ((key ^ prefix) & himask) == 0u) atomicAdd(&s_hist[wave][(key >> shift) & (kBins - 1)], 1u);
      }
      __syncthreads();
      if (wave == 0) radix_pick<kLocWaves>(s_hist, lane, first, k, s_sel);
      __syncthreads();
      if (first) n_valid = s_sel[2];
      const int need = a.min_valid > 1 ? a.min_valid : 1;
      if (n_valid < need) break;   // workgroup-uniform; nothing was selected
      prefix |= (uint32_t)s_sel[0] << shift;
      himask |= (uint32_t)(kBins - 1) << shift;
      k = s_sel[1];
    }
    if (tid == 0) store_result(out, slot, a, w, n_valid, prefix);
    __syncthreads();   // s_sel and the histograms are free for the next slot
  }
}

}  // namespace
}  // namespace unina

extern "C" int unina_locate_async(const GpuDetection* d_dets, const int* d_count, const unina_depth* depth, const unina_pinhole* cam,
                                  const unina_locate_params* p, unina_cone3d* d_out, hipStream_t stream) {
  using namespace unina;
  if (!record_io_ok(d_dets, d_count, d_out) || !depth || !p || !depth->plane) return UNINA_ERR_ARG;
  if (!plane_dims_ok(depth->width, depth->height) || !pinhole_ok(cam)) return UNINA_ERR_ARG;
  if (!window_params_ok(p->sx, p->sy, p->shrink, p->min_depth, p->max_depth)) return UNINA_ERR_ARG;
  if (depth->format != UNINA_DEPTH_F32 && depth->format != UNINA_DEPTH_U16) return UNINA_ERR_ARG;
  const int elem = depth->format == UNINA_DEPTH_F32 ? 4 : 2;
  if ((long long)depth->pitch < (long long)depth->width * elem || depth->pitch % elem != 0) return UNINA_ERR_ARG;
  if (((uintptr_t)depth->plane & (uintptr_t)(elem - 1)) || !finite_pos(depth->unit)) return UNINA_ERR_ARG;
  if (p->max_side < 1 || p->max_side > 256 || p->min_valid < 0) return UNINA_ERR_ARG;
  LocateArgs a;
  a.plane = static_cast<const unsigned char*>(depth->plane);
  a.format = depth->format;
  a.width = depth->width;
  a.height = depth->height;
  a.pitch = depth->pitch;
  a.unit = depth->unit;
  a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
  a.sx = p->sx; a.sy = p->sy; a.shrink = p->shrink; a.min_depth = p->min_depth; a.max_depth = p->max_depth;
  a.max_side = p->max_side;
  a.min_valid = p->min_valid;
  hipLaunchKernelGGL(locate_kernel, dim3(MAX_DETECTIONS / kLocWaves), dim3(kLocBlock), 0, stream, d_dets, d_count, a, d_out);
  return launch_status();
}
