// Detections lifted to 3-D cone positions from a LiDAR sweep on the device: one call per frame behind the call that produced the
// records (include/unina_mi355.h "3-D localisation from a LiDAR sweep"; localize.locate_lidar_numpy is the definition, bit for
// bit). The per-point half -- transform, projection, pixel, key -- is csrc/lidar_project.h; the window, the point and the checks
// are the depth route's (csrc/locate_window.h, csrc/locate_checks.h), the cloud's and the workspace's plumbing csrc/cloud_io.h.
//
// The work is N points (30 000 .. 260 000 a sweep) against at most 1024 windows, so the points are first sorted by image cell
// (32 x 32 pixels) with a counting sort, and a record then reads only the cells its window touches. Four kernels, enqueued by the
// one call behind a memset of the cell counters, nothing synchronised:
//   project  a thread per point: 16-byte loads where the base and the stride allow, three dwords otherwise; the point's
//            unina_lidar_pixel leaves as one 16-byte store. A projectable point takes a position in its cell: a sweep puts
//            neighbouring lanes in one cell, so the lanes of a wave that share a cell are folded first and ONE integer atomic per
//            distinct cell and wave returns the base of their positions.
//   scan     one workgroup of 1024 threads, four cells a thread: the exclusive prefix of the counts, 4096 cells a pass.
//   scatter  a thread per point: (u, v, key) to offset[cell] + position. No atomics.
//   select   as csrc/locate.hip: a workgroup is 4 waves and owns 4 consecutive record slots, the grid covers all MAX_DETECTIONS
//            slots, the slots at and beyond the count are zeroed by the same launch. The cells of a window that lie in one cell
//            row are ONE contiguous range of the sorted array; its entries are the record's CANDIDATES, those inside the exact
//            pixel rectangle its members.
//            phase 1, a WAVE per slot with at most 64 candidates (a cone beyond 10 m holds a handful of points): a candidate per
//                     lane, ranked with broadcasts -- no LDS, no barrier.
//            phase 2, the WORKGROUP per remaining slot: radix select over the four key bytes from the top, per-wave 256-bin
//                     histograms in LDS, the bin picked by csrc/radix_select.h. A wave walks every fourth cell row of the window.
//                     The first pass compacts the valid keys into LDS; where all of them fit (kCache), the later passes read
//                     them there, otherwise they walk the candidates again.
// Every counter is an integer; a float is never added atomically. The order of the entries inside a cell differs from run to run
// (it is the order in which the atomics arrive), and nothing downstream depends on it: members are counted, the median is
// selected by counting. So two runs, and any permutation of the cloud, give the same unina_cone3d bytes, and they are numpy's.
#include <hip/hip_runtime.h>

#include <new>

#include "lidar_project.h"
#include "locate_checks.h"
#include "radix_select.h"
#include "wave_block.h"

struct unina_lidar {
  int device = 0;
  int max_points = 0, max_width = 0, max_height = 0;
  unsigned char* d_mem = nullptr;   // the workspace; allocated by the first call that needs it
};

namespace unina {
namespace {

constexpr int kPtBlock = 256;                 // project, scatter
constexpr int kSelWaves = 4;
constexpr int kSelBlock = kSelWaves * kWave;
constexpr int kCache = 8192;                  // valid keys of one record kept in LDS between the passes (32 KB)

static_assert(kLidarMaxDim == UNINA_LIDAR_MAX_DIM && kCloudMaxPoints == UNINA_LIDAR_MAX_POINTS, "header limits");
static_assert(kLidarMaxDim <= 1 << 16, "a sorted entry packs u and v into 16 bits each");
static_assert(MAX_DETECTIONS % kSelWaves == 0, "slots per workgroup");
static_assert(sizeof(unina_cone3d) == 32 && sizeof(GpuDetection) == 32, "record layouts");
static_assert(sizeof(unina_lidar_pixel) == 16 && sizeof(LidarPixel) == 16, "a pixel is one 16-byte word");

// The workspace. `sorted` holds one entry per projectable point, grouped by cell: cell c owns offset[c] .. offset[c + 1] - 1.
// INVARIANT: the order of the entries INSIDE a cell is the arrival order of the project kernel's atomics and differs from run to
// run; a reader may count and select among them, never depend on their order.
struct Workspace {
  uint4* pixels;      // max_points: the unina_lidar_pixel of every point, in point order
  uint2* sorted;      // max_points: x = u | v << 16, y = key
  uint32_t* pos;      // max_points: a projectable point's position inside its cell
  uint32_t* count;    // cells, rounded up to kScanPer: points per cell
  uint32_t* offset;   // cells + 1: exclusive prefix of count
};

// the arrays at `base`; returns the bytes they take
size_t workspace_layout(const unina_lidar* l, uintptr_t base, Workspace* w) {
  const size_t np = (size_t)l->max_points;
  const size_t cells = (size_t)lidar_cells(l->max_width) * (size_t)lidar_cells(l->max_height);
  size_t at = 0;
  w->pixels = carve<uint4>(base, at, np);
  w->sorted = carve<uint2>(base, at, np);
  w->pos = carve<uint32_t>(base, at, np);
  w->count = carve<uint32_t>(base, at, cells + kScanPer);
  w->offset = carve<uint32_t>(base, at, cells + 1);
  return at;
}

// ---------------------------------------------------------------- project + count
template <bool VEC>
__global__ void __launch_bounds__(kPtBlock) lidar_project_kernel(const unsigned char* __restrict__ points, int n, int stride, LidarCamera cam,
                                                                 int cells_x, uint4* __restrict__ pixels, uint32_t* __restrict__ pos,
                                                                 uint32_t* __restrict__ count) {
  const int i = (int)blockIdx.x * kPtBlock + (int)threadIdx.x;   // < 2^22 + 256
  const int lane = (int)threadIdx.x & (kWave - 1);
  int cell = -1;   // no lane leaves before the fold: every lane takes part in its shuffles
  if (i < n) {
    uint32_t x, y, z;
    load_xyz<VEC>(points, i, stride, &x, &y, &z);
    const LidarPixel p = lidar_project(cam, bits_float(x), bits_float(y), bits_float(z));
    pixels[i] = make_uint4((uint32_t)p.u, (uint32_t)p.v, p.key, (uint32_t)p.projectable);
    if (p.projectable) cell = lidar_cell(p.u, p.v, cells_x);   // < cells_x * cells_y: the pixel is inside the image
  }
  // the lanes of this wave that share a cell take consecutive positions behind one atomic
  unsigned long long todo = __ballot(cell >= 0);
  uint32_t mine = 0u;
  while (todo) {   // wave-uniform
    KeyGroup g;
    wave_first_group(todo, cell, g);
    uint32_t base = 0u;
    if (lane == g.leader) base = atomicAdd(&count[g.key], (uint32_t)__popcll(g.lanes));
    base = (uint32_t)__shfl((int)base, g.leader, kWave);
    if (cell == g.key) mine = base + (uint32_t)__popcll(g.lanes & ((1ull << lane) - 1ull));
    todo &= ~g.lanes;
  }
  if (cell >= 0) pos[i] = mine;
}

// ---------------------------------------------------------------- scan: offset[c] = count[0] + .. + count[c - 1], offset[n_cells] = all
// `count` is readable (and zero) up to n_cells rounded up to kScanPer.
__global__ void __launch_bounds__(kScanBlock) lidar_scan_kernel(const uint32_t* __restrict__ count, uint32_t* __restrict__ offset, int n_cells) {
  __shared__ int s_wave[kScanWaves];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  int running = 0;   // every count and every sum is at most 2^22
  for (int base = 0; base < n_cells; base += kScanBlock * kScanPer) {   // workgroup-uniform
    const int i = base + kScanPer * tid;
    uint4 c = make_uint4(0u, 0u, 0u, 0u);
    if (i < n_cells) c = *reinterpret_cast<const uint4*>(count + i);
    const int mine = (int)(c.x + c.y + c.z + c.w);
    const int incl = wave_incl_scan(mine, lane);
    __syncthreads();   // s_wave is free again
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < kScanWaves; ++v) {
      const int t = s_wave[v];
      if (v < wave) before += t;
      total += t;
    }
    const uint32_t o0 = (uint32_t)(running + before + incl - mine);
    const uint4 o = make_uint4(o0, o0 + c.x, o0 + c.x + c.y, o0 + c.x + c.y + c.z);
    if (i + kScanPer <= n_cells) {
      *reinterpret_cast<uint4*>(offset + i) = o;
    } else if (i < n_cells) {
      offset[i] = o.x;
      if (i + 1 < n_cells) offset[i + 1] = o.y;
      if (i + 2 < n_cells) offset[i + 2] = o.z;
    }
    running += total;
  }
  if (tid == 0) offset[n_cells] = (uint32_t)running;
}

// ---------------------------------------------------------------- scatter
__global__ void __launch_bounds__(kPtBlock) lidar_scatter_kernel(const uint4* __restrict__ pixels, const uint32_t* __restrict__ pos,
                                                                 const uint32_t* __restrict__ offset, int n, int cells_x,
                                                                 uint2* __restrict__ sorted) {
  const int i = (int)blockIdx.x * kPtBlock + (int)threadIdx.x;
  if (i >= n) return;
  const uint4 p = pixels[i];
  if (!p.w) return;
  const int cell = lidar_cell((int)p.x, (int)p.y, cells_x);
  sorted[offset[cell] + pos[i]] = make_uint2(p.x | (p.y << 16), p.z);   // < offset[cell + 1] <= n
}

// ---------------------------------------------------------------- select
struct SelectArgs {
  float fx, fy, cx, cy;
  float sx, sy, shrink;
  int width, height, cells_x, min_valid;
};

__device__ __forceinline__ LocateWindow slot_window(const GpuDetection* __restrict__ dets, int slot, const SelectArgs& a) {
  const float4 b = *reinterpret_cast<const float4*>(dets + slot);   // x1, y1, x2, y2
  return locate_window(b.x, b.y, b.z, b.w, a.sx, a.sy, a.shrink, a.width, a.height, kLidarMaxDim);   // stride 1
}

// the candidates of window w in cell row r (counted from the window's first): entries lo .. hi - 1 of the sorted array
__device__ __forceinline__ void row_range(const uint32_t* __restrict__ offset, const SelectArgs& a, const LocateWindow& w, int r, uint32_t* lo,
                                          uint32_t* hi) {
  const int first = ((w.v0 >> kLidarCellShift) + r) * a.cells_x;
  *lo = offset[first + (w.u0 >> kLidarCellShift)];
  *hi = offset[first + (w.u1 >> kLidarCellShift) + 1];   // index <= cells: the scan wrote that many + 1
}

__device__ __forceinline__ bool is_member(const uint2 e, const LocateWindow& w) {
  const int u = (int)(e.x & 0xffffu), v = (int)(e.x >> 16);
  return u >= w.u0 && u <= w.u1 && v >= w.v0 && v <= w.v1;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// the record of a non-empty window: the point where enough members are valid, zeros in x, y, z otherwise
__device__ __forceinline__ void store_result(unina_cone3d* __restrict__ out, int slot, const SelectArgs& a, const LocateWindow& w, int n_samples,
                                             int n_valid, uint32_t median_key) {
  RecordWords<unina_cone3d> c;
  c.r.x = c.r.y = c.r.z = 0.0f;
  c.r.u = w.uc;
  c.r.v = w.vc;
  c.r.n_valid = n_valid;
  c.r.n_samples = n_samples;
  const int need = a.min_valid > 1 ? a.min_valid : 1;
  c.r.valid = n_valid >= need ? 1 : 0;
  if (c.r.valid) {
    float xyz[3];
    locate_point(w.uc, w.vc, __uint_as_float(median_key), a.fx, a.fy, a.cx, a.cy, xyz);
    c.r.x = xyz[0];
    c.r.y = xyz[1];
    c.r.z = xyz[2];
  }
  store_record(out + slot, c);
}

__global__ void __launch_bounds__(kSelBlock) lidar_select_kernel(const GpuDetection* __restrict__ dets, const int* __restrict__ d_count,
                                                                 SelectArgs a, const uint32_t* __restrict__ offset,
                                                                 const uint2* __restrict__ sorted, unina_cone3d* __restrict__ out) {
  __shared__ uint32_t s_cache[kCache];
  __shared__ uint32_t s_hist[kSelWaves][kRadixBins];
  __shared__ int s_big[kSelWaves];
  __shared__ int s_sel[3];   // bin, rank inside the bin, n_valid
  __shared__ int s_cnt[2];   // members, valid keys offered to the cache

  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int n = record_count(d_count);
  const int slot0 = (int)blockIdx.x * kSelWaves;

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
      } else {
        const int rows = (w.v1 >> kLidarCellShift) - (w.v0 >> kLidarCellShift) + 1;
        int cand = 0;
        for (int r0 = 0; r0 < rows; r0 += kWave) {   // a cell row per lane
          uint32_t lo = 0u, hi = 0u;
          if (r0 + lane < rows) row_range(offset, a, w, r0 + lane, &lo, &hi);
          cand += (int)(hi - lo);
        }
        cand = wave_sum(cand);
        if (cand > kWave) {
          big = 1;
        } else {
          // candidate j goes to lane j: the non-empty rows (at most `cand` of them) are handed out one after another
          uint2 e = make_uint2(0u, 0u);
          bool have = false;
          int given = 0;
          for (int r0 = 0; r0 < rows; r0 += kWave) {
            uint32_t lo = 0u, hi = 0u;
            if (r0 + lane < rows) row_range(offset, a, w, r0 + lane, &lo, &hi);
            unsigned long long todo = __ballot(hi > lo);
            while (todo) {   // wave-uniform
              const int src = __ffsll((long long)todo) - 1;
              todo &= todo - 1ull;
              const uint32_t rlo = (uint32_t)__shfl((int)lo, src, kWave);
              const int rlen = (int)((uint32_t)__shfl((int)hi, src, kWave) - rlo);
              if (lane >= given && lane < given + rlen) {
                e = sorted[rlo + (uint32_t)(lane - given)];
                have = true;
              }
              given += rlen;
            }
          }
          const bool member = have && is_member(e, w);
          const uint32_t key = member ? e.y : 0u;
          const int n_samples = __popcll(__ballot(member));
          const int n_valid = __popcll(__ballot(key != 0u));
          const int k = (n_valid - 1) / 2;
          // rank among the valid keys in (key, lane) order: a permutation of 0 .. n_valid - 1, so one lane holds rank k
          int rank = 0;
          for (int j = 0; j < cand; ++j) {
            const uint32_t kj = (uint32_t)__shfl((int)key, j, kWave);
            rank += (kj != 0u && (kj < key || (kj == key && j < lane))) ? 1 : 0;
          }
          const unsigned long long hit = __ballot(key != 0u && rank == k);
          const int src = hit ? __ffsll((long long)hit) - 1 : 0;
          const uint32_t median = (uint32_t)__shfl((int)key, src, kWave);
          if (lane == 0) store_result(out, slot, a, w, n_samples, n_valid, median);
        }
      }
    }
    if (lane == 0) s_big[wave] = big;
  }
  __syncthreads();

  // ---- phase 2: the workgroup per slot with more than 64 candidates
  for (int q = 0; q < kSelWaves; ++q) {
    if (!s_big[q]) continue;   // workgroup-uniform
    const int slot = slot0 + q;
    const LocateWindow w = slot_window(dets, slot, a);
    const int rows = (w.v1 >> kLidarCellShift) - (w.v0 >> kLidarCellShift) + 1;
    const int need = a.min_valid > 1 ? a.min_valid : 1;
    uint32_t prefix = 0u, himask = 0u;   // the bytes above the current one: fixed by the earlier passes
    int k = 0, n_valid = 0, n_samples = 0;
    bool cached = false;
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int i = tid; i < kSelWaves * kRadixBins; i += kSelBlock) (&s_hist[0][0])[i] = 0u;
      const bool first = shift == 24;
      if (first && tid < 2) s_cnt[tid] = 0;
      __syncthreads();
      if (first || !cached) {
        int members = 0;
        for (int r = wave; r < rows; r += kSelWaves) {   // wave-uniform, and so are lo and hi
          uint32_t lo, hi;
          row_range(offset, a, w, r, &lo, &hi);
          for (uint32_t i0 = lo; i0 < hi; i0 += kWave) {
            const uint32_t i = i0 + (uint32_t)lane;
            uint2 e = make_uint2(0u, 0u);
            if (i < hi) e = sorted[i];
            const bool member = i < hi && is_member(e, w);
            const uint32_t key = member ? e.y : 0u;
            members += member ? 1 : 0;
            if (first) {
              // the valid keys are compacted into the cache, a wave's at consecutive places; those past its end are dropped
              const unsigned long long v = __ballot(key != 0u);
              if (v) {   // wave-uniform
                const int leader = __ffsll((long long)v) - 1;
                int base = 0;
                if (lane == leader) base = atomicAdd(&s_cnt[1], __popcll(v));
                base = __shfl(base, leader, kWave);
                const int at = base + __popcll(v & ((1ull << lane) - 1ull));
                if (key != 0u && at < kCache) s_cache[at] = key;
              }
            }
            if (key != 0u && ((key ^ prefix) & himask) == 0u) atomicAdd(&s_hist[wave][(key >> shift) & (kRadixBins - 1)], 1u);
          }
        }
        if (first) {
          members = wave_sum(members);
          if (lane == 0 && members) atomicAdd(&s_cnt[0], members);
        }
      } else {
        for (int s = tid; s < n_valid; s += kSelBlock) {
          const uint32_t key = s_cache[s];
          if (((key ^ prefix) & himask) == 0u) atomicAdd(&s_hist[wave][(key >> shift) & (kRadixBins - 1)], 1u);
        }
      }
      __syncthreads();
      if (wave == 0) radix_pick<kSelWaves>(s_hist, lane, first, k, s_sel);
      __syncthreads();
      if (first) {
        n_valid = s_sel[2];
        n_samples = s_cnt[0];
        cached = n_valid <= kCache;   // s_cnt[1] == n_valid: every valid key was given a place
      }
      if (n_valid < need) break;   // workgroup-uniform; nothing was selected
      prefix |= (uint32_t)s_sel[0] << shift;
      himask |= (uint32_t)(kRadixBins - 1) << shift;
      k = s_sel[1];
    }
    if (tid == 0) store_result(out, slot, a, w, n_samples, n_valid, prefix);
    __syncthreads();   // s_sel, s_cnt and the histograms are free for the next slot
  }
}

}  // namespace
}  // namespace unina

extern "C" int unina_lidar_create(int device_id, int max_points, int max_width, int max_height, unina_lidar_t** out) {
  using namespace unina;
  if (!out) return UNINA_ERR_ARG;
  *out = nullptr;
  if (!cloud_limits_ok(device_id, max_points)) return UNINA_ERR_ARG;
  if (max_width < 1 || max_width > kLidarMaxDim || max_height < 1 || max_height > kLidarMaxDim) return UNINA_ERR_ARG;
  unina_lidar* l = new (std::nothrow) unina_lidar();
  if (!l) return UNINA_ERR_IO;
  l->device = device_id;
  l->max_points = max_points;
  l->max_width = max_width;
  l->max_height = max_height;
  *out = l;
  return UNINA_OK;
}

extern "C" void unina_lidar_destroy(unina_lidar_t* l) {
  if (!l) return;
  unina::workspace_release(l->device, l->d_mem);
  delete l;
}

extern "C" int unina_locate_lidar_async(unina_lidar_t* l, const GpuDetection* d_dets, const int* d_count, const unina_cloud* cloud,
                                        const float lidar_to_cam[12], const unina_pinhole* cam, int width, int height,
                                        const unina_lidar_params* p, unina_cone3d* d_out, hipStream_t stream) {
  using namespace unina;
  if (!l || !p || !record_io_ok(d_dets, d_count, d_out)) return UNINA_ERR_ARG;
  if (!cloud_ok(cloud, l->max_points) || !extrinsic_ok(lidar_to_cam)) return UNINA_ERR_ARG;
  if (width < 1 || width > l->max_width || height < 1 || height > l->max_height) return UNINA_ERR_ARG;
  if (!pinhole_ok(cam) || !window_params_ok(p->sx, p->sy, p->shrink, p->min_depth, p->max_depth) || p->min_valid < 0) return UNINA_ERR_ARG;
  Workspace ws;
  if (const int rc = workspace_ensure(l->device, &l->d_mem, workspace_layout(l, 0, &ws))) return rc;   // allocated on first use
  workspace_layout(l, (uintptr_t)l->d_mem, &ws);
  const int n = cloud->n_points;
  const int cells_x = lidar_cells(width), n_cells = cells_x * lidar_cells(height);
  LidarCamera c;
  for (int i = 0; i < 12; ++i) c.m[i] = lidar_to_cam[i];
  c.fx = cam->fx; c.fy = cam->fy; c.cx = cam->cx; c.cy = cam->cy;
  c.width = width;
  c.height = height;
  c.min_depth = p->min_depth;
  c.max_depth = p->max_depth;
  SelectArgs a;
  a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
  a.sx = p->sx; a.sy = p->sy; a.shrink = p->shrink;
  a.width = width;
  a.height = height;
  a.cells_x = cells_x;
  a.min_valid = p->min_valid;

  const size_t counted = ((size_t)n_cells + kScanPer - 1) / kScanPer * kScanPer;   // what the scan reads
  if (hipMemsetAsync(ws.count, 0, counted * sizeof(uint32_t), stream) != hipSuccess) return UNINA_ERR_HIP;
  const unsigned char* points = static_cast<const unsigned char*>(cloud->points);
  const dim3 per_point((unsigned)((n + kPtBlock - 1) / kPtBlock));
  if (n > 0) {
    UNINA_LAUNCH_VEC(cloud_vec16(cloud), lidar_project_kernel, per_point, dim3(kPtBlock), stream, points, n, cloud->stride, c, cells_x,
                     ws.pixels, ws.pos, ws.count);
    if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  }
  hipLaunchKernelGGL(lidar_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, ws.count, ws.offset, n_cells);
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  if (n > 0) {
    hipLaunchKernelGGL(lidar_scatter_kernel, per_point, dim3(kPtBlock), 0, stream, ws.pixels, ws.pos, ws.offset, n, cells_x, ws.sorted);
    if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  }
  hipLaunchKernelGGL(lidar_select_kernel, dim3(MAX_DETECTIONS / kSelWaves), dim3(kSelBlock), 0, stream, d_dets, d_count, a, ws.offset, ws.sorted,
                     d_out);
  return launch_status();
}

extern "C" int unina_lidar_buffers(unina_lidar_t* l, const unina_lidar_pixel** d_pixels) {
  using namespace unina;
  if (!l) return UNINA_ERR_ARG;
  if (!l->d_mem) return UNINA_ERR_STATE;
  Workspace ws;
  workspace_layout(l, (uintptr_t)l->d_mem, &ws);
  if (d_pixels) *d_pixels = reinterpret_cast<const unina_lidar_pixel*>(ws.pixels);
  return UNINA_OK;
}
