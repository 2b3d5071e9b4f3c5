// The ground stripped from a LiDAR sweep on the device, in front of unina_locate_lidar_async (include/unina_mi355.h "ground
// removal from a LiDAR sweep"; ground.ground_numpy is the definition, bit for bit). The per-point and per-cell halves -- transform,
// cell, key, envelope term, label -- are csrc/ground_cell.h, the cloud's and the workspace's plumbing csrc/cloud_io.h.
//
// N points (30 000 .. 260 000 a sweep) against a grid of at most 1024 x 1024 cells. Five kernels, enqueued by the one call behind
// a memset of the call's nx * ny cell keys to 0xff and of the header to 0, nothing synchronised; a stage boundary is a launch
// boundary, no kernel waits on another workgroup:
//   seed      a thread per point: 16-byte loads where the base and the stride allow, three dwords otherwise. (cell or -1, bits of
//             zl) leave as one 8-byte store, so no later kernel transforms a point again. A sweep puts neighbouring lanes in one
//             cell, so the seeds of a wave that share a cell are folded first and ONE integer atomicMin per distinct cell and wave
//             carries their minimum key.
//   envelope  a thread per cell, a workgroup per tile of 32 x 8 cells: the tile and a halo of `reach` cells go to LDS (EMPTY
//             outside the grid), each thread takes the minimum of the (2 * reach + 1)^2 terms around it. Seeded cells are counted:
//             a ballot, one integer atomic per wave.
//   classify  a thread per point, workgroups of 1024: the label byte and the bits of h; the labels are counted with a ballot per
//             wave and label into LDS, then ONE integer atomic per workgroup and label (the five counters share a cache line: an
//             atomic per wave queued 16 times as many on it); the kept points of the workgroup are counted (block_rank) into one
//             word.
//   scan      one workgroup of 1024 threads, four words a thread: the exclusive prefix of the at most 4096 workgroup counts in one
//             pass; n_points and n_kept go into the header.
//   scatter   a thread per point i, the workgroups of classify: r = the kept points before i. A kept point stores (x, y, z, h) to
//             entry r, any other point the NaN entry to n_kept + (i - r): every thread one 16-byte store, the n_points entries
//             covered exactly once.
// Every counter and every minimum is an integer; a float is never combined atomically. So two runs give the same bytes, and a
// permuted cloud the same grids, header and per-point labels.
#include <hip/hip_runtime.h>

#include <new>

#include "ground_cell.h"
#include "record_io.h"
#include "wave_block.h"

struct unina_ground {
  int device = 0;
  int max_points = 0;
  unsigned char* d_mem = nullptr;   // the workspace; allocated by the first call
};

namespace unina {
namespace {

constexpr int kSeedBlock = 256;
constexpr int kTileX = 32, kTileY = 8;        // envelope: cells a workgroup owns; a wave is two rows of the tile
constexpr int kEnvBlock = kTileX * kTileY;
constexpr int kHaloX = kTileX + 2 * kGroundMaxReach, kHaloY = kTileY + 2 * kGroundMaxReach;
constexpr int kPtBlock = 1024;                // classify, scatter: the workgroup whose kept points are one word of the scan
constexpr int kPtWaves = kPtBlock / kWave;
constexpr int kMaxBlocks = kCloudMaxPoints / kPtBlock;   // 4096: one pass of the scan

static_assert(kGroundMaxSide == UNINA_GROUND_MAX_SIDE && kGroundMaxReach == UNINA_GROUND_MAX_REACH, "header limits");
static_assert(kCloudMaxPoints == UNINA_LIDAR_MAX_POINTS && kMaxBlocks == kScanBlock * kScanPer, "the scan is one pass");
static_assert(sizeof(unina_ground_header) == 32 && sizeof(unina_ground_params) == 48, "record layouts");
static_assert(sizeof(GroundGrid) == 48 + sizeof(unina_ground_params), "GroundGrid is the extrinsic and the parameters");
static_assert(kEnvBlock % kWave == 0 && kSeedBlock % kWave == 0, "whole waves");

// The workspace. labels, cellmin, ground and header are what unina_ground_buffers hands out.
struct Workspace {
  uint2* cellz;        // max_points: x = cell or 0xffffffff, y = the bits of zl
  uint32_t* h;         // max_points: the bits of zl - g, the NaN word where there is no envelope
  uint8_t* labels;     // max_points
  uint32_t* cellmin;   // kGroundMaxSide^2; the first nx * ny are the call's
  uint32_t* ground;    // kGroundMaxSide^2
  uint32_t* kept;      // kMaxBlocks: kept points per classify workgroup
  uint32_t* offset;    // kMaxBlocks: exclusive prefix of kept
  unina_ground_header* header;
};

// the arrays at `base`; returns the bytes they take
size_t workspace_layout(const unina_ground* g, uintptr_t base, Workspace* w) {
  const size_t np = (size_t)g->max_points;
  const size_t cells = (size_t)kGroundMaxSide * kGroundMaxSide;
  size_t at = 0;
  w->cellz = carve<uint2>(base, at, np);
  w->h = carve<uint32_t>(base, at, np);
  w->labels = carve<uint8_t>(base, at, np);
  w->cellmin = carve<uint32_t>(base, at, cells);
  w->ground = carve<uint32_t>(base, at, cells);
  w->kept = carve<uint32_t>(base, at, kMaxBlocks);
  w->offset = carve<uint32_t>(base, at, kMaxBlocks);
  w->header = carve<unina_ground_header>(base, at, 1);
  return at;
}

// ---------------------------------------------------------------- seed
template <bool VEC>
__global__ void __launch_bounds__(kSeedBlock) ground_seed_kernel(const unsigned char* __restrict__ points, int n, int stride, GroundGrid grid,
                                                                 uint2* __restrict__ cellz, uint32_t* __restrict__ cellmin) {
  const int i = (int)blockIdx.x * kSeedBlock + (int)threadIdx.x;   // < 2^22 + 256
  const int lane = (int)threadIdx.x & (kWave - 1);
  int cell = -1;   // of a seed; no lane leaves before the fold: every lane takes part in its shuffles
  uint32_t key = kGroundEmpty;
  if (i < n) {
    uint32_t x, y, z;
    load_xyz<VEC>(points, i, stride, &x, &y, &z);
    const GroundPoint p = ground_point(grid, bits_float(x), bits_float(y), bits_float(z));
    cellz[i] = make_uint2((uint32_t)p.cell, p.z_bits);
    if (p.seed) {
      cell = p.cell;   // < nx * ny: IN_GRID
      key = ground_key(bits_float(p.z_bits));
    }
  }
  unsigned long long todo = __ballot(cell >= 0);
  while (todo) {   // wave-uniform
    KeyGroup g;
    wave_first_group(todo, cell, g);
    uint32_t m = cell == g.key ? key : kGroundEmpty;
    if (g.lanes & (g.lanes - 1ull)) {   // wave-uniform: more than one lane in this cell
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)m, o, kWave);
        m = t < m ? t : m;
      }
    }
    if (lane == g.leader) atomicMin(&cellmin[g.key], m);
    todo &= ~g.lanes;
  }
}

// ---------------------------------------------------------------- envelope
__global__ void __launch_bounds__(kEnvBlock) ground_envelope_kernel(const uint32_t* __restrict__ cellmin, int nx, int ny, int reach, float rise,
                                                                    uint32_t* __restrict__ ground, unina_ground_header* __restrict__ header) {
  __shared__ uint32_t s_tile[kHaloY][kHaloX];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1);
  const int x0 = (int)blockIdx.x * kTileX - reach, y0 = (int)blockIdx.y * kTileY - reach;
  const int w = kTileX + 2 * reach, h = kTileY + 2 * reach;   // <= kHaloX, kHaloY: reach <= kGroundMaxReach
  for (int t = tid; t < w * h; t += kEnvBlock) {
    const int ty = t / w, tx = t - ty * w;
    const int gx = x0 + tx, gy = y0 + ty;
    s_tile[ty][tx] = (gx >= 0 && gx < nx && gy >= 0 && gy < ny) ? cellmin[gy * nx + gx] : kGroundEmpty;
  }
  __syncthreads();
  const int lx = tid % kTileX, ly = tid / kTileX;
  const int cx = (int)blockIdx.x * kTileX + lx, cy = (int)blockIdx.y * kTileY + ly;
  const bool inside = cx < nx && cy < ny;
  uint32_t best = kGroundEmpty;
  for (int dj = -reach; dj <= reach; ++dj) {
    for (int di = -reach; di <= reach; ++di) {
      const uint32_t v = s_tile[ly + reach + dj][lx + reach + di];
      const int aj = dj < 0 ? -dj : dj, ai = di < 0 ? -di : di;
      if (v != kGroundEmpty) {
        const uint32_t t = ground_term(v, aj > ai ? aj : ai, rise);
        best = t < best ? t : best;
      }
    }
  }
  if (inside) ground[cy * nx + cx] = best;
  const int seeded = __popcll(__ballot(inside && s_tile[ly + reach][lx + reach] != kGroundEmpty));
  if (lane == 0 && seeded) atomicAdd(&header->n_cells_seeded, seeded);
}

// ---------------------------------------------------------------- classify
__global__ void __launch_bounds__(kPtBlock) ground_classify_kernel(const uint2* __restrict__ cellz, int n, GroundGrid grid,
                                                                   const uint32_t* __restrict__ ground, uint8_t* __restrict__ labels,
                                                                   uint32_t* __restrict__ h, uint32_t* __restrict__ kept,
                                                                   unina_ground_header* __restrict__ header) {
  __shared__ int s_cnt[kPtWaves];
  __shared__ int s_label[kGroundLabels];
  const int i = (int)blockIdx.x * kPtBlock + (int)threadIdx.x;   // < 2^22 + 1024
  const int lane = (int)threadIdx.x & (kWave - 1);
  if (threadIdx.x < kGroundLabels) s_label[threadIdx.x] = 0;
  __syncthreads();
  int label = -1;   // a thread behind the cloud has none; it still takes part in the ballots and the barriers
  if (i < n) {
    const uint2 cz = cellz[i];
    const int cell = (int)cz.x;
    const uint32_t g = cell >= 0 ? ground[cell] : kGroundEmpty;   // cell < nx * ny
    uint32_t h_bits;
    label = ground_label(grid, cell, bits_float(cz.y), g, &h_bits);
    labels[i] = (uint8_t)label;
    h[i] = h_bits;
  }
#pragma unroll
  for (int l = 0; l < kGroundLabels; ++l) {
    const int c = __popcll(__ballot(label == l));
    if (lane == 0 && c) atomicAdd(&s_label[l], c);
  }
  int total;
  (void)block_rank<kPtWaves>(label >= 0 && ground_kept(label, grid.keep_unknown), s_cnt, &total);   // its barriers stand behind every wave's LDS adds
  if (threadIdx.x == 0) kept[blockIdx.x] = (uint32_t)total;
  if (threadIdx.x < kGroundLabels && s_label[threadIdx.x]) atomicAdd(&header->n_label[threadIdx.x], s_label[threadIdx.x]);
}

// ---------------------------------------------------------------- scan: offset[b] = kept[0] + .. + kept[b - 1]; the header's n_points, n_kept
__global__ void __launch_bounds__(kScanBlock) ground_scan_kernel(const uint32_t* __restrict__ kept, uint32_t* __restrict__ offset, int n_blocks,
                                                                 int n_points, unina_ground_header* __restrict__ header) {
  __shared__ int s_wave[kScanWaves];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int i = kScanPer * tid;   // n_blocks <= kMaxBlocks = kScanPer * kScanBlock, and both arrays hold kMaxBlocks words
  uint4 c = make_uint4(0u, 0u, 0u, 0u);
  if (i < n_blocks) c = *reinterpret_cast<const uint4*>(kept + i);
  if (i + 1 >= n_blocks) c.y = 0u;   // the words behind n_blocks are readable and hold whatever an earlier call left
  if (i + 2 >= n_blocks) c.z = 0u;
  if (i + 3 >= n_blocks) c.w = 0u;
  const int mine = (int)(c.x + c.y + c.z + c.w);   // every count and every sum is at most 2^22
  const int incl = wave_incl_scan(mine, lane);
  if (lane == kWave - 1) s_wave[wave] = incl;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int v = 0; v < kScanWaves; ++v) {
    const int t = s_wave[v];
    if (v < wave) before += t;
    total += t;
  }
  const uint32_t o0 = (uint32_t)(before + incl - mine);
  if (i < n_blocks) *reinterpret_cast<uint4*>(offset + i) = make_uint4(o0, o0 + c.x, o0 + c.x + c.y, o0 + c.x + c.y + c.z);
  if (tid == 0) {
    header->n_points = n_points;
    header->n_kept = total;
  }
}

// ---------------------------------------------------------------- scatter
template <bool VEC>
__global__ void __launch_bounds__(kPtBlock) ground_scatter_kernel(const unsigned char* __restrict__ points, int n, int stride, int keep_unknown,
                                                                  const uint8_t* __restrict__ labels, const uint32_t* __restrict__ h,
                                                                  const uint32_t* __restrict__ offset,
                                                                  const unina_ground_header* __restrict__ header, uint4* __restrict__ out) {
  __shared__ int s_cnt[kPtWaves];
  const int i = (int)blockIdx.x * kPtBlock + (int)threadIdx.x;
  const bool live = i < n;
  const bool kept = live && ground_kept((int)labels[live ? i : 0], keep_unknown);   // n > 0: the kernel is not launched otherwise
  int total;
  const int rank = block_rank<kPtWaves>(kept, s_cnt, &total);   // the flags and the order of ground_classify_kernel's count
  if (!live) return;
  const int r = (int)offset[blockIdx.x] + rank;   // kept points before i: <= i, and < n_kept where i is kept
  if (kept) {
    uint32_t x, y, z;
    load_xyz<VEC>(points, i, stride, &x, &y, &z);
    out[r] = make_uint4(x, y, z, h[i]);
  } else {
    out[header->n_kept + (i - r)] = make_uint4(kGroundNaN, kGroundNaN, kGroundNaN, kGroundNaN);   // i - r < n - n_kept: the others before i
  }
}

bool params_ok(const unina_ground_params* p) {
  if (!finite(p->x_min) || !finite(p->y_min) || !finite_pos(p->cell)) return false;
  if (p->nx < 1 || p->nx > kGroundMaxSide || p->ny < 1 || p->ny > kGroundMaxSide) return false;
  if (!finite(p->z_lo) || !finite(p->z_hi) || !finite(p->rise) || !finite(p->band) || !finite(p->max_height)) return false;
  if (p->z_lo > p->z_hi || p->rise < 0.0f || p->band < 0.0f || p->max_height < p->band) return false;
  return p->reach >= 0 && p->reach <= kGroundMaxReach;
}

}  // namespace
}  // namespace unina

extern "C" int unina_ground_create(int device_id, int max_points, unina_ground_t** out) {
  using namespace unina;
  if (!out) return UNINA_ERR_ARG;
  *out = nullptr;
  if (!cloud_limits_ok(device_id, max_points)) return UNINA_ERR_ARG;
  unina_ground* g = new (std::nothrow) unina_ground();
  if (!g) return UNINA_ERR_IO;
  g->device = device_id;
  g->max_points = max_points;
  *out = g;
  return UNINA_OK;
}

extern "C" void unina_ground_destroy(unina_ground_t* g) {
  if (!g) return;
  unina::workspace_release(g->device, g->d_mem);
  delete g;
}

extern "C" int unina_ground_filter_async(unina_ground_t* g, const unina_cloud* cloud, const float lidar_to_level[12],
                                         const unina_ground_params* p, void* d_out, hipStream_t stream) {
  using namespace unina;
  if (!g || !p || !d_out || ((uintptr_t)d_out & 15)) return UNINA_ERR_ARG;
  if (!cloud_ok(cloud, g->max_points) || !extrinsic_ok(lidar_to_level) || !params_ok(p)) return UNINA_ERR_ARG;
  const int n = cloud->n_points;
  {
    const uintptr_t in = (uintptr_t)cloud->points, out = (uintptr_t)d_out;
    if (n > 0 && in < out + (uintptr_t)n * 16u && out < in + (uintptr_t)n * (uintptr_t)cloud->stride) return UNINA_ERR_ARG;
  }
  Workspace ws;
  if (const int rc = workspace_ensure(g->device, &g->d_mem, workspace_layout(g, 0, &ws))) return rc;   // allocated on first use
  workspace_layout(g, (uintptr_t)g->d_mem, &ws);
  GroundGrid grid;
  for (int i = 0; i < 12; ++i) grid.m[i] = lidar_to_level[i];
  grid.x_min = p->x_min; grid.y_min = p->y_min; grid.cell = p->cell;
  grid.nx = p->nx; grid.ny = p->ny;
  grid.z_lo = p->z_lo; grid.z_hi = p->z_hi; grid.rise = p->rise; grid.band = p->band; grid.max_height = p->max_height;
  grid.reach = p->reach; grid.keep_unknown = p->keep_unknown;
  const size_t cells = (size_t)p->nx * (size_t)p->ny;

  if (hipMemsetAsync(ws.cellmin, 0xff, cells * sizeof(uint32_t), stream) != hipSuccess) return UNINA_ERR_HIP;
  if (hipMemsetAsync(ws.header, 0, sizeof(unina_ground_header), stream) != hipSuccess) return UNINA_ERR_HIP;
  const unsigned char* points = static_cast<const unsigned char*>(cloud->points);
  const bool vec = cloud_vec16(cloud);
  if (n > 0) {
    const dim3 blocks((unsigned)((n + kSeedBlock - 1) / kSeedBlock));
    UNINA_LAUNCH_VEC(vec, ground_seed_kernel, blocks, dim3(kSeedBlock), stream, points, n, cloud->stride, grid, ws.cellz, ws.cellmin);
    if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  }
  hipLaunchKernelGGL(ground_envelope_kernel, dim3((unsigned)((p->nx + kTileX - 1) / kTileX), (unsigned)((p->ny + kTileY - 1) / kTileY)),
                     dim3(kEnvBlock), 0, stream, ws.cellmin, p->nx, p->ny, p->reach, p->rise, ws.ground, ws.header);
  if (n == 0) return launch_status();
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  const int n_blocks = (n + kPtBlock - 1) / kPtBlock;   // <= kMaxBlocks
  hipLaunchKernelGGL(ground_classify_kernel, dim3((unsigned)n_blocks), dim3(kPtBlock), 0, stream, ws.cellz, n, grid, ws.ground, ws.labels, ws.h,
                     ws.kept, ws.header);
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  hipLaunchKernelGGL(ground_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, ws.kept, ws.offset, n_blocks, n, ws.header);
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  uint4* out = static_cast<uint4*>(d_out);
  UNINA_LAUNCH_VEC(vec, ground_scatter_kernel, dim3((unsigned)n_blocks), dim3(kPtBlock), stream, points, n, cloud->stride, p->keep_unknown,
                   ws.labels, ws.h, ws.offset, ws.header, out);
  return launch_status();
}

extern "C" int unina_ground_buffers(unina_ground_t* g, const uint8_t** d_labels, const uint32_t** d_cellmin, const uint32_t** d_ground,
                                    const unina_ground_header** d_header) {
  using namespace unina;
  if (!g) return UNINA_ERR_ARG;
  if (!g->d_mem) return UNINA_ERR_STATE;
  Workspace ws;
  workspace_layout(g, (uintptr_t)g->d_mem, &ws);
  if (d_labels) *d_labels = ws.labels;
  if (d_cellmin) *d_cellmin = ws.cellmin;
  if (d_ground) *d_ground = ws.ground;
  if (d_header) *d_header = ws.header;
  return UNINA_OK;
}
