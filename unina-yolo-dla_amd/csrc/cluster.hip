// A ground-free LiDAR sweep clustered into cone candidates on the device, behind unina_ground_filter_async and in front of
// unina_track_update_async (include/unina_mi355.h "cone candidates from a ground-free LiDAR sweep"; cluster.cluster_numpy is the
// definition, bit for bit). The per-point and per-component halves -- cell, keys, offsets, position, gate, records -- are
// csrc/cluster_cell.h, the cloud's and the workspace's plumbing csrc/cloud_io.h.
//
// N points (a few thousand behind the ground filter, up to 260 000 without it) against a grid of at most 1024 x 1024 cells. Eleven
// kernels, enqueued by the one call behind a memset of the call's nx * ny occupancy words and of the header to 0, nothing
// synchronised; a stage boundary is a launch boundary, NO kernel waits on another workgroup (no flag, no spin, no grid sync):
//   mark      a thread per point (16-byte loads where the base and the stride allow): occ[cell] = 1, a plain store of the one
//             value every writer stores; the IN_GRID points counted per workgroup, one integer atomic each.
//   label     a thread per cell, a workgroup per tile of 32 x 32 cells with a halo of one EMPTY cell in LDS: every occupied cell
//             starts as its own label (its index in the tile), then takes the minimum of the 3 x 3 labels around it and of that
//             label's label until a sweep changes nothing. Labels only decrease, so the loop ends; a cell's label is then the
//             smallest cell of its component WITHIN the tile. parent[c] = that cell's grid index, -1 for an empty cell.
//   merge     a thread per cell: for each of the four neighbours behind it (W, NW, N, NE) that lies in ANOTHER tile and is
//             occupied, the two trees are united in the global parent array: find both roots, link the larger under the smaller
//             with atomicMin, go on from what the atomicMin returns. parent[c] <= c always, so every chain ends and the root of
//             a tree is its smallest cell.
//   flatten   a thread per cell, workgroups of 1024 cells: the root of the cell's tree goes to occ[c] as root + 1 (parent is only
//             read); the roots of the workgroup are counted (block_rank) into one word.
//   scan      one workgroup: the exclusive prefix of the at most 1024 counts; n_points and n_components into the header.
//   rank      a thread per cell: a root's position in the table = the roots before it; it goes to parent[root], the root into
//             the table entry, and the entry's sums are cleared. Only n_components entries are touched, never max_points.
//   cells     a thread per cell: the occupied cells of a wave that share a component are folded, the waves of a workgroup meet
//             in LDS slots, ONE integer atomicAdd per component and workgroup.
//   sums      a thread per point, workgroups of 1024: its component (occ, parent) goes to the per-point array; the points of a
//             wave that share a component are folded -- six minima / maxima of keys, a count, two sums --, the sixteen waves
//             meet in LDS slots, and ONE thread per component and workgroup does the nine integer atomics. A wall of 10 000
//             points in one component is 10 atomics a word, not 10 000.
//   finish    a thread per component: position, extents, gate -> the table entry; the CONE components of a workgroup counted.
//   scan      the same pass over those counts; n_cones, n_written, n_dropped into the header, n_written into *d_count.
//   emit      a thread per component: the r-th CONE component writes records r (r < MAX_DETECTIONS); thread t of the first
//             workgroup zeroes slot t >= n_written. All MAX_DETECTIONS entries of both arrays are written by every call.
// Dense per-cell memory is occ and parent, 8 bytes a cell; everything else is per point or per component. Every counter, minimum,
// maximum and sum is an integer: two runs give the same bytes, a permuted cloud the same table, records and header.
#include <hip/hip_runtime.h>

#include <new>

#include "cluster_cell.h"
#include "record_io.h"
#include "wave_block.h"

struct unina_clusterer {
  int device = 0;
  int max_points = 0;
  unsigned char* d_mem = nullptr;   // the workspace; allocated by the first call
};

namespace unina {
namespace {

constexpr int kPtBlock = 256;                  // mark: a thread per point
constexpr int kPtWaves = kPtBlock / kWave;
constexpr int kSumBlock = 1024;                // sums: a thread per point, sixteen waves that meet in LDS before they go to the table
constexpr int kTile = 32;                      // label, merge: the cells a workgroup owns are kTile x kTile
constexpr int kTileBlock = kTile * kTile;
constexpr int kHalo = kTile + 2;               // the tile in LDS with its halo of one cell
constexpr int kNoLabel = 0x7fffffff;           // an empty cell of the tile, and every cell of the halo
constexpr int kRowBlock = 1024;                // flatten, rank, cells, finish, emit: cells or components a workgroup counts into one word
constexpr int kRowWaves = kRowBlock / kWave;
constexpr int kMaxBlocks = kCloudMaxPoints / kRowBlock;   // 4096: one pass of the scan; the cells need 1024 of them at most

static_assert(kMaxBlocks == kScanBlock * kScanPer, "the scan is one pass");
static_assert(kGroundMaxSide * kGroundMaxSide / kRowBlock <= kMaxBlocks, "the cells' counts fit the scan");
static_assert(kTileBlock == 1024 && kTileBlock % kWave == 0 && kPtBlock % kWave == 0, "whole waves");
static_assert(sizeof(unina_cluster) == 48 && sizeof(unina_cluster_params) == 48 && sizeof(unina_cluster_header) == 32, "record layouts");
static_assert(sizeof(ClusterGrid) == 48 + sizeof(unina_cluster_params) && sizeof(ClusterSums) == 48, "ClusterGrid is the extrinsic and the parameters");
static_assert(MAX_DETECTIONS <= kRowBlock, "the first workgroup of emit zeroes every free slot");

// The workspace. table, point_component and header are what unina_cluster_buffers hands out.
struct Workspace {
  uint32_t* occ;            // kGroundMaxSide^2; the first nx * ny are the call's: 0 empty, 1 occupied (mark), root + 1 (flatten)
  int* parent;              // kGroundMaxSide^2: -1 empty, else a cell of the same component, <= the cell; a root's rank after `rank`
  ClusterSums* sums;        // max_points
  unina_cluster* table;     // max_points
  int* point_component;     // max_points
  uint32_t* count;          // kMaxBlocks: roots per flatten workgroup, then cones per finish workgroup
  uint32_t* offset;         // kMaxBlocks: exclusive prefix of count
  unina_cluster_header* header;
};

size_t workspace_layout(const unina_clusterer* g, uintptr_t base, Workspace* w) {
  const size_t np = (size_t)g->max_points;
  const size_t cells = (size_t)kGroundMaxSide * kGroundMaxSide;
  size_t at = 0;
  w->occ = carve<uint32_t>(base, at, cells);
  w->parent = carve<int>(base, at, cells);
  w->sums = carve<ClusterSums>(base, at, np);
  w->table = carve<unina_cluster>(base, at, np);
  w->point_component = carve<int>(base, at, np);
  w->count = carve<uint32_t>(base, at, kMaxBlocks);
  w->offset = carve<uint32_t>(base, at, kMaxBlocks);
  w->header = carve<unina_cluster_header>(base, at, 1);
  return at;
}

// a parent word that another workgroup of the same launch may have written
__device__ __forceinline__ int load_parent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---------------------------------------------------------------- mark
template <bool VEC>
__global__ void __launch_bounds__(kPtBlock) cluster_mark_kernel(const unsigned char* __restrict__ points, int n, int stride, ClusterGrid grid,
                                                                uint32_t* __restrict__ occ, unina_cluster_header* __restrict__ header) {
  __shared__ int s_cnt[kPtWaves];
  const int i = (int)blockIdx.x * kPtBlock + (int)threadIdx.x;   // < 2^22 + 256
  int cell = -1;
  if (i < n) {
    uint32_t x, y, z;
    load_xyz<VEC>(points, i, stride, &x, &y, &z);
    cell = cluster_point(grid, bits_float(x), bits_float(y), bits_float(z)).cell;
    if (cell >= 0) occ[cell] = 1u;   // cell < nx * ny: IN_GRID
  }
  int total;
  (void)block_rank<kPtWaves>(cell >= 0, s_cnt, &total);
  if (threadIdx.x == 0 && total) atomicAdd(&header->n_in_grid, total);
}

// ---------------------------------------------------------------- label
__global__ void __launch_bounds__(kTileBlock) cluster_label_kernel(const uint32_t* __restrict__ occ, int nx, int ny, int* __restrict__ parent,
                                                                   unina_cluster_header* __restrict__ header) {
  __shared__ int s_label[kHalo * kHalo];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1);
  const int lx = tid % kTile, ly = tid / kTile;
  const int cx = (int)blockIdx.x * kTile + lx, cy = (int)blockIdx.y * kTile + ly;
  const bool inside = cx < nx && cy < ny;
  const bool mine = inside && occ[cy * nx + cx] != 0u;
  const int at = (ly + 1) * kHalo + (lx + 1);
  for (int t = tid; t < kHalo * kHalo; t += kTileBlock) s_label[t] = kNoLabel;   // the halo stays so: a tile is labelled on its own
  __syncthreads();
  if (mine) s_label[at] = at;
  __syncthreads();   // the first sweep reads every cell's own label, not the fill
  const int occupied = __popcll(__ballot(mine));
  if (lane == 0 && occupied) atomicAdd(&header->n_cells, occupied);
  // Every label is the index of an occupied cell of the same component and only ever decreases: the loop ends. A sweep reads
  // labels that other threads lower meanwhile; whichever value it sees is such an index. A sweep in which no thread stores ends
  // the loop, and in it every thread read the final labels: neighbours are then equal, and the common label L has label[L] = L,
  // which only the smallest cell of the component satisfies.
  while (true) {
    int changed = 0;
    if (mine) {
      const int cur = s_label[at];
      int m = cur;
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj) {
#pragma unroll
        for (int di = -1; di <= 1; ++di) {
          const int v = s_label[at + dj * kHalo + di];
          m = v < m ? v : m;
        }
      }
      const int up = s_label[m];   // m <= cur is an occupied cell of the tile: its label is one too
      m = up < m ? up : m;
      if (m < cur) {
        s_label[at] = m;
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  if (inside) {
    int p = -1;
    if (mine) {
      const int m = s_label[at];
      p = ((int)blockIdx.y * kTile + m / kHalo - 1) * nx + (int)blockIdx.x * kTile + m % kHalo - 1;   // row-major in the tile as in the grid: the smallest
    }
    parent[cy * nx + cx] = p;
  }
}

// ---------------------------------------------------------------- merge
// Unites the trees of cells a and b. Every read of a parent word is an agent-scope atomic load, every write the atomicMin: a
// word only ever decreases and always names a cell of the same component, so whatever a load returns is an ancestor.
__device__ void unite(int* parent, int a, int b) {
  while (true) {
    for (int p = load_parent(parent + a); p != a; p = load_parent(parent + a)) a = p;   // parent[a] < a off the root: ends
    for (int p = load_parent(parent + b); p != b; p = load_parent(parent + b)) b = p;
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);   // b < a
    if (old == a) return;                       // a was still a root: it hangs under b now
    // a had been linked under old < a meanwhile, and is linked under min(old, b) now: old's tree and b's are still to unite
    a = old;
  }
}

__global__ void __launch_bounds__(kTileBlock) cluster_merge_kernel(int nx, int ny, int* __restrict__ parent) {
  const int tid = (int)threadIdx.x;
  const int lx = tid % kTile, ly = tid / kTile;
  const int cx = (int)blockIdx.x * kTile + lx, cy = (int)blockIdx.y * kTile + ly;
  if (cx >= nx || cy >= ny) return;
  if (lx != 0 && ly != 0 && lx != kTile - 1) return;   // W, NW, N and NE of every other cell lie in its own tile
  const int c = cy * nx + cx;
  if (load_parent(parent + c) < 0) return;
  const int dx[4] = {-1, -1, 0, 1}, dy[4] = {0, -1, -1, -1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ox = cx + dx[k], oy = cy + dy[k];
    if (ox < 0 || ox >= nx || oy < 0) continue;
    if (ox / kTile == cx / kTile && oy / kTile == cy / kTile) continue;   // joined by label already
    const int o = oy * nx + ox;
    if (load_parent(parent + o) < 0) continue;
    unite(parent, c, o);
  }
}

// ---------------------------------------------------------------- flatten
__global__ void __launch_bounds__(kRowBlock) cluster_flatten_kernel(const int* __restrict__ parent, int cells, uint32_t* __restrict__ occ,
                                                                    uint32_t* __restrict__ count) {
  __shared__ int s_cnt[kRowWaves];
  const int c = (int)blockIdx.x * kRowBlock + (int)threadIdx.x;
  bool root = false;
  if (c < cells) {
    int r = parent[c];
    if (r >= 0) {
      for (int p = parent[r]; p != r; p = parent[r]) r = p;   // parent is not written here
      occ[c] = (uint32_t)r + 1u;
      root = r == c;
    }
  }
  int total;
  (void)block_rank<kRowWaves>(root, s_cnt, &total);
  if (threadIdx.x == 0) count[blockIdx.x] = (uint32_t)total;
}

// ---------------------------------------------------------------- scan: offset[b] = count[0] + .. + count[b - 1], and the header words
// that follow from the total. CONES false: behind flatten (n_points, n_components); true: behind finish (n_cones, n_written,
// n_dropped, *d_count).
template <bool CONES>
__global__ void __launch_bounds__(kScanBlock) cluster_scan_kernel(const uint32_t* __restrict__ count, uint32_t* __restrict__ offset, int n_blocks,
                                                                  int n_points, unina_cluster_header* __restrict__ header, int* __restrict__ d_count) {
  __shared__ int s_wave[kScanWaves];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int i = kScanPer * tid;   // n_blocks <= kMaxBlocks = kScanPer * kScanBlock, and both arrays hold kMaxBlocks words
  uint4 c = make_uint4(0u, 0u, 0u, 0u);
  if (i < n_blocks) c = *reinterpret_cast<const uint4*>(count + i);
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
    if (CONES) {
      const int written = total < MAX_DETECTIONS ? total : MAX_DETECTIONS;
      header->n_cones = total;
      header->n_written = written;
      header->n_dropped = total - written;
      *d_count = written;
    } else {
      header->n_points = n_points;
      header->n_components = total;
    }
  }
}

// ---------------------------------------------------------------- rank
__global__ void __launch_bounds__(kRowBlock) cluster_rank_kernel(const uint32_t* __restrict__ occ, int cells, const uint32_t* __restrict__ offset,
                                                                 int* __restrict__ parent, ClusterSums* __restrict__ sums,
                                                                 unina_cluster* __restrict__ table) {
  __shared__ int s_cnt[kRowWaves];
  const int c = (int)blockIdx.x * kRowBlock + (int)threadIdx.x;
  const bool root = c < cells && occ[c] == (uint32_t)c + 1u;   // the flags and the order of cluster_flatten_kernel's count
  int total;
  const int rank = block_rank<kRowWaves>(root, s_cnt, &total);
  if (!root) return;
  const int r = (int)offset[blockIdx.x] + rank;   // roots before c: < n_components <= the IN_GRID points <= max_points
  parent[c] = r;                                  // no other thread reads or writes a root's word in this launch
  ClusterSums s;
  cluster_sums_clear(s);
  sums[r] = s;
  table[r].root = c;
}

// ---------------------------------------------------------------- the fold of a workgroup by component, in LDS
// A wave folds its lanes by component (wave_first_group); the waves of a workgroup then meet in kSlots LDS slots, and the
// workgroup does its global atomics once per slot. A ring of a raw sweep is one component of 10 000 points: an atomic per wave
// and word put 20 000 of them on one line and cost 0.59 of the call's 0.67 ms at 260 000 points (the section on this unit).
// The slot of a component is claimed with an integer compare-and-swap on its key, kProbes slots from key % kSlots on; a
// component that finds none goes to global memory directly. Every operation is an integer minimum, maximum or sum, so the
// result does not depend on which way a value took.
constexpr int kSlots = 64;
constexpr int kProbes = 4;

__device__ __forceinline__ int claim_slot(int* s_key, int key) {
#pragma unroll
  for (int t = 0; t < kProbes; ++t) {
    const int h = (key + t) & (kSlots - 1);
    const int prev = atomicCAS(&s_key[h], -1, key);
    if (prev == -1 || prev == key) return h;
  }
  return -1;
}

// ---------------------------------------------------------------- cells
__global__ void __launch_bounds__(kRowBlock) cluster_cells_kernel(const uint32_t* __restrict__ occ, int cells, const int* __restrict__ parent,
                                                                  ClusterSums* __restrict__ sums) {
  __shared__ int s_key[kSlots], s_n[kSlots];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1);
  const int c = (int)blockIdx.x * kRowBlock + tid;
  if (tid < kSlots) {
    s_key[tid] = -1;
    s_n[tid] = 0;
  }
  __syncthreads();
  int comp = -1;   // no lane leaves before the fold: every lane takes part in its shuffles, every thread in the barriers
  if (c < cells) {
    const uint32_t o = occ[c];
    if (o) comp = parent[o - 1u];   // the root's rank
  }
  unsigned long long todo = __ballot(comp >= 0);
  while (todo) {   // wave-uniform
    KeyGroup g;
    wave_first_group(todo, comp, g);
    if (lane == g.leader) {
      const int slot = claim_slot(s_key, g.key);
      if (slot >= 0) atomicAdd(&s_n[slot], __popcll(g.lanes));
      else atomicAdd(&sums[g.key].n_cells, __popcll(g.lanes));
    }
    todo &= ~g.lanes;
  }
  __syncthreads();
  if (tid < kSlots && s_key[tid] >= 0) atomicAdd(&sums[s_key[tid]].n_cells, s_n[tid]);
}

// ---------------------------------------------------------------- sums
// one component's share of a wave or of a workgroup into the table: nine integer atomics
__device__ __forceinline__ void sums_add(ClusterSums* s, uint32_t x_lo, uint32_t x_hi, uint32_t y_lo, uint32_t y_hi, uint32_t z_lo, uint32_t z_hi,
                                         int n_points, int qx, int qy) {
  atomicMin(&s->kx_lo, x_lo); atomicMax(&s->kx_hi, x_hi);
  atomicMin(&s->ky_lo, y_lo); atomicMax(&s->ky_hi, y_hi);
  atomicMin(&s->kz_lo, z_lo); atomicMax(&s->kz_hi, z_hi);
  atomicAdd(&s->n_points, n_points);
  atomicAdd(&s->sx, (unsigned long long)qx);
  atomicAdd(&s->sy, (unsigned long long)qy);
}

template <bool VEC>
__global__ void __launch_bounds__(kSumBlock) cluster_sums_kernel(const unsigned char* __restrict__ points, int n, int stride, ClusterGrid grid,
                                                                 const uint32_t* __restrict__ occ, const int* __restrict__ parent,
                                                                 int* __restrict__ point_component, ClusterSums* __restrict__ sums) {
  __shared__ int s_key[kSlots], s_n[kSlots], s_qx[kSlots], s_qy[kSlots];   // 1024 offsets below 2^18: a workgroup's sum fits an int
  __shared__ uint32_t s_lo[3][kSlots], s_hi[3][kSlots];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1);
  const int i = (int)blockIdx.x * kSumBlock + tid;   // < 2^22 + 1024
  if (tid < kSlots) {
    s_key[tid] = -1;
    s_n[tid] = s_qx[tid] = s_qy[tid] = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      s_lo[k][tid] = 0xffffffffu;
      s_hi[k][tid] = 0u;
    }
  }
  __syncthreads();
  int comp = -1;   // no lane leaves before the fold: every lane takes part in its shuffles, every thread in the barriers
  ClusterPoint p;
  p.cell = -1; p.kx = p.ky = p.kz = 0u; p.qx = p.qy = 0;
  if (i < n) {
    uint32_t x, y, z;
    load_xyz<VEC>(points, i, stride, &x, &y, &z);
    p = cluster_point(grid, bits_float(x), bits_float(y), bits_float(z));
    const uint32_t o = p.cell >= 0 ? occ[p.cell] : 0u;   // mark saw this point: its cell is occupied, occ holds root + 1
    if (o) comp = parent[o - 1u];
    point_component[i] = comp;
  }
  unsigned long long todo = __ballot(comp >= 0);
  while (todo) {   // wave-uniform
    KeyGroup g;
    wave_first_group(todo, comp, g);
    const bool in = comp == g.key;
    uint32_t lo[3] = {in ? p.kx : 0xffffffffu, in ? p.ky : 0xffffffffu, in ? p.kz : 0xffffffffu};
    uint32_t hi[3] = {in ? p.kx : 0u, in ? p.ky : 0u, in ? p.kz : 0u};
    int qx = in ? p.qx : 0, qy = in ? p.qy : 0;   // 64 offsets below 2^18: the wave's sum fits an int
    if (g.lanes & (g.lanes - 1ull)) {   // wave-uniform: more than one lane in this component
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const uint32_t a = (uint32_t)__shfl_xor((int)lo[k], o, kWave), b = (uint32_t)__shfl_xor((int)hi[k], o, kWave);
          lo[k] = a < lo[k] ? a : lo[k];
          hi[k] = b > hi[k] ? b : hi[k];
        }
        qx += __shfl_xor(qx, o, kWave);
        qy += __shfl_xor(qy, o, kWave);
      }
    }
    if (lane == g.leader) {
      const int members = __popcll(g.lanes);
      const int slot = claim_slot(s_key, g.key);
      if (slot >= 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          atomicMin(&s_lo[k][slot], lo[k]);
          atomicMax(&s_hi[k][slot], hi[k]);
        }
        atomicAdd(&s_n[slot], members);
        atomicAdd(&s_qx[slot], qx);
        atomicAdd(&s_qy[slot], qy);
      } else {
        sums_add(sums + g.key, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], members, qx, qy);   // g.key < n_components
      }
    }
    todo &= ~g.lanes;
  }
  __syncthreads();
  if (tid < kSlots && s_key[tid] >= 0)
    sums_add(sums + s_key[tid], s_lo[0][tid], s_hi[0][tid], s_lo[1][tid], s_hi[1][tid], s_lo[2][tid], s_hi[2][tid], s_n[tid], s_qx[tid], s_qy[tid]);
}

// ---------------------------------------------------------------- finish
__global__ void __launch_bounds__(kRowBlock) cluster_finish_kernel(const ClusterSums* __restrict__ sums, ClusterGrid grid,
                                                                   const unina_cluster_header* __restrict__ header, unina_cluster* __restrict__ table,
                                                                   uint32_t* __restrict__ count) {
  __shared__ int s_cnt[kRowWaves];
  const int k = (int)blockIdx.x * kRowBlock + (int)threadIdx.x;
  bool cone = false;
  if (k < header->n_components) {   // <= max_points: the grid covers min(n_points, cells) entries, which bounds n_components
    const unina_cluster c = cluster_finish(grid, sums[k], table[k].root);
    table[k] = c;
    cone = c.cone != 0;
  }
  int total;
  (void)block_rank<kRowWaves>(cone, s_cnt, &total);
  if (threadIdx.x == 0) count[blockIdx.x] = (uint32_t)total;
}

// ---------------------------------------------------------------- emit
__global__ void __launch_bounds__(kRowBlock) cluster_emit_kernel(const unina_cluster* __restrict__ table, ClusterGrid grid,
                                                                 const uint32_t* __restrict__ offset, const unina_cluster_header* __restrict__ header,
                                                                 GpuDetection* __restrict__ dets, unina_cone3d* __restrict__ cones) {
  __shared__ int s_cnt[kRowWaves];
  const int k = (int)blockIdx.x * kRowBlock + (int)threadIdx.x;
  const bool live = k < header->n_components;
  const bool cone = live && table[k].cone != 0;   // the flags and the order of cluster_finish_kernel's count
  int total;
  const int rank = block_rank<kRowWaves>(cone, s_cnt, &total);
  if (blockIdx.x == 0 && (int)threadIdx.x < MAX_DETECTIONS && (int)threadIdx.x >= header->n_written) {   // a slot no component writes
    store_zero_record(dets + threadIdx.x);
    store_zero_record(cones + threadIdx.x);
  }
  if (!cone) return;
  const int r = (int)offset[blockIdx.x] + rank;   // CONE components before k
  if (r >= MAX_DETECTIONS) return;                // counted in n_dropped
  RecordWords<GpuDetection> d;
  RecordWords<unina_cone3d> c;
  cluster_records(grid, table[k], &d.r, &c.r);
  store_record(dets + r, d);
  store_record(cones + r, c);
}

bool params_ok(const unina_cluster_params* p) {
  if (!finite(p->x_min) || !finite(p->y_min) || !finite_pos(p->cell)) return false;
  if (p->nx < 1 || p->nx > kGroundMaxSide || p->ny < 1 || p->ny > kGroundMaxSide) return false;
  if (p->min_points < 1 || p->max_points < p->min_points) return false;
  if (!finite(p->min_height) || !finite(p->max_height) || !finite(p->max_width)) return false;
  if (p->min_height < 0.0f || p->max_height < p->min_height || p->max_width < 0.0f) return false;
  return p->confidence == p->confidence;   // a NaN fails
}

// the n bytes at a and the m bytes at b share a byte
bool overlap(uintptr_t a, uintptr_t n, uintptr_t b, uintptr_t m) { return n > 0 && m > 0 && a < b + m && b < a + n; }

}  // namespace
}  // namespace unina

extern "C" int unina_cluster_create(int device_id, int max_points, unina_cluster_t** out) {
  using namespace unina;
  if (!out) return UNINA_ERR_ARG;
  *out = nullptr;
  if (!cloud_limits_ok(device_id, max_points)) return UNINA_ERR_ARG;
  unina_clusterer* g = new (std::nothrow) unina_clusterer();
  if (!g) return UNINA_ERR_IO;
  g->device = device_id;
  g->max_points = max_points;
  *out = g;
  return UNINA_OK;
}

extern "C" void unina_cluster_destroy(unina_cluster_t* g) {
  if (!g) return;
  unina::workspace_release(g->device, g->d_mem);
  delete g;
}

extern "C" int unina_cluster_async(unina_cluster_t* g, const unina_cloud* cloud, const float lidar_to_level[12], const unina_cluster_params* p,
                                   GpuDetection* d_dets, int* d_count, unina_cone3d* d_cones, hipStream_t stream) {
  using namespace unina;
  if (!g || !p || !record_io_ok(d_dets, d_count, d_cones)) return UNINA_ERR_ARG;
  if (!cloud_ok(cloud, g->max_points) || !extrinsic_ok(lidar_to_level) || !params_ok(p)) return UNINA_ERR_ARG;
  const int n = cloud->n_points;
  {
    const uintptr_t in = (uintptr_t)cloud->points, bytes = (uintptr_t)n * (uintptr_t)cloud->stride;
    if (overlap(in, bytes, (uintptr_t)d_dets, MAX_DETECTIONS * sizeof(GpuDetection)) ||
        overlap(in, bytes, (uintptr_t)d_cones, MAX_DETECTIONS * sizeof(unina_cone3d)) || overlap(in, bytes, (uintptr_t)d_count, sizeof(int)))
      return UNINA_ERR_ARG;
  }
  Workspace ws;
  if (const int rc = workspace_ensure(g->device, &g->d_mem, workspace_layout(g, 0, &ws))) return rc;   // allocated on first use
  workspace_layout(g, (uintptr_t)g->d_mem, &ws);
  ClusterGrid grid;
  for (int i = 0; i < 12; ++i) grid.m[i] = lidar_to_level[i];
  grid.x_min = p->x_min; grid.y_min = p->y_min; grid.cell = p->cell;
  grid.nx = p->nx; grid.ny = p->ny;
  grid.min_points = p->min_points; grid.max_points = p->max_points;
  grid.min_height = p->min_height; grid.max_height = p->max_height; grid.max_width = p->max_width;
  grid.confidence = p->confidence; grid.class_id = p->class_id;

  if (hipMemsetAsync(ws.header, 0, sizeof(unina_cluster_header), stream) != hipSuccess) return UNINA_ERR_HIP;
  if (n == 0) {   // no point, no cell, no component: the all-zero answer
    if (hipMemsetAsync(d_dets, 0, MAX_DETECTIONS * sizeof(GpuDetection), stream) != hipSuccess) return UNINA_ERR_HIP;
    if (hipMemsetAsync(d_cones, 0, MAX_DETECTIONS * sizeof(unina_cone3d), stream) != hipSuccess) return UNINA_ERR_HIP;
    return hipMemsetAsync(d_count, 0, sizeof(int), stream) == hipSuccess ? UNINA_OK : UNINA_ERR_HIP;
  }
  const int cells = p->nx * p->ny;   // <= 2^20
  if (hipMemsetAsync(ws.occ, 0, (size_t)cells * sizeof(uint32_t), stream) != hipSuccess) return UNINA_ERR_HIP;
  const unsigned char* points = static_cast<const unsigned char*>(cloud->points);
  const bool vec = cloud_vec16(cloud);
  const dim3 pt_blocks((unsigned)((n + kPtBlock - 1) / kPtBlock));
  const dim3 tiles((unsigned)((p->nx + kTile - 1) / kTile), (unsigned)((p->ny + kTile - 1) / kTile));
  const int cell_blocks = (cells + kRowBlock - 1) / kRowBlock;                      // <= 1024
  const int comp_blocks = ((n < cells ? n : cells) + kRowBlock - 1) / kRowBlock;    // n_components <= min(n, cells); >= 1, <= kMaxBlocks

  UNINA_LAUNCH_VEC(vec, cluster_mark_kernel, pt_blocks, dim3(kPtBlock), stream, points, n, cloud->stride, grid, ws.occ, ws.header);
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  hipLaunchKernelGGL(cluster_label_kernel, tiles, dim3(kTileBlock), 0, stream, ws.occ, p->nx, p->ny, ws.parent, ws.header);
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  if (tiles.x * tiles.y > 1u) {   // one tile has no border to join across
    hipLaunchKernelGGL(cluster_merge_kernel, tiles, dim3(kTileBlock), 0, stream, p->nx, p->ny, ws.parent);
    if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  }
  hipLaunchKernelGGL(cluster_flatten_kernel, dim3((unsigned)cell_blocks), dim3(kRowBlock), 0, stream, ws.parent, cells, ws.occ, ws.count);
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  hipLaunchKernelGGL(cluster_scan_kernel<false>, dim3(1), dim3(kScanBlock), 0, stream, ws.count, ws.offset, cell_blocks, n, ws.header, d_count);
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  hipLaunchKernelGGL(cluster_rank_kernel, dim3((unsigned)cell_blocks), dim3(kRowBlock), 0, stream, ws.occ, cells, ws.offset, ws.parent, ws.sums,
                     ws.table);
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  hipLaunchKernelGGL(cluster_cells_kernel, dim3((unsigned)cell_blocks), dim3(kRowBlock), 0, stream, ws.occ, cells, ws.parent, ws.sums);
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  UNINA_LAUNCH_VEC(vec, cluster_sums_kernel, dim3((unsigned)((n + kSumBlock - 1) / kSumBlock)), dim3(kSumBlock), stream, points, n, cloud->stride, grid, ws.occ, ws.parent,
                   ws.point_component, ws.sums);
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  hipLaunchKernelGGL(cluster_finish_kernel, dim3((unsigned)comp_blocks), dim3(kRowBlock), 0, stream, ws.sums, grid, ws.header, ws.table, ws.count);
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  hipLaunchKernelGGL(cluster_scan_kernel<true>, dim3(1), dim3(kScanBlock), 0, stream, ws.count, ws.offset, comp_blocks, n, ws.header, d_count);
  if (launch_status() != UNINA_OK) return UNINA_ERR_HIP;
  hipLaunchKernelGGL(cluster_emit_kernel, dim3((unsigned)comp_blocks), dim3(kRowBlock), 0, stream, ws.table, grid, ws.offset, ws.header, d_dets,
                     d_cones);
  return launch_status();
}

extern "C" int unina_cluster_buffers(unina_cluster_t* g, const unina_cluster** d_components, const int** d_point_component,
                                     const unina_cluster_header** d_header) {
  using namespace unina;
  if (!g) return UNINA_ERR_ARG;
  if (!g->d_mem) return UNINA_ERR_STATE;
  Workspace ws;
  workspace_layout(g, (uintptr_t)g->d_mem, &ws);
  if (d_components) *d_components = ws.table;
  if (d_point_component) *d_point_component = ws.point_component;
  if (d_header) *d_header = ws.header;
  return UNINA_OK;
}
