// kmeans.hip -- the k-means coreset: MFMA assignment, full-batch Lloyd loop without a host round-trip, nearest-row selection.
//
// Role in the reference (active_learning.py):
//   kmeans_*_kernel ........ coreset_selection_kmeans, the clustering        :194-200 (MiniBatchKMeans there; full-batch Lloyd here)
//   nearest_*_kernel ....... coreset_selection_kmeans, the selection loop    :203-209 (line for line)
//
// scikit-learn's mini-batch trajectory and RNG stream cannot be reproduced, so the clustering arithmetic is this build's own
// specification: per iteration  |c|^2 -> assign -> update -> inertia.
//   assign : label[i] = argmin_j |c_j|^2 - 2 <x_i, c_j>, the LOWEST index winning exact ties; the dot products run on the
//            f32-input MFMA (v_mfma_f32_32x32x2_f32: a d-ordered fmaf chain, one rounding per product). Non-finite values are
//            not validated: the running minimum starts at (+inf, 0) and only `s < best` replaces it, so a NaN score never
//            wins and a row all of whose scores are NaN or +inf takes label 0 (include/unina_mi355.h).
//   update : c_j = (sum of member rows in ascending row index, fp32) / count_j; a cluster without members keeps its centroid.
//   inertia: sum_i sum_d (x_id - c_{label_i,d})^2 with the NEW centroids, differences and sums in double.
// The rule of mining.hip holds: every reduction has a fixed order and there are no float atomics (the one atomic is an integer
// count of changed labels), so two runs give identical bits. Compiled with -ffp-contract=off; fused operations are written
// as fmaf where they are meant.
#include <cmath>
#include <climits>

#include "kernels.h"
#include "wave_block.h"

namespace unina {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;

// control words at the head of the workspace
constexpr int kCtlStop = 0;      // 0 = run, 1 = converged, 2 = init row out of range: every later kernel returns at once
constexpr int kCtlChanged = 1;   // labels changed by the assignment of the current iteration
constexpr int kCtlIters = 2;     // iterations executed
constexpr int kCtlInts = 16;     // (64 bytes: what follows stays 16-byte aligned)

constexpr int kConvergedBit = 1 << 30;

// assignment tile: a workgroup owns kTileR rows (32 per wave) and walks the centroids in chunks of kTileC (4 MFMA tiles)
constexpr int kTileR = 128;
constexpr int kTileC = 128;
constexpr int kTileD = 32;                // channels staged per step
constexpr int kLds = kTileD + 1;          // odd row stride: the 64 lanes of an operand read hit 64 different banks
constexpr int kAccTiles = kTileC / 32;

constexpr int kInertiaMaxBlocks = 1024;   // partial sums: one double per wave

typedef float f32x16 __attribute__((ext_vector_type(16)));

// First kernel of a call: checks the init rows ON THE DEVICE. Out of range -> stop = 2, d_iters = -1 and nothing else is
// written by the call. Otherwise the control words are cleared and the history is filled with NaN ("not executed").
__global__ void __launch_bounds__(kBlock) kmeans_begin_kernel(const int* __restrict__ init_rows, int n, int k, int max_iter,
                                                              double* __restrict__ history, int* __restrict__ d_iters, int* __restrict__ ctrl) {
  const int tid = (int)threadIdx.x;
  int bad = 0;
  if (init_rows)
    for (int j = tid; j < k; j += kBlock) {
      const int r = init_rows[j];
      bad |= (r < 0 || r >= n);
    }
  bad = __syncthreads_or(bad);
  if (bad) {
    if (tid == 0) {
      ctrl[kCtlStop] = 2;
      *d_iters = -1;
    }
    return;
  }
  if (history)
    for (int t = tid; t < max_iter; t += kBlock) history[t] = (double)NAN;
  if (tid == 0) {
    ctrl[kCtlStop] = 0;
    ctrl[kCtlChanged] = 0;
    ctrl[kCtlIters] = 0;
    *d_iters = 0;
  }
}

// start centroids = the given rows
__global__ void __launch_bounds__(kBlock) kmeans_gather_kernel(const float* __restrict__ emb, int dim, const int* __restrict__ init_rows,
                                                               float* __restrict__ centroids, const int* __restrict__ ctrl) {
  if (ctrl[kCtlStop]) return;
  const int j = (int)blockIdx.x;
  const float4* src = reinterpret_cast<const float4*>(emb + (size_t)init_rows[j] * dim);
  float4* dst = reinterpret_cast<float4*>(centroids + (size_t)j * dim);
  for (int q = (int)threadIdx.x; q < dim / 4; q += kBlock) dst[q] = src[q];
}

// |c_j|^2, one wave per centroid: each lane an fmaf chain over its float4s in ascending order, then the xor tree.
// Workgroup 0 also clears the changed-label count of the iteration that starts here.
__global__ void __launch_bounds__(kBlock) kmeans_norms_kernel(const float* __restrict__ centroids, int k, int dim, float* __restrict__ cnorm,
                                                              int* __restrict__ ctrl) {
  if (ctrl[kCtlStop]) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) ctrl[kCtlChanged] = 0;
  const int lane = (int)threadIdx.x & (kWave - 1);
  const int j = (int)blockIdx.x * kWaves + (int)threadIdx.x / kWave;
  if (j >= k) return;
  const float* c = centroids + (size_t)j * dim;
  float acc = 0.f;
  for (int d = lane * 4; d < dim; d += kWave * 4) {
    const float4 v = *reinterpret_cast<const float4*>(c + d);
    acc = fmaf(v.x, v.x, acc);
    acc = fmaf(v.y, v.y, acc);
    acc = fmaf(v.z, v.z, acc);
    acc = fmaf(v.w, v.w, acc);
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
  if (lane == 0) cnorm[j] = acc;
}

// kTileR (or kTileC) rows x kTileD channels of a row-major [rows, dim] matrix into LDS, zeros outside the matrix.
__device__ __forceinline__ void stage_tile(const float* __restrict__ src, int rows, int dim, int r0, int d0, float* __restrict__ lds) {
#pragma unroll
  for (int i = 0; i < kTileR * kTileD / 4 / kBlock; ++i) {
    const int idx = (int)threadIdx.x + i * kBlock;
    const int r = idx / (kTileD / 4), q = idx % (kTileD / 4);
    const int gr = r0 + r, d = d0 + 4 * q;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gr < rows && d < dim) v = *reinterpret_cast<const float4*>(src + (size_t)gr * dim + d);   // dim % 4 == 0
    float* p = lds + r * kLds + 4 * q;
    p[0] = v.x;
    p[1] = v.y;
    p[2] = v.z;
    p[3] = v.w;
  }
}

// label[i] = argmin_j cnorm[j] - 2 <x_i, c_j>.  D = C_tile (A operand, 32 centroids) x X_tile^T (B operand, 32 rows):
// lane l holds A[centroid l&31][d + (l>>5)] and B[d + (l>>5)][row l&31]; the accumulator has the ROW on the lane (l&31) and
// the centroids (reg&3) + 8*(reg>>2) + 4*(l>>5) in its 16 registers, ascending with the register number. So the running
// minimum is per lane and in ascending centroid order (strict < keeps the lowest index), and one lexicographic
// (score, index) exchange between the two lane halves ends it.
__global__ void __launch_bounds__(kBlock) kmeans_assign_kernel(const float* __restrict__ emb, int n, int dim, const float* __restrict__ centroids,
                                                               int k, const float* __restrict__ cnorm, int* __restrict__ labels, int first,
                                                               int* __restrict__ ctrl) {
  if (ctrl[kCtlStop]) return;
  __shared__ float xs[kTileR * kLds];
  __shared__ float cs[kTileC * kLds];
  __shared__ float cn[kTileC];
  const int tid = (int)threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int r = lane & 31, h = lane >> 5;
  const int row0 = (int)blockIdx.x * kTileR;
  float best = INFINITY;
  int best_j = 0;
  for (int c0 = 0; c0 < k; c0 += kTileC) {
    const int tiles = min(kAccTiles, (k - c0 + 31) / 32);   // uniform: MFMA tiles of this chunk that hold a centroid
    f32x16 acc[kAccTiles];
#pragma unroll
    for (int t = 0; t < kAccTiles; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    for (int d0 = 0; d0 < dim; d0 += kTileD) {
      __syncthreads();   // the previous step's operand reads (and the previous chunk's cn reads) are done
      stage_tile(emb, n, dim, row0, d0, xs);
      stage_tile(centroids, k, dim, c0, d0, cs);
      if (d0 == 0 && tid < kTileC) cn[tid] = c0 + tid < k ? cnorm[c0 + tid] : 0.f;
      __syncthreads();
      const float* xb = xs + (wave * 32 + r) * kLds + h;
      const float* cb = cs + r * kLds + h;
#pragma unroll
      for (int kk = 0; kk < kTileD; kk += 2) {
        const float b = xb[kk];
#pragma unroll
        for (int t = 0; t < kAccTiles; ++t)
          if (t < tiles) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(cb[t * 32 * kLds + kk], b, acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < kAccTiles; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int jl = t * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        const float s = fmaf(-2.0f, acc[t][e], cn[jl]);
        if (c0 + jl < k && s < best) {
          best = s;
          best_j = c0 + jl;
        }
      }
  }
  const float ob = __shfl_xor(best, 32, kWave);
  const int oj = __shfl_xor(best_j, 32, kWave);
  if (ob < best || (ob == best && oj < best_j)) best_j = oj;
  const int row = row0 + wave * 32 + r;
  bool changed = false;
  if (h == 0 && row < n) {
    changed = first || labels[row] != best_j;
    labels[row] = best_j;
  }
  const unsigned long long m = __ballot(changed);
  if (lane == 0 && m) atomicAdd(&ctrl[kCtlChanged], __popcll(m));   // integer: the count does not depend on the order
}

// c_j = (sum of member rows, ascending row index) / count_j for channel blockIdx.y * kBlock + tid. The workgroup scans the
// label array kBlock entries at a time, compacts the members of cluster j in order into LDS, and every thread adds those
// rows' values of its channel. count_j == 0: the centroid is left as it is.
__global__ void __launch_bounds__(kBlock) kmeans_update_kernel(const float* __restrict__ emb, int n, int dim, const int* __restrict__ labels,
                                                               float* __restrict__ centroids, const int* __restrict__ ctrl) {
  if (ctrl[kCtlStop]) return;
  __shared__ int list[kBlock];
  __shared__ int wcnt[kWaves];
  const int tid = (int)threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int j = (int)blockIdx.x;
  const int ch = (int)blockIdx.y * kBlock + tid;
  float acc = 0.f;
  int count = 0;
  for (int base = 0; base < n; base += kBlock) {
    const int i = base + tid;
    const bool member = i < n && labels[i] == j;
    const unsigned long long m = __ballot(member);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int off = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) off += wcnt[w];
      total += wcnt[w];
    }
    if (member) list[off] = i;
    __syncthreads();
    if (ch < dim)
      for (int q = 0; q < total; ++q) acc += emb[(size_t)list[q] * dim + ch];
    count += total;
    __syncthreads();   // list / wcnt are rewritten by the next step
  }
  if (count > 0 && ch < dim) centroids[(size_t)j * dim + ch] = acc / (float)count;
}

// One wave per row: sum_d (x - c_label)^2 in double, lane-strided float4s, rows wave, wave + nwaves, ...; xor tree; one
// partial per wave.
__global__ void __launch_bounds__(kBlock) kmeans_inertia_kernel(const float* __restrict__ emb, int n, int dim, const int* __restrict__ labels,
                                                                const float* __restrict__ centroids, double* __restrict__ partial,
                                                                const int* __restrict__ ctrl) {
  if (ctrl[kCtlStop]) return;
  const int lane = (int)threadIdx.x & (kWave - 1);
  const int wave = ((int)blockIdx.x * kBlock + (int)threadIdx.x) / kWave;
  const int nwaves = (int)gridDim.x * kWaves;
  double acc = 0.0;
  for (int row = wave; row < n; row += nwaves) {
    const float* a = emb + (size_t)row * dim;
    const float* b = centroids + (size_t)labels[row] * dim;
    for (int d = lane * 4; d < dim; d += kWave * 4) {
      const float4 x = *reinterpret_cast<const float4*>(a + d);
      const float4 y = *reinterpret_cast<const float4*>(b + d);
      const double d0 = (double)x.x - (double)y.x, d1 = (double)x.y - (double)y.y;
      const double d2 = (double)x.z - (double)y.z, d3 = (double)x.w - (double)y.w;
      acc += d0 * d0;
      acc += d1 * d1;
      acc += d2 * d2;
      acc += d3 * d3;
    }
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
  if (lane == 0) partial[wave] = acc;
}

// Last kernel of an iteration, ONE workgroup: the partials in a fixed order -> history[iter]; iterations executed; and the
// only place the stop flag is set: no label changed -> every kernel enqueued behind this one returns at once.
__global__ void __launch_bounds__(kBlock) kmeans_finish_kernel(const double* __restrict__ partial, int npartial, int iter,
                                                               double* __restrict__ history, int* __restrict__ d_iters, int* __restrict__ ctrl) {
  if (ctrl[kCtlStop]) return;
  __shared__ double sm[kWaves];
  const int tid = (int)threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < npartial; i += kBlock) acc += partial[i];
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
  if ((tid & (kWave - 1)) == 0) sm[tid / kWave] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = sm[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += sm[w];
    if (history) history[iter] = s;
    const bool converged = ctrl[kCtlChanged] == 0;
    ctrl[kCtlIters] = iter + 1;
    *d_iters = (iter + 1) | (converged ? kConvergedBit : 0);
    if (converged) ctrl[kCtlStop] = 1;
  }
}

// ---- nearest rows (the reference's selection loop) ------------------------------------------------------------------
constexpr int kNrRowsPerWave = 8;
constexpr int kNrMaxBlocks = 8192;
constexpr int kNrArgBlock = 1024;

// One wave per row, kcenter_dist_kernel's direct form: dist[row] = sqrt(sum (a - b)^2) to centroid `step`. A row chosen by
// an earlier step holds -1 and keeps it; the row chosen last (read from device memory) gets it here.
__global__ void __launch_bounds__(kBlock) nearest_dist_kernel(const float* __restrict__ emb, int n, int dim, const float* __restrict__ centroids,
                                                              float* __restrict__ dist, const int* __restrict__ selected, int step) {
  const int lane = (int)threadIdx.x & (kWave - 1);
  const int wave = ((int)blockIdx.x * kBlock + (int)threadIdx.x) / kWave;
  const int nwaves = (int)gridDim.x * kWaves;
  const int last = step > 0 ? selected[step - 1] : -1;
  const float* b = centroids + (size_t)step * dim;
  for (int row = wave; row < n; row += nwaves) {
    const float* a = emb + (size_t)row * dim;
    float acc = 0.f;
    for (int j = lane * 4; j < dim; j += kWave * 4) {
      const float4 x = *reinterpret_cast<const float4*>(a + j);
      const float4 y = *reinterpret_cast<const float4*>(b + j);
      const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
      acc += d0 * d0;
      acc += d1 * d1;
      acc += d2 * d2;
      acc += d3 * d3;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
    if (lane == 0) {
      float d = sqrtf(acc);
      if (row == last || (step > 0 && dist[row] < 0.f)) d = -1.0f;
      dist[row] = d;
    }
  }
}

__device__ __forceinline__ bool nr_better(float v, int i, float bv, int bi) { return v < bv || (v == bv && i < bi); }

// arg-min of dist over the rows not chosen yet (-1 = chosen = the reference's inf), the LOWEST index winning ties (numpy's
// argmin); one workgroup, the result in device memory for the next step's launch.
__global__ void __launch_bounds__(kNrArgBlock) nearest_argmin_kernel(const float* __restrict__ dist, int n, int* __restrict__ selected, int step) {
  __shared__ float sv[kNrArgBlock / kWave];
  __shared__ int si[kNrArgBlock / kWave];
  const int tid = (int)threadIdx.x;
  float bv = INFINITY;
  int bi = INT_MAX;
  for (int i = tid; i < n; i += kNrArgBlock) {
    const float v = dist[i];
    if (v >= 0.f && nr_better(v, i, bv, bi)) {   // ascending i: an equal value never replaces an earlier one
      bv = v;
      bi = i;
    }
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, kWave);
    const int oi = __shfl_xor(bi, o, kWave);
    if (nr_better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if ((tid & (kWave - 1)) == 0) {
    sv[tid / kWave] = bv;
    si[tid / kWave] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kNrArgBlock / kWave; ++w)
      if (nr_better(sv[w], si[w], bv, bi)) {
        bv = sv[w];
        bi = si[w];
      }
    selected[step] = bi == INT_MAX ? 0 : bi;   // (all-NaN data: the next step must read a row that exists)
  }
}

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

int inertia_blocks(int n) {
  const int b = (n + 31) / 32;   // 8 rows per wave
  return b > kInertiaMaxBlocks ? kInertiaMaxBlocks : b;
}

bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace
}  // namespace unina

// workspace: [control words | |c|^2 of the k centroids | one inertia partial per wave]
extern "C" size_t unina_kmeans_workspace_bytes(int n, int dim, int k) {
  using namespace unina;
  if (n < 1 || dim < 4 || dim % 4 || k < 1 || k > n) return 0;
  return kCtlInts * sizeof(int) + align16(sizeof(float) * (size_t)k) + sizeof(double) * (size_t)inertia_blocks(n) * kWaves;
}

extern "C" int unina_kmeans(const float* d_embeddings, int n, int dim, int k, const int* d_init_rows, int max_iter, float* d_centroids,
                            int* d_labels, double* d_inertia_history, int* d_iters, void* d_workspace, hipStream_t stream) {
  using namespace unina;
  if (!d_embeddings || !d_centroids || !d_labels || !d_iters) return UNINA_ERR_ARG;
  if (n < 1 || dim < 4 || dim % 4 || k < 1 || k > n || max_iter < 1) return UNINA_ERR_ARG;
  if (misaligned(d_embeddings, 16) || misaligned(d_centroids, 16) || misaligned(d_workspace, 16) || misaligned(d_labels, 4) ||
      misaligned(d_init_rows, 4) || misaligned(d_iters, 4) || misaligned(d_inertia_history, 8))
    return UNINA_ERR_ARG;
  void* owned = nullptr;
  if (!d_workspace) {
    if (hipMalloc(&owned, unina_kmeans_workspace_bytes(n, dim, k)) != hipSuccess) return UNINA_ERR_HIP;
    d_workspace = owned;
  }
  int* ctrl = static_cast<int*>(d_workspace);
  float* cnorm = reinterpret_cast<float*>(ctrl + kCtlInts);
  double* partial = reinterpret_cast<double*>(reinterpret_cast<char*>(cnorm) + align16(sizeof(float) * (size_t)k));
  const int iblocks = inertia_blocks(n);
  hipLaunchKernelGGL(kmeans_begin_kernel, dim3(1), dim3(kBlock), 0, stream, d_init_rows, n, k, max_iter, d_inertia_history, d_iters, ctrl);
  if (d_init_rows)
    hipLaunchKernelGGL(kmeans_gather_kernel, dim3(k), dim3(kBlock), 0, stream, d_embeddings, dim, d_init_rows, d_centroids, ctrl);
  // every iteration is enqueued now; the stop flag turns the ones behind the converged one into empty launches
  for (int it = 0; it < max_iter; ++it) {
    hipLaunchKernelGGL(kmeans_norms_kernel, dim3((k + kWaves - 1) / kWaves), dim3(kBlock), 0, stream, d_centroids, k, dim, cnorm, ctrl);
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((n + kTileR - 1) / kTileR), dim3(kBlock), 0, stream, d_embeddings, n, dim, d_centroids, k,
                       cnorm, d_labels, it == 0 ? 1 : 0, ctrl);
    hipLaunchKernelGGL(kmeans_update_kernel, dim3(k, (dim + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, d_embeddings, n, dim, d_labels,
                       d_centroids, ctrl);
    hipLaunchKernelGGL(kmeans_inertia_kernel, dim3(iblocks), dim3(kBlock), 0, stream, d_embeddings, n, dim, d_labels, d_centroids, partial,
                       ctrl);
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3(1), dim3(kBlock), 0, stream, partial, iblocks * kWaves, it, d_inertia_history, d_iters,
                       ctrl);
  }
  hipError_t err = hipGetLastError();
  if (owned) {   // the call owns the workspace: it has to outlive the launches
    const hipError_t se = hipStreamSynchronize(stream);
    if (err == hipSuccess) err = se;
    (void)hipFree(owned);
  }
  return err == hipSuccess ? UNINA_OK : UNINA_ERR_HIP;
}

extern "C" int unina_nearest_rows(const float* d_embeddings, int n, int dim, const float* d_centroids, int k, int* d_selected,
                                  float* d_workspace, hipStream_t stream) {
  using namespace unina;
  if (!d_embeddings || !d_centroids || !d_selected) return UNINA_ERR_ARG;
  if (n < 1 || dim < 4 || dim % 4 || k < 1 || k > n) return UNINA_ERR_ARG;
  if (misaligned(d_embeddings, 16) || misaligned(d_centroids, 16) || misaligned(d_selected, 4) || misaligned(d_workspace, 4))
    return UNINA_ERR_ARG;
  float* owned = nullptr;
  if (!d_workspace) {
    if (hipMalloc(&owned, sizeof(float) * (size_t)n) != hipSuccess) return UNINA_ERR_HIP;
    d_workspace = owned;
  }
  const int waves = (n + kNrRowsPerWave - 1) / kNrRowsPerWave;
  int blocks = (waves + kWaves - 1) / kWaves;
  if (blocks > kNrMaxBlocks) blocks = kNrMaxBlocks;
  for (int step = 0; step < k; ++step) {
    hipLaunchKernelGGL(nearest_dist_kernel, dim3(blocks), dim3(kBlock), 0, stream, d_embeddings, n, dim, d_centroids, d_workspace, d_selected,
                       step);
    hipLaunchKernelGGL(nearest_argmin_kernel, dim3(1), dim3(kNrArgBlock), 0, stream, d_workspace, n, d_selected, step);
  }
  hipError_t err = hipGetLastError();
  if (owned) {
    const hipError_t se = hipStreamSynchronize(stream);
    if (err == hipSuccess) err = se;
    (void)hipFree(owned);
  }
  return err == hipSuccess ? UNINA_OK : UNINA_ERR_HIP;
}
