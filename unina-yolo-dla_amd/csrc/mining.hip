// mining.hip -- the data-mining path: per-image difficulty scores, the P4 embedding and k-center greedy selection.
//
// Role in the reference (active_learning.py):
//   mine_score_kernel ...... ActiveLearner.compute_difficulty_scores        :234-305 (modes "entropy" and "loc_var")
//   gap_embed_kernel ....... extract_backbone_embeddings                    :31-99   (adaptive_avg_pool2d of features[2])
//   kcenter_*_kernel ....... coreset_selection_kcenter                      :104-163 (the numpy loop, one step per launch pair)
//
// Everything here is plain fp32 in the order the reference writes it (the unit is compiled with -ffp-contract=off), every
// reduction has a fixed order (no float atomics), so two runs give identical bits. All three are memory-bound: 0.54 MB of
// logits and 0.82 MB of P4 per 640x640 frame, n * dim * 4 bytes of embeddings per k-center step.
#include "mining.h"

#include "kernels.h"
#include "wave_block.h"

namespace unina {
namespace {

constexpr int kWaves = kMineBlock / kWave;

// The max of the scores is numpy's / torch's, which KEEPS a NaN operand; fmaxf drops it. For NaN-free operands this is fmaxf,
// bit for bit, so a level that holds a NaN logit reports NaN and every other result is unchanged.
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = max_nan(v, __shfl_xor(v, o, kWave));
  return v;
}

// max over the workgroup; valid in thread 0. `sm`: kWaves floats of LDS.
__device__ __forceinline__ float block_max(float v, float* sm) {
  v = wave_max(v);
  __syncthreads();   // (sm may still be read from an earlier call)
  if ((threadIdx.x & (kWave - 1)) == 0) sm[threadIdx.x / kWave] = v;
  __syncthreads();
  float r = sm[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) r = max_nan(r, sm[w]);
  return r;
}

// One thread per cell of one level: binary entropy of every class (max) and 1 - |max_c p_c - 0.5| * 2, both as the reference
// computes them (active_learning.py:287-301). Every value is >= 0 or NaN, so 0 is the neutral element of the max (idle threads);
// a NaN logit makes the cell's entropy, its conf and with it its loc_var NaN, and max_nan carries that to the level's scores.
__global__ void __launch_bounds__(kMineBlock) mine_score_kernel(MineParams p) {
  __shared__ float sm[kWaves];
  const int b = (int)blockIdx.x;
  const int level = b >= p.blk0[2] ? 2 : (b >= p.blk0[1] ? 1 : 0);
  const int cells = p.cells[level];
  const int cell = (b - p.blk0[level]) * kMineBlock + (int)threadIdx.x;
  float ent = 0.f, loc = 0.f;
  if (cell < cells) {
    const float* x = p.cls[level] + cell;
    float conf = 0.f;   // probabilities are > 0
    for (int c = 0; c < p.num_classes; ++c) {
      const float v = x[(size_t)c * cells];
      const float pr = 1.0f / (1.0f + expf(-v));
      const float e = -(pr * logf(pr + 1e-10f) + (1.0f - pr) * logf(1.0f - pr + 1e-10f));
      ent = max_nan(ent, e);
      conf = max_nan(conf, pr);
    }
    loc = 1.0f - fabsf(conf - 0.5f) * 2.0f;
  }
  const float be = block_max(ent, sm);
  const float bl = block_max(loc, sm);
  if (threadIdx.x == 0) {
    p.score_partial[2 * b] = be;
    p.score_partial[2 * b + 1] = bl;
  }
}

// 8 channels of one pixel as fp32, decoded exactly as unina_debug_read_buffer does it on the host.
template <int ACT>
__device__ __forceinline__ void load8(const MineParams& p, size_t elem, float* v) {
  if constexpr (ACT == kF16 || ACT == kS16) {
    const uint4 q = *reinterpret_cast<const uint4*>(static_cast<const char*>(p.src) + elem * 2);
    const _Float16* h = reinterpret_cast<const _Float16*>(&q);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
    if constexpr (ACT == kS16) {   // value = hi + lo
      const uint4 ql = *reinterpret_cast<const uint4*>(static_cast<const char*>(p.src) + p.lo_off + elem * 2);
      const _Float16* l = reinterpret_cast<const _Float16*>(&ql);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = v[i] + (float)l[i];
    }
  } else if constexpr (ACT == kF32) {
    const float4 a = *reinterpret_cast<const float4*>(static_cast<const char*>(p.src) + elem * 4);
    const float4 b = *reinterpret_cast<const float4*>(static_cast<const char*>(p.src) + elem * 4 + 16);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {   // int8 codes
    const uint2 q = *reinterpret_cast<const uint2*>(static_cast<const char*>(p.src) + elem);
    const signed char* s = reinterpret_cast<const signed char*>(&q);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)s[i] * p.scale;
  }
}

// Column sums of one strip of pixels. NHWC makes the pool a column sum: thread (row r, chunk g) adds kGapPixPerRow pixels of
// channels [8g, 8g + 8), then the rows of the workgroup are added in row order. Fixed order throughout.
template <int ACT>
__global__ void __launch_bounds__(kMineBlock) gap_embed_kernel(MineParams p) {
  __shared__ float sm[kGapMaxChannels];
  const int chunks = p.c / kGapChunk;
  const int rows = kMineBlock / chunks;
  const int tid = (int)threadIdx.x;
  const int g = tid % chunks, r = tid / chunks;
  if (r < rows) {
    float acc[kGapChunk];
#pragma unroll
    for (int i = 0; i < kGapChunk; ++i) acc[i] = 0.f;
    const int p0 = (int)blockIdx.x * rows * kGapPixPerRow;
#pragma unroll
    for (int k = 0; k < kGapPixPerRow; ++k) {
      const int pix = p0 + k * rows + r;
      if (pix < p.hw) {
        float v[kGapChunk];
        load8<ACT>(p, (size_t)pix * p.ctot + p.coff + g * kGapChunk, v);
#pragma unroll
        for (int i = 0; i < kGapChunk; ++i) acc[i] += v[i];
      }
    }
#pragma unroll
    for (int i = 0; i < kGapChunk; ++i) sm[r * p.c + g * kGapChunk + i] = acc[i];
  }
  __syncthreads();
  for (int ch = tid; ch < p.c; ch += kMineBlock) {
    float s = sm[ch];
    for (int k = 1; k < rows; ++k) s += sm[k * p.c + ch];
    p.gap_partial[(size_t)blockIdx.x * p.c + ch] = s;
  }
}

// Second stage of both reductions: workgroup 0 -> the 8 scores, workgroups 1.. -> the embedding (strip sums in strip order,
// divided by the pixel count as adaptive_avg_pool2d does).
__global__ void __launch_bounds__(kMineBlock) mine_finish_kernel(MineParams p) {
  __shared__ float sm[kWaves];
  const int tid = (int)threadIdx.x;
  if (blockIdx.x == 0) {
    float out[6];
    for (int level = 0; level < 3; ++level) {
      float ent = 0.f, loc = 0.f;
      for (int b = p.blk0[level] + tid; b < p.blk0[level + 1]; b += kMineBlock) {
        ent = max_nan(ent, p.score_partial[2 * b]);
        loc = max_nan(loc, p.score_partial[2 * b + 1]);
      }
      out[level] = block_max(ent, sm);
      out[3 + level] = block_max(loc, sm);
    }
    if (tid == 0) {
      for (int i = 0; i < 6; ++i) p.scores[i] = out[i];
      p.scores[6] = max_nan(max_nan(out[0], out[1]), out[2]);
      p.scores[7] = max_nan(max_nan(out[3], out[4]), out[5]);
    }
    return;
  }
  const int ch = ((int)blockIdx.x - 1) * kMineBlock + tid;
  if (ch >= p.c) return;
  float s = p.gap_partial[ch];
  for (int k = 1; k < p.strips; ++k) s += p.gap_partial[(size_t)k * p.c + ch];
  p.embed[ch] = s / (float)p.hw;
}

// ---- k-center greedy -------------------------------------------------------------------------------------------------
constexpr int kKcRowsPerWave = 8;
constexpr int kKcMaxBlocks = 8192;
constexpr int kKcArgBlock = 1024;

__global__ void kcenter_init_kernel(int* selected, int first) {
  if (threadIdx.x == 0 && blockIdx.x == 0) selected[0] = first;
}

// One wave per row: d = sqrt(sum (a - b)^2) to the row chosen last (read from device memory), min_dist = min(min_dist, d),
// the chosen row forced to -1 (rows chosen earlier already hold -1 and min keeps it). step 1 has no earlier min_dist (inf).
template <bool VEC4>
__global__ void __launch_bounds__(kMineBlock) kcenter_dist_kernel(const float* __restrict__ emb, int n, int dim, float* __restrict__ min_dist,
                                                                  const int* __restrict__ selected, int step) {
  const int lane = (int)threadIdx.x & (kWave - 1);
  const int wave = ((int)blockIdx.x * kMineBlock + (int)threadIdx.x) / kWave;
  const int nwaves = (int)gridDim.x * kWaves;
  const int last = selected[step - 1];
  const float* b = emb + (size_t)last * dim;
  for (int row = wave; row < n; row += nwaves) {
    const float* a = emb + (size_t)row * dim;
    float acc = 0.f;
    if constexpr (VEC4) {
      for (int j = lane * 4; j < dim; j += kWave * 4) {
        const float4 x = *reinterpret_cast<const float4*>(a + j);
        const float4 y = *reinterpret_cast<const float4*>(b + j);
        const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
        acc += d0 * d0;
        acc += d1 * d1;
        acc += d2 * d2;
        acc += d3 * d3;
      }
    } else {
      for (int j = lane; j < dim; j += kWave) {
        const float d = a[j] - b[j];
        acc += d * d;
      }
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
    if (lane == 0) {
      const float d = sqrtf(acc);
      float md = step == 1 ? d : fminf(min_dist[row], d);
      if (row == last) md = -1.0f;
      min_dist[row] = md;
    }
  }
}

// arg-max of min_dist, the LOWEST index winning ties (numpy's argmax): one workgroup, so the result is in device memory
// for the next step's launch without a host round-trip.
__device__ __forceinline__ bool kc_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__global__ void __launch_bounds__(kKcArgBlock) kcenter_argmax_kernel(const float* __restrict__ min_dist, int n, int* __restrict__ selected, int step) {
  __shared__ float sv[kKcArgBlock / kWave];
  __shared__ int si[kKcArgBlock / kWave];
  const int tid = (int)threadIdx.x;
  float bv = -2.0f;   // below every stored value (distances >= 0, chosen rows -1)
  int bi = 0;          // (all-NaN data selects row 0: the next step must read a row that exists)
  for (int i = tid; i < n; i += kKcArgBlock) {
    const float v = min_dist[i];
    if (v > bv) {   // ascending i: strict > keeps the lowest index
      bv = v;
      bi = i;
    }
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, kWave);
    const int oi = __shfl_xor(bi, o, kWave);
    if (kc_better(ov, oi, bv, bi)) {
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
    for (int w = 1; w < kKcArgBlock / kWave; ++w)
      if (kc_better(sv[w], si[w], bv, bi)) {
        bv = sv[w];
        bi = si[w];
      }
    selected[step] = bi;
  }
}

}  // namespace

void mine_plan(MineParams* p) {
  int b = 0;
  for (int l = 0; l < 3; ++l) {
    p->blk0[l] = b;
    b += (p->cells[l] + kMineBlock - 1) / kMineBlock;
  }
  p->blk0[3] = b;
  p->strips = 0;
  if (p->c > 0) {
    const int rows = kMineBlock / (p->c / kGapChunk);
    const int per = rows * kGapPixPerRow;
    p->strips = (p->hw + per - 1) / per;
  }
}

size_t mine_workspace_floats(const MineParams& p) {
  const size_t score = ((size_t)2 * p.blk0[3] + 3) & ~(size_t)3;
  return score + (size_t)p.strips * p.c;
}

hipError_t mine_launch(const MineParams& p, hipStream_t stream) {
  if (p.blk0[3] < 1 || p.num_classes < 1 || !p.score_partial || !p.scores) return hipErrorInvalidValue;
  const bool embed = p.src != nullptr;
  if (embed) {
    // the pool kernel's 16-byte (int8: 8-byte) chunks and its LDS tile
    if (p.c < kGapChunk || p.c % kGapChunk || p.coff % kGapChunk || p.ctot % kGapChunk || p.c > kGapMaxChannels ||
        p.coff + p.c > p.ctot || p.hw < 1 || p.strips < 1 || !p.gap_partial || !p.embed)
      return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(mine_score_kernel, dim3(p.blk0[3]), dim3(kMineBlock), 0, stream, p);
  if (embed) {
    const dim3 grid(p.strips), block(kMineBlock);
    switch (p.act) {
      case kF16: hipLaunchKernelGGL(gap_embed_kernel<kF16>, grid, block, 0, stream, p); break;
      case kS16: hipLaunchKernelGGL(gap_embed_kernel<kS16>, grid, block, 0, stream, p); break;
      case kF32: hipLaunchKernelGGL(gap_embed_kernel<kF32>, grid, block, 0, stream, p); break;
      case kI8: hipLaunchKernelGGL(gap_embed_kernel<kI8>, grid, block, 0, stream, p); break;
      default: return hipErrorInvalidValue;
    }
  }
  const int finish = 1 + (embed ? (p.c + kMineBlock - 1) / kMineBlock : 0);
  hipLaunchKernelGGL(mine_finish_kernel, dim3(finish), dim3(kMineBlock), 0, stream, p);
  return hipGetLastError();
}

}  // namespace unina

extern "C" int unina_kcenter(const float* d_embeddings, int n, int dim, int k, int first_index, int* d_selected, float* d_min_dist,
                             hipStream_t stream) {
  using namespace unina;
  if (!d_embeddings || !d_selected || n < 1 || dim < 1 || k < 1 || k > n || first_index < 0 || first_index >= n) return UNINA_ERR_ARG;
  if (((uintptr_t)d_embeddings & 15) || ((uintptr_t)d_selected & 3) || ((uintptr_t)d_min_dist & 3)) return UNINA_ERR_ARG;
  float* owned = nullptr;
  if (!d_min_dist && k > 1) {
    if (hipMalloc(&owned, sizeof(float) * (size_t)n) != hipSuccess) return UNINA_ERR_HIP;
    d_min_dist = owned;
  }
  hipLaunchKernelGGL(kcenter_init_kernel, dim3(1), dim3(kWave), 0, stream, d_selected, first_index);
  const int waves = (n + kKcRowsPerWave - 1) / kKcRowsPerWave;
  int blocks = (waves + kWaves - 1) / kWaves;
  if (blocks > kKcMaxBlocks) blocks = kKcMaxBlocks;
  const bool vec4 = dim % 4 == 0;
  for (int step = 1; step < k; ++step) {
    if (vec4)
      hipLaunchKernelGGL(kcenter_dist_kernel<true>, dim3(blocks), dim3(kMineBlock), 0, stream, d_embeddings, n, dim, d_min_dist, d_selected, step);
    else
      hipLaunchKernelGGL(kcenter_dist_kernel<false>, dim3(blocks), dim3(kMineBlock), 0, stream, d_embeddings, n, dim, d_min_dist, d_selected, step);
    hipLaunchKernelGGL(kcenter_argmax_kernel, dim3(1), dim3(kKcArgBlock), 0, stream, d_min_dist, n, d_selected, step);
  }
  hipError_t err = hipGetLastError();
  if (owned) {   // the call owns the workspace: it has to outlive the launches
    const hipError_t se = hipStreamSynchronize(stream);
    if (err == hipSuccess) err = se;
    (void)hipFree(owned);
  }
  return err == hipSuccess ? UNINA_OK : UNINA_ERR_HIP;
}
