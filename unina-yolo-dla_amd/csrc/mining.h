// mining.h -- launch parameters of the data-mining kernels (mining.hip), shared with the engine calls in engine.hip.
//
// Role in the reference: active_learning.py -- ActiveLearner.compute_difficulty_scores (:234-305), extract_backbone_embeddings
// (:31-99) and coreset_selection_kcenter (:104-163). The kernels run BEHIND the raw-head forward (unina_enqueue's launch
// sequence); the frame path (unina_infer*) never launches them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace unina {

constexpr int kMineBlock = 256;        // threads per workgroup of the score / pool kernels
constexpr int kGapChunk = 8;           // channels per thread of the pool kernel (one 16-byte fp16 load)
constexpr int kGapPixPerRow = 4;       // pixels each thread of the pool kernel sums before the workgroup combines
constexpr int kGapMaxChannels = 2048;  // LDS tile of the pool kernel: kMineBlock * kGapChunk floats

struct MineParams {
  // scores: the three fp32 planar cls planes [C,H,W]
  const float* cls[3];
  int cells[3];            // H*W of each level
  int num_classes;
  int blk0[4];             // first workgroup of each level in the score grid; blk0[3] = grid size
  float* score_partial;    // [blk0[3]][2]: per-workgroup (entropy max, loc_var max)
  float* scores;           // out: 8 floats (unina_mi355.h UNINA_MINE_SCORES)
  // embedding: a channel slice [coff, coff + c) of an NHWC activation buffer with `ctot` channels per pixel
  const void* src;         // nullptr: no embedding in this call
  long long lo_off;        // split-fp16 storage: byte distance from the hi plane to the lo plane
  int act;                 // element type: kernels.h kF16 / kF32 / kI8 / kS16
  float scale;             // int8 storage: value = code * scale
  int hw, ctot, coff, c;
  int strips;              // workgroups of the pool kernel
  float* gap_partial;      // [strips][c] column sums of each strip of pixels
  float* embed;            // out: c floats
};

// Geometry of the two grids for an engine: fills blk0 / strips of `p` from cells / num_classes / hw / c.
void mine_plan(MineParams* p);
// Floats of workspace the two partial arrays need together (score_partial first, gap_partial behind it, 16-byte aligned).
size_t mine_workspace_floats(const MineParams& p);
// mine_score_kernel (+ gap_embed_kernel when p.src) + mine_finish_kernel on `stream`.
hipError_t mine_launch(const MineParams& p, hipStream_t stream);

}  // namespace unina
