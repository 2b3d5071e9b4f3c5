// calib.h -- launch interface of the INT8 calibration kernel (calib.hip), shared with the engine calls in engine.hip.
//
// Role in the reference: the collection half of qat.py:171-220 `calibrate_model` (pytorch-quantization's HistogramCalibrator
// folding |x| of every quantizer input, 30 batches in train.py:809). An fp16 tensor has at most 32 768 distinct |x| (the sign
// bit drops out), so "how many elements carry each 15-bit pattern" is a LOSSLESS summary of it for everything a calibrator
// does with |x|; export.HistogramCalibrator.collect_counts folds such a table exactly as collect folds the tensor. The kernel
// runs BEHIND the raw-head forward (unina_enqueue's launch sequence); the frame path (unina_infer*) never launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace unina {

constexpr int kCalibBins = 32768;            // UNINA_CALIB_BINS: patterns of bits & 0x7fff
constexpr int kCalibBlock = 1024;            // threads per workgroup: one workgroup per CU (the table fills 128 KB of its LDS)
constexpr int kCalibLoads = 4;               // 16-byte loads each thread has in flight per loop step
constexpr size_t kCalibMinChunk = 1u << 17;  // elements per workgroup below which a buffer is not split further: the flush walks
                                             // all 32 768 LDS bins, 256 KB of input amortise it

// One array of a launch. A workgroup w of the grid belongs to the descriptor with wg0 <= w < wg0 + nwg and counts the elements
// [(w - wg0) * chunk, ... + chunk) of it, chunk = calib_chunk(n, nwg), into row `row` of the table.
struct CalibDesc {
  const void* ptr;          // fp16 elements, 16-byte aligned
  unsigned long long n;     // element count (any: tails are covered)
  unsigned row;             // row of counts[][kCalibBins] this array adds to
  unsigned wg0, nwg;        // first workgroup and number of workgroups (calib_plan)
  unsigned pad;
};

// Elements per workgroup: n split `nwg` ways, rounded up to whole 16-byte vectors.
__host__ __device__ inline unsigned long long calib_chunk(unsigned long long n, unsigned nwg) {
  return ((n + nwg - 1) / nwg + 7) & ~7ull;
}

hipError_t calib_init();   // LDS limit of the two kernels on the current device (kernels_init; the launchers also see to it)
// Fills wg0 / nwg of `count` descriptors (ptr / n / row given) from the current device's CU count; returns the grid size,
// 0 on error (a device query failed).
unsigned calib_plan(CalibDesc* descs, int count);
// One array: counts[0..kCalibBins) += pattern counts of the n elements at `ptr`. The table must be zero.
hipError_t calib_launch_one(const void* ptr, size_t n, uint32_t* counts, hipStream_t stream);
// `count` arrays in ONE launch: `d_descs` is the planned table in device memory, `grid` what calib_plan returned.
hipError_t calib_launch_table(const CalibDesc* d_descs, int count, unsigned grid, uint32_t* counts, hipStream_t stream);

}  // namespace unina
