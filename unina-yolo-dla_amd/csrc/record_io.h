// record_io.h -- what every stage behind the frame does with the kept records (csrc/evalmatch.hip, locate.hip, stereo.hip,
// track.hip), one copy each: a record as 16-byte words, its vector loads and stores, the clamped device count, the check of the
// three device pointers and the status of a launch. A new record stage starts from here.
#ifndef UNINA_RECORD_IO_H
#define UNINA_RECORD_IO_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/unina_mi355.h"

namespace unina {

// a record and the 16-byte words it travels in (every record array of the ABI is 16-byte aligned)
template <typename T>
union RecordWords {
  static_assert(sizeof(T) % 16 == 0, "a record is whole 16-byte words");
  T r;
  uint4 q[sizeof(T) / 16];
};

template <typename T>
__device__ __forceinline__ RecordWords<T> load_record(const T* p) {
  RecordWords<T> w;
#pragma unroll
  for (size_t i = 0; i < sizeof(T) / 16; ++i) w.q[i] = reinterpret_cast<const uint4*>(p)[i];
  return w;
}

template <typename T>
__device__ __forceinline__ void store_record(T* p, const RecordWords<T>& w) {
#pragma unroll
  for (size_t i = 0; i < sizeof(T) / 16; ++i) reinterpret_cast<uint4*>(p)[i] = w.q[i];
}

template <typename T>
__device__ __forceinline__ void zero_record(RecordWords<T>& w) {
#pragma unroll
  for (size_t i = 0; i < sizeof(T) / 16; ++i) w.q[i] = make_uint4(0u, 0u, 0u, 0u);
}

template <typename T>
__device__ __forceinline__ void store_zero_record(T* p) {
  RecordWords<T> w;
  zero_record(w);
  store_record(p, w);
}

// the device count word as every stage reads it: 0 .. MAX_DETECTIONS
__device__ __forceinline__ int record_count(const int* d_count) {
  const int n = *d_count;
  return n < 0 ? 0 : (n > MAX_DETECTIONS ? MAX_DETECTIONS : n);
}

// host: the records, the count and a second record array (the stage's output, or the cones the tracker reads) are there and aligned
inline bool record_io_ok(const GpuDetection* d_dets, const int* d_count, const void* d_out) {
  return d_dets && d_count && d_out && !((uintptr_t)d_dets & 15) && !((uintptr_t)d_count & 3) && !((uintptr_t)d_out & 15);
}

// host: the answer of an entry point whose last act was a kernel launch
inline int launch_status() { return hipGetLastError() == hipSuccess ? UNINA_OK : UNINA_ERR_HIP; }

}  // namespace unina
#endif  // UNINA_RECORD_IO_H
