// calib.hip -- INT8 calibration on the device: exact |x| value counts of fp16 buffers (calib.h).
//
// counts[bits & 0x7fff] += 1 for every 16-bit element: +0 and -0 meet in bin 0, Inf / NaN patterns are counted like any other
// (the kernel does not interpret values). Counts are integers, so the table does not depend on scheduling: two runs give the
// same bytes and a row sums to its buffer's element count.
//
// Shape: one workgroup per CU with the WHOLE table in LDS (32 768 x 4 B = 128 KB of the CU's 160 KB), 16-byte loads of eight
// halves, LDS atomic adds, then the non-zero bins go to the global table with one global atomic each. Two things keep the LDS
// atomics from serialising on real activations: pattern 0 (about half of a post-ReLU buffer) is counted in a register and
// added once per wave, and a value that all live lanes of a wave share in one load slot (constant regions, padding channels)
// is added once with the lane count. The grid comes from the CU count and a minimum chunk per workgroup (calib_plan).
#include "calib.h"

#include <atomic>

#include "kernels.h"
#include "wave_block.h"

namespace unina {

namespace {

// One 15-bit pattern per lane; every lane of the wave calls this together (`ok`: the lane holds an element).
__device__ __forceinline__ void calib_add(unsigned h, bool ok, unsigned* bins, unsigned& zeros) {
  const unsigned long long live = __ballot(ok);
  if (live == 0) return;
  const unsigned first = (unsigned)__builtin_amdgcn_readlane((int)h, __ffsll((long long)live) - 1);
  const unsigned long long same = __ballot(ok && h == first);
  if (same == live) {   // one value in the whole wave: one add of the lane count
    if ((threadIdx.x & (kWave - 1)) == 0) {
      const unsigned c = (unsigned)__popcll(live);
      if (first == 0) zeros += c;
      else atomicAdd(&bins[first], c);
    }
  } else if (ok) {
    if (h == 0) ++zeros;
    else atomicAdd(&bins[h], 1u);
  }
}

// Workgroup `w` of descriptor `d`: its chunk into the LDS table, then the table into row d.row of `counts`.
__device__ __forceinline__ void calib_count(const CalibDesc& d, unsigned w, unsigned* bins, uint32_t* counts) {
  const unsigned tid = threadIdx.x;
  for (unsigned i = tid; i < kCalibBins / 4; i += kCalibBlock) reinterpret_cast<uint4*>(bins)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();

  const unsigned long long chunk = calib_chunk(d.n, d.nwg);
  const unsigned long long lo = (unsigned long long)w * chunk;   // multiple of 8
  const unsigned long long n8 = d.n & ~7ull;                     // elements in whole 16-byte vectors
  const unsigned long long hi8 = lo + chunk < n8 ? lo + chunk : n8;
  const unsigned long long v0 = lo / 8, v1 = hi8 / 8;            // this workgroup's vectors [v0, v1); empty when lo >= n8
  const uint4* src = static_cast<const uint4*>(d.ptr);
  unsigned zeros = 0;
  for (unsigned long long base = v0; base < v1; base += (unsigned long long)kCalibBlock * kCalibLoads) {   // uniform trip count
    uint4 q[kCalibLoads];
    bool ok[kCalibLoads];
#pragma unroll
    for (int u = 0; u < kCalibLoads; ++u) {
      const unsigned long long idx = base + (unsigned long long)u * kCalibBlock + tid;
      ok[u] = idx < v1;
      q[u] = ok[u] ? src[idx] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < kCalibLoads; ++u) {
      const unsigned wd[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        calib_add(wd[j] & 0x7fffu, ok[u], bins, zeros);
        calib_add((wd[j] >> 16) & 0x7fffu, ok[u], bins, zeros);
      }
    }
  }
  // the array's last n % 8 elements, by the workgroup whose chunk holds their vector slot
  if (tid < kWave) {
    const bool mine = n8 < d.n && lo <= n8 && n8 < lo + chunk;
    const bool ok = mine && n8 + tid < d.n;
    const unsigned h = ok ? (unsigned)static_cast<const unsigned short*>(d.ptr)[n8 + tid] & 0x7fffu : 0u;
    calib_add(h, ok, bins, zeros);
  }
  for (int o = kWave / 2; o > 0; o >>= 1) zeros += __shfl_xor(zeros, o, kWave);
  if ((tid & (kWave - 1)) == 0 && zeros) atomicAdd(&bins[0], zeros);
  __syncthreads();

  uint32_t* row = counts + (size_t)d.row * kCalibBins;
  for (unsigned b = tid; b < kCalibBins; b += kCalibBlock) {
    const unsigned c = bins[b];
    if (c) atomicAdd(&row[b], c);
  }
}

extern __shared__ unsigned calib_bins[];

__global__ __launch_bounds__(kCalibBlock) void calib_one_kernel(CalibDesc d, uint32_t* counts) {
  if (blockIdx.x >= d.nwg) return;
  calib_count(d, blockIdx.x, calib_bins, counts);
}

// Every buffer of a frame in one launch: the workgroup finds its descriptor in the prefix of first workgroups (wg0 ascending).
__global__ __launch_bounds__(kCalibBlock) void calib_table_kernel(const CalibDesc* tab, int count, uint32_t* counts) {
  int a = 0, b = count - 1;
  while (a < b) {
    const int m = (a + b + 1) / 2;
    if (tab[m].wg0 <= blockIdx.x) a = m;
    else b = m - 1;
  }
  const CalibDesc d = tab[a];
  if (blockIdx.x < d.wg0 || blockIdx.x - d.wg0 >= d.nwg) return;
  calib_count(d, blockIdx.x - d.wg0, calib_bins, counts);
}

struct CalibRow {
  const void* fn;
};
const CalibRow kCalib[] = {{reinterpret_cast<const void*>(calib_one_kernel)}, {reinterpret_cast<const void*>(calib_table_kernel)}};

constexpr int kMaxDevices = 64;
std::atomic<int> g_cus[kMaxDevices];   // CU count of each device, read once (0: not yet); set after the LDS limits are

// CU count of the current device; the first call on a device also raises the kernels' dynamic-LDS limit there.
int calib_cus() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
  int cus = g_cus[dev].load(std::memory_order_acquire);
  if (cus > 0) return cus;
  if (set_lds_limits(kCalib) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) return 0;
  g_cus[dev].store(cus, std::memory_order_release);
  return cus;
}

constexpr unsigned kCalibLds = kCalibBins * sizeof(unsigned);

}  // namespace

hipError_t calib_init() { return calib_cus() > 0 ? hipSuccess : hipErrorInvalidDevice; }

unsigned calib_plan(CalibDesc* descs, int count) {
  const int cus = calib_cus();
  if (cus < 1 || count < 1) return 0;
  unsigned long long total = 0;
  for (int i = 0; i < count; ++i) total += descs[i].n;
  unsigned long long per = (total + cus - 1) / cus;   // elements per workgroup at one workgroup per CU ...
  if (per < kCalibMinChunk) per = kCalibMinChunk;     // ... but never so few that the 32 768-bin flush dominates
  unsigned wg = 0;
  for (int i = 0; i < count; ++i) {
    const unsigned long long want = (descs[i].n + per - 1) / per;
    descs[i].wg0 = wg;
    descs[i].nwg = want < 1 ? 1u : (unsigned)want;
    descs[i].pad = 0;
    wg += descs[i].nwg;
  }
  return wg;
}

hipError_t calib_launch_one(const void* ptr, size_t n, uint32_t* counts, hipStream_t stream) {
  CalibDesc d = {ptr, n, 0, 0, 0, 0};
  const unsigned grid = calib_plan(&d, 1);
  if (!grid) return hipErrorInvalidDevice;
  hipLaunchKernelGGL(calib_one_kernel, dim3(grid), dim3(kCalibBlock), kCalibLds, stream, d, counts);
  return hipGetLastError();
}

hipError_t calib_launch_table(const CalibDesc* d_descs, int count, unsigned grid, uint32_t* counts, hipStream_t stream) {
  if (!d_descs || count < 1 || !grid || calib_cus() < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(calib_table_kernel, dim3(grid), dim3(kCalibBlock), kCalibLds, stream, d_descs, count, counts);
  return hipGetLastError();
}

}  // namespace unina

extern "C" int unina_abs_histogram_f16(const void* d_half, size_t n, uint32_t* d_counts, hipStream_t stream) {
  using namespace unina;
  if (!d_half || !d_counts || n == 0 || ((uintptr_t)d_half & 15) || ((uintptr_t)d_counts & 15)) return UNINA_ERR_ARG;
  if (hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * kCalibBins, stream) != hipSuccess) return UNINA_ERR_HIP;
  return calib_launch_one(d_half, n, d_counts, stream) == hipSuccess ? UNINA_OK : UNINA_ERR_HIP;
}
