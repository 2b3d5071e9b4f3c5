// Do two streams run on the chip at the same time? (unina_debug_streams_overlap, include/unina_mi355.h debug section.)
//
// The HIP runtime maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES per priority, default 4); two streams that
// share a queue run strictly one after the other, however independent their work is. Nothing in the API reports the
// mapping, so this measures it: one single-wave kernel on each stream holds its compute unit for 300 us of the 100 MHz
// wall clock and stamps its start and end; the two intervals intersect exactly when the streams ran concurrently. The
// kernel waits on nothing but the clock (a probe that waits for its partner would never end on a shared queue), and an
// iteration cap ends it whatever the clock does.
#include <hip/hip_runtime.h>

#include "../../include/unina_mi355.h"

namespace unina {

constexpr long long kProbeTicks = 30000;   // 300 us at 100 MHz: far above the host's skew between the two launches
constexpr int kProbeIterCap = 1 << 20;     // a clock read takes >= tens of ns, so the time ends the loop long before this does
constexpr int kProbeMaxReps = 64;

__global__ void __launch_bounds__(64) stream_probe_kernel(long long* stamp) {
  const long long t0 = wall_clock64();
  long long t = t0;
  for (int i = 0; i < kProbeIterCap && t - t0 < kProbeTicks; ++i) t = wall_clock64();
  if (threadIdx.x == 0) {
    stamp[0] = t0;
    stamp[1] = t;
  }
}

}  // namespace unina

// stamps (host, reps x 4): start and end of the kernel on `a`, start and end of the kernel on `b`, per repetition.
// *overlapped = the number of repetitions whose two intervals intersect. a == b is the negative control: 0.
extern "C" int unina_debug_streams_overlap(int device, hipStream_t a, hipStream_t b, int reps, long long* stamps, int* overlapped) {
  if (!stamps || !overlapped || reps < 1 || reps > unina::kProbeMaxReps) return UNINA_ERR_ARG;
  *overlapped = 0;
  if (hipSetDevice(device) != hipSuccess) return UNINA_ERR_HIP;
  long long* d = nullptr;
  const size_t bytes = sizeof(long long) * 4 * (size_t)reps;
  if (hipMalloc(&d, bytes) != hipSuccess) return UNINA_ERR_HIP;
  hipError_t err = hipSuccess;
  for (int r = 0; r < reps && err == hipSuccess; ++r) {
    hipLaunchKernelGGL(unina::stream_probe_kernel, dim3(1), dim3(64), 0, a, d + 4 * r);
    err = hipGetLastError();
    if (err == hipSuccess) {
      hipLaunchKernelGGL(unina::stream_probe_kernel, dim3(1), dim3(64), 0, b, d + 4 * r + 2);
      err = hipGetLastError();
    }
    // (both, whatever the launches returned: nothing may still write d when it is freed)
    const hipError_t sa = hipStreamSynchronize(a), sb = hipStreamSynchronize(b);
    if (err == hipSuccess) err = sa != hipSuccess ? sa : sb;
  }
  if (err == hipSuccess) err = hipMemcpy(stamps, d, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (err != hipSuccess) return UNINA_ERR_HIP;
  for (int r = 0; r < reps; ++r) {
    const long long* s = stamps + 4 * r;
    const long long start = s[0] > s[2] ? s[0] : s[2], end = s[1] < s[3] ? s[1] : s[3];
    if (start < end) ++*overlapped;
  }
  return UNINA_OK;
}
