// A LiDAR sweep de-skewed for the vehicle's motion on the device, in front of unina_ground_filter_async, unina_cluster_async or
// unina_locate_lidar_async (include/unina_mi355.h "motion de-skew of a LiDAR sweep"; deskew.table_numpy and deskew.deskew_numpy are
// the definition, bit for bit). The call is stateless: it reads the cloud and the point times and writes a cloud of 16-byte points
// and a header. The arithmetic of both halves is csrc/deskew_math.h, the cloud's plumbing csrc/cloud_io.h.
//
// Host half. The K poses (float64, absolute stamps, odometry coordinates) become K float32 rows relative to the pose at t_ref:
// deskew_table, before any HIP call. The rows travel in the kernel arguments by value (64 x 32 bytes + the rest, below the 4 KB
// a launch carries), so the call needs no upload, no workspace and no handle.
//
// Device half. N points (30 000 .. 260 000 a sweep), one memset of the header and ONE kernel: a thread per point, workgroups of
// kDeskewBlock.
//   table    each workgroup first copies the rows into 2.25 KB of LDS (the argument segment is memory: 2 x n_keys threads load 16
//            bytes of it each, by their own index). A point reads the table at a divergent index, seven probes and four half rows:
//            LDS serves that, the arguments would serve it as global loads. The key times get an array of their own, so the
//            probes of the bisection read neighbouring words; the lanes of a wave are neighbours in time and mostly share a
//            segment, so the probes and the two rows of a segment (two 16-byte LDS reads each) broadcast.
//   point    one 16-byte load where the base and the stride allow it, three dwords otherwise; the time word and the carried word
//            are one dword each, from the cache line the point came from unless the times are a plane. About 60 fp32
//            operations, one square root and five divides: nothing beside the 32 .. 68 bytes a point moves. One 16-byte store.
//   header   counts are folded per wave with a ballot and a popcount, the shift with six shuffles, then per workgroup in four LDS
//            words; thread 0 sends one integer atomic per non-zero value. All atomics of a call land on one 32-byte line and are
//            served one after the other (about 10 ns each), so they are kept few: n_moved is n_points minus the invalid points --
//            workgroup 0 adds n_points, a workgroup with invalid points takes its count off -- and the maximum is sent only
//            where a load finds a smaller one. A sweep without invalid or out-of-range points sends at most one atomic a
//            workgroup. With one atomic per wave and counter (8 126 on 260 000 points) a call took 0.097 ms; folded, 0.019 ms at 30 000
//            and at 260 000 points, which is the rate at which the host enqueues the memset and the kernel (tools/bench_deskew.py).
// Every counter is an integer and the maximum is over unsigned bit patterns; a float is never combined atomically. So two runs
// give the same bytes, and a permuted cloud the same header and the permuted points.
#include <hip/hip_runtime.h>

#include "deskew_math.h"
#include "record_io.h"
#include "wave_block.h"

namespace unina {
namespace {

constexpr int kDeskewBlock = 256;   // threads, and points, of a workgroup
enum { kFoldInvalid, kFoldBefore, kFoldAfter, kFoldShift, kFoldWords };   // what a workgroup folds in LDS before it goes to the header
static_assert(kDeskewBlock % kWave == 0 && kDeskewBlock >= 2 * kDeskewMaxKeys, "whole waves; a thread copies at most one 16-byte half row");

struct DeskewArgs {
  const unsigned char* points;
  const unsigned char* times;
  const unsigned char* carry;   // points + carry_offset, or nullptr
  uint4* out;
  unina_deskew_header* header;
  int n, stride, time_stride, format, n_keys;
  unina_deskew_key keys[kDeskewMaxKeys];
};
static_assert(sizeof(DeskewArgs) <= 4096, "the table travels in the kernel arguments");

template <bool VEC>
__global__ void __launch_bounds__(kDeskewBlock) deskew_kernel(DeskewArgs a) {
  __shared__ __align__(16) float s_keys[kDeskewMaxKeys * 8];
  __shared__ float s_t[kDeskewMaxKeys];
  __shared__ uint32_t s_fold[kFoldWords];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1);
  if (tid < kFoldWords) s_fold[tid] = 0u;
  if (tid < 2 * a.n_keys) {   // n_keys <= kDeskewMaxKeys: checked by the host
    const unina_deskew_key& key = a.keys[tid >> 1];
    const float4 half = (tid & 1) ? make_float4(key.px, key.py, key.pz, key.t) : make_float4(key.qw, key.qx, key.qy, key.qz);
    reinterpret_cast<float4*>(s_keys)[tid] = half;
    if (tid & 1) s_t[tid >> 1] = key.t;
  }
  __syncthreads();

  const int i = (int)blockIdx.x * kDeskewBlock + tid;   // < 2^22 + 256
  const bool live = i < a.n;                            // a thread behind the cloud still takes part in the ballots and shuffles
  DeskewPoint p;
  p.x = p.y = p.z = kDeskewNaN;
  p.shift2 = 0u;
  p.invalid = p.before = p.after = 0;
  if (live) {
    uint32_t x, y, z;
    load_xyz<VEC>(a.points, i, a.stride, &x, &y, &z);
    const uint32_t time_word = *reinterpret_cast<const uint32_t*>(a.times + (size_t)i * (size_t)a.time_stride);
    const uint32_t carry = a.carry ? *reinterpret_cast<const uint32_t*>(a.carry + (size_t)i * (size_t)a.stride) : kDeskewNaN;
    p = deskew_point(s_t, s_keys, a.n_keys, a.format, x, y, z, time_word);
    a.out[i] = make_uint4(p.x, p.y, p.z, p.invalid ? kDeskewNaN : carry);
  }
  // the fold: per wave a ballot and a popcount, or six shuffles; per workgroup four LDS words; then thread 0 alone goes to the header
  const int n_invalid = __popcll(__ballot(live && p.invalid));
  const int n_before = __popcll(__ballot(p.before != 0));
  const int n_after = __popcll(__ballot(p.after != 0));
  uint32_t shift = p.shift2;
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)shift, o, kWave);
    shift = other > shift ? other : shift;
  }
  if (lane == 0) {
    if (n_invalid) atomicAdd(&s_fold[kFoldInvalid], (uint32_t)n_invalid);
    if (n_before) atomicAdd(&s_fold[kFoldBefore], (uint32_t)n_before);
    if (n_after) atomicAdd(&s_fold[kFoldAfter], (uint32_t)n_after);
    if (shift) atomicMax(&s_fold[kFoldShift], shift);
  }
  __syncthreads();
  if (tid == 0) {
    unina_deskew_header* h = a.header;
    if (blockIdx.x == 0) {
      h->n_points = a.n;
      atomicAdd(&h->n_moved, a.n);   // n_moved = n_points - n_invalid: the workgroups that hold invalid points take theirs off
    }
    if (const int v = (int)s_fold[kFoldInvalid]) {
      atomicSub(&h->n_moved, v);
      atomicAdd(&h->n_invalid, v);
    }
    if (const int v = (int)s_fold[kFoldBefore]) atomicAdd(&h->n_before, v);
    if (const int v = (int)s_fold[kFoldAfter]) atomicAdd(&h->n_after, v);
    // a maximum that is already there needs no atomic; the load only saves work, the result is the maximum either way
    const uint32_t m = s_fold[kFoldShift];
    if (m && m > __hip_atomic_load(&h->max_shift2_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&h->max_shift2_bits, m);
  }
}

struct Span {
  uintptr_t lo, hi;
};
bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }

bool times_ok(const unina_point_times* t, int n_points) {
  if (!t || (n_points > 0 && !t->t) || ((uintptr_t)t->t & 3)) return false;
  if (t->stride < 4 || t->stride % 4 != 0) return false;
  return t->format == UNINA_TIME_F32_S || t->format == UNINA_TIME_U32_NS;
}

}  // namespace
}  // namespace unina

extern "C" int unina_deskew_table(const unina_deskew_pose* poses, int n_keys, double t_sweep, double t_ref, unina_deskew_key* out) {
  return unina::deskew_table(poses, n_keys, t_sweep, t_ref, out);
}

extern "C" int unina_deskew_async(const unina_cloud* cloud, const unina_point_times* times, int carry_offset, const unina_deskew_pose* poses,
                                  int n_keys, double t_sweep, double t_ref, void* d_out, unina_deskew_header* d_header, hipStream_t stream) {
  using namespace unina;
  if (!d_out || !d_header || ((uintptr_t)d_out & 15) || ((uintptr_t)d_header & 3)) return UNINA_ERR_ARG;
  if (!cloud_ok(cloud, kCloudMaxPoints) || !times_ok(times, cloud->n_points)) return UNINA_ERR_ARG;
  if (carry_offset != -1 && (carry_offset < 12 || carry_offset % 4 != 0 || carry_offset > cloud->stride - 4)) return UNINA_ERR_ARG;
  const int n = cloud->n_points;
  if (n > 0) {
    const uintptr_t un = (uintptr_t)n;
    const Span out{(uintptr_t)d_out, (uintptr_t)d_out + un * 16u};
    const Span in{(uintptr_t)cloud->points, (uintptr_t)cloud->points + un * (uintptr_t)cloud->stride};
    const Span tm{(uintptr_t)times->t, (uintptr_t)times->t + (un - 1u) * (uintptr_t)times->stride + 4u};
    const Span hd{(uintptr_t)d_header, (uintptr_t)d_header + sizeof(unina_deskew_header)};
    if (overlap(out, in) || overlap(out, tm) || overlap(out, hd)) return UNINA_ERR_ARG;
  }
  DeskewArgs args;
  if (const int rc = deskew_table(poses, n_keys, t_sweep, t_ref, args.keys)) return rc;
  for (int k = n_keys; k < kDeskewMaxKeys; ++k) args.keys[k] = unina_deskew_key{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};

  if (hipMemsetAsync(d_header, 0, sizeof(unina_deskew_header), stream) != hipSuccess) return UNINA_ERR_HIP;
  if (n == 0) return UNINA_OK;
  args.points = static_cast<const unsigned char*>(cloud->points);
  args.times = static_cast<const unsigned char*>(times->t);
  args.carry = carry_offset < 0 ? nullptr : args.points + carry_offset;
  args.out = static_cast<uint4*>(d_out);
  args.header = d_header;
  args.n = n;
  args.stride = cloud->stride;
  args.time_stride = times->stride;
  args.format = times->format;
  args.n_keys = n_keys;
  UNINA_LAUNCH_VEC(cloud_vec16(cloud), deskew_kernel, dim3((unsigned)((n + kDeskewBlock - 1) / kDeskewBlock)), dim3(kDeskewBlock), stream, args);
  return launch_status();
}
