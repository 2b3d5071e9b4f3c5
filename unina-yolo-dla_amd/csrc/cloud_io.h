// cloud_io.h -- what every stage that reads a unina_cloud does with it (csrc/lidar.hip, ground.hip, cluster.hip), one copy each: the limit
// of a sweep, one row of an extrinsic applied to a point, the float/bits casts, the checks of the cloud and the extrinsic; then,
// for hipcc alone (the stand-alone programs under tests/ compile the first half without HIP): the loads of a point, the launch
// of a kernel's 16-byte-load form, the workspace of a handle. Every unit that includes it is compiled with -ffp-contract=off.
// A new sweep stage starts from here.
#ifndef UNINA_CLOUD_IO_H
#define UNINA_CLOUD_IO_H

#include <stdint.h>
#include <string.h>

#if !defined(__HIPCC__) && !defined(UNINA_NO_HIP_HEADERS)
#define UNINA_NO_HIP_HEADERS   // a host compiler takes unina_cloud from the public header without HIP's
#endif
#include "../../include/unina_mi355.h"
#include "hd.h"

namespace unina {

constexpr int kCloudMaxPoints = 1 << 22;
static_assert(kCloudMaxPoints == UNINA_LIDAR_MAX_POINTS, "header limits");

// one row (r0, r1, r2, t) of a row-major 3 x 4 [R|t] applied to a point of the LiDAR frame
UNINA_HD float cloud_transform_row(const float* row, float x, float y, float z) { return ((row[0] * x + row[1] * y) + row[2] * z) + row[3]; }

UNINA_HD uint32_t float_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
UNINA_HD float bits_float(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

// host: what a create call that bounds its workspace by a sweep accepts
inline bool cloud_limits_ok(int device_id, int max_points) { return device_id >= 0 && max_points >= 1 && max_points <= kCloudMaxPoints; }

// host: the checks every entry point that takes a cloud shares; it adds its own and touches HIP only after the last has passed
inline bool cloud_ok(const unina_cloud* c, int max_points) {
  if (!c || c->n_points < 0 || c->n_points > max_points || (c->n_points > 0 && !c->points)) return false;
  return !(c->stride < 12 || c->stride % 4 != 0 || ((uintptr_t)c->points & 3));
}

inline bool extrinsic_ok(const float m[12]) {
  for (int i = 0; m && i < 12; ++i)
    if (!finite(m[i])) return false;
  return m != nullptr;
}

// host: every point of the cloud can be read with one 16-byte load
inline bool cloud_vec16(const unina_cloud* c) { return c->stride % 16 == 0 && ((uintptr_t)c->points & 15) == 0; }

#if defined(__HIPCC__)
// the three words of point i: one 16-byte load where cloud_vec16 holds (VEC), three dwords otherwise
template <bool VEC>
__device__ __forceinline__ void load_xyz(const unsigned char* __restrict__ points, int i, int stride, uint32_t* x, uint32_t* y, uint32_t* z) {
  const unsigned char* src = points + (size_t)i * (size_t)stride;
  if (VEC) {
    const uint4 q = *reinterpret_cast<const uint4*>(src);
    *x = q.x; *y = q.y; *z = q.z;
  } else {
    const uint32_t* f = reinterpret_cast<const uint32_t*>(src);
    *x = f[0]; *y = f[1]; *z = f[2];
  }
}

// host: the one launch of a `template <bool VEC>` kernel: kernel<true> where vec, kernel<false> otherwise
#define UNINA_LAUNCH_VEC(vec, kernel, grid, block, stream, ...)                    \
  do {                                                                            \
    if (vec) hipLaunchKernelGGL(kernel<true>, grid, block, 0, stream, __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel<false>, grid, block, 0, stream, __VA_ARGS__);    \
  } while (0)

// host: the arrays of a workspace one behind the other from `base` (hipMalloc's: 256-byte aligned); `at` ends as their bytes
inline size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }
template <typename T>
T* carve(uintptr_t base, size_t& at, size_t count) {
  T* p = reinterpret_cast<T*>(base + at);
  at += round16(count * sizeof(T));
  return p;
}

// host: sets the device; allocates the workspace on first use
inline int workspace_ensure(int device, unsigned char** d_mem, size_t bytes) {
  if (hipSetDevice(device) != hipSuccess) return UNINA_ERR_HIP;
  if (*d_mem) return UNINA_OK;
  void* mem = nullptr;
  if (hipMalloc(&mem, bytes) != hipSuccess) return UNINA_ERR_HIP;
  *d_mem = static_cast<unsigned char*>(mem);
  return UNINA_OK;
}

// host: waits for the device, frees; a null workspace is a no-op
inline void workspace_release(int device, void* d_mem) {
  if (!d_mem) return;
  if (hipSetDevice(device) == hipSuccess) (void)hipDeviceSynchronize();
  (void)hipFree(d_mem);
}
#endif  // __HIPCC__

}  // namespace unina
#endif  // UNINA_CLOUD_IO_H
