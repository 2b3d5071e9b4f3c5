// hd.h -- the one host/device function macro and the finite tests of the headers that are compiled twice: by hipcc for the
// kernels and by a plain host compiler for the stand-alone programs under tests/ (no HIP there).
#ifndef UNINA_HD_H
#define UNINA_HD_H

#if defined(__HIPCC__)
#define UNINA_HD __host__ __device__ __forceinline__
#else
#define UNINA_HD inline
#endif

namespace unina {

UNINA_HD bool finite(float v) { return v - v == 0.0f; }   // false for NaN and +-inf
UNINA_HD bool finite_pos(float v) { return v > 0.0f && finite(v); }

}  // namespace unina
#endif  // UNINA_HD_H
