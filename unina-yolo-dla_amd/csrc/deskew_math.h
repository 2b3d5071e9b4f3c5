// deskew_math.h -- the arithmetic of unina_deskew_async (include/unina_mi355.h "motion de-skew of a LiDAR sweep"), one copy each:
// the float64 key table of the host half and the fp32 per-point half csrc/deskew.hip calls. tests/deskew_math_host.cpp compiles
// both with a host compiler (no HIP) and runs them on case files; deskew.table_numpy and deskew.deskew_numpy are their twins, bit
// for bit. Every unit that includes this header is compiled with -ffp-contract=off: each operation below is rounded once, where it
// is written.
#ifndef UNINA_DESKEW_MATH_H
#define UNINA_DESKEW_MATH_H

#include <math.h>

#include "cloud_io.h"

namespace unina {

constexpr int kDeskewMaxKeys = 64;
constexpr uint32_t kDeskewNaN = 0x7fc00000u;   // the ground filter's "absent" word
static_assert(kDeskewMaxKeys == UNINA_DESKEW_MAX_KEYS, "header limits");
static_assert(sizeof(unina_deskew_key) == 32 && sizeof(unina_deskew_pose) == 64 && sizeof(unina_deskew_header) == 32, "record layouts");

// ---------------------------------------------------------------- the per-point half: fp32
// tau of a time word: float32 seconds as they are, uint32 nanoseconds by one conversion and one multiply
UNINA_HD float deskew_tau(int format, uint32_t word) { return format == UNINA_TIME_U32_NS ? (float)word * 1e-9f : bits_float(word); }

// (the number of keys with t[j] <= tau) - 1, clamped to 0 .. n_keys - 2. t: the n_keys key times, strictly increasing, so the
// count is found by bisection: seven probes whatever n_keys <= 64 is, each at an index below n_keys. A NaN tau counts no key.
UNINA_HD int deskew_segment(const float* t, int n_keys, float tau) {
  int cnt = 0;
#pragma unroll
  for (int step = kDeskewMaxKeys; step >= 1; step >>= 1) {
    const int j = cnt + step;
    if (j <= n_keys && t[j - 1] <= tau) cnt = j;
  }
  const int k = cnt - 1;
  return k < 0 ? 0 : (k > n_keys - 2 ? n_keys - 2 : k);
}

// s of tau in the segment [ta, tb], clamped to [0, 1]; tau == tb gives 1 exactly
UNINA_HD float deskew_fraction(float ta, float tb, float tau) {
  const float s = (tau - ta) / (tb - ta);
  return s < 0.0f ? 0.0f : (s > 1.0f ? 1.0f : s);
}

UNINA_HD float deskew_lerp(float a, float b, float s) { return a + s * (b - a); }

// The pose at fraction s between the key rows a and b (qw, qx, qy, qz, px, py, pz, t each) as the rows of [R|t]: seven
// interpolations, the quaternion's norm, four divides, then the nine elements of R.
UNINA_HD void deskew_pose(const float* a, const float* b, float s, float m[12]) {
  float w = deskew_lerp(a[0], b[0], s), x = deskew_lerp(a[1], b[1], s), y = deskew_lerp(a[2], b[2], s), z = deskew_lerp(a[3], b[3], s);
  const float n = sqrtf(((w * w + x * x) + y * y) + z * z);
  w = w / n; x = x / n; y = y / n; z = z / n;
  m[0] = 1.0f - 2.0f * (y * y + z * z); m[1] = 2.0f * (x * y - w * z);        m[2] = 2.0f * (x * z + w * y);
  m[4] = 2.0f * (x * y + w * z);        m[5] = 1.0f - 2.0f * (x * x + z * z); m[6] = 2.0f * (y * z - w * x);
  m[8] = 2.0f * (x * z - w * y);        m[9] = 2.0f * (y * z + w * x);        m[10] = 1.0f - 2.0f * (x * x + y * y);
  m[3] = deskew_lerp(a[4], b[4], s);
  m[7] = deskew_lerp(a[5], b[5], s);
  m[11] = deskew_lerp(a[6], b[6], s);
}

// the word a result leaves as: its bits, a NaN (an overflowed product) as the one word kDeskewNaN whatever the platform made of it
UNINA_HD uint32_t deskew_word(float v) { return v != v ? kDeskewNaN : float_bits(v); }

struct DeskewPoint {
  uint32_t x, y, z;      // the output words; kDeskewNaN each where the point is INVALID
  uint32_t shift2;       // deskew_word of (dx * dx + dy * dy) + dz * dz, 0 where the point is INVALID
  int invalid, before, after;
};

// One point. t, keys: the n_keys key times and the n_keys rows of eight floats (device: LDS; host: the table).
UNINA_HD DeskewPoint deskew_point(const float* t, const float* keys, int n_keys, int format, uint32_t xb, uint32_t yb, uint32_t zb,
                                  uint32_t time_word) {
  const float x = bits_float(xb), y = bits_float(yb), z = bits_float(zb), tau = deskew_tau(format, time_word);
  DeskewPoint r;
  r.invalid = !(finite(x) && finite(y) && finite(z) && finite(tau));
  r.x = r.y = r.z = kDeskewNaN;
  r.shift2 = 0u;
  r.before = r.after = 0;
  if (r.invalid) return r;
  const int k = deskew_segment(t, n_keys, tau);
  r.before = tau < t[0];
  r.after = tau > t[n_keys - 1];
  float m[12];
  deskew_pose(keys + 8 * k, keys + 8 * (k + 1), deskew_fraction(t[k], t[k + 1], tau), m);
  const float xo = cloud_transform_row(m, x, y, z), yo = cloud_transform_row(m + 4, x, y, z), zo = cloud_transform_row(m + 8, x, y, z);
  const float dx = xo - x, dy = yo - y, dz = zo - z;
  r.x = deskew_word(xo);
  r.y = deskew_word(yo);
  r.z = deskew_word(zo);
  r.shift2 = deskew_word((dx * dx + dy * dy) + dz * dz);
  return r;
}

// ---------------------------------------------------------------- the host half: float64
inline bool finite64(double v) { return v - v == 0.0; }

struct Quat64 { double w, x, y, z; };
inline double dot64(const Quat64& a, const Quat64& b) { return ((a.w * b.w + a.x * b.x) + a.y * b.y) + a.z * b.z; }
inline Quat64 neg64(const Quat64& q) { return Quat64{-q.w, -q.x, -q.y, -q.z}; }
// q / |q|; false where the norm is not a positive finite number
inline bool normalise64(Quat64* q) {
  const double n = sqrt(dot64(*q, *q));
  if (!(n > 0.0) || !finite64(n)) return false;
  q->w = q->w / n; q->x = q->x / n; q->y = q->y / n; q->z = q->z / n;
  return true;
}
// the Hamilton product a (x) b
inline Quat64 mul64(const Quat64& a, const Quat64& b) {
  return Quat64{((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z, ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y,
                ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x, ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w};
}

// unina_deskew_table: the K relative poses of the keys, seen from the pose at t_ref, as float32 rows. The steps are those of the
// public header, in its order. UNINA_OK or UNINA_ERR_ARG; `out` is written only on UNINA_OK.
inline int deskew_table(const unina_deskew_pose* poses, int n_keys, double t_sweep, double t_ref, unina_deskew_key* out) {
  if (!poses || !out || n_keys < 2 || n_keys > kDeskewMaxKeys || !finite64(t_sweep) || !finite64(t_ref)) return UNINA_ERR_ARG;
  Quat64 q[kDeskewMaxKeys];
  float tf[kDeskewMaxKeys];
  for (int k = 0; k < n_keys; ++k) {
    const unina_deskew_pose& p = poses[k];
    if (!finite64(p.t) || !finite64(p.q[0]) || !finite64(p.q[1]) || !finite64(p.q[2]) || !finite64(p.q[3]) || !finite64(p.p[0]) ||
        !finite64(p.p[1]) || !finite64(p.p[2]))
      return UNINA_ERR_ARG;
    q[k] = Quat64{p.q[0], p.q[1], p.q[2], p.q[3]};
    if (!normalise64(&q[k])) return UNINA_ERR_ARG;                                   // step 1
    tf[k] = (float)(p.t - t_sweep);
    if (!finite(tf[k]) || (k > 0 && !(tf[k] > tf[k - 1]))) return UNINA_ERR_ARG;     // the device's times: finite, strictly increasing
  }
  if (!(t_ref >= poses[0].t && t_ref <= poses[n_keys - 1].t)) return UNINA_ERR_ARG;
  // step 2: the reference pose. The float32 times increase strictly, so the float64 times do
  int cnt = 0;
  for (int k = 0; k < n_keys; ++k) cnt += poses[k].t <= t_ref;
  const int r = cnt - 1 > n_keys - 2 ? n_keys - 2 : cnt - 1;   // cnt >= 1: t_ref >= t_0
  const double s = (t_ref - poses[r].t) / (poses[r + 1].t - poses[r].t);
  const Quat64 a = q[r];
  const Quat64 b = dot64(a, q[r + 1]) < 0.0 ? neg64(q[r + 1]) : q[r + 1];
  Quat64 qr{a.w + s * (b.w - a.w), a.x + s * (b.x - a.x), a.y + s * (b.y - a.y), a.z + s * (b.z - a.z)};
  if (!normalise64(&qr)) return UNINA_ERR_ARG;
  double pr[3];
  for (int c = 0; c < 3; ++c) pr[c] = poses[r].p[c] + s * (poses[r + 1].p[c] - poses[r].p[c]);
  // R(conj(q_ref))
  const Quat64 c{qr.w, -qr.x, -qr.y, -qr.z};
  const double R[9] = {1.0 - 2.0 * (c.y * c.y + c.z * c.z), 2.0 * (c.x * c.y - c.w * c.z),       2.0 * (c.x * c.z + c.w * c.y),
                       2.0 * (c.x * c.y + c.w * c.z),       1.0 - 2.0 * (c.x * c.x + c.z * c.z), 2.0 * (c.y * c.z - c.w * c.x),
                       2.0 * (c.x * c.z - c.w * c.y),       2.0 * (c.y * c.z + c.w * c.x),       1.0 - 2.0 * (c.x * c.x + c.y * c.y)};
  Quat64 D[kDeskewMaxKeys];
  double d[kDeskewMaxKeys][3];
  for (int k = 0; k < n_keys; ++k) {
    D[k] = mul64(c, q[k]);                                                           // step 3
    if (!normalise64(&D[k])) return UNINA_ERR_ARG;
    const double vx = poses[k].p[0] - pr[0], vy = poses[k].p[1] - pr[1], vz = poses[k].p[2] - pr[2];
    for (int i = 0; i < 3; ++i) d[k][i] = (R[3 * i] * vx + R[3 * i + 1] * vy) + R[3 * i + 2] * vz;
    // step 4: D_0 on the hemisphere w >= 0, every later key on its predecessor's
    if (k == 0 ? D[0].w < 0.0 : dot64(D[k], D[k - 1]) < 0.0) D[k] = neg64(D[k]);
    if (k > 0 && !(dot64(D[k], D[k - 1]) >= 0.5)) return UNINA_ERR_ARG;             // more than 120 degrees between two keys
  }
  for (int k = 0; k < n_keys; ++k)                                                  // a translation beyond fp32 is not finite either
    if (!finite((float)d[k][0]) || !finite((float)d[k][1]) || !finite((float)d[k][2])) return UNINA_ERR_ARG;
  // step 5. x + 0.0 is x, but +0.0 for -0.0: the sign of a zero is all that -q for q can change up to here
  for (int k = 0; k < n_keys; ++k)
    out[k] = unina_deskew_key{(float)(D[k].w + 0.0),  (float)(D[k].x + 0.0),  (float)(D[k].y + 0.0),  (float)(D[k].z + 0.0),
                              (float)(d[k][0] + 0.0), (float)(d[k][1] + 0.0), (float)(d[k][2] + 0.0), tf[k]};
  return UNINA_OK;
}

}  // namespace unina
#endif  // UNINA_DESKEW_MATH_H
