// pose_math.h -- the arithmetic of unina_pose_async (include/unina_mi355.h "pose from the tracked cones") as __host__ __device__
// functions: the composition of the prior, the tests of a usable record and of a landmark, the move of a point, the fixed-point
// terms of a pair and the closed form of the correction. csrc/pose.hip calls them on the device, tests/pose_math_host.cpp runs the
// whole stage with them on the host, pose.pose_numpy is their numpy twin. fp32 and float64, one rounding per operation in the order
// written: every translation unit that includes this header is compiled with -ffp-contract=off.
#ifndef UNINA_POSE_MATH_H
#define UNINA_POSE_MATH_H

#include <math.h>

#include "track_math.h"

namespace unina {

constexpr float kPoseLimit = 32768.0f;    // |x|, |y| of a point or a landmark that may vote, metres
constexpr float kPoseScale = 1024.0f;     // fixed-point steps per metre: 2^25 steps at the limit, a product of two below 2^50
constexpr int kPoseOk = 0, kPoseTooFew = 1, kPoseDegenerate = 2;   // UNINA_POSE_*

struct PoseCorr {
  float c, s, tx, ty;
};

struct PoseSums {
  long long n, px, py, mx, my, dot, cross;
};

// o = a o b, row-major 3 x 4 [R|t]; o is neither a nor b
UNINA_HD void pose_compose(const float* a, const float* b, float* o) {
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) {
      const float v = (a[4 * r] * b[k] + a[4 * r + 1] * b[4 + k]) + a[4 * r + 2] * b[8 + k];
      o[4 * r + k] = k == 3 ? v + a[4 * r + 3] : v;
    }
}

UNINA_HD bool pose_in_field(float x, float y) { return x <= kPoseLimit && x >= -kPoseLimit && y <= kPoseLimit && y >= -kPoseLimit; }   // a NaN fails

UNINA_HD bool pose_usable(const TrackPoint& p) { return p.usable != 0 && pose_in_field(p.x, p.y); }

UNINA_HD bool pose_landmark(int id, int hits, float x, float y, int min_hits) { return id != 0 && hits >= min_hits && pose_in_field(x, y); }

UNINA_HD void pose_move(const PoseCorr& k, float px, float py, float* qx, float* qy) {
  *qx = (k.c * px - k.s * py) + k.tx;
  *qy = (k.s * px + k.c * py) + k.ty;
}

// a coordinate inside the field in steps of 2^-10 m: the product is exact, |result| <= 2^25
UNINA_HD long long pose_fixed(float v) { return (long long)rintf(v * kPoseScale); }

// the terms of one pair, from the UNMOVED point and the landmark
UNINA_HD void pose_terms(float px, float py, float mx, float my, PoseSums* t) {
  t->n = 1;
  t->px = pose_fixed(px);
  t->py = pose_fixed(py);
  t->mx = pose_fixed(mx);
  t->my = pose_fixed(my);
  t->dot = t->px * t->mx + t->py * t->my;
  t->cross = t->px * t->my - t->py * t->mx;
}

// the whole correction from the sums of n >= 1 pairs; returns kPoseOk or kPoseDegenerate
UNINA_HD int pose_solve(const PoseSums& u, PoseCorr* k) {
  const double n = (double)u.n, px = (double)u.px, py = (double)u.py, mx = (double)u.mx, my = (double)u.my;
  const double a = (double)u.dot - (px * mx + py * my) / n;
  const double b = (double)u.cross - (px * my - py * mx) / n;
  const float af = (float)a, bf = (float)b;
  const float h = sqrtf(af * af + bf * bf);
  int status = kPoseOk;
  if (finite_pos(h)) {
    k->c = af / h;
    k->s = bf / h;
  } else {
    k->c = 1.0f;
    k->s = 0.0f;
    status = kPoseDegenerate;
  }
  const double c = (double)k->c, s = (double)k->s;
  k->tx = (float)(((mx - (c * px - s * py)) / n) / 1024.0);
  k->ty = (float)(((my - (s * px + c * py)) / n) / 1024.0);
  return status;
}

// the corrected pose: rows 0 and 1 turned and shifted, row 2 the prior's; o is not P
UNINA_HD void pose_corrected(const PoseCorr& k, const float* P, float* o) {
  for (int i = 0; i < 4; ++i) {
    const float a = k.c * P[i] - k.s * P[4 + i], b = k.s * P[i] + k.c * P[4 + i];
    o[i] = i == 3 ? a + k.tx : a;
    o[4 + i] = i == 3 ? b + k.ty : b;
    o[8 + i] = P[8 + i];
  }
}

}  // namespace unina
#endif  // UNINA_POSE_MATH_H
