// boundary_math.h -- the arithmetic of unina_boundary_async (include/unina_mi355.h "track limits and centre line") as __host__
// __device__ functions: the origin and the heading from the pose, the candidate test, the planar distance, the test of a link, the
// direction of the next link and a rung's point. csrc/boundary.hip calls them on the device, tests/boundary_math_host.cpp runs the
// whole stage with them on the host, boundary.boundary_numpy is their numpy twin. The key order is track_math.h's, the field's
// bound pose_math.h's. fp32 throughout, one rounding per operation in the order written: every translation unit that includes this
// header is compiled with -ffp-contract=off.
#ifndef UNINA_BOUNDARY_MATH_H
#define UNINA_BOUNDARY_MATH_H

#include "pose_math.h"

namespace unina {

constexpr int kBoundaryMaxChain = 64;                                                              // UNINA_BOUNDARY_MAX_CHAIN
constexpr int kBoundaryNoFirst = 0, kBoundaryNoNext = 1, kBoundaryFull = 2, kBoundaryNoHeading = 3;   // UNINA_BOUNDARY_*

struct BoundaryStart {
  float ox, oy, hx, hy;
  int ok;   // 0: UNINA_BOUNDARY_NO_HEADING
};

struct BoundaryPoint {
  float x, y, z;
  int ref;
};

// the vehicle's position and heading in the plane of the tracking frame
UNINA_HD BoundaryStart boundary_start(const float* P, const float* f) {
  BoundaryStart s;
  s.ox = P[3];
  s.oy = P[7];
  s.hx = (P[0] * f[0] + P[1] * f[1]) + P[2] * f[2];
  s.hy = (P[4] * f[0] + P[5] * f[1]) + P[6] * f[2];
  s.ok = (finite(s.ox) && finite(s.oy) && finite_pos(s.hx * s.hx + s.hy * s.hy)) ? 1 : 0;
  return s;
}

// the side a slot is a candidate of: 0 left, 1 right, -1 none (class_left != class_right)
UNINA_HD int boundary_side(int id, int hits, int class_id, float x, float y, int min_hits, int class_left, int class_right) {
  if (!pose_landmark(id, hits, x, y, min_hits)) return -1;
  return class_id == class_left ? 0 : (class_id == class_right ? 1 : -1);
}

// squared planar distance from b to a; never negative
UNINA_HD float boundary_d2(float ax, float ay, float bx, float by) {
  const float dx = ax - bx, dy = ay - by;
  return dx * dx + dy * dy;
}

// may link m go from c, arriving in direction d, to (x, y)? gate2 is the link's own: first_gate^2 for m = 0, else step_gate^2.
// *d2 is the distance the key orders by. A NaN fails every test.
UNINA_HD bool boundary_eligible(bool first, float cx, float cy, float ddx, float ddy, float x, float y, float gate2, float cos2, float* d2) {
  const float dx = x - cx, dy = y - cy;
  *d2 = dx * dx + dy * dy;
  const float dot = dx * ddx + dy * ddy;
  if (!track_gated(*d2, gate2)) return false;
  if (first) return dot >= 0.0f;
  return dot > 0.0f && dot * dot >= cos2 * (*d2 * (ddx * ddx + ddy * ddy));
}

// the direction of the link behind link m, which went from c to (x, y): h still for m = 0
UNINA_HD void boundary_turn(int m, float cx, float cy, float x, float y, float* ddx, float* ddy) {
  if (m >= 1) {
    *ddx = x - cx;
    *ddy = y - cy;
  }
}

// the centre point of the rung between L[i] and R[j]
UNINA_HD BoundaryPoint boundary_rung(const BoundaryPoint& l, const BoundaryPoint& r, int i, int j) {
  BoundaryPoint c;
  c.x = (l.x + r.x) * 0.5f;
  c.y = (l.y + r.y) * 0.5f;
  c.z = (l.z + r.z) * 0.5f;
  c.ref = i | (j << 16);
  return c;
}

// does the ladder advance i (else j)? has_i / has_j: i + 1 < nL, j + 1 < nR, not both false; a = d2(L[i+1], R[j]), b = d2(L[i], R[j+1])
UNINA_HD bool boundary_advance_left(bool has_i, bool has_j, float a, float b) { return has_i && (!has_j || a <= b); }

}  // namespace unina
#endif  // UNINA_BOUNDARY_MATH_H
