// track_math.h -- the arithmetic of unina_track_update_async (include/unina_mi355.h "tracking") as __host__ __device__ functions:
// the pose transform, the gated distance, the pair key and the slot update. csrc/track.hip calls them on the device,
// tests/track_math_host.cpp sweeps them on the host, tracking.update_numpy is their numpy twin. fp32 throughout, one rounding
// per operation in the order written: every translation unit that includes this header is compiled with -ffp-contract=off.
#ifndef UNINA_TRACK_MATH_H
#define UNINA_TRACK_MATH_H

#include <limits.h>
#include <stdint.h>
#include <string.h>

#include "hd.h"

namespace unina {

constexpr int kTrackMaxHits = 1000000000;
constexpr uint64_t kTrackNoKey = ~(uint64_t)0;   // above every pair key: d2's bits are at most +inf's

struct TrackPoint {
  float x, y, z;
  int usable;   // 1: the cone is valid and the point is finite
};

UNINA_HD uint32_t track_bits(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
}

// camera frame -> tracking frame through the row-major 3 x 4 pose [R|t]
UNINA_HD TrackPoint track_point(const float* pose, float x, float y, float z, int valid) {
  TrackPoint p;
  p.x = ((pose[0] * x + pose[1] * y) + pose[2] * z) + pose[3];
  p.y = ((pose[4] * x + pose[5] * y) + pose[6] * z) + pose[7];
  p.z = ((pose[8] * x + pose[9] * y) + pose[10] * z) + pose[11];
  p.usable = (valid != 0 && finite(p.x) && finite(p.y) && finite(p.z)) ? 1 : 0;
  return p;
}

// squared distance of a point to a track; never negative, NaN where an operand is not finite
UNINA_HD float track_d2(float px, float py, float pz, float tx, float ty, float tz) {
  const float dx = px - tx, dy = py - ty, dz = pz - tz;
  return (dx * dx + dy * dy) + dz * dz;
}

UNINA_HD bool track_gated(float d2, float gate2) { return d2 <= gate2; }   // a NaN d2 fails

// (d2, index) as one unsigned key: ascending keys are ascending (d2, index)
UNINA_HD uint64_t track_key(float d2, uint32_t index) { return ((uint64_t)track_bits(d2) << 32) | index; }

// one coordinate of a matched slot: the dx of the gate, then the step
UNINA_HD float track_step(float t, float alpha, float p) {
  const float d = p - t;
  return t + alpha * d;
}

UNINA_HD int track_hit(int hits) { return hits < kTrackMaxHits ? hits + 1 : kTrackMaxHits; }
UNINA_HD int track_miss(int missed) { return missed < INT_MAX ? missed + 1 : INT_MAX; }

// how many of `births` birth candidates are taken: the first m, the rest are dropped
UNINA_HD int track_births_taken(int births, int free_slots, int next_id) {
  const int ids = INT_MAX - next_id;   // next_id >= 1
  int m = births < free_slots ? births : free_slots;
  return m < ids ? m : ids;
}

}  // namespace unina
#endif  // UNINA_TRACK_MATH_H
