// pose_math_host.cpp -- stand-alone host driver of csrc/pose_math.h for tests/test_pose_cpu.py: the whole of unina_pose_async as
// plain loops over the functions csrc/pose.hip calls, and the closed form alone, built by a host compiler (no HIP, no GPU) and run
// on cases from a file.
//   pose_math_host IN OUT
// IN : 3 int32 -- magic, mode, n
//      mode 0 (n = 1): 12 float32 inc, 1 float32 gate, 4 int32 class_aware, min_hits, iterations, min_pairs, 1 int32 has_prev,
//                      16 float32 prev, 1 int32 count, 5 words unused; then 1024 records, 1024 cones and 1024 slots of 8 words each
//      mode 1: n cases of 7 int64 -- N, Spx, Spy, Smx, Smy, Sdot, Scross
// OUT: mode 0: 1024 cones of 8 words, 16 words of the result, 8 words of the header
//      mode 1: 8 int32 per case -- bits of c, s, tx, ty, status, 0, 0, 0
#include "../unina-yolo-dla_amd/csrc/pose_math.h"

#include <cstdio>
#include <vector>

using namespace unina;

namespace {

constexpr int kMax = 1024;

union Word {
  float f;
  int32_t i;
  uint32_t u;
};

struct Rec {
  Word w[8];
};

int whole(FILE* f, std::vector<int32_t>& out) {
  Word h[40];
  std::vector<Rec> dets(kMax), cones(kMax), slots(kMax);
  if (fread(h, sizeof h, 1, f) != 1 || fread(dets.data(), sizeof(Rec), kMax, f) != kMax || fread(cones.data(), sizeof(Rec), kMax, f) != kMax ||
      fread(slots.data(), sizeof(Rec), kMax, f) != kMax)
    return 4;
  float inc[12], prev[12], P[12];
  for (int i = 0; i < 12; ++i) inc[i] = h[i].f, prev[i] = h[18 + i].f;
  const float gate2 = h[12].f * h[12].f;
  const int class_aware = h[13].i, min_hits = h[14].i, iterations = h[15].i, min_pairs = h[16].i, has_prev = h[17].i;
  if (iterations < 1 || iterations > 8 || min_pairs < 2 || min_hits < 1) return 4;
  int n = h[34].i;
  n = n < 0 ? 0 : (n > kMax ? kMax : n);
  if (has_prev) {
    pose_compose(prev, inc, P);
  } else {
    for (int i = 0; i < 12; ++i) P[i] = inc[i];
  }
  // cones: x, y, z, u, v, n_valid, n_samples, valid; records: ..., confidence, class_id, ...; slots: x, y, z, confidence, id, class_id, hits, missed
  std::vector<TrackPoint> pt((size_t)n);
  std::vector<int> use, lms;
  for (int j = 0; j < n; ++j) {
    pt[j] = track_point(P, cones[j].w[0].f, cones[j].w[1].f, cones[j].w[2].f, cones[j].w[7].i);
    if (pose_usable(pt[j])) use.push_back(j);
  }
  for (int s = 0; s < kMax; ++s)
    if (pose_landmark(slots[s].w[4].i, slots[s].w[6].i, slots[s].w[0].f, slots[s].w[1].f, min_hits)) lms.push_back(s);
  PoseCorr k = {1.0f, 0.0f, 0.0f, 0.0f};
  int status = kPoseOk, updates = 0;
  long long n_pairs = 0;
  uint32_t max_bits = 0;
  std::vector<uint64_t> mine(kMax), best(kMax);
  for (int it = 0; it < iterations; ++it) {
    for (int s = 0; s < kMax; ++s) best[s] = kTrackNoKey;
    for (int j : use) {
      float qx, qy;
      pose_move(k, pt[j].x, pt[j].y, &qx, &qy);
      mine[j] = kTrackNoKey;
      for (int s : lms) {
        const float d2 = track_d2(qx, qy, pt[j].z, slots[s].w[0].f, slots[s].w[1].f, slots[s].w[2].f);
        if (!track_gated(d2, gate2) || (class_aware != 0 && slots[s].w[5].i != dets[j].w[5].i)) continue;
        const uint64_t to_lm = track_key(d2, (uint32_t)s), to_rec = track_key(d2, (uint32_t)j);
        if (to_lm < mine[j]) mine[j] = to_lm;
        if (to_rec < best[s]) best[s] = to_rec;
      }
    }
    PoseSums u = {0, 0, 0, 0, 0, 0, 0};
    max_bits = 0;
    for (int j : use) {
      if (mine[j] == kTrackNoKey) continue;
      const int s = (int)(uint32_t)mine[j];
      if (best[s] != ((mine[j] & 0xffffffff00000000ull) | (uint64_t)j)) continue;
      PoseSums t;
      pose_terms(pt[j].x, pt[j].y, slots[s].w[0].f, slots[s].w[1].f, &t);
      u.n += 1, u.px += t.px, u.py += t.py, u.mx += t.mx, u.my += t.my, u.dot += t.dot, u.cross += t.cross;
      const uint32_t bits = (uint32_t)(mine[j] >> 32);
      if (bits > max_bits) max_bits = bits;
    }
    n_pairs = u.n;
    if (u.n < min_pairs) {
      status = kPoseTooFew;
      break;
    }
    status = pose_solve(u, &k);
    ++updates;
  }
  for (int j = 0; j < kMax; ++j) {
    Rec r = cones[j];
    if (j < n) {
      pose_move(k, pt[j].x, pt[j].y, &r.w[0].f, &r.w[1].f);
      r.w[2].f = pt[j].z;
    }
    for (int i = 0; i < 8; ++i) out.push_back(r.w[i].i);
  }
  Word res[16];
  float corrected[12];
  pose_corrected(k, P, corrected);
  for (int i = 0; i < 12; ++i) res[i].f = corrected[i];
  res[12].f = k.c, res[13].f = k.s, res[14].f = k.tx, res[15].f = k.ty;
  for (int i = 0; i < 16; ++i) out.push_back(res[i].i);
  const int32_t head[8] = {n, (int32_t)use.size(), (int32_t)lms.size(), (int32_t)n_pairs, updates, status, (int32_t)max_bits, 0};
  out.insert(out.end(), head, head + 8);
  return 0;
}

int closed_form(FILE* f, int n, std::vector<int32_t>& out) {
  std::vector<long long> sums((size_t)n * 7);
  if (n && fread(sums.data(), 7 * sizeof(long long), (size_t)n, f) != (size_t)n) return 4;
  for (int i = 0; i < n; ++i) {
    const long long* s = &sums[(size_t)i * 7];
    if (s[0] < 1) return 4;
    const PoseSums u = {s[0], s[1], s[2], s[3], s[4], s[5], s[6]};
    PoseCorr k;
    const int status = pose_solve(u, &k);
    const int32_t rec[8] = {(int32_t)track_bits(k.c), (int32_t)track_bits(k.s), (int32_t)track_bits(k.tx), (int32_t)track_bits(k.ty), status, 0, 0, 0};
    out.insert(out.end(), rec, rec + 8);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[3];
  if (fread(h, sizeof h, 1, f) != 1 || h[0] != 0x504f5331 || h[2] < 0 || h[1] < 0 || h[1] > 1 || (h[1] == 0 && h[2] != 1)) return 4;
  std::vector<int32_t> out;
  const int rc = h[1] == 0 ? whole(f, out) : closed_form(f, h[2], out);
  fclose(f);
  if (rc) return rc;
  f = fopen(argv[2], "wb");
  if (!f || (!out.empty() && fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size()) || fclose(f)) return 5;
  return 0;
}
