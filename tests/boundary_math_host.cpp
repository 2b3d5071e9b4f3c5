// boundary_math_host.cpp -- stand-alone host driver of csrc/boundary_math.h for tests/test_boundary_cpu.py: the whole of
// unina_boundary_async as plain loops over the functions csrc/boundary.hip calls, built by a host compiler (no HIP, no GPU) and run
// on a case from a file.
//   boundary_math_host IN OUT
// IN : 1 int32 magic; 12 float32 pose, 3 float32 forward, 4 float32 first_gate, step_gate, cos_turn, width_gate, 4 int32 class_left,
//      class_right, min_hits, max_chain (unina_boundary_params, 23 words); 1 int32 has_device_pose, 12 float32 device pose; then
//      1024 slots of 8 words each
// OUT: 8 words of the header, 256 points of 4 words
#include "../unina-yolo-dla_amd/csrc/boundary_math.h"

#include <cstdio>
#include <vector>

using namespace unina;

namespace {

constexpr int kMax = 1024;

union Word {
  float f;
  int32_t i;
};

struct Slot {
  Word w[8];   // x, y, z, confidence, id, class_id, hits, missed
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  Word h[37];
  std::vector<Slot> slots(kMax);
  if (fread(h, sizeof h, 1, f) != 1 || h[0].i != 0x424e4431 || fread(slots.data(), sizeof(Slot), kMax, f) != kMax) return 4;
  fclose(f);
  float P[12], fwd[3];
  const int has_pose = h[24].i;
  for (int i = 0; i < 12; ++i) P[i] = has_pose ? h[25 + i].f : h[1 + i].f;
  for (int i = 0; i < 3; ++i) fwd[i] = h[13 + i].f;
  const float first2 = h[16].f * h[16].f, step2 = h[17].f * h[17].f, cos2 = h[18].f * h[18].f, width2 = h[19].f * h[19].f;
  const int class_left = h[20].i, class_right = h[21].i, min_hits = h[22].i, max_chain = h[23].i;
  if (max_chain < 1 || max_chain > kBoundaryMaxChain || min_hits < 1 || class_left == class_right) return 4;

  int32_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // n_candidates[2], n_chain[2], end[2], n_centre, n_wide
  std::vector<BoundaryPoint> pts(4 * kBoundaryMaxChain, BoundaryPoint{0.0f, 0.0f, 0.0f, 0});
  const BoundaryStart st = boundary_start(P, fwd);
  if (!st.ok) {
    head[4] = head[5] = kBoundaryNoHeading;
  } else {
    int n_chain[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
      std::vector<int> cand;
      for (int s = 0; s < kMax; ++s)
        if (boundary_side(slots[s].w[4].i, slots[s].w[6].i, slots[s].w[5].i, slots[s].w[0].f, slots[s].w[1].f, min_hits, class_left, class_right) == k)
          cand.push_back(s);
      std::vector<char> used(cand.size(), 0);
      float cx = st.ox, cy = st.oy, ddx = st.hx, ddy = st.hy;
      int m = 0, end;
      for (;;) {
        if (m == max_chain) {
          end = kBoundaryFull;
          break;
        }
        uint64_t best = kTrackNoKey;
        for (size_t e = 0; e < cand.size(); ++e) {
          if (used[e]) continue;
          const Slot& s = slots[cand[e]];
          float d2;
          if (!boundary_eligible(m == 0, cx, cy, ddx, ddy, s.w[0].f, s.w[1].f, m == 0 ? first2 : step2, cos2, &d2)) continue;
          const uint64_t key = track_key(d2, (uint32_t)e);
          if (key < best) best = key;
        }
        if (best == kTrackNoKey) {
          end = m == 0 ? kBoundaryNoFirst : kBoundaryNoNext;
          break;
        }
        const size_t e = (size_t)(uint32_t)best;
        const Slot& s = slots[cand[e]];
        used[e] = 1;
        pts[(size_t)(k * kBoundaryMaxChain + m)] = BoundaryPoint{s.w[0].f, s.w[1].f, s.w[2].f, s.w[4].i};
        boundary_turn(m, cx, cy, s.w[0].f, s.w[1].f, &ddx, &ddy);
        cx = s.w[0].f;
        cy = s.w[1].f;
        ++m;
      }
      head[k] = (int32_t)cand.size();
      head[2 + k] = n_chain[k] = m;
      head[4 + k] = end;
    }
    const BoundaryPoint *L = &pts[0], *R = &pts[kBoundaryMaxChain];
    const int nl = n_chain[0], nr = n_chain[1];
    if (nl > 0 && nr > 0) {
      int i = 0, j = 0;
      for (;;) {
        if (track_gated(boundary_d2(L[i].x, L[i].y, R[j].x, R[j].y), width2)) {
          pts[(size_t)(2 * kBoundaryMaxChain + head[6]++)] = boundary_rung(L[i], R[j], i, j);
        } else {
          ++head[7];
        }
        const bool has_i = i + 1 < nl, has_j = j + 1 < nr;
        if (!has_i && !has_j) break;
        const float a = has_i ? boundary_d2(L[i + 1].x, L[i + 1].y, R[j].x, R[j].y) : 0.0f;
        const float b = has_j ? boundary_d2(L[i].x, L[i].y, R[j + 1].x, R[j + 1].y) : 0.0f;
        if (boundary_advance_left(has_i, has_j, a, b)) {
          ++i;
        } else {
          ++j;
        }
      }
    }
  }
  std::vector<int32_t> out(head, head + 8);
  for (const BoundaryPoint& p : pts) {
    Word w[3];
    w[0].f = p.x, w[1].f = p.y, w[2].f = p.z;
    out.push_back(w[0].i);
    out.push_back(w[1].i);
    out.push_back(w[2].i);
    out.push_back(p.ref);
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size() || fclose(f)) return 5;
  return 0;
}
