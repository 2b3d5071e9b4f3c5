// track_math_host.cpp -- stand-alone host driver of csrc/track_math.h for tests/test_track_cpu.py: the pose transform, the gated
// distance, the pair key and the slot update csrc/track.hip calls, built by a host compiler (no HIP, no GPU) and run on cases
// from a file.
//   track_math_host IN OUT
// IN : 3 int32 -- magic, mode, n -- then n cases of 16 words each
//      mode 0: 12 float32 pose, 3 float32 x, y, z, 1 int32 valid
//      mode 1: 6 float32 px, py, pz, tx, ty, tz, 1 float32 gate2, 1 uint32 index, 8 words unused
//      mode 2: 3 float32 t, alpha, p, 5 int32 hits, missed, births, free_slots, next_id, 8 words unused
// OUT: 4 int32 per case
//      mode 0: bits of px, py, pz, usable          mode 1: bits of d2, gated, key low word, key high word
//      mode 2: bits of the stepped coordinate, hits, missed, births taken
#include "../unina-yolo-dla_amd/csrc/track_math.h"

#include <cstdio>
#include <vector>

using namespace unina;

struct Case {
  union {
    float f[16];
    int32_t i[16];
    uint32_t u[16];
  };
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[3];
  if (fread(h, sizeof h, 1, f) != 1 || h[0] != 0x54524b31 || h[2] < 0 || h[1] < 0 || h[1] > 2) return 4;
  const int mode = h[1], n = h[2];
  std::vector<Case> cases((size_t)n);
  if (n && fread(cases.data(), sizeof(Case), (size_t)n, f) != (size_t)n) return 4;
  fclose(f);
  std::vector<int32_t> out;
  out.reserve((size_t)n * 4);
  for (const Case& c : cases) {
    int32_t rec[4];
    if (mode == 0) {
      const TrackPoint p = track_point(c.f, c.f[12], c.f[13], c.f[14], c.i[15]);
      rec[0] = (int32_t)track_bits(p.x);
      rec[1] = (int32_t)track_bits(p.y);
      rec[2] = (int32_t)track_bits(p.z);
      rec[3] = p.usable;
    } else if (mode == 1) {
      const float d2 = track_d2(c.f[0], c.f[1], c.f[2], c.f[3], c.f[4], c.f[5]);
      const uint64_t key = track_key(d2, c.u[7]);
      if (key == kTrackNoKey) return 6;   // the empty key must stay above every pair key
      rec[0] = (int32_t)track_bits(d2);
      rec[1] = track_gated(d2, c.f[6]) ? 1 : 0;
      rec[2] = (int32_t)(uint32_t)key;
      rec[3] = (int32_t)(uint32_t)(key >> 32);
    } else {
      if (c.i[7] < 1 || c.i[5] < 0 || c.i[6] < 0) return 4;
      rec[0] = (int32_t)track_bits(track_step(c.f[0], c.f[1], c.f[2]));
      rec[1] = track_hit(c.i[3]);
      rec[2] = track_miss(c.i[4]);
      rec[3] = track_births_taken(c.i[5], c.i[6], c.i[7]);
    }
    out.insert(out.end(), rec, rec + 4);
  }
  f = fopen(argv[2], "wb");
  if (!f || (!out.empty() && fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size()) || fclose(f)) return 5;
  return 0;
}
