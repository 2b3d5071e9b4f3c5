// Host check of the stride-2 register-queue tiles' LDS image (csrc/regq_s2.h): for every tile given on the command line as
// "ESZ TH TW CIN NT" (bytes per element, tile, input channels, threads), enumerate
//   * every request of the patch: each (row, column, chunk) is fetched exactly once and lands in a slot of its own inside the
//     image;
//   * every ds_read_b128 of the K loop -- pixel subtile x k-block x 64 lanes -- : the slot a lane reads holds exactly the
//     (row, column, chunk) the MFMA wants there, and no two lanes of one of the instruction's four 16-lane groups read different
//     addresses on one 16-byte slot of the 256-byte bank row.
// Prints, per tile, the extra LDS cycles (bank conflicts) of the image and, for comparison, of the stride-1 image the tiles
// had before (block_pipeline.h, make_img). Exit status 1 on any violation.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "../unina-yolo-dla_amd/csrc/regq_s2.h"

namespace s2 = unina::s2;

// the four lane groups of ds_read_b128 on gfx950
static const int kGroups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                   {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                   {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                   {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

// extra LDS cycles of one instruction whose lane l reads the 16-byte slot slots[l]
static int extra_cycles(const int (&slots)[64]) {
  int extra = 0;
  for (const auto& g : kGroups) {
    std::map<int, std::set<int>> on;   // bank slot -> distinct addresses
    for (int l : g) on[slots[l] & 15].insert(slots[l]);
    size_t worst = 1;
    for (const auto& kv : on) worst = kv.second.size() > worst ? kv.second.size() : worst;
    extra += (int)worst - 1;
  }
  return extra;
}

// the stride-1 image: pixel r at r * nch, chunk c at slot c ^ key(r)
static int old_slot(int r, int c, int nch) {
  const int sh = nch % 16 == 0 ? 0 : (nch % 8 == 0 ? 1 : 2), mask = nch % 16 == 0 ? 15 : (nch % 8 == 0 ? 7 : 3);
  return r * nch + (c ^ ((r >> sh) & mask));
}

int main(int argc, char** argv) {
  int bad = 0;
  for (int a = 1; a + 4 < argc; a += 5) {
    const int esz = atoi(argv[a]), th = atoi(argv[a + 1]), tw = atoi(argv[a + 2]), cin = atoi(argv[a + 3]), nt = atoi(argv[a + 4]);
    const int nch = cin * esz / 16, r0w = 2 * (tw - 1) + 3, r0h = 2 * (th - 1) + 3, P = s2::pitch(tw, r0w), H = s2::half_w(r0w);
    const int nslots = s2::image_bytes(r0h, P, nch) / 16, cb_n = nch / 4, kb_n = 9 * cb_n, bm = th * tw, ms = (bm + 15) / 16;
    if (!s2::nch_ok(nch) || (tw != 8 && tw != 16)) {
      printf("tile %d %d %d %d: not covered\n", esz, th, tw, cin);
      bad = 1;
      continue;
    }
    // requests
    std::vector<int> holds(nslots, -1);   // slot -> (ry * r0w + rx) * nch + chunk
    const int nreq = s2::requests(r0h, r0w, nch);
    if (nreq != r0h * r0w * nch || s2::loads(r0h, r0w, nch, nt) * nt < nreq || (s2::loads(r0h, r0w, nch, nt) - 1) * nt >= nreq) bad = 1;
    for (int s = 0; s < nreq; ++s) {
      const s2::Request r = s2::request(s, r0w, nch);
      if (r.ry < 0 || r.ry >= r0h || r.rx < 0 || r.rx >= r0w || r.chunk < 0 || r.chunk >= nch || (r.ry * r0w + r.rx) * nch + r.chunk != s) { bad = 1; continue; }
      const int slot = s2::slot(s2::pixel(r.ry, r.rx, P, H), r.chunk, nch);
      if (slot < 0 || slot >= nslots || holds[slot] != -1) { bad = 1; continue; }
      holds[slot] = s;
    }
    // fragment reads
    long reads = 0, extra_new = 0, extra_old = 0;
    int worst_new = 0, worst_old = 0;
    for (int sub = 0; sub < ms; ++sub)
      for (int kb = 0; kb < kb_n; ++kb) {
        const int tap = kb / cb_n, cb = kb - tap * cb_n, ky = tap / 3, kx = tap - 3 * ky;
        int now[64], old[64];
        for (int lane = 0; lane < 64; ++lane) {
          const int l15 = lane & 15, lq = lane >> 4;
          int pp = sub * 16 + l15;
          pp = pp < bm ? pp : bm - 1;
          const int yy = pp / tw, x = pp % tw, chunk = cb * 4 + lq;
          const int row0 = s2::pixel(2 * yy, 2 * x, P, H);                      // as the kernel forms the address: per-lane base ...
          now[lane] = s2::slot(row0 + s2::pixel(ky, kx, P, H), chunk, nch);     // ... plus the tap's compile-time offset
          const int ry = 2 * yy + ky, rx = 2 * x + kx;
          if (now[lane] < 0 || now[lane] >= nslots || holds[now[lane]] != (ry * r0w + rx) * nch + chunk) bad = 1;
          old[lane] = old_slot(2 * (yy * r0w + x) + ky * r0w + kx, chunk, nch);
        }
        const int en = extra_cycles(now), eo = extra_cycles(old);
        extra_new += en;
        extra_old += eo;
        worst_new = en > worst_new ? en : worst_new;
        worst_old = eo > worst_old ? eo : worst_old;
        ++reads;
      }
    if (extra_new) bad = 1;
    printf("tile esz %d %dx%d cin %d: pitch %d px, image %d bytes, %ld fragment reads, extra LDS cycles per read: %.2f (worst %d); stride-1 image: %.2f (worst %d)\n",
           esz, th, tw, cin, P, nslots * 16, reads, (double)extra_new / reads, worst_new, (double)extra_old / reads, worst_old);
  }
  return bad;
}
