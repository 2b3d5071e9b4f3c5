// Track limits and centre line from the tracked cones: one stateless launch per frame behind unina_track_update_async
// (include/unina_mi355.h "track limits and centre line"; boundary.boundary_numpy is the definition, bit for bit). The confirmed
// tracks of the left and of the right class are chained from the vehicle onwards into two ordered polylines, and the two chains
// are walked as a ladder whose rungs' midpoints are the centre line. The table and the pose are read where the tracker and
// unina_pose_async left them on the device.
//
// Work split. ONE workgroup of 1024 threads (16 waves), the tracker's shape; thread t owns slot t.
//   setup    the pose, the origin and the heading in every thread's registers (NO_HEADING: zeros and out, wave-uniform, in front
//            of every barrier); the own slot's side; the candidates of each side compacted in ascending slot order into LDS as
//            (x, y, z, id) by block_rank, 2 x 16 KB. Ascending list index is ascending slot, so the key (d2 bits, list index)
//            orders as the definition's (d2 bits, slot).
//   chains   ONE wave per side (wave 0 left, wave 1 right) walks its chain with no barrier: per link a lane tests the list
//            entries lane, lane + 64, ... (ceil(n / 64) LDS reads, four in flight), keeps its least key and that entry's (x, y)
//            in registers; the wave's least d2 word comes from six data-parallel (DPP) steps in the vector unit, the least entry
//            among the lanes that hold it from a ballot (one lane, but for a tie), the winner's (x, y) from two v_readlane: no
//            LDS access between a link's reads and the next link's. The winning lane sets the entry's bit in its own mask of
//            used entries (16 bits are enough) and copies the entry to the chain. The sides end on their own; the other 14
//            waves wait at the barrier behind.
//   ladder   all threads fill the nL x nR table of d2(L[i], R[j]) in LDS (16 KB, at most 4 entries a thread); thread 0 walks
//            it: a rung is two LDS reads (the two ways on) and a compare, the rung's (i, j) goes to LDS, the midpoints are
//            left to the tail.
//   tail     threads 0..255 store one point each (a chain point, a rung's midpoint or zeros), thread 0 the header.
// The form kept is this one, not the pose kernel's barrier per link with every thread on its own slot, which was not built: a
// link there is a 1024-thread barrier, an LDS 64-bit minimum over all waves and a second barrier, 64 times over for a full chain
// and once per side, where here a link is one wave's LDS read, about forty vector instructions and three v_readlane, and the two
// sides run side by side. A first version of this form took the wave's minimum of the 64-bit key by six __shfl_xor steps (twelve
// ds_bpermute) and read the winner's entry back from LDS, one list read in flight: it measured 0.053 ms on 36 + 36 cones and
// 0.188 ms on 960 + 64 candidates with two full chains. Cost: links x (ceil(n / 256) LDS latencies + the tests + the minimum) per
// side, then the table fill and at most 127 rungs of two dependent LDS reads on one lane. No float atomic, no atomic at all, no
// cross-workgroup wait: the bytes do not depend on the order of arrival.
#include <hip/hip_runtime.h>

#include "boundary_math.h"
#include "record_io.h"
#include "wave_block.h"

namespace unina {
namespace {

constexpr int kBoundaryBlock = 1024;
constexpr int kBoundaryWaves = kBoundaryBlock / kWave;
constexpr int kBoundaryPoints = 4 * kBoundaryMaxChain;

static_assert(UNINA_TRACK_MAX == kBoundaryBlock, "a thread owns one slot");
static_assert(UNINA_BOUNDARY_MAX_CHAIN == kBoundaryMaxChain && kBoundaryMaxChain == kWave, "a chain is at most one wave long");
static_assert(kBoundaryBlock / kWave <= 32, "the used entries of a lane fit one 32-bit mask");
static_assert(sizeof(unina_boundary_params) == 92 && sizeof(unina_boundary_point) == 16 && sizeof(unina_boundary_header) == 32, "boundary layouts");
static_assert(UNINA_BOUNDARY_NO_FIRST == kBoundaryNoFirst && UNINA_BOUNDARY_NO_NEXT == kBoundaryNoNext && UNINA_BOUNDARY_FULL == kBoundaryFull &&
                  UNINA_BOUNDARY_NO_HEADING == kBoundaryNoHeading, "end codes");

struct BoundaryArgs {
  float pose[12], forward[3];
  float first2, step2, cos2, width2;
  int class_left, class_right, min_hits, max_chain;
};

// The wave's least 32-bit word, in every lane: four row_shr steps fold a row of 16 lanes into its lane 15, row_bcast:15 folds rows
// 0 and 2 into rows 1 and 3, row_bcast:31 the lower half into the upper one, lane 63 holds the result. Data-parallel moves in the
// vector unit, no LDS crossbar as under __shfl. A lane without a source keeps the identity. Every lane of the wave calls it.
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned dpp_min_step(unsigned v) {
  const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROWS, 0xf, false);
  return o < v ? o : v;
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  v = dpp_min_step<0x111, 0xf>(v);   // row_shr:1
  v = dpp_min_step<0x112, 0xf>(v);   // row_shr:2
  v = dpp_min_step<0x114, 0xf>(v);   // row_shr:4
  v = dpp_min_step<0x118, 0xf>(v);   // row_shr:8
  v = dpp_min_step<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v = dpp_min_step<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
  return (unsigned)__builtin_amdgcn_readlane((int)v, kWave - 1);
}

__device__ __forceinline__ BoundaryPoint as_point(const float4& v) { return {v.x, v.y, v.z, __float_as_int(v.w)}; }

__global__ void __launch_bounds__(kBoundaryBlock) boundary_kernel(const unina_track* __restrict__ tracks, const unina_pose_result* __restrict__ d_pose,
                                                                  BoundaryArgs a, unina_boundary_point* __restrict__ points,
                                                                  unina_boundary_header* __restrict__ hdr) {
  __shared__ float4 s_cand[2][kBoundaryBlock];                          // side k, list entry e: x, y, z, id bits
  __shared__ float4 s_chain[2][kBoundaryMaxChain];                      // side k, link m: the same four words
  __shared__ float s_d2[kBoundaryMaxChain * kBoundaryMaxChain];         // d2(L[i], R[j]) at i * 64 + j
  __shared__ int s_rung[2 * kBoundaryMaxChain];                         // centre point c: i | j << 16
  __shared__ int s_n[2], s_end[2], s_centre[2];                         // links and end of a side; n_centre, n_wide
  __shared__ int s_wave[kBoundaryWaves];                                // block_rank's, and only its

  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wid = tid >> 6;

  // ---- setup: the origin and the heading, the own slot's side, the two candidate lists
  float P[12];
  if (d_pose) {
    const RecordWords<unina_pose_result> pw = load_record(d_pose);
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = pw.r.pose[i];
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = a.pose[i];
  }
  const BoundaryStart st = boundary_start(P, a.forward);
  if (!st.ok) {                                                         // the same words for every thread: nobody reaches a barrier
    if (tid < kBoundaryPoints) store_zero_record(points + tid);
    if (tid == 0) {
      RecordWords<unina_boundary_header> h;
      zero_record(h);
      h.r.end[0] = h.r.end[1] = kBoundaryNoHeading;
      store_record(hdr, h);
    }
    return;
  }
  const RecordWords<unina_track> tw = load_record(tracks + tid);
  const int side = boundary_side(tw.r.id, tw.r.hits, tw.r.class_id, tw.r.x, tw.r.y, a.min_hits, a.class_left, a.class_right);
  int n_cand[2];
  const int e_left = block_rank<kBoundaryWaves>(side == 0, s_wave, &n_cand[0]);
  const int e_right = block_rank<kBoundaryWaves>(side == 1, s_wave, &n_cand[1]);
  if (side >= 0) s_cand[side][side == 0 ? e_left : e_right] = make_float4(tw.r.x, tw.r.y, tw.r.z, __int_as_float(tw.r.id));
  __syncthreads();

  // ---- the chains: wave 0 the left one, wave 1 the right one, no barrier inside
  if (wid < 2) {
    const float4* const cand = s_cand[wid];
    const int n = n_cand[wid], rounds = (n + kWave - 1) >> 6;             // rounds <= 16
    float cx = st.ox, cy = st.oy, ddx = st.hx, ddy = st.hy;
    unsigned used = 0u;                                                 // bit r: the entry lane + 64 r is in the chain
    int m = 0, end;
    for (;;) {
      if (m == a.max_chain) {
        end = kBoundaryFull;
        break;
      }
      const bool first = m == 0;
      const float gate2 = first ? a.first2 : a.step2;
      unsigned long long key = kTrackNoKey;                             // the lane's least (d2 bits, entry), and that entry's place
      float bx = 0.0f, by = 0.0f;
      const auto visit = [&](int r, const float4& c) {
        float d2;
        if (lane + kWave * r < n && !((used >> r) & 1u) && boundary_eligible(first, cx, cy, ddx, ddy, c.x, c.y, gate2, a.cos2, &d2)) {
          const unsigned long long k = track_key(d2, (uint32_t)(lane + kWave * r));
          if (k < key) key = k, bx = c.x, by = c.y;
        }
      };
      for (int r = 0; r < rounds; r += 4) {   // four reads in flight, then four tests: the LDS latency is paid once per four (r + k <= 15: inside the list)
        const float4 c0 = cand[lane + kWave * r], c1 = cand[lane + kWave * min(r + 1, kBoundaryWaves - 1)];
        const float4 c2 = cand[lane + kWave * min(r + 2, kBoundaryWaves - 1)], c3 = cand[lane + kWave * min(r + 3, kBoundaryWaves - 1)];
        visit(r, c0);
        if (r + 1 < rounds) visit(r + 1, c1);
        if (r + 2 < rounds) visit(r + 2, c2);
        if (r + 3 < rounds) visit(r + 3, c3);
      }
      // the wave's least key: the least d2 word over the lanes, then the least entry among the lanes that hold it (one, but for a tie)
      const unsigned bits = (unsigned)(key >> 32), least = wave_min_u32(bits);   // wave-uniform from here: every lane takes the same way
      if (least == ~0u) {                                               // no lane has a key: a d2 inside a finite gate is below +inf's bits
        end = first ? kBoundaryNoFirst : kBoundaryNoNext;
        break;
      }
      unsigned long long tied = __ballot(bits == least);
      int winner = __ffsll((long long)tied) - 1, e = __builtin_amdgcn_readlane((int)(unsigned)key, winner);
      for (tied &= tied - 1; tied; tied &= tied - 1) {
        const int l = __ffsll((long long)tied) - 1, v = __builtin_amdgcn_readlane((int)(unsigned)key, l);
        if (v < e) e = v, winner = l;
      }
      const float wx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bx), winner));
      const float wy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(by), winner));
      if (lane == winner) {                                             // e = winner + 64 r < n <= 1024, m < max_chain <= 64
        used |= 1u << (e >> 6);
        s_chain[wid][m] = cand[e];                                      // off the links' critical path
      }
      boundary_turn(m, cx, cy, wx, wy, &ddx, &ddy);
      cx = wx;
      cy = wy;
      ++m;
    }
    if (lane == 0) {
      s_n[wid] = m;
      s_end[wid] = end;
    }
  }
  __syncthreads();

  // ---- the ladder: the table of rung lengths by everyone, the walk by thread 0
  const int nl = s_n[0], nr = s_n[1];
  if (nl > 0 && nr > 0) {                                               // the same words for every thread
    for (int e = tid; e < kBoundaryMaxChain * kBoundaryMaxChain; e += kBoundaryBlock) {
      const int i = e >> 6, j = e & (kBoundaryMaxChain - 1);
      if (i < nl && j < nr) {
        const float4 l = s_chain[0][i], r = s_chain[1][j];
        s_d2[e] = boundary_d2(l.x, l.y, r.x, r.y);
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    int n_centre = 0, n_wide = 0;
    if (nl > 0 && nr > 0) {
      int i = 0, j = 0;
      float w2 = s_d2[0];
      for (;;) {                                                        // nl + nr - 1 <= 127 rungs
        if (track_gated(w2, a.width2)) {
          s_rung[n_centre++] = i | (j << 16);
        } else {
          ++n_wide;
        }
        const bool has_i = i + 1 < nl, has_j = j + 1 < nr;
        if (!has_i && !has_j) break;
        const float fa = has_i ? s_d2[(i + 1) * kBoundaryMaxChain + j] : 0.0f, fb = has_j ? s_d2[i * kBoundaryMaxChain + j + 1] : 0.0f;
        if (boundary_advance_left(has_i, has_j, fa, fb)) {
          ++i;
          w2 = fa;
        } else {
          ++j;
          w2 = fb;
        }
      }
    }
    s_centre[0] = n_centre;
    s_centre[1] = n_wide;
  }
  __syncthreads();

  // ---- tail: the 256 points, the header
  if (tid < kBoundaryPoints) {
    RecordWords<unina_boundary_point> o;
    zero_record(o);
    if (tid < 2 * kBoundaryMaxChain) {
      const int k = tid >> 6, m = tid & (kBoundaryMaxChain - 1);
      if (m < s_n[k]) {
        const BoundaryPoint p = as_point(s_chain[k][m]);
        o.r.x = p.x, o.r.y = p.y, o.r.z = p.z, o.r.ref = p.ref;
      }
    } else if (tid - 2 * kBoundaryMaxChain < s_centre[0]) {
      const int ref = s_rung[tid - 2 * kBoundaryMaxChain], i = ref & 0xffff, j = ref >> 16;
      const BoundaryPoint p = boundary_rung(as_point(s_chain[0][i]), as_point(s_chain[1][j]), i, j);
      o.r.x = p.x, o.r.y = p.y, o.r.z = p.z, o.r.ref = p.ref;
    }
    store_record(points + tid, o);
  }
  if (tid == 0) {
    RecordWords<unina_boundary_header> h;
    h.r.n_candidates[0] = n_cand[0];
    h.r.n_candidates[1] = n_cand[1];
    h.r.n_chain[0] = nl;
    h.r.n_chain[1] = nr;
    h.r.end[0] = s_end[0];
    h.r.end[1] = s_end[1];
    h.r.n_centre = s_centre[0];
    h.r.n_wide = s_centre[1];
    store_record(hdr, h);
  }
}

bool gate_ok(float g) { return g > 0.0f && unina::finite(g) && unina::finite(g * g); }

}  // namespace
}  // namespace unina

extern "C" int unina_boundary_async(const unina_track* d_tracks, const unina_pose_result* d_pose, const unina_boundary_params* p,
                                    unina_boundary_point* d_points, unina_boundary_header* d_header, hipStream_t stream) {
  using namespace unina;
  if (!d_tracks || !p || !d_points || !d_header) return UNINA_ERR_ARG;
  if (((uintptr_t)d_tracks & 15) || ((uintptr_t)d_pose & 15) || ((uintptr_t)d_points & 15) || ((uintptr_t)d_header & 15)) return UNINA_ERR_ARG;
  if (!d_pose)
    for (int i = 0; i < 12; ++i)
      if (!unina::finite(p->pose[i])) return UNINA_ERR_ARG;
  for (int i = 0; i < 3; ++i)
    if (!unina::finite(p->forward[i])) return UNINA_ERR_ARG;
  if (!gate_ok(p->first_gate) || !gate_ok(p->step_gate) || !gate_ok(p->width_gate)) return UNINA_ERR_ARG;
  if (!(p->cos_turn >= 0.0f && p->cos_turn < 1.0f)) return UNINA_ERR_ARG;   // a NaN fails
  if (p->min_hits < 1 || p->max_chain < 1 || p->max_chain > UNINA_BOUNDARY_MAX_CHAIN) return UNINA_ERR_ARG;
  if (p->class_left < 0 || p->class_right < 0 || p->class_left == p->class_right) return UNINA_ERR_ARG;
  const uintptr_t pts = (uintptr_t)d_points, head = (uintptr_t)d_header;
  if (pts < head + sizeof(unina_boundary_header) && head < pts + sizeof(unina_boundary_point) * kBoundaryPoints) return UNINA_ERR_ARG;
  if (hipMemsetAsync(d_header, 0, sizeof(unina_boundary_header), stream) != hipSuccess) return UNINA_ERR_HIP;
  BoundaryArgs a;
  for (int i = 0; i < 12; ++i) a.pose[i] = d_pose ? 0.0f : p->pose[i];
  for (int i = 0; i < 3; ++i) a.forward[i] = p->forward[i];
  a.first2 = p->first_gate * p->first_gate;
  a.step2 = p->step_gate * p->step_gate;
  a.cos2 = p->cos_turn * p->cos_turn;
  a.width2 = p->width_gate * p->width_gate;
  a.class_left = p->class_left;
  a.class_right = p->class_right;
  a.min_hits = p->min_hits;
  a.max_chain = p->max_chain;
  hipLaunchKernelGGL(boundary_kernel, dim3(1), dim3(kBoundaryBlock), 0, stream, d_tracks, d_pose, a, d_points, d_header);
  return launch_status();
}
