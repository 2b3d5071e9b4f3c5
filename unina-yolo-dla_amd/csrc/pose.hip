// The camera's pose from the tracked cones: one stateless launch per frame in front of unina_track_update_async
// (include/unina_mi355.h "pose from the tracked cones"; pose.pose_numpy is the definition, bit for bit). The frame's located cones
// are aligned with the tracker's confirmed tracks by a planar rigid correction (yaw about z, tx, ty); the corrected pose stays on
// the device for the next frame's call, the cones leave in the tracking frame, and the tracker behind runs with the identity.
//
// Work split. ONE workgroup of 1024 threads (16 waves), the tracker's shape; thread t owns record t AND slot t.
//   setup      the prior P = prev o inc (or inc) in every thread's registers; the own record's point under P; the landmarks --
//              slots with enough hits inside the field -- compacted in ascending slot order into LDS as (x, y, z, class), 16 KB,
//              read as broadcasts.
//   iteration  A usable record moves its point by the correction in LDS and walks the WHOLE landmark list: per gated pair it keeps
//              its own minimum of (d2, k) in a register and sends (d2 bits << 32 | record) to the landmark's 64-bit LDS minimum
//              (ds_min_u64; double-buffered, as in the tracker). Barrier. A record whose landmark's minimum names it is a pair: its
//              seven integer terms are folded over the wave by shuffles and added to LDS by 64-bit integer adds, the largest d2 by
//              an integer maximum. Barrier. Thread 0 turns the sums into (c, s, tx, ty) in float64 and fp32 and leaves them in LDS.
//              Three barriers an iteration. No float atomic anywhere: the bytes do not depend on the order of arrival.
//   tail       every thread moves and stores its record (records behind the count are copied), thread 0 the result and the header.
// The tracker's shrinking walk range does not carry over: there the candidates of a record only became fewer, here the points move
// between iterations and a landmark outside the gate now may be inside it next time. A walk is not bounded at all; waves without a
// usable record skip it. What is bounded is the number of walks: an iteration is a pure function of the correction it starts from
// (the points, the landmarks and the parameters do not change), and it solves for the whole correction from the unmoved points. So
// when an iteration returns the very bits it started from, every later one would repeat it -- the same pairs, sums, correction,
// status, n_pairs and max_d2 -- and the loop ends with `iterations` set as if they had run. Once the set of pairs has settled
// that happens one iteration later. Cost: walks x (n_landmarks LDS broadcasts and distances per usable record + 3 barriers).
#include <hip/hip_runtime.h>

#include "pose_math.h"
#include "record_io.h"
#include "wave_block.h"

namespace unina {
namespace {

constexpr int kPoseBlock = 1024;
constexpr int kPoseWaves = kPoseBlock / kWave;

static_assert(UNINA_TRACK_MAX == kPoseBlock && MAX_DETECTIONS == kPoseBlock, "a thread owns one record and one slot");
static_assert(sizeof(unina_pose_params) == 68 && sizeof(unina_pose_result) == 64 && sizeof(unina_pose_header) == 32, "pose layouts");
static_assert(UNINA_POSE_OK == kPoseOk && UNINA_POSE_TOO_FEW == kPoseTooFew && UNINA_POSE_DEGENERATE == kPoseDegenerate, "status codes");

struct PoseArgs {
  float inc[12];
  float gate2;
  int class_aware, min_hits, iterations, min_pairs;
};

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;   // lane 0 holds the wave's sum
}

// cones / out_cones and prev / result may be the same arrays: no __restrict__ on them
__global__ void __launch_bounds__(kPoseBlock) pose_kernel(const GpuDetection* __restrict__ dets, const int* __restrict__ d_count,
                                                          const unina_cone3d* cones, const unina_track* __restrict__ tracks,
                                                          const unina_pose_result* prev, PoseArgs a, unina_cone3d* out_cones,
                                                          unina_pose_result* result, unina_pose_header* __restrict__ hdr) {
  __shared__ float4 s_lm[kPoseBlock];                                   // landmark k: x, y, z, class bits
  __shared__ __align__(16) unsigned long long s_best[2][kPoseBlock];    // landmark k: min (d2 bits << 32 | record) of the iteration
  __shared__ unsigned long long s_sum[8];                               // N, Spx, Spy, Smx, Smy, Sdot, Scross of the iteration
  __shared__ float s_corr[4];                                           // c, s, tx, ty
  __shared__ unsigned s_maxd2[2];                                       // of the pairing under way, of the last pairing made
  __shared__ int s_ctl[4];                                              // stop, status, iterations that updated, pairs of the last pairing
  __shared__ int s_wave[kPoseWaves];                                    // block_rank's, and only its

  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1);
  const int n = record_count(d_count);

  // ---- setup: the prior, the own record's point, the own slot
  float P[12];
  if (prev) {
    RecordWords<unina_pose_result> pw = load_record(prev);
    pose_compose(pw.r.pose, a.inc, P);
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = a.inc[i];
  }
  RecordWords<unina_cone3d> cw = load_record(cones + tid);
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  int rcls = 0;
  bool usable = false;
  if (tid < n) {
    const uint4 d = reinterpret_cast<const uint4*>(dets + tid)[1];      // confidence, class_id, valid, _pad
    const TrackPoint p = track_point(P, cw.r.x, cw.r.y, cw.r.z, cw.r.valid);
    px = p.x;
    py = p.y;
    pz = p.z;
    usable = pose_usable(p);
    rcls = (int)d.y;
  }
  const RecordWords<unina_track> tw = load_record(tracks + tid);
  const bool lm = pose_landmark(tw.r.id, tw.r.hits, tw.r.x, tw.r.y, a.min_hits);
  s_best[0][tid] = kTrackNoKey;
  s_best[1][tid] = kTrackNoKey;
  if (tid < 8) s_sum[tid] = 0ull;
  if (tid < 4) {
    s_corr[tid] = tid == 0 ? 1.0f : 0.0f;
    s_ctl[tid] = 0;
  }
  if (tid < 2) s_maxd2[tid] = 0u;
  int n_list, n_usable;
  const int k_own = block_rank<kPoseWaves>(lm, s_wave, &n_list);        // the own slot's place in the landmark list
  if (lm) s_lm[k_own] = make_float4(tw.r.x, tw.r.y, tw.r.z, __int_as_float(tw.r.class_id));
  (void)block_rank<kPoseWaves>(usable, s_wave, &n_usable);

  // ---- the iterations: one round of mutual nearest neighbours, the sums, the closed form
  for (int it = 0; it < a.iterations; ++it) {
    __syncthreads();                                                    // the landmark list, the correction, the cleared minima and sums
    if (s_ctl[0]) break;                                                // too few pairs, or a fixed point: the same word for every thread
    const PoseCorr k = {s_corr[0], s_corr[1], s_corr[2], s_corr[3]};
    unsigned long long* const best = s_best[it & 1];
    unsigned long long mine = kTrackNoKey;
    if (usable) {
      float qx, qy;
      pose_move(k, px, py, &qx, &qy);
      const auto visit = [&](int kk, const float4& t, float d2) {
        if (track_gated(d2, a.gate2) && (a.class_aware == 0 || __float_as_int(t.w) == rcls)) {
          const unsigned long long key = track_key(d2, (uint32_t)kk);
          mine = key < mine ? key : mine;
          atomicMin(&best[kk], track_key(d2, (uint32_t)tid));
        }
      };
      int kk = 0;
      for (; kk + 4 <= n_list; kk += 4) {   // four broadcasts in flight, then four distances: the LDS latency is paid once per four
        const float4 t0 = s_lm[kk], t1 = s_lm[kk + 1], t2 = s_lm[kk + 2], t3 = s_lm[kk + 3];
        const float d0 = track_d2(qx, qy, pz, t0.x, t0.y, t0.z), d1 = track_d2(qx, qy, pz, t1.x, t1.y, t1.z);
        const float d2 = track_d2(qx, qy, pz, t2.x, t2.y, t2.z), d3 = track_d2(qx, qy, pz, t3.x, t3.y, t3.z);
        visit(kk, t0, d0);
        visit(kk + 1, t1, d1);
        visit(kk + 2, t2, d2);
        visit(kk + 3, t3, d3);
      }
      for (; kk < n_list; ++kk) {
        const float4 t = s_lm[kk];
        visit(kk, t, track_d2(qx, qy, pz, t.x, t.y, t.z));
      }
    }
    __syncthreads();
    bool pair = false;
    PoseSums t = {0, 0, 0, 0, 0, 0, 0};
    if (mine != kTrackNoKey) {
      const int kk = (int)(uint32_t)mine;
      if (best[kk] == ((mine & 0xffffffff00000000ull) | (unsigned long long)tid)) {
        pair = true;
        const float4 m = s_lm[kk];
        pose_terms(px, py, m.x, m.y, &t);
      }
    }
    const unsigned long long pairs = __ballot(pair);
    if (pairs) {                                                        // wave-uniform: every lane takes part in the shuffles
      const long long spx = wave_sum_ll(t.px), spy = wave_sum_ll(t.py), smx = wave_sum_ll(t.mx), smy = wave_sum_ll(t.my);
      const long long sdot = wave_sum_ll(t.dot), scross = wave_sum_ll(t.cross);
      unsigned d2max = pair ? (unsigned)(mine >> 32) : 0u;
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_down((int)d2max, off, kWave);
        d2max = o > d2max ? o : d2max;
      }
      if (lane == 0) {
        atomicAdd(&s_sum[0], (unsigned long long)__popcll(pairs));
        atomicAdd(&s_sum[1], (unsigned long long)spx);
        atomicAdd(&s_sum[2], (unsigned long long)spy);
        atomicAdd(&s_sum[3], (unsigned long long)smx);
        atomicAdd(&s_sum[4], (unsigned long long)smy);
        atomicAdd(&s_sum[5], (unsigned long long)sdot);
        atomicAdd(&s_sum[6], (unsigned long long)scross);
        atomicMax(&s_maxd2[0], d2max);
      }
    }
    s_best[(it + 1) & 1][tid] = kTrackNoKey;                            // last read in the iteration before this one
    __syncthreads();
    if (tid == 0) {
      const PoseSums u = {(long long)s_sum[0], (long long)s_sum[1], (long long)s_sum[2], (long long)s_sum[3],
                          (long long)s_sum[4], (long long)s_sum[5], (long long)s_sum[6]};
      s_ctl[3] = (int)u.n;
      s_maxd2[1] = s_maxd2[0];
      s_maxd2[0] = 0u;
      if (u.n < (long long)a.min_pairs) {
        s_ctl[0] = 1;
        s_ctl[1] = kPoseTooFew;
      } else {
        PoseCorr c;
        s_ctl[1] = pose_solve(u, &c);
        if (track_bits(c.c) == track_bits(s_corr[0]) && track_bits(c.s) == track_bits(s_corr[1]) && track_bits(c.tx) == track_bits(s_corr[2]) &&
            track_bits(c.ty) == track_bits(s_corr[3])) {
          s_ctl[0] = 1;                                                 // a fixed point: every later iteration would repeat this one, bit for bit
          s_ctl[2] = a.iterations;
        } else {
          s_corr[0] = c.c;
          s_corr[1] = c.s;
          s_corr[2] = c.tx;
          s_corr[3] = c.ty;
          s_ctl[2] = it + 1;
        }
      }
#pragma unroll
      for (int i = 0; i < 7; ++i) s_sum[i] = 0ull;                      // the next adds come two barriers later
    }
  }
  __syncthreads();

  // ---- tail: the records in the tracking frame, the result, the header
  const PoseCorr k = {s_corr[0], s_corr[1], s_corr[2], s_corr[3]};
  if (tid < n) {
    float qx, qy;
    pose_move(k, px, py, &qx, &qy);
    cw.r.x = qx;
    cw.r.y = qy;
    cw.r.z = pz;
  }
  store_record(out_cones + tid, cw);
  if (tid == 0) {
    RecordWords<unina_pose_result> r;
    pose_corrected(k, P, r.r.pose);
    r.r.c = k.c;
    r.r.s = k.s;
    r.r.tx = k.tx;
    r.r.ty = k.ty;
    store_record(result, r);
    RecordWords<unina_pose_header> h;
    h.r.n_records = n;
    h.r.n_usable = n_usable;
    h.r.n_landmarks = n_list;
    h.r.n_pairs = s_ctl[3];
    h.r.iterations = s_ctl[2];
    h.r.status = s_ctl[1];
    h.r.max_d2_bits = s_maxd2[1];
    h.r.reserved = 0;
    store_record(hdr, h);
  }
}

bool apart_or_same(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x == y || x + bytes <= y || y + bytes <= x;
}

}  // namespace
}  // namespace unina

extern "C" int unina_pose_async(const GpuDetection* d_dets, const int* d_count, const unina_cone3d* d_cones, const unina_track* d_tracks,
                                const unina_pose_result* d_prev, const unina_pose_params* p, unina_cone3d* d_out_cones,
                                unina_pose_result* d_result, unina_pose_header* d_header, hipStream_t stream) {
  using namespace unina;
  if (!p || !record_io_ok(d_dets, d_count, d_cones) || !d_tracks || !d_out_cones || !d_result || !d_header) return UNINA_ERR_ARG;
  if (((uintptr_t)d_tracks & 15) || ((uintptr_t)d_prev & 15) || ((uintptr_t)d_out_cones & 15) || ((uintptr_t)d_result & 15) ||
      ((uintptr_t)d_header & 15))
    return UNINA_ERR_ARG;
  if (!apart_or_same(d_cones, d_out_cones, sizeof(unina_cone3d) * MAX_DETECTIONS)) return UNINA_ERR_ARG;
  if (d_prev && !apart_or_same(d_prev, d_result, sizeof(unina_pose_result))) return UNINA_ERR_ARG;
  for (int i = 0; i < 12; ++i)
    if (!unina::finite(p->inc[i])) return UNINA_ERR_ARG;
  if (!(p->gate > 0.0f && unina::finite(p->gate * p->gate))) return UNINA_ERR_ARG;
  if (p->min_hits < 1 || p->iterations < 1 || p->iterations > UNINA_POSE_MAX_ITERATIONS || p->min_pairs < 2) return UNINA_ERR_ARG;
  if (hipMemsetAsync(d_header, 0, sizeof(unina_pose_header), stream) != hipSuccess) return UNINA_ERR_HIP;
  PoseArgs a;
  for (int i = 0; i < 12; ++i) a.inc[i] = p->inc[i];
  a.gate2 = p->gate * p->gate;
  a.class_aware = p->class_aware;
  a.min_hits = p->min_hits;
  a.iterations = p->iterations;
  a.min_pairs = p->min_pairs;
  hipLaunchKernelGGL(pose_kernel, dim3(1), dim3(kPoseBlock), 0, stream, d_dets, d_count, d_cones, d_tracks, d_prev, a, d_out_cones, d_result,
                     d_header);
  return launch_status();
}
