// LiDAR cone candidates fused with camera records on the device: one launch behind unina_cluster_async and a locator, in front of
// ONE unina_track_update_async (include/unina_mi355.h "fusion of LiDAR cone candidates with camera records"; fusion.fuse_numpy is
// the definition, bit for bit). The call is stateless: it reads the two record lists and writes one, with a link per record.
//
// The association is the greedy matching over all candidate pairs in ascending (d2 bits, camera record i, LiDAR cone j). It is
// computed as rounds of MUTUAL NEAREST NEIGHBOURS, which give the same matching: in a round every free boxed record takes the
// minimum of (d2, j) over its free candidate cones, every free projected cone the minimum of (d2, i) over its free candidate
// records, and every pair that chose each other is matched. The least free pair in (d2, i, j) order is always mutual: a free pair
// (d2', i, j') below the record's choice (d2, j) would be below the least pair in (d2, i, j) order, and a free pair (d2', i', j)
// below the cone's choice (d2, i) likewise. So a round with a free candidate pair matches at least one, and the loop ends after at
// most min(nc, nl) rounds. And a mutual pair (d2, i, j) is preceded in (d2, i, j) order by no free pair that shares its record --
// that pair would have a smaller (d2', j') -- or its cone -- a smaller (d2', i') -- so the greedy loop, which has taken exactly
// the pairs of the earlier rounds when it reaches this one, takes it too. All counters are integers, every minimum is over
// unsigned keys and every fp32 operation has one fixed place in one fixed order (csrc/fuse_math.h; the unit is compiled with
// -ffp-contract=off): two runs give the same bytes, and they are numpy's.
//
// Work split. ONE workgroup of 1024 threads (16 waves); thread t owns camera record t AND LiDAR cone t, both held in registers.
//   setup    the projected cones are compacted in ascending j into LDS as (u, v, zc, j) -- 16 KB, read as broadcasts; a cone's
//            transformed point stays in its thread's registers for the tail.
//   round    camera side: an active record walks its part of the list; per free candidate it keeps its own minimum (d2, list
//            index -- the list is in ascending j) in a register and sends (d2 bits << 32 | i) to the entry's 64-bit LDS minimum
//            (ds_min_u64; a minimum does not depend on the order of arrival). Barrier. A record whose entry's minimum names it is
//            matched: it leaves its index with the entry and overwrites the entry's u with NaN, which fails every later gate. A
//            record that found no candidate can never find one again (cones only get taken) and retires. The minima are
//            double-buffered, so a round costs two barriers. Waves without an active record skip the walk. A record keeps the
//            index range between the first and the last free candidate of its last walk: candidates only become fewer.
//   tail     a matched cone's thread writes the fused cone into its record's slot; one prefix scan (ballot + 16 wave totals) ranks
//            the usable unmatched cones into the slots behind the camera's; everything at and beyond n_written is zeroed. Records,
//            links and d_lidar_slot leave as 16-byte vector stores.
// Expected: a box gates the few cones whose pixels fall into it, so one or two rounds finish the frame; the worst case is a chain of
// shrinking gaps, one pair per round. tools/bench_fuse.py times a typical frame, two full lists and the 64-round chain.
#include <hip/hip_runtime.h>

#include "fuse_math.h"
#include "record_io.h"
#include "wave_block.h"

namespace unina {
namespace {

constexpr int kFuseBlock = 1024;
constexpr int kFuseWaves = kFuseBlock / kWave;

static_assert(MAX_DETECTIONS == kFuseBlock, "a thread owns one camera record, one LiDAR cone and one output slot");
static_assert(sizeof(unina_cone3d) == 32 && sizeof(GpuDetection) == 32 && sizeof(unina_fuse_link) == 16 && sizeof(unina_fuse_header) == 32,
              "record layouts");
static_assert(sizeof(unina_fuse_params) == 100, "parameter layout");

__global__ void __launch_bounds__(kFuseBlock) fuse_kernel(const GpuDetection* __restrict__ dets, const int* __restrict__ d_count,
                                                          const unina_cone3d* __restrict__ cones, const GpuDetection* __restrict__ ldets,
                                                          const int* __restrict__ d_lcount, const unina_cone3d* __restrict__ lcones,
                                                          unina_fuse_params a, GpuDetection* __restrict__ out_dets, int* __restrict__ out_count,
                                                          unina_cone3d* __restrict__ out_cones, unina_fuse_link* __restrict__ links,
                                                          int* __restrict__ lidar_slot, unina_fuse_header* __restrict__ header) {
  __shared__ float4 s_lid[kFuseBlock];                                  // list entry k: u, v, zc, j bits; u = NaN once taken
  __shared__ __align__(16) unsigned long long s_best[2][kFuseBlock];    // list entry k: min (d2 bits << 32 | i) of the round
  __shared__ int s_match[kFuseBlock];                                   // list entry k: the camera record it matched, or -1
  __shared__ __align__(16) int s_slot[kFuseBlock];                      // LiDAR cone j: its output slot, or -1
  __shared__ int s_wave[kFuseWaves];                                    // block_rank's, and only its
  __shared__ int s_matched;

  const int tid = (int)threadIdx.x;
  const int nc = record_count(d_count), nl = record_count(d_lcount);

  // ---- setup: the own camera record, the own LiDAR cone
  RecordWords<GpuDetection> dw;
  RecordWords<unina_cone3d> cw;
  zero_record(dw);
  zero_record(cw);
  FuseBox box;
  box.uc = box.vc = box.hw = box.hh = 0.0f;
  box.boxed = 0;
  if (tid < nc) {
    dw = load_record(dets + tid);
    cw = load_record(cones + tid);
    box = fuse_box(dw.r.x1, dw.r.y1, dw.r.x2, dw.r.y2, a.sx, a.sy, a.grow, a.pad);
  }
  const int has_depth = cw.r.valid != 0 ? 1 : 0;
  const float cz = cw.r.z;

  RecordWords<unina_cone3d> lw;
  zero_record(lw);
  FusePoint lp;
  lp.xc = lp.yc = lp.zc = lp.u = lp.v = 0.0f;
  lp.usable = lp.projected = 0;
  if (tid < nl) {
    lw = load_record(lcones + tid);
    lp = fuse_point(a.level_to_cam, a.cam.fx, a.cam.fy, a.cam.cx, a.cam.cy, a.lift, a.min_depth, a.max_depth, lw.r.x, lw.r.y, lw.r.z,
                    lw.r.valid);
  }
  const bool projected = lp.projected != 0;

  s_best[0][tid] = kFuseNoKey;
  s_best[1][tid] = kFuseNoKey;
  s_match[tid] = -1;
  if (tid == 0) s_matched = 0;
  int n_list;
  const int k_own = block_rank<kFuseWaves>(projected, s_wave, &n_list);   // the own cone's place in the list
  if (projected) s_lid[k_own] = make_float4(lp.u, lp.v, lp.zc, __int_as_float(tid));

  // ---- rounds of mutual nearest neighbours
  bool active = box.boxed != 0 && n_list > 0;
  int matched_j = -1;          // the cone this record matched
  uint32_t matched_d2 = 0u;    // and the bits of the pair's d2
  int lo = 0, hi = n_list;     // the part of the list this record still has to walk
  for (int round = 0; __syncthreads_or(active ? 1 : 0); ++round) {   // the barrier also orders the setup's and the last round's LDS writes
    unsigned long long* const best = s_best[round & 1];
    unsigned long long mine = kFuseNoKey;
    if (active) {
      int first = hi, end = lo;
      for (int k = lo; k < hi; ++k) {
        const float4 t = s_lid[k];
        float d2;
        if (fuse_candidate(t.x, t.y, t.z, box.uc, box.vc, box.hw, box.hh, has_depth, cz, a.range_abs, a.range_rel, &d2)) {
          const unsigned long long key = fuse_key(d2, (uint32_t)k);
          mine = key < mine ? key : mine;
          atomicMin(&best[k], (unsigned long long)fuse_key(d2, (uint32_t)tid));
          first = first < k ? first : k;
          end = k + 1;
        }
      }
      lo = first;   // the free candidates only become fewer: the next walk stays between the first and the last one found now
      hi = end;
    }
    __syncthreads();
    if (active) {
      if (mine == kFuseNoKey) {
        active = false;   // no free candidate now: none later
      } else {
        const int k = (int)(uint32_t)mine;
        if (best[k] == ((mine & 0xffffffff00000000ull) | (unsigned long long)tid)) {
          s_match[k] = tid;
          matched_j = __float_as_int(s_lid[k].w);
          matched_d2 = (uint32_t)(mine >> 32);
          s_lid[k].x = __uint_as_float(0x7fc00000u);
          active = false;
        }
      }
    }
    s_best[(round + 1) & 1][tid] = kFuseNoKey;   // last read in the round before this one
  }

  // ---- tail: the slots of the LiDAR cones
  const int mi = projected ? s_match[k_own] : -1;   // the camera record the own cone matched
  {
    const unsigned long long m = __ballot(matched_j >= 0);
    if ((tid & (kWave - 1)) == 0 && m) atomicAdd(&s_matched, __popcll(m));
  }
  const bool only = lp.usable != 0 && mi < 0;
  int n_only;
  const int kl = block_rank<kFuseWaves>(only, s_wave, &n_only);   // its barriers also order s_matched
  const int n_matched = s_matched;
  const int n_written = fuse_written(nc, n_only, kFuseBlock);
  const int own_slot = mi >= 0 ? mi : ((only && nc + kl < kFuseBlock) ? nc + kl : -1);
  s_slot[tid] = own_slot;

  // camera record tid -> slot tid
  if (tid < nc) {
    store_record(out_dets + tid, dw);
    if (matched_j < 0) store_record(out_cones + tid, cw);
    RecordWords<unina_fuse_link> l;
    l.r.camera = tid;
    l.r.lidar = matched_j;
    l.r.d2 = bits_float(matched_d2);
    l.r.kind = matched_j >= 0 ? UNINA_FUSE_BOTH : UNINA_FUSE_CAMERA;
    store_record(links + tid, l);
  }
  // LiDAR cone tid -> its record's slot, or one behind the camera's
  if (own_slot >= 0) {
    RecordWords<unina_cone3d> o;
    o.r.x = lp.xc;
    o.r.y = lp.yc;
    o.r.z = lp.zc;
    o.r.u = lp.u;
    o.r.v = lp.v;
    o.r.n_valid = lw.r.n_valid;
    o.r.n_samples = lw.r.n_samples;
    o.r.valid = 1;
    store_record(out_cones + own_slot, o);
    if (mi < 0) {
      const uint4 src = reinterpret_cast<const uint4*>(ldets + tid)[1];   // confidence, class_id, valid, _pad
      RecordWords<GpuDetection> d;
      zero_record(d);
      if (projected) {
        d.r.x1 = d.r.x2 = fuse_record_coord(lp.u, a.sx);
        d.r.y1 = d.r.y2 = fuse_record_coord(lp.v, a.sy);
      }
      d.q[1] = make_uint4(src.x, src.y, 1u, 0u);
      store_record(out_dets + own_slot, d);
      RecordWords<unina_fuse_link> l;
      l.r.camera = -1;
      l.r.lidar = tid;
      l.r.d2 = 0.0f;
      l.r.kind = UNINA_FUSE_LIDAR;
      store_record(links + own_slot, l);
    }
  }
  if (tid >= n_written) {
    store_zero_record(out_dets + tid);
    store_zero_record(out_cones + tid);
    store_zero_record(links + tid);
  }
  __syncthreads();

  if (lidar_slot) {
    if ((reinterpret_cast<uintptr_t>(lidar_slot) & 15) == 0) {
      if (tid < kFuseBlock / 4) reinterpret_cast<uint4*>(lidar_slot)[tid] = reinterpret_cast<const uint4*>(s_slot)[tid];
    } else {
      lidar_slot[tid] = s_slot[tid];
    }
  }
  if (tid == 0) {
    RecordWords<unina_fuse_header> o;
    o.r.n_camera = nc;
    o.r.n_lidar = nl;
    o.r.n_projected = n_list;
    o.r.n_matched = n_matched;
    o.r.n_camera_only = nc - n_matched;
    o.r.n_lidar_only = n_only;
    o.r.n_written = n_written;
    o.r.n_dropped = n_only - (n_written - nc);
    store_record(header, o);
    *out_count = n_written;
  }
}

struct Span {
  uintptr_t lo, hi;
};

Span span_of(const void* p, size_t bytes) { return Span{(uintptr_t)p, (uintptr_t)p + bytes}; }
bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }

bool fuse_params_ok(const unina_fuse_params* p) {
  if (!extrinsic_ok(p->level_to_cam)) return false;
  if (!finite(p->cam.fx) || !finite(p->cam.fy) || !finite(p->cam.cx) || !finite(p->cam.cy) || p->cam.fx == 0.0f || p->cam.fy == 0.0f) return false;
  if (!finite_pos(p->sx) || !finite_pos(p->sy) || !finite(p->lift)) return false;
  if (!finite_pos(p->min_depth) || !finite(p->max_depth) || !(p->max_depth >= p->min_depth)) return false;
  const float nonneg[4] = {p->grow, p->pad, p->range_abs, p->range_rel};
  for (float v : nonneg)
    if (!finite(v) || !(v >= 0.0f)) return false;
  return true;
}

}  // namespace
}  // namespace unina

extern "C" int unina_fuse_async(const GpuDetection* d_dets, const int* d_count, const unina_cone3d* d_cones, const GpuDetection* d_ldets,
                                const int* d_lcount, const unina_cone3d* d_lcones, const unina_fuse_params* p, GpuDetection* d_out_dets,
                                int* d_out_count, unina_cone3d* d_out_cones, unina_fuse_link* d_links, int* d_lidar_slot,
                                unina_fuse_header* d_header, hipStream_t stream) {
  using namespace unina;
  if (!p || !record_io_ok(d_dets, d_count, d_cones) || !record_io_ok(d_ldets, d_lcount, d_lcones) ||
      !record_io_ok(d_out_dets, d_out_count, d_out_cones))
    return UNINA_ERR_ARG;
  if (!d_links || !d_header || ((uintptr_t)d_links & 15) || ((uintptr_t)d_header & 15) || ((uintptr_t)d_lidar_slot & 3)) return UNINA_ERR_ARG;
  if (!fuse_params_ok(p)) return UNINA_ERR_ARG;
  const size_t recs = sizeof(GpuDetection) * MAX_DETECTIONS, pts = sizeof(unina_cone3d) * MAX_DETECTIONS;
  const Span in[6] = {span_of(d_dets, recs),  span_of(d_count, sizeof(int)),  span_of(d_cones, pts),
                      span_of(d_ldets, recs), span_of(d_lcount, sizeof(int)), span_of(d_lcones, pts)};
  const Span out[6] = {span_of(d_out_dets, recs), span_of(d_out_count, sizeof(int)), span_of(d_out_cones, pts),
                       span_of(d_links, sizeof(unina_fuse_link) * MAX_DETECTIONS), span_of(d_header, sizeof(unina_fuse_header)),
                       span_of(d_lidar_slot, d_lidar_slot ? sizeof(int) * MAX_DETECTIONS : 0)};
  for (int o = 0; o < 6; ++o) {
    for (int i = 0; i < 6; ++i)
      if (overlap(out[o], in[i])) return UNINA_ERR_ARG;
    for (int q = o + 1; q < 6; ++q)
      if (overlap(out[o], out[q])) return UNINA_ERR_ARG;
  }
  hipLaunchKernelGGL(fuse_kernel, dim3(1), dim3(kFuseBlock), 0, stream, d_dets, d_count, d_cones, d_ldets, d_lcount, d_lcones, *p, d_out_dets,
                     d_out_count, d_out_cones, d_links, d_lidar_slot, d_header);
  return launch_status();
}
