// Located cones tracked across frames on the device: one launch per frame behind unina_locate_async (include/unina_mi355.h
// "tracking"; tracking.update_numpy is the definition, bit for bit). The table -- a 32-byte header and UNINA_TRACK_MAX 32-byte
// slots -- lives in device memory between the launches; nothing is read back by the host.
//
// The association is the greedy matching over all gated pairs in ascending (d2 bits, slot, record). It is computed as rounds of
// MUTUAL NEAREST NEIGHBOURS, which give the same matching: in a round every free usable record takes the minimum of (d2, slot)
// over its free candidate slots, every free live slot the minimum of (d2, record) over its free candidate records, and every
// pair that chose each other is matched. The least free pair in (d2, slot, record) order is always mutual, so a round with a
// free candidate pair matches at least one; and a mutual pair is preceded in that order by no free pair that shares its slot
// or its record, so the greedy loop takes it too. All counters are integers, every minimum is over unsigned keys and every fp32
// operation has one fixed place in one fixed order (csrc/track_math.h; the unit is compiled with -ffp-contract=off): two runs
// give the same bytes, and they are numpy's.
//
// Work split. ONE workgroup of 1024 threads (16 waves); thread t owns record t AND slot t, both held in registers.
//   setup    the live slots are compacted in ascending slot order into LDS as (x, y, z, class) -- 16 KB, read as broadcasts --
//            and the records' points as (px, py, pz, confidence), 16 KB, for the slot threads' updates.
//   round    record side: an active record walks its part of the live list; per gated free pair it keeps its own minimum in a register
//            and sends (d2 bits << 32 | record) to the slot's 64-bit LDS minimum (ds_min_u64; a minimum does not depend on the
//            order of arrival). Barrier. A record whose slot's minimum names it is matched: it leaves its index with the slot
//            and overwrites the slot's x in LDS with NaN, which fails every later gate. A record that found no candidate can
//            never find one again (slots only get taken) and retires. The minima are double-buffered, so a round costs two
//            barriers. Waves without an active record skip the walk.
//   tail     slot side: update, age or free the own slot; two prefix scans (ballot + 16 wave totals) rank the birth candidates
//            and the free slots, the k-th birth goes to the k-th free slot; table and assign leave as 16-byte vector stores.
// No gate-bit rows are kept (128 KB for all records). A record keeps the index range of the live list between the first and
// the last free candidate of its last walk instead: candidates only become fewer, so the next walk stays inside it. A track's
// neighbours in space are mostly neighbours in the list, so the first walk covers the list and the later ones a few entries;
// waves without an active record skip the walk, and a record is active only while it has a free candidate. Expected: tracks are
// metres apart and the gate is a fraction of that, so nearly every record has one candidate and one or two rounds finish the
// frame (the seeded 150-cone sequence of the tests: at most 4). The worst case is a chain of shrinking gaps, which matches one
// pair per round: r rounds cost one walk of the live list plus r x (a walk of the record's few candidates + 2 barriers and the
// workgroup-wide vote). tools/bench_track.py times a typical frame, a full table with every record gated to several slots,
// and the 64-round chain.
#include <hip/hip_runtime.h>

#include <new>

#include "record_io.h"
#include "track_math.h"
#include "wave_block.h"

struct unina_tracker {
  int device = 0;
  unsigned char* d_mem = nullptr;   // header, then the slots; allocated by the first call that needs it
};

namespace unina {
namespace {

constexpr int kTrkBlock = 1024;
constexpr int kTrkWaves = kTrkBlock / kWave;

static_assert(UNINA_TRACK_MAX == kTrkBlock && MAX_DETECTIONS == kTrkBlock, "a thread owns one record and one slot");
static_assert(sizeof(unina_track) == 32 && sizeof(unina_track_header) == 32 && sizeof(unina_cone3d) == 32 && sizeof(GpuDetection) == 32,
              "record layouts");
static_assert(sizeof(unina_track_params) == 72, "parameter layout");

struct TrackArgs {
  float pose[12];
  float gate2, alpha, birth_confidence;
  int class_aware, confirm_hits, max_missed;
};

__device__ __forceinline__ void block_add(bool flag, int* counter) {
  const unsigned long long m = __ballot(flag);
  if (((int)threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd(counter, __popcll(m));
}

__global__ void __launch_bounds__(kTrkBlock) track_reset_kernel(unina_track_header* __restrict__ hdr, unina_track* __restrict__ tracks) {
  store_zero_record(tracks + threadIdx.x);
  if (threadIdx.x == 0) {
    RecordWords<unina_track_header> w;
    zero_record(w);
    w.r.next_id = 1;
    store_record(hdr, w);
  }
}

__global__ void __launch_bounds__(kTrkBlock) track_update_kernel(const GpuDetection* __restrict__ dets, const int* __restrict__ d_count,
                                                                 const unina_cone3d* __restrict__ cones, TrackArgs a,
                                                                 unina_track_header* hdr, unina_track* tracks, int* __restrict__ assign) {
  __shared__ float4 s_slot[kTrkBlock];                                  // live list entry k: x, y, z, class bits; x = NaN once taken
  __shared__ float4 s_rec[kTrkBlock];                                   // record j: px, py, pz, confidence
  __shared__ __align__(16) unsigned long long s_best[2][kTrkBlock];     // live list entry k: min (d2 bits << 32 | record) of the round
  __shared__ int s_rcls[kTrkBlock];                                     // record j: class_id
  __shared__ int s_match[kTrkBlock];                                    // live list entry k: the record it matched, or -1
  __shared__ int s_wave[kTrkWaves];                                     // block_rank's, and only its
  __shared__ int s_cnt[4];                                              // matched, died, live, confirmed
  int* const s_birth = reinterpret_cast<int*>(&s_best[0][0]);           // after the rounds: k-th birth candidate's record
  int* const s_assign = reinterpret_cast<int*>(&s_best[1][0]);          // after the rounds: the assign words

  const int tid = (int)threadIdx.x;
  const int n = record_count(d_count);
  const RecordWords<unina_track_header> hw = load_record(hdr);

  // ---- setup: the own slot, the own record
  RecordWords<unina_track> tw = load_record(tracks + tid);
  bool live = tw.r.id != 0;

  float px = 0.0f, py = 0.0f, pz = 0.0f, conf = 0.0f;
  int rcls = 0;
  bool usable = false;
  if (tid < n) {
    const float4 c = reinterpret_cast<const float4*>(cones + tid)[0];   // x, y, z, u
    const uint4 cv = reinterpret_cast<const uint4*>(cones + tid)[1];    // v, n_valid, n_samples, valid
    const uint4 d = reinterpret_cast<const uint4*>(dets + tid)[1];      // confidence, class_id, valid, _pad
    const TrackPoint p = track_point(a.pose, c.x, c.y, c.z, (int)cv.w);
    px = p.x;
    py = p.y;
    pz = p.z;
    usable = p.usable != 0;
    conf = __uint_as_float(d.x);
    rcls = (int)d.y;
  }
  s_rec[tid] = make_float4(px, py, pz, conf);
  s_rcls[tid] = rcls;
  s_best[0][tid] = kTrackNoKey;
  s_best[1][tid] = kTrackNoKey;
  s_match[tid] = -1;
  if (tid < 4) s_cnt[tid] = 0;
  int n_list;
  const int k_own = block_rank<kTrkWaves>(live, s_wave, &n_list);   // the own slot's place in the live list
  if (live) s_slot[k_own] = make_float4(tw.r.x, tw.r.y, tw.r.z, __int_as_float(tw.r.class_id));

  // ---- rounds of mutual nearest neighbours
  bool active = usable && n_list > 0;
  bool matched_rec = false;
  int lo = 0, hi = n_list;   // the part of the live list this record still has to walk
  for (int round = 0; __syncthreads_or(active ? 1 : 0); ++round) {   // the barrier also orders the last round's LDS writes
    unsigned long long* const best = s_best[round & 1];
    unsigned long long mine = kTrackNoKey;
    if (active) {
      int first = hi, end = lo;
      for (int k = lo; k < hi; ++k) {
        const float4 t = s_slot[k];
        const float d2 = track_d2(px, py, pz, t.x, t.y, t.z);
        if (track_gated(d2, a.gate2) && (a.class_aware == 0 || __float_as_int(t.w) == rcls)) {
          const unsigned long long key = track_key(d2, (uint32_t)k);
          mine = key < mine ? key : mine;
          atomicMin(&best[k], track_key(d2, (uint32_t)tid));
          first = first < k ? first : k;
          end = k + 1;
        }
      }
      lo = first;   // the free candidates only become fewer: the next walk stays between the first and the last one found now
      hi = end;
    }
    __syncthreads();
    if (active) {
      if (mine == kTrackNoKey) {
        active = false;   // no free candidate now: none later
      } else {
        const int k = (int)(uint32_t)mine;
        if (best[k] == ((mine & 0xffffffff00000000ull) | (unsigned long long)tid)) {
          s_match[k] = tid;
          s_slot[k].x = __uint_as_float(0x7fc00000u);
          matched_rec = true;
          active = false;
        }
      }
    }
    s_best[(round + 1) & 1][tid] = kTrackNoKey;   // last read in the round before this one
  }

  // ---- slot side: update, age or free the own slot
  s_assign[tid] = 0;
  __syncthreads();
  const int mj = live ? s_match[k_own] : -1;
  bool died = false;
  if (live) {
    if (mj >= 0) {
      const float4 r = s_rec[mj];
      tw.r.x = track_step(tw.r.x, a.alpha, r.x);
      tw.r.y = track_step(tw.r.y, a.alpha, r.y);
      tw.r.z = track_step(tw.r.z, a.alpha, r.z);
      tw.r.confidence = r.w;
      tw.r.class_id = s_rcls[mj];
      tw.r.hits = track_hit(tw.r.hits);
      tw.r.missed = 0;
      s_assign[mj] = tw.r.id;
    } else {
      tw.r.missed = track_miss(tw.r.missed);
      if (tw.r.missed > a.max_missed) {
        zero_record(tw);
        died = true;
        live = false;
      }
    }
  }
  block_add(mj >= 0, &s_cnt[0]);
  block_add(died, &s_cnt[1]);

  // ---- births: the k-th candidate record founds a track in the k-th free slot
  const bool wants = usable && !matched_rec && conf >= a.birth_confidence;   // a NaN confidence fails
  int n_wants, n_free;
  const int kb = block_rank<kTrkWaves>(wants, s_wave, &n_wants);
  const int kf = block_rank<kTrkWaves>(!live, s_wave, &n_free);
  const int n_born = track_births_taken(n_wants, n_free, hw.r.next_id);
  if (wants && kb < n_born) {
    s_birth[kb] = tid;
    s_assign[tid] = hw.r.next_id + kb;
  }
  __syncthreads();
  if (!live && kf < n_born) {
    const int j = s_birth[kf];
    const float4 r = s_rec[j];
    tw.r.x = r.x;
    tw.r.y = r.y;
    tw.r.z = r.z;
    tw.r.confidence = r.w;
    tw.r.id = hw.r.next_id + kf;
    tw.r.class_id = s_rcls[j];
    tw.r.hits = 1;
    tw.r.missed = 0;
    live = true;
  }
  store_record(tracks + tid, tw);
  block_add(live, &s_cnt[2]);
  block_add(live && tw.r.hits >= a.confirm_hits, &s_cnt[3]);
  __syncthreads();

  if (assign) {
    if ((reinterpret_cast<uintptr_t>(assign) & 15) == 0) {
      if (tid < kTrkBlock / 4) reinterpret_cast<uint4*>(assign)[tid] = reinterpret_cast<const uint4*>(s_assign)[tid];
    } else {
      assign[tid] = s_assign[tid];
    }
  }
  if (tid == 0) {
    RecordWords<unina_track_header> o;
    o.r.frame = (int)((unsigned)hw.r.frame + 1u);
    o.r.n_live = s_cnt[2];
    o.r.n_confirmed = s_cnt[3];
    o.r.next_id = hw.r.next_id + n_born;
    o.r.n_matched = s_cnt[0];
    o.r.n_born = n_born;
    o.r.n_died = s_cnt[1];
    o.r.n_dropped = n_wants - n_born;
    store_record(hdr, o);
  }
}

unina_track_header* header_of(unina_tracker* t) { return reinterpret_cast<unina_track_header*>(t->d_mem); }
unina_track* slots_of(unina_tracker* t) { return reinterpret_cast<unina_track*>(t->d_mem + sizeof(unina_track_header)); }

int launch_reset(unina_tracker* t, hipStream_t stream) {
  hipLaunchKernelGGL(track_reset_kernel, dim3(1), dim3(kTrkBlock), 0, stream, header_of(t), slots_of(t));
  return launch_status();
}

// allocates the table on first use and resets it on `stream`; *fresh tells the caller that this call did
int track_ensure(unina_tracker* t, hipStream_t stream, bool* fresh) {
  *fresh = false;
  if (hipSetDevice(t->device) != hipSuccess) return UNINA_ERR_HIP;
  if (t->d_mem) return UNINA_OK;
  void* mem = nullptr;
  if (hipMalloc(&mem, sizeof(unina_track_header) + sizeof(unina_track) * UNINA_TRACK_MAX) != hipSuccess) return UNINA_ERR_HIP;
  t->d_mem = static_cast<unsigned char*>(mem);
  if (launch_reset(t, stream) != UNINA_OK) {
    (void)hipFree(t->d_mem);
    t->d_mem = nullptr;
    return UNINA_ERR_HIP;
  }
  *fresh = true;
  return UNINA_OK;
}

}  // namespace
}  // namespace unina

extern "C" int unina_track_create(int device_id, unina_tracker_t** out) {
  if (!out) return UNINA_ERR_ARG;
  *out = nullptr;
  if (device_id < 0) return UNINA_ERR_ARG;
  unina_tracker* t = new (std::nothrow) unina_tracker();
  if (!t) return UNINA_ERR_IO;
  t->device = device_id;
  *out = t;
  return UNINA_OK;
}

extern "C" void unina_track_destroy(unina_tracker_t* t) {
  if (!t) return;
  if (t->d_mem) {
    if (hipSetDevice(t->device) == hipSuccess) (void)hipDeviceSynchronize();
    (void)hipFree(t->d_mem);
  }
  delete t;
}

extern "C" int unina_track_reset_async(unina_tracker_t* t, hipStream_t stream) {
  using namespace unina;
  if (!t) return UNINA_ERR_ARG;
  bool fresh;
  if (const int rc = track_ensure(t, stream, &fresh)) return rc;
  return fresh ? UNINA_OK : launch_reset(t, stream);
}

extern "C" int unina_track_update_async(unina_tracker_t* t, const GpuDetection* d_dets, const int* d_count, const unina_cone3d* d_cones,
                                        const unina_track_params* p, int* d_assign, hipStream_t stream) {
  using namespace unina;
  if (!t || !p || !record_io_ok(d_dets, d_count, d_cones) || ((uintptr_t)d_assign & 3)) return UNINA_ERR_ARG;
  for (int i = 0; i < 12; ++i)
    if (!unina::finite(p->pose[i])) return UNINA_ERR_ARG;
  if (!(p->gate > 0.0f && unina::finite(p->gate * p->gate))) return UNINA_ERR_ARG;   // a finite gate2 keeps every stored coordinate free of NaN
  if (!(p->alpha > 0.0f && p->alpha <= 1.0f)) return UNINA_ERR_ARG;
  if (p->birth_confidence != p->birth_confidence) return UNINA_ERR_ARG;
  if (p->confirm_hits < 1 || p->max_missed < 0) return UNINA_ERR_ARG;
  bool fresh;
  if (const int rc = track_ensure(t, stream, &fresh)) return rc;
  TrackArgs a;
  for (int i = 0; i < 12; ++i) a.pose[i] = p->pose[i];
  a.gate2 = p->gate * p->gate;
  a.alpha = p->alpha;
  a.birth_confidence = p->birth_confidence;
  a.class_aware = p->class_aware;
  a.confirm_hits = p->confirm_hits;
  a.max_missed = p->max_missed;
  hipLaunchKernelGGL(track_update_kernel, dim3(1), dim3(kTrkBlock), 0, stream, d_dets, d_count, d_cones, a, header_of(t), slots_of(t),
                     d_assign);
  return launch_status();
}

extern "C" int unina_track_buffers(unina_tracker_t* t, const unina_track** d_tracks, const unina_track_header** d_header) {
  using namespace unina;
  if (!t) return UNINA_ERR_ARG;
  if (!t->d_mem) return UNINA_ERR_STATE;
  if (d_tracks) *d_tracks = slots_of(t);
  if (d_header) *d_header = header_of(t);
  return UNINA_OK;
}

extern "C" int unina_track_read(unina_tracker_t* t, unina_track_header* hdr, unina_track* tracks, size_t cap, hipStream_t stream) {
  using namespace unina;
  if (!t || !hdr || (cap > 0 && !tracks)) return UNINA_ERR_ARG;
  bool fresh;
  if (const int rc = track_ensure(t, stream, &fresh)) return rc;
  const size_t n = cap < (size_t)UNINA_TRACK_MAX ? cap : (size_t)UNINA_TRACK_MAX;
  if (hipMemcpyAsync(hdr, header_of(t), sizeof(*hdr), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      (n && hipMemcpyAsync(tracks, slots_of(t), sizeof(unina_track) * n, hipMemcpyDeviceToHost, stream) != hipSuccess) ||
      hipStreamSynchronize(stream) != hipSuccess)
    return UNINA_ERR_HIP;
  return UNINA_OK;
}
