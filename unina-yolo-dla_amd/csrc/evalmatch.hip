// Detections against labels on the device: the small-object counters of metrics.SmallObjectMetric.update, the conformal
// scores of metrics.conformal_quantile and the per-detection true-positive masks of metrics.ap_rows_numpy, one launch per
// image behind the frame that produced the records (include/unina_mi355.h "evaluation").
//
// One workgroup of 11 waves per image. The workgroup first derives the stable descending-confidence order of the records
// (rank = number of records that sort in front) and stages them in LDS in that order. Then every wave runs the SAME greedy
// matcher on its own rule, the detections one after another, its 64 lanes spread over the labels (lane l owns labels l,
// l + 64, l + 128, l + 192), a wave reduction picking the best unmatched same-class label (lowest index on equal IoU: the host
// loops take `>` in index order):
//   wave 0      SmallObjectMetric: normalised centre-format boxes, small labels only, TP at best IoU >= iou_threshold
//   wave 1 + j  conformal_quantile's matcher at t_j = (10 + j) / 20.0 (xyxy boxes in imgsz pixels); wave 1 appends the
//               scores 1 - best_iou, every wave sets bit j of the detection's mask
// The arithmetic is the host's, operation for operation, so that every comparison decides as the host's does and the scores
// are the host's bits (the unit is compiled with -ffp-contract=off): evaluate() scales the fp32 record fields in fp32,
// detections_to_coco forms x2 - x1 in fp32, everything after that is double -- EXCEPT inside metrics._box_iou_xyxy, where numpy
// keeps fp32 wherever both operands come from the fp32 record (its area, and an intersection side whose two edges are both the
// record's); box_iou_xyxy below carries that distinction.
#include <hip/hip_runtime.h>

#include <new>

#include "record_io.h"
#include "wave_block.h"

namespace unina {
namespace {

constexpr int kEvalWaves = 11;                     // wave 0: small-object metric; waves 1..10: IoU thresholds 0.50 .. 0.95
constexpr int kEvalBlock = kEvalWaves * kWave;
constexpr int kSlots = UNINA_EVAL_MAX_LABELS / kWave;   // labels per lane
constexpr int kDetWords = MAX_DETECTIONS / kWave;       // detections per lane in the per-wave match bits (16)
constexpr int kGuard = 8;                          // canary elements behind each list (unina_eval_read checks them)
constexpr unsigned long long kCanary64 = 0x5ca1ab1ec0ffee11ull;
constexpr unsigned kCanary32 = 0x5ca1ab1eu;

static_assert(UNINA_EVAL_MAX_LABELS % kWave == 0 && MAX_DETECTIONS % kWave == 0 && kDetWords <= 32, "lane layout");

// device-side state of a handle: the counters of every update since the last reset
struct EvalCounters {
  unsigned long long tp, fp, fn;          // SmallObjectMetric
  unsigned long long n_scores, n_rows;    // TRUE totals, also past the capacity of the lists
  unsigned long long overflow;            // bit 0: scores ran past max_scores, bit 1: rows ran past max_rows
  unsigned long long label_counts[UNINA_EVAL_MAX_CLASSES];
};

// the order of np.argsort(-confidence, kind="stable"): greater confidence first, NaN last, equal keys by index. A total order
// for any bit pattern, so the ranks are always a permutation of 0..n-1.
__device__ __forceinline__ bool sorts_before(float cj, int j, float ci, int i) {
  const bool nj = cj != cj, ni = ci != ci;
  if (nj || ni) return nj == ni ? j < i : ni;
  return cj > ci || (cj == ci && j < i);
}

// (iou, index) arg-max over the wave, the LOWEST index winning equal IoU; idx < 0 = no candidate. IoU is never negative or
// NaN here, so its bit pattern orders as the value does.
__device__ __forceinline__ void wave_best(double& iou, int& idx) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double oi = __shfl_xor(iou, o, kWave);
    const int ox = __shfl_xor(idx, o, kWave);
    if (ox >= 0 && (idx < 0 || oi > iou || (oi == iou && ox < idx))) {
      iou = oi;
      idx = ox;
    }
  }
}

// metrics.SmallObjectMetric._iou on corner boxes already formed as the host forms them (all double)
__device__ __forceinline__ double iou_centre(double ax1, double ay1, double ax2, double ay2, double bx1, double by1, double bx2,
                                             double by2) {
  const double iw = (bx2 < ax2 ? bx2 : ax2) - (bx1 > ax1 ? bx1 : ax1);   // min(ax2, bx2) - max(ax1, bx1)
  const double ih = (by2 < ay2 ? by2 : ay2) - (by1 > ay1 ? by1 : ay1);
  const double inter = (iw > 0.0 ? iw : 0.0) * (ih > 0.0 ? ih : 0.0);
  const double uni = (ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1) - inter;
  return uni <= 0 ? 0.0 : inter / uni;
}

// metrics._box_iou_xyxy(a, b) with a = four np.float32 (the record) and b = four np.float64 (the label). Python's max / min
// return the FIRST argument unless the second is strictly greater / smaller, and numpy computes float32 op float32 in fp32:
// a side of the intersection whose two edges both come from `a` is an fp32 difference, the product of two such sides an fp32
// product, and the record's own area (area_a) is fp32 throughout. Everything else is double.
__device__ __forceinline__ double box_iou_xyxy(float a0, float a1, float a2, float a3, float area_a, double b0, double b1, double b2,
                                               double b3, double area_b) {
  const bool fx1 = !(b0 > (double)a0), fy1 = !(b1 > (double)a1), fx2 = !(b2 < (double)a2), fy2 = !(b3 < (double)a3);   // edge taken from a
  const double x1 = fx1 ? (double)a0 : b0, y1 = fy1 ? (double)a1 : b1, x2 = fx2 ? (double)a2 : b2, y2 = fy2 ? (double)a3 : b3;
  if (x2 <= x1 || y2 <= y1) return 0.0;
  const bool fw = fx1 && fx2, fh = fy1 && fy2;
  const float wf = a2 - a0, hf = a3 - a1;
  const double w = fw ? (double)wf : x2 - x1, h = fh ? (double)hf : y2 - y1;
  const double inter = fw && fh ? (double)(wf * hf) : w * h;
  const double uni = (double)area_a + area_b - inter;
  return uni > 0 ? inter / uni : 0.0;
}

__global__ void __launch_bounds__(kEvalBlock) evalmatch_kernel(const float* __restrict__ dets, const int* __restrict__ d_count,
                                                               const double* __restrict__ labels, int n_labels, unina_eval_params p,
                                                               unsigned what, int num_classes, EvalCounters* __restrict__ ctr,
                                                               double* __restrict__ scores, unsigned long long max_scores,
                                                               unina_eval_row* __restrict__ rows, unsigned long long max_rows) {
  __shared__ float s_raw[MAX_DETECTIONS];                  // confidences in record order (ranking)
  __shared__ float s_x1[MAX_DETECTIONS], s_y1[MAX_DETECTIONS], s_x2[MAX_DETECTIONS], s_y2[MAX_DETECTIONS], s_conf[MAX_DETECTIONS];
  __shared__ int s_cls[MAX_DETECTIONS];                    // the records in matching order
  __shared__ unsigned s_bits[kEvalWaves - 1][kWave];       // wave 1 + j: bit (k / 64) of lane (k % 64) = detection k matched at t_j

  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int n = record_count(d_count);
  const unsigned long long row_base = ctr->n_rows, score_base = ctr->n_scores;   // read by everyone before anyone updates them

  for (int i = tid; i < n; i += kEvalBlock) s_raw[i] = dets[8 * i + 4];
  __syncthreads();
  for (int i = tid; i < n; i += kEvalBlock) {
    const float ci = s_raw[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += sorts_before(s_raw[j], j, ci, i) ? 1 : 0;
    const float* d = dets + 8 * i;
    s_x1[rank] = d[0];
    s_y1[rank] = d[1];
    s_x2[rank] = d[2];
    s_y2[rank] = d[3];
    s_conf[rank] = ci;
    s_cls[rank] = reinterpret_cast<const int*>(d)[5];
  }
  __syncthreads();

  if (wave == 0) {
    if (what & UNINA_EVAL_SMALL) {
      // labels of this lane as corner boxes (SmallObjectMetric._iou's b2); non-small ones are masked out, which leaves the
      // index order of the host's filtered list
      double bx1[kSlots], by1[kSlots], bx2[kSlots], by2[kSlots];
      int bcls[kSlots];
      unsigned open = 0;   // bit s: slot s holds a small label that is not matched yet
      const double image_size = (double)p.imgsz, limit = p.size_threshold;
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        const int g = lane + s * kWave;
        bx1[s] = by1[s] = bx2[s] = by2[s] = 0.0;
        bcls[s] = 0;
        if (g < n_labels) {
          const double* l = labels + 5 * (size_t)g;
          const double xc = l[1], yc = l[2], w = l[3], h = l[4];
          if (w * image_size < limit && h * image_size < limit) open |= 1u << s;
          bcls[s] = (int)l[0];
          bx1[s] = xc - w / 2;
          by1[s] = yc - h / 2;
          bx2[s] = xc + w / 2;
          by2[s] = yc + h / 2;
        }
      }
      int n_small = __popc(open);
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) n_small += __shfl_xor(n_small, o, kWave);
      unsigned long long tp = 0, fp = 0;
      if (n_small > 0) {   // (an image without a small label counts nothing, update's first `continue`)
        const double width = (double)p.width, height = (double)p.height;
        for (int k = 0; k < n; ++k) {
          // evaluate(): fp32 scale; detections_to_coco: fp32 x2 - x1; coco_to_metric_rows: double from here on
          const float x1 = s_x1[k] * p.sx, x2 = s_x2[k] * p.sx, y1 = s_y1[k] * p.sy, y2 = s_y2[k] * p.sy;
          const double bw = (double)(x2 - x1), bh = (double)(y2 - y1);
          const double xc = ((double)x1 + bw / 2) / width, yc = ((double)y1 + bh / 2) / height, wn = bw / width, hn = bh / height;
          const double ax1 = xc - wn / 2, ay1 = yc - hn / 2, ax2 = xc + wn / 2, ay2 = yc + hn / 2;
          const int cls = s_cls[k];
          double best = 0.0;
          int idx = -1;
#pragma unroll
          for (int s = 0; s < kSlots; ++s) {
            if (!((open >> s) & 1u) || bcls[s] != cls) continue;
            const double iou = iou_centre(ax1, ay1, ax2, ay2, bx1[s], by1[s], bx2[s], by2[s]);
            if (iou > best) {
              best = iou;
              idx = lane + s * kWave;
            }
          }
          if (__ballot(idx >= 0)) wave_best(best, idx);
          if (idx >= 0 && best >= p.iou_threshold) {
            ++tp;
            if ((idx & (kWave - 1)) == lane) open &= ~(1u << (idx / kWave));
          } else if (wn * image_size < limit && hn * image_size < limit) {
            ++fp;   // a false positive only if the prediction is itself small
          }
        }
      }
      if (lane == 0) {   // one workgroup per launch, launches stream-ordered: plain read-modify-write
        ctr->tp += tp;
        ctr->fp += fp;
        ctr->fn += (unsigned long long)n_small - tp;
      }
    }
  } else if (what & (UNINA_EVAL_CONFORMAL | UNINA_EVAL_AP)) {
    const int j = wave - 1;
    const double thr = (10 + j) / 20.0;
    const bool append = j == 0 && (what & UNINA_EVAL_CONFORMAL);
    // labels of this lane in imgsz pixels (conformal_quantile's gts: ONE size for both axes)
    double g0[kSlots], g1[kSlots], g2[kSlots], g3[kSlots], garea[kSlots];
    int gcls[kSlots];
    unsigned open = 0;
    const double imgsz = (double)p.imgsz;
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      const int g = lane + s * kWave;
      g0[s] = g1[s] = g2[s] = g3[s] = garea[s] = 0.0;
      gcls[s] = 0;
      if (g < n_labels) {
        const double* l = labels + 5 * (size_t)g;
        open |= 1u << s;
        gcls[s] = (int)l[0];
        g0[s] = (l[1] - l[3] / 2) * imgsz;
        g1[s] = (l[2] - l[4] / 2) * imgsz;
        g2[s] = (l[1] + l[3] / 2) * imgsz;
        g3[s] = (l[2] + l[4] / 2) * imgsz;
        garea[s] = (g2[s] - g0[s]) * (g3[s] - g1[s]);
      }
    }
    unsigned bits = 0;
    unsigned long long matches = 0;
    for (int k = 0; k < n; ++k) {
      const float a0 = s_x1[k] * p.cx, a2 = s_x2[k] * p.cx, a1 = s_y1[k] * p.cy, a3 = s_y2[k] * p.cy;   // evaluate(): fp32 scale to imgsz pixels
      const float area_a = (a2 - a0) * (a3 - a1);
      const int cls = s_cls[k];
      double best = 0.0;
      int idx = -1;
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        if (!((open >> s) & 1u) || gcls[s] != cls) continue;
        const double iou = box_iou_xyxy(a0, a1, a2, a3, area_a, g0[s], g1[s], g2[s], g3[s], garea[s]);
        if (iou > best && iou >= thr) {
          best = iou;
          idx = lane + s * kWave;
        }
      }
      if (__ballot(idx >= 0) == 0) continue;
      wave_best(best, idx);
      if ((idx & (kWave - 1)) == lane) open &= ~(1u << (idx / kWave));
      if ((k & (kWave - 1)) == lane) bits |= 1u << (k / kWave);
      if (append && lane == 0 && score_base + matches < max_scores) scores[score_base + matches] = 1.0 - best;
      ++matches;
    }
    s_bits[j][lane] = bits;
    if (append && lane == 0) {
      ctr->n_scores = score_base + matches;
      if (score_base + matches > max_scores) atomicOr(&ctr->overflow, 1ull);
    }
  }
  __syncthreads();

  if (what & UNINA_EVAL_AP) {
    for (int k = tid; k < n; k += kEvalBlock) {
      if (row_base + k >= max_rows) continue;
      unsigned mask = 0;
#pragma unroll
      for (int j = 0; j < kEvalWaves - 1; ++j) mask |= ((s_bits[j][k & (kWave - 1)] >> (k / kWave)) & 1u) << j;
      unina_eval_row r;
      r.confidence = s_conf[k];
      r.class_id = s_cls[k];
      r.tp_mask = mask;
      rows[row_base + k] = r;
    }
    for (int g = tid; g < n_labels; g += kEvalBlock) {
      const int cls = (int)labels[5 * (size_t)g];
      if (cls >= 0 && cls < num_classes) atomicAdd(&ctr->label_counts[cls], 1ull);
    }
    if (tid == 0) {
      ctr->n_rows = row_base + (unsigned long long)n;
      if (row_base + (unsigned long long)n > max_rows) atomicOr(&ctr->overflow, 2ull);
    }
  }
}

__global__ void eval_canary_kernel(double* scores_guard, unina_eval_row* rows_guard) {
  const int t = (int)threadIdx.x;
  if (t < kGuard) {
    reinterpret_cast<unsigned long long*>(scores_guard)[t] = kCanary64;
    unsigned* w = reinterpret_cast<unsigned*>(rows_guard + t);
    w[0] = w[1] = w[2] = kCanary32;
  }
}

}  // namespace
}  // namespace unina

struct unina_eval {
  int device = 0, num_classes = 0;
  size_t max_scores = 0, max_rows = 0;
  unina::EvalCounters* d_ctr = nullptr;   // device memory is allocated by the first call that needs it
  double* d_scores = nullptr;             // max_scores + kGuard
  unina_eval_row* d_rows = nullptr;       // max_rows + kGuard
};

namespace unina {
namespace {

void eval_free(unina_eval* ev) {
  if (ev->d_ctr) (void)hipFree(ev->d_ctr);
  if (ev->d_scores) (void)hipFree(ev->d_scores);
  if (ev->d_rows) (void)hipFree(ev->d_rows);
  ev->d_ctr = nullptr;
  ev->d_scores = nullptr;
  ev->d_rows = nullptr;
}

// first use: the counters (zeroed), the two lists and the canaries behind them, all ordered on `stream` in front of the caller's work
int eval_ensure(unina_eval* ev, hipStream_t stream) {
  if (hipSetDevice(ev->device) != hipSuccess) return UNINA_ERR_HIP;
  if (ev->d_ctr) return UNINA_OK;
  if (hipMalloc(&ev->d_ctr, sizeof(EvalCounters)) != hipSuccess ||
      hipMalloc(&ev->d_scores, sizeof(double) * (ev->max_scores + kGuard)) != hipSuccess ||
      hipMalloc(&ev->d_rows, sizeof(unina_eval_row) * (ev->max_rows + kGuard)) != hipSuccess) {
    eval_free(ev);
    return UNINA_ERR_HIP;
  }
  if (hipMemsetAsync(ev->d_ctr, 0, sizeof(EvalCounters), stream) != hipSuccess) {
    eval_free(ev);
    return UNINA_ERR_HIP;
  }
  hipLaunchKernelGGL(eval_canary_kernel, dim3(1), dim3(kWave), 0, stream, ev->d_scores + ev->max_scores, ev->d_rows + ev->max_rows);
  if (hipGetLastError() != hipSuccess) {
    (void)hipStreamSynchronize(stream);
    eval_free(ev);
    return UNINA_ERR_HIP;
  }
  return UNINA_OK;
}

}  // namespace
}  // namespace unina

extern "C" int unina_eval_create(int device_id, int num_classes, size_t max_scores, size_t max_rows, unina_eval_t** out) {
  if (!out) return UNINA_ERR_ARG;
  *out = nullptr;
  if (device_id < 0 || num_classes < 1 || num_classes > UNINA_EVAL_MAX_CLASSES) return UNINA_ERR_ARG;
  if (max_scores > ((size_t)1 << 40) || max_rows > ((size_t)1 << 40)) return UNINA_ERR_ARG;
  unina_eval* ev = new (std::nothrow) unina_eval;
  if (!ev) return UNINA_ERR_HIP;
  ev->device = device_id;
  ev->num_classes = num_classes;
  ev->max_scores = max_scores;
  ev->max_rows = max_rows;
  *out = ev;
  return UNINA_OK;
}

extern "C" void unina_eval_destroy(unina_eval_t* ev) {
  if (!ev) return;
  if (ev->d_ctr && hipSetDevice(ev->device) == hipSuccess) (void)hipDeviceSynchronize();
  unina::eval_free(ev);
  delete ev;
}

extern "C" int unina_eval_reset_async(unina_eval_t* ev, hipStream_t stream) {
  using namespace unina;
  if (!ev) return UNINA_ERR_ARG;
  const bool fresh = !ev->d_ctr;
  if (const int rc = eval_ensure(ev, stream)) return rc;
  if (!fresh && hipMemsetAsync(ev->d_ctr, 0, sizeof(EvalCounters), stream) != hipSuccess) return UNINA_ERR_HIP;
  return UNINA_OK;
}

extern "C" int unina_eval_update_async(unina_eval_t* ev, const GpuDetection* d_dets, const int* d_count, const double* d_labels,
                                       int n_labels, const unina_eval_params* p, unsigned what, hipStream_t stream) {
  using namespace unina;
  if (!ev || !d_dets || !d_count || !p) return UNINA_ERR_ARG;
  if (n_labels < 0 || n_labels > UNINA_EVAL_MAX_LABELS || (n_labels > 0 && !d_labels)) return UNINA_ERR_ARG;
  if (what == 0 || (what & ~(unsigned)(UNINA_EVAL_SMALL | UNINA_EVAL_CONFORMAL | UNINA_EVAL_AP))) return UNINA_ERR_ARG;
  if (p->width < 1 || p->height < 1 || p->imgsz < 1 || !(p->iou_threshold > 0.0)) return UNINA_ERR_ARG;
  if (((uintptr_t)d_dets & 3) || ((uintptr_t)d_count & 3) || ((uintptr_t)d_labels & 7)) return UNINA_ERR_ARG;
  if (const int rc = eval_ensure(ev, stream)) return rc;
  hipLaunchKernelGGL(evalmatch_kernel, dim3(1), dim3(kEvalBlock), 0, stream, reinterpret_cast<const float*>(d_dets), d_count, d_labels,
                     n_labels, *p, what, ev->num_classes, ev->d_ctr, ev->d_scores, (unsigned long long)ev->max_scores, ev->d_rows,
                     (unsigned long long)ev->max_rows);
  return launch_status();
}

extern "C" int unina_eval_read(unina_eval_t* ev, unina_eval_result* res, double* scores, size_t score_cap, unina_eval_row* rows,
                               size_t row_cap, hipStream_t stream) {
  using namespace unina;
  if (!ev || !res || (score_cap > 0 && !scores) || (row_cap > 0 && !rows)) return UNINA_ERR_ARG;
  if (const int rc = eval_ensure(ev, stream)) return rc;
  EvalCounters c;
  unsigned long long sg[kGuard];
  unina_eval_row rg[kGuard];
  if (hipMemcpyAsync(&c, ev->d_ctr, sizeof(c), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipMemcpyAsync(sg, ev->d_scores + ev->max_scores, sizeof(sg), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipMemcpyAsync(rg, ev->d_rows + ev->max_rows, sizeof(rg), hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return UNINA_ERR_HIP;
  size_t ns = c.n_scores < ev->max_scores ? (size_t)c.n_scores : ev->max_scores;
  size_t nr = c.n_rows < ev->max_rows ? (size_t)c.n_rows : ev->max_rows;
  ns = ns < score_cap ? ns : score_cap;
  nr = nr < row_cap ? nr : row_cap;
  if ((ns && hipMemcpyAsync(scores, ev->d_scores, sizeof(double) * ns, hipMemcpyDeviceToHost, stream) != hipSuccess) ||
      (nr && hipMemcpyAsync(rows, ev->d_rows, sizeof(unina_eval_row) * nr, hipMemcpyDeviceToHost, stream) != hipSuccess) ||
      hipStreamSynchronize(stream) != hipSuccess)
    return UNINA_ERR_HIP;
  res->tp = (long long)c.tp;
  res->fp = (long long)c.fp;
  res->fn = (long long)c.fn;
  res->n_scores = c.n_scores;
  res->n_rows = c.n_rows;
  res->overflow = (int)c.overflow;
  res->guard_intact = 1;
  for (int i = 0; i < kGuard; ++i) {
    const unsigned* w = reinterpret_cast<const unsigned*>(&rg[i]);
    if (sg[i] != kCanary64 || w[0] != kCanary32 || w[1] != kCanary32 || w[2] != kCanary32) res->guard_intact = 0;
  }
  for (int k = 0; k < UNINA_EVAL_MAX_CLASSES; ++k) res->label_counts[k] = k < ev->num_classes ? (long long)c.label_counts[k] : 0;
  return UNINA_OK;
}
