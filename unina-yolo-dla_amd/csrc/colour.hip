// Class from pixels for records without one: a memset of the header and one launch behind unina_fuse_async (or any locator), in
// front of unina_track_update_async (include/unina_mi355.h "class from pixels"; colour.colour_numpy is the definition, bit for
// bit). The call is stateless. The window's floats are fp32 in one fixed order (csrc/colour_math.h, csrc/locate_window.h; the unit
// is compiled with -ffp-contract=off); everything behind the window is an integer, so the order in which the counts arrive does not
// matter: two runs give the same bytes, and they are numpy's.
//
// Work split. ONE workgroup of 256 threads (4 waves) per record slot, MAX_DETECTIONS of them; a workgroup reads and writes its own
// record only, so d_out_dets may be d_dets. Everything that decides whether a workgroup leaves early is the same in all its
// threads, so no barrier is ever reached by a part of one.
//   slot >= n, not selected, no window: thread 0 stores the two records (zeros, or the copy) and the workgroup is done.
//   samples  sample s = c + k * cols goes to thread s mod 256 in pass s / 256. A sample inside the silhouette fetches its pixel --
//            one dword for a 4-channel pixel at a 4-byte address, else three byte loads, never a byte behind the pixel -- and
//            finds its bin. The 64 samples of a wave in a pass lie in the rows base / cols .. (base + 63) / cols, which the
//            wave walks: per row six __ballot counts (five bins and the mask), added to the row's six LDS words by lanes 0..5
//            in one ds_add. With cols = 64 a wave's pass is one row.
//   rows     after one barrier wave 0 holds row k in lane k: the totals are a butterfly of __shfl_xor, the row letters two
//            __ballot masks, the stripes the popcount of a third; lane 0 stores the two records and adds to the header.
// LDS: 64 rows of 6 words at a stride of 7 (lane k reads row k: an odd stride keeps the 32 lanes of a half on 32 banks).
#include <hip/hip_runtime.h>

#include "colour_math.h"
#include "record_io.h"
#include "wave_block.h"

namespace unina {
namespace {

constexpr int kColourBlock = 256;
constexpr int kColourRowStride = kColourBins + 1;

static_assert(UNINA_COLOUR_MAX_SIDE == kWave, "wave 0 holds a row per lane and the row letters are 64-bit masks");
static_assert(sizeof(unina_colour) == 32 && sizeof(unina_colour_header) == 32 && sizeof(GpuDetection) == 32 && sizeof(unina_cone3d) == 32,
              "record layouts");
static_assert(sizeof(unina_colour_params) == 112, "parameter layout");

struct ColourImage {
  const uint8_t* data;
  int width, height, pitch, channels;
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// dets and out_dets may be one array: neither is __restrict__
__global__ void __launch_bounds__(kColourBlock) colour_kernel(const GpuDetection* dets, const int* __restrict__ d_count,
                                                              const unina_cone3d* __restrict__ cones, ColourImage img, float fx, float fy,
                                                              unina_colour_params p, GpuDetection* out_dets, unina_colour* __restrict__ colour,
                                                              unina_colour_header* __restrict__ header) {
  __shared__ int s_rows[UNINA_COLOUR_MAX_SIDE * kColourRowStride];

  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = (int)blockIdx.x;
  const int n = record_count(d_count);
  if (i == 0 && tid == 0) header->n_records = n;   // behind the memset, and no other thread writes this word
  if (i >= n) {
    if (tid == 0) {
      store_zero_record(out_dets + i);
      store_zero_record(colour + i);
    }
    return;
  }

  RecordWords<GpuDetection> dw = load_record(dets + i);
  const bool selected = p.only_class < 0 || dw.r.class_id == p.only_class;
  ColourWindow cw;
  cw.w.empty = 1;
  cw.size = 0;
  if (selected) {
    RecordWords<unina_cone3d> cone;
    zero_record(cone);
    if (cones) cone = load_record(cones + i);
    cw = colour_window(dw.r.x1, dw.r.y1, dw.r.x2, dw.r.y2, cones ? 1 : 0, cone.r.valid, cone.r.u, cone.r.v, cone.r.z, fx, fy, p, img.width,
                       img.height);
  }
  if (cw.w.empty) {
    if (tid == 0) {
      store_record(out_dets + i, dw);
      RecordWords<unina_colour> c;
      zero_record(c);
      c.r.status = selected ? UNINA_COLOUR_SELECTED : 0;
      store_record(colour + i, c);
      if (selected) atomicAdd(&header->n_selected, 1);
    }
    return;
  }

  // ---- samples -> the rows' counts
  const LocateWindow w = cw.w;
  for (int t = tid; t < UNINA_COLOUR_MAX_SIDE * kColourRowStride; t += kColourBlock) s_rows[t] = 0;
  __syncthreads();
  const int cols = w.cols, ns = w.n_samples;
  for (int base = wave * kWave; base < ns; base += kColourBlock) {
    const int s = base + lane;
    const int k = s / cols, c = s - k * cols;
    int bin = kColourOther;
    bool in = false;
    if (s < ns && colour_inside(c, k, cols, w.rows, p.taper)) {
      in = true;
      const uint8_t* px = img.data + (size_t)(w.v0 + k * w.stride_y) * (size_t)img.pitch + (size_t)(w.u0 + c * w.stride_x) * (size_t)img.channels;
      bin = colour_pixel(colour_fetch(px, img.channels), p);
    }
    const int last = base + kWave - 1 < ns ? base + kWave - 1 : ns - 1;
    const int k_hi = last / cols;
    for (int kk = base / cols; kk <= k_hi; ++kk) {   // wave-uniform bounds: every lane takes part in every ballot
      const bool mine = in && k == kk;
      const unsigned long long m = __ballot(mine);
      if (m == 0ull) continue;
      int add = lane == kColourMask ? __popcll(m) : 0;
#pragma unroll
      for (int b = 0; b < kColourMask; ++b) {
        const int cnt = __popcll(__ballot(mine && bin == b));
        if (lane == b) add = cnt;
      }
      if (lane < kColourBins && add) atomicAdd(&s_rows[kk * kColourRowStride + lane], add);
    }
  }
  __syncthreads();
  if (wave != 0) return;

  // ---- rows -> the record: lane k holds row k
  int cnt[kColourBins], tot[kColourBins];
#pragma unroll
  for (int b = 0; b < kColourBins; ++b) {
    cnt[b] = lane < w.rows ? s_rows[lane * kColourRowStride + b] : 0;
    tot[b] = wave_sum(cnt[b]);
  }
  int best, second;
  colour_rank(tot, &best, &second);
  const int letter = colour_row_letter(cnt[kColourMask], colour_pick(cnt, best), best == UNINA_COLOUR_YELLOW ? cnt[kColourBlack] : cnt[kColourWhite]);
  const unsigned long long body = __ballot(letter == 1), stripe = __ballot(letter == 2);
  const int n_stripes = __popcll(__ballot(colour_run_start(body, stripe, lane)));
  const ColourDecision d = colour_decide(tot, best, second, tot[kColourMask], n_stripes, p);
  if (lane == 0) {
    if (d.decided) dw.r.class_id = d.class_id;
    store_record(out_dets + i, dw);
    RecordWords<unina_colour> c;
    c.r.votes[0] = tot[0];
    c.r.votes[1] = tot[1];
    c.r.votes[2] = tot[2];
    c.r.n_white = tot[kColourWhite];
    c.r.n_black = tot[kColourBlack];
    c.r.n_mask = tot[kColourMask];
    c.r.n_stripes = n_stripes;
    c.r.status = colour_status(cw.size, best, d);
    store_record(colour + i, c);
    atomicAdd(&header->n_selected, 1);
    atomicAdd(&header->n_window, 1);
    if (d.decided) {
      atomicAdd(&header->n_decided, 1);
      atomicAdd(&header->n_class[d.index], 1);
    }
  }
}

struct Span {
  uintptr_t lo, hi;
};

Span span_of(const void* p, size_t bytes) { return Span{(uintptr_t)p, (uintptr_t)p + bytes}; }
bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }
bool within(int v, int lo, int hi) { return v >= lo && v <= hi; }

bool colour_params_ok(const unina_colour_params* p) {
  if (!finite_pos(p->sx) || !finite_pos(p->sy) || !finite(p->shrink) || !(p->shrink > 0.0f) || !(p->shrink <= 1.0f)) return false;
  const float nonneg[3] = {p->half_width, p->above, p->below};
  for (float v : nonneg)
    if (!finite(v) || !(v >= 0.0f)) return false;
  if (!within(p->max_side, 1, UNINA_COLOUR_MAX_SIDE) || (p->order != UNINA_COLOUR_BGR && p->order != UNINA_COLOUR_RGB)) return false;
  if (!within(p->black_max, 0, 255) || !within(p->val_min, 0, 255) || !within(p->white_min, 0, 255) || !within(p->sat_min, 1, 256)) return false;
  for (int c = 0; c < 3; ++c)
    if (!within(p->hue_lo[c], 0, 1535) || !within(p->hue_hi[c], 0, 1535)) return false;
  return within(p->taper, 0, 256) && within(p->min_share, 0, 256) && within(p->max_rival, 0, 256) && p->min_pixels >= 1;
}

}  // namespace
}  // namespace unina

extern "C" int unina_colour_async(const GpuDetection* d_dets, const int* d_count, const unina_cone3d* d_cones, const unina_image* image,
                                  const unina_pinhole* cam, const unina_colour_params* p, GpuDetection* d_out_dets, unina_colour* d_colour,
                                  unina_colour_header* d_header, hipStream_t stream) {
  using namespace unina;
  if (!image || !cam || !p || !record_io_ok(d_dets, d_count, d_out_dets) || !d_colour || !d_header || !image->data) return UNINA_ERR_ARG;
  if (((uintptr_t)d_cones & 15) || ((uintptr_t)d_colour & 15) || ((uintptr_t)d_header & 15)) return UNINA_ERR_ARG;
  if ((image->channels != 3 && image->channels != 4) || !within(image->width, 1, kColourMaxDim) || !within(image->height, 1, kColourMaxDim) ||
      (long long)image->pitch < (long long)image->width * image->channels)
    return UNINA_ERR_ARG;
  if (!finite(cam->cx) || !finite(cam->cy) || !finite_pos(cam->fx) || !finite_pos(cam->fy)) return UNINA_ERR_ARG;
  if (!colour_params_ok(p)) return UNINA_ERR_ARG;
  const size_t recs = sizeof(GpuDetection) * MAX_DETECTIONS;
  const Span in = span_of(d_dets, recs), out = span_of(d_out_dets, recs), col = span_of(d_colour, sizeof(unina_colour) * MAX_DETECTIONS);
  if ((d_out_dets != d_dets && overlap(out, in)) || overlap(col, in) || overlap(col, out)) return UNINA_ERR_ARG;
  if (hipMemsetAsync(d_header, 0, sizeof(unina_colour_header), stream) != hipSuccess) return UNINA_ERR_HIP;
  const ColourImage img = {image->data, image->width, image->height, image->pitch, image->channels};
  hipLaunchKernelGGL(colour_kernel, dim3(MAX_DETECTIONS), dim3(kColourBlock), 0, stream, d_dets, d_count, d_cones, img, cam->fx, cam->fy, *p,
                     d_out_dets, d_colour, d_header);
  return launch_status();
}
