// engine.hip -- engine handle behind the C ABI of include/unina_mi355.h.
//
// Role in the reference: class TensorRTEngine (ros2_ws/src/perception/src/perception_node.cpp:223-351) plus
// the per-frame body of processGpuBuffer (perception_node.cpp:612-656). Here the "plan" is an explicit op
// table (engine_format.h) executed as hand-written HIP kernels; the whole forward is captured once into a
// hipGraph and replayed per frame (52 launches -> one graph launch), the post-process is one more launch.
//
// Memory: one HBM blob for all folded weights (10 MB fp16), one arena for the NHWC fp16 activation buffers
// (86 MB at 640^2 -- every tensor keeps its own slot; with 288 GB there is nothing to gain from aliasing and
// distinct slots keep two handles = two frames in flight trivially independent).
#include <cstdarg>
#include <cstdio>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "calib.h"
#include "engine_format.h"
#include "engine_validate.h"
#include "kernels.h"
#include "mining.h"

using namespace unina;

static_assert(kMaxClasses == (uint32_t)kMaxNumClasses, "the validator's class-count limit is the post-process's class field");

hipError_t unina::kernels_init() {
  for (hipError_t (*init)() : {conv_init, c3k2_init, head_init, pair_init, block_dual_init, stem_pool_init, post_init, calib_init}) {
    const hipError_t e = init();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

namespace {

thread_local std::string g_load_error = "";

struct Buffer {
  BufferDesc d;
  void* ptr = nullptr;    // current device address (engine-owned or caller-bound)
  void* owned = nullptr;  // engine-owned allocation (inside the arena), if any
  size_t bytes = 0;
};

struct PlannedOp {
  OpDesc d;
  ConvParams cp;
  int cfg = -1;             // conv: tile configuration (conv_plan)
  StemParams sp;
  PoolParams pp;
  QuantParams qp;
  unina_op_info info;
  // fused C3k2 block (c3k2_fused.hip): role 1 = first op of a fusable group (launches the whole block when fusion is
  // on), 2 = absorbed by the group's first op (no launch of its own when fusion is on), 0 = ordinary op
  int fuse_role = 0;
  int fuse_kind = 0;        // role 1: 1 = C3k2 block (c3k2_fused.hip), 2 = DetectionHead (head_fused.hip), 4 = conv pair (conv_pair.hip)
  HeadParams hp;
  PairParams pr;            // fuse_kind 4: two consecutive 1x1 convs (conv_pair.hip)
  int group_last = -1;      // role 1: index of the group's last op (cv3 / the head's output convs)
  int dual_with = -1;       // >= 0: this conv and conv `dual_with` (independent, same kernel family) run as ONE grid
  int dual_kind = -1;
  bool dual_absorbed = false;   // runs inside an earlier op's dual launch
  int tail_op = -1;         // role 1, C3k2: index of the 1x1 conv that runs as the block kernel's last step
  int tail_kind = 0;        // 1: lateral 1x1 + x2 upsample store; 2: plain 1x1 ConvBlock (same resolution); 3: 1 with int8 in, fp16 out
  uint64_t wt_off = 0;      // stem: blob offset of the transposed weights [27][Co] (appended at load)
  uint64_t w_lane_off[2] = {0, 0};   // conv: blob offset of each slice's weights in LANE order (appended at load; 0 = none)
  int fuse_pre = 0;         // role 1, C3k2: 1 = this op is the 3x3/s2 conv in front of the block (the block's cv1|cv2 is the NEXT op)
  int quant_op = -1;        // role 1, fp16 C3k2 in an INT8 engine: the QUANT op of the block's output that the kernel's store absorbs
  int hid = 0, nb = 0;      // role 1: hidden width, bottleneck count
  uint64_t stream_off = 0, fbias_off = 0;   // role 1: blob offsets of the packed stage stream / concatenated biases
  C3k2Params fp;
};

struct DeviceResult {  // what the fused post-process writes; one D2H brings count + records
  int count;
  int candidates;
  unsigned int seq;    // host block only: the sequence number the post-process stores last (unina_infer's completion word)
  int pad[5];
  GpuDetection det[MAX_DETECTIONS];
  long long pad_stamps[16]; // debug phase stamps of the post-process kernel (UNINA_POST_STAMPS=1) / of a conv or a dual conv launch
};
static_assert(kPostStampCount <= (int)(sizeof(DeviceResult::pad_stamps) / sizeof(long long)), "every PostStamp slot fits pad_stamps");

}  // namespace

struct unina_engine {
  int device = 0;
  FileHeader h;
  std::vector<Buffer> bufs;
  std::vector<PlannedOp> ops;
  void* d_blob = nullptr;
  void* d_arena = nullptr;
  void* d_zeros = nullptr;          // zero page read by out-of-image taps
  std::vector<int> force_cfg;       // per-op tile configuration override (-1 = heuristic)
  bool fuse = false;                // run fusable C3k2 groups as one launch each (fp16 engines; UNINA_FUSE=0 / unina_set_fusion)
  int n_groups = 0;                 // fusable groups found at load
  int images_buf = -1;
  int out_buf[6] = {-1, -1, -1, -1, -1, -1};
  // post-process workspace
  GpuDetection* d_cand = nullptr;
  int* d_block_count = nullptr;
  unsigned int* d_ticket = nullptr;
  void* d_post_ws = nullptr;         // two-launch post-process workspace (sorted candidates, mask tiles, second ticket)
  DeviceResult* d_result = nullptr;
  DeviceResult* h_result = nullptr;  // pinned
  DeviceResult* h_result_dev = nullptr;  // the same block as the device addresses it (hipHostGetDevicePointer)
  unsigned int result_seq = 0;           // synchronous calls so far (infer_sync's completion word)
  int post_blocks = 0;
  // graph
  bool use_graph = true;
  bool plan_dirty = true;
  double t_submit_us = 0, t_wait_us = 0, t_copy_us = 0;   // UNINA_TIMING=1: host-side split of unina_infer (printed at unload)
  long t_calls = 0;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  // full-frame graph (unina_infer / unina_infer_async): stem + forward + post-process as ONE hipGraphLaunch. The two
  // nodes whose parameters change from frame to frame (input pointer; thresholds / output buffers) are re-pointed with
  // hipGraphExecKernelNodeSetParams instead of being launched separately (which cost a ~9 us bubble in front of the
  // post-process and a separate submission for the stem).
  bool full_graph = true;
  hipGraph_t fgraph = nullptr;
  hipGraphExec_t fexec = nullptr;
  hipGraphNode_t stem_node = nullptr, post_node = nullptr, post_node2 = nullptr;
  bool post_split = true;            // post-process kPostSplit: two launches, compact candidate list, sort-free NMS (UNINA_POST_SPLIT=0: kPostOneLaunch)
  bool fold_heads = true;            // full-frame graph: the heads' output convs run inside the decode launch (UNINA_POST_FOLD=0: off)
  int fold_op[3] = {-1, -1, -1};     // per head: the output-conv op the decode launch absorbs (-1: the head is read from its planes)
  int stem_op = -1;
  StemParams f_stem;
  PostParams f_post;
  // data mining (mining.hip): the conv op whose output slice is the embedding's source (backbone.stage3_c3k2.cv3; -1: the
  // engine has none, graph (B)), and the partial / staging workspace allocated by the first mining call
  int embed_op = -1;
  float* d_mine_ws = nullptr;
  // sliced inference: UNINA_MAX_TILES detection slots ([tile][MAX_DETECTIONS] records, then the counts), allocated by the first
  // tiled call
  GpuDetection* d_tile_slots = nullptr;
  // INT8 calibration (calib.hip): the kBufF16Nhwc buffers in file order and their descriptor table on the device, built by the
  // first calibration call (those buffers live in the arena: their addresses never change)
  std::vector<int> calib_bufs;
  CalibDesc* d_calib_tab = nullptr;
  unsigned calib_grid = 0;
  std::string err;
};

namespace {

int fail(unina_engine* e, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (e) e->err = buf; else g_load_error = buf;
  return code;
}

#define HIPCHK(e, call)                                                                          \
  do {                                                                                           \
    hipError_t _err = (call);                                                                    \
    if (_err != hipSuccess) return fail((e), UNINA_ERR_HIP, "%s: %s", #call, hipGetErrorString(_err)); \
  } while (0)

size_t buffer_bytes(const BufferDesc& d) {
  const size_t n = (size_t)d.h * d.w * d.c;
  return d.dtype == kBufF16Nhwc ? n * 2 : (d.dtype == kBufI8Nhwc ? n : n * 4);   // (kBufS16Nhwc: two fp16 planes, hi then lo)
}
// split fp16 buffers: byte distance from the hi plane to the lo plane
long long lo_plane(const BufferDesc& d) { return d.dtype == kBufS16Nhwc ? (long long)d.h * d.w * d.c * 2 : 0; }

// element type of an NHWC activation buffer (-1: not an activation buffer)
int act_dtype_of(uint32_t buf_dtype) {
  return buf_dtype == kBufF16Nhwc ? kF16 : (buf_dtype == kBufF32Nhwc ? kF32 : (buf_dtype == kBufI8Nhwc ? kI8 : (buf_dtype == kBufS16Nhwc ? kS16 : -1)));
}
size_t dtype_size(int dt) { return dt == kF32 ? 4 : (dt == kI8 ? 1 : 2); }        // bytes per element of one plane (addressing)
double dtype_bytes(int dt) { return dt == kS16 ? 4.0 : (double)dtype_size(dt); }   // bytes per value (traffic accounting)

int engine_dtype(const unina_engine* e);

// The library keeps NO stream of its own. The runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues per priority
// (default 4) when they are created: a fresh queue while there is one, after that the least-referenced existing one -- and
// two streams on one queue run one after the other. A stream that only ever records a graph still holds its queue, so one
// per handle (as it was until round 5) pushed the caller's second frame stream onto a shared queue (profiles/r05). A
// capture therefore makes its stream, records, and destroys it again, on every path out: once per plan, never per frame.
// Per capture, not per process: the capture mode is thread-local and two threads may capture at once.
std::atomic<int> g_owned_streams{0};   // streams of the library alive in this process (unina_debug_owned_streams): 0 at rest

struct CaptureStream {
  hipStream_t s = nullptr;
  bool open = false;
  hipError_t begin() {
    hipError_t err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (err != hipSuccess) {
      s = nullptr;
      return err;
    }
    ++g_owned_streams;
    err = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    open = err == hipSuccess;
    return err;
  }
  hipError_t end(hipGraph_t* graph) {
    open = false;
    return hipStreamEndCapture(s, graph);
  }
  ~CaptureStream() {
    if (open) {   // a return between begin and end: close the capture, drop what it recorded
      hipGraph_t g = nullptr;
      if (hipStreamEndCapture(s, &g) == hipSuccess && g) (void)hipGraphDestroy(g);
    }
    if (s) {
      (void)hipStreamDestroy(s);
      --g_owned_streams;
    }
  }
  CaptureStream() = default;
  CaptureStream(const CaptureStream&) = delete;
  CaptureStream& operator=(const CaptureStream&) = delete;
};

void drop_graph(unina_engine* e) {
  if (e->exec) (void)hipGraphExecDestroy(e->exec);
  if (e->graph) (void)hipGraphDestroy(e->graph);
  if (e->fexec) (void)hipGraphExecDestroy(e->fexec);
  if (e->fgraph) (void)hipGraphDestroy(e->fgraph);
  e->exec = nullptr;
  e->graph = nullptr;
  e->fexec = nullptr;
  e->fgraph = nullptr;
  e->stem_node = e->post_node = e->post_node2 = nullptr;
}

int engine_dtype(const unina_engine* e) { return e->h.precision == kFp32 ? kF32 : (e->h.precision == kSplit16 ? kS16 : kF16); }

// ---- dependency analysis over the op table (buffer id + channel range granularity) ----
struct Region {
  int buf, c0, c1;
};
bool overlaps(const Region& a, const Region& b) { return a.buf == b.buf && a.c0 < b.c1 && b.c0 < a.c1; }
Region whole(int buf) { return {buf, INT_MIN, INT_MAX}; }   // every channel of a buffer

// What op `d` reads and writes, as the op table describes it (no fusion). Where a kernel's access is wider than its slices
// the footprint is too: QUANT (and UPSAMPLE, which no kernel executes) covers whole buffers, the SPPF pool reads its
// whole buffer (x and the maps it chains through) and writes y1..y3 behind x, a residual is a read of its whole buffer.
void footprint(const OpDesc& d, std::vector<Region>* reads, std::vector<Region>* writes) {
  const bool whole_bufs = d.kind == kOpQuant || d.kind == kOpUpsample;
  for (uint32_t s = 0; s < d.nseg; ++s) {
    const SegDesc& sd = d.seg[s];
    const int cin = d.kind == kOpStem ? 3 : (int)d.cin;
    const bool ranged = d.kind == kOpConv || d.kind == kOpStem;
    reads->push_back(ranged ? Region{(int)d.src_buf, (int)sd.src_coff, (int)sd.src_coff + cin} : whole((int)d.src_buf));
    writes->push_back(whole_bufs ? whole((int)sd.dst_buf) : Region{(int)sd.dst_buf, (int)sd.dst_coff, (int)(sd.dst_coff + sd.n_count)});
  }
  if (d.kind == kOpSppfPool) {
    const int c0 = (int)d.seg[0].src_coff, C = (int)d.cin;
    writes->push_back({(int)d.src_buf, c0 + C, c0 + 4 * C});
  }
  if (d.res_buf >= 0) reads->push_back(whole(d.res_buf));
}

// Does any op outside ops [lo, hi] read or write region `r`? (The fusion matchers' test that a tensor is private to a group.)
bool touched_outside(const unina_engine* e, const Region& r, size_t lo, size_t hi) {
  std::vector<Region> rw;   // reads and writes alike
  for (size_t k = 0; k < e->ops.size(); ++k) {
    if (k >= lo && k <= hi) continue;
    rw.clear();
    footprint(e->ops[k].d, &rw, &rw);
    for (const Region& x : rw)
      if (overlaps(r, x)) return true;
  }
  return false;
}

void op_regions(const unina_engine* e, size_t i, std::vector<Region>* reads, std::vector<Region>* writes) {
  const OpDesc& d = e->ops[i].d;
  reads->clear();
  writes->clear();
  if (e->fuse && e->ops[i].fuse_role == 2) return;
  if (e->ops[i].dual_absorbed) return;
  if (e->ops[i].dual_with >= 0 && !e->ops[i].fuse_role) {   // the pair's reads / writes, at the leader's position
    const int pair[2] = {(int)i, e->ops[i].dual_with};
    for (int k : pair) {
      const OpDesc& dk = e->ops[k].d;
      for (uint32_t s = 0; s < dk.nseg; ++s) {
        reads->push_back({(int)dk.src_buf, (int)dk.seg[s].src_coff, (int)(dk.seg[s].src_coff + dk.cin)});
        writes->push_back({(int)dk.seg[s].dst_buf, (int)dk.seg[s].dst_coff, (int)(dk.seg[s].dst_coff + dk.seg[s].n_count)});
      }
    }
    return;
  }
  if (e->fuse && e->ops[i].fuse_role == 1) {
    const OpDesc& last = e->ops[e->ops[i].group_last].d;
    reads->push_back({(int)d.src_buf, (int)d.seg[0].src_coff, (int)(d.seg[0].src_coff + d.cin)});
    if (e->ops[i].fuse_kind == 1 && e->ops[i].fuse_pre) {   // pre-conv: the block also reads the part of its input the pre-conv does not produce
      const OpDesc& blk = e->ops[i + 1].d;
      if (d.seg[0].n_count < blk.cin)
        reads->push_back({(int)blk.src_buf, (int)(blk.seg[0].src_coff + d.seg[0].n_count), (int)(blk.seg[0].src_coff + blk.cin)});
    }
    if (e->ops[i].fuse_kind == 4) {   // the first conv's output goes to HBM too
      const OpDesc& c1 = e->ops[i + e->ops[i].fuse_pre].d;
      writes->push_back({(int)c1.seg[0].dst_buf, (int)c1.seg[0].dst_coff, (int)(c1.seg[0].dst_coff + c1.seg[0].n_count)});
    }
    for (uint32_t s = 0; s < last.nseg; ++s)
      writes->push_back({(int)last.seg[s].dst_buf, (int)last.seg[s].dst_coff, (int)(last.seg[s].dst_coff + last.seg[s].n_count)});
    if (e->ops[i].tail_op >= 0) {
      const SegDesc& ts = e->ops[e->ops[i].tail_op].d.seg[0];
      writes->push_back({(int)ts.dst_buf, (int)ts.dst_coff, (int)(ts.dst_coff + ts.n_count)});
    }
    if (e->ops[i].quant_op >= 0) {
      const SegDesc& qs = e->ops[e->ops[i].quant_op].d.seg[0];
      writes->push_back({(int)qs.dst_buf, (int)qs.dst_coff, (int)(qs.dst_coff + qs.n_count)});
    }
    if (e->ops[i].dual_with >= 0) {   // block dual: the partner group's reads / writes happen here too
      const PlannedOp& hb = e->ops[e->ops[i].dual_with];
      const OpDesc& hl = e->ops[hb.group_last].d;
      reads->push_back({(int)hb.d.src_buf, (int)hb.d.seg[0].src_coff, (int)(hb.d.seg[0].src_coff + hb.d.cin)});
      for (uint32_t s = 0; s < hl.nseg; ++s)
        writes->push_back({(int)hl.seg[s].dst_buf, (int)hl.seg[s].dst_coff, (int)(hl.seg[s].dst_coff + hl.seg[s].n_count)});
    }
    return;
  }
  footprint(d, reads, writes);
}

// Which heads' output convs (model.py:292,299: Conv2d(C, nc | 4, 1) with bias, the `.2` layers) can run inside the decode
// launch of the post-process (postprocess.hip, fold): a plain fp16 1x1 conv op of two slices that write the head's cls
// and reg planes, at most 16 output channels each. A head whose output conv already lives in a fused launch (the P2
// head kernel) is read from its planes instead.
void find_fold_ops(unina_engine* e) {
  for (int h = 0; h < 3; ++h) e->fold_op[h] = -1;
  if (!e->fold_heads || !e->post_split) return;
  for (size_t i = 0; i < e->ops.size(); ++i) {
    const PlannedOp& op = e->ops[i];
    if (op.d.kind != kOpConv || (e->fuse && op.fuse_role)) continue;
    const ConvParams& c = op.cp;
    if ((c.dtype != kF16 && c.dtype != kS16) || c.ksize != 1 || c.stride != 1 || c.relu || c.res || c.nseg != 2 || (c.Cin & 31)) continue;
    for (int h = 0; h < 3; ++h) {
      const void* pc = e->bufs[e->out_buf[2 * h]].ptr;
      const void* pr = e->bufs[e->out_buf[2 * h + 1]].ptr;
      if (!pc || !pr || c.seg[0].dst_planar != pc || c.seg[1].dst_planar != pr) continue;
      if (c.seg[0].n_count > 16 || c.seg[1].n_count > 16 || c.seg[0].mult || c.seg[1].mult) continue;
      if (c.M != (int)(e->bufs[e->out_buf[2 * h]].d.w * e->bufs[e->out_buf[2 * h]].d.h)) continue;
      e->fold_op[h] = (int)i;
    }
  }
}

// Kernel parameters and info of op `i` as a launch of its own. Kinds, types, slices, offsets and channel multiples are what
// validate_engine (engine_validate.h) accepted at load; what is left here depends on the device and the handle.
int plan_op(unina_engine* e, size_t i) {
  const char* blob = static_cast<const char*>(e->d_blob);
  PlannedOp& op = e->ops[i];
  const OpDesc& d = op.d;
  const Buffer& src = e->bufs[d.src_buf];
  unina_op_info& info = op.info;
  memset(&info, 0, sizeof info);
  snprintf(info.name, sizeof info.name, "%s", d.name);
  info.kind = (int)d.kind;
  if (d.kind == kOpConv) {
    ConvParams& p = op.cp;
    memset(&p, 0, sizeof p);
    const int dt = act_dtype_of(src.d.dtype);
    p.dtype = dt;
    p.src = src.ptr;
    p.src_lo = lo_plane(src.d);
    p.src_ld = (int)src.d.c;
    p.H = (int)d.in_h; p.W = (int)d.in_w; p.Cin = (int)d.cin;
    p.Ho = (int)d.out_h; p.Wo = (int)d.out_w; p.M = p.Ho * p.Wo;
    p.ksize = (int)d.ksize; p.stride = (int)d.stride; p.pad = (int)d.ksize / 2;
    p.relu = (int)d.relu;
    if (d.res_buf >= 0) {
      const Buffer& rb = e->bufs[d.res_buf];
      const int rdt = act_dtype_of(rb.d.dtype);
      p.res = static_cast<const char*>(rb.ptr) + (size_t)d.res_coff * dtype_size(rdt);
      p.res_ld = (int)rb.d.c;
      p.res_dtype = rdt;
      p.res_lo = lo_plane(rb.d);
      p.res_scale = rb.d.scale;
    }
    p.nseg = (int)d.nseg;
    p.zeros = e->d_zeros;
    p.force_cfg = i < e->force_cfg.size() ? e->force_cfg[i] : -1;
    int ntot = 0;
    double out_bytes = 0;
    for (int s = 0; s < p.nseg; ++s) {
      const SegDesc& sd = d.seg[s];
      const Buffer& db = e->bufs[sd.dst_buf];
      ConvSeg& cs = p.seg[s];
      cs.w = blob + sd.w_off;
      cs.w_lane = op.w_lane_off[s] ? blob + op.w_lane_off[s] : nullptr;
      cs.bias = reinterpret_cast<const float*>(blob + sd.b_off);
      cs.mult = sd.m_off ? reinterpret_cast<const float*>(blob + sd.m_off) : nullptr;
      cs.src_coff = (int)sd.src_coff;
      cs.n_count = (int)sd.n_count;
      cs.up2 = (sd.flags & kSegUp2) ? 1 : 0;
      if (sd.flags & kSegPlanarF32) {
        cs.dst_planar = static_cast<float*>(db.ptr);
        cs.dst = nullptr;
        cs.dst_ld = 0;
        cs.out_dtype = kF32;
        out_bytes += 4.0 * sd.n_count * p.M;
      } else {
        const int odt = act_dtype_of(db.d.dtype);
        cs.dst = static_cast<char*>(db.ptr) + (size_t)sd.dst_coff * dtype_size(odt);
        cs.dst_planar = nullptr;
        cs.dst_ld = (int)db.d.c;
        cs.out_dtype = odt;
        cs.dst_lo = lo_plane(db.d);
        cs.out_inv_scale = odt == kI8 ? 1.0f / db.d.scale : 1.0f;
        out_bytes += dtype_bytes(odt) * sd.n_count * p.M * (cs.up2 ? 4 : 1);
      }
      ntot += (int)sd.n_count;
    }
    if (p.force_cfg >= 0 && !conv_config_valid(p, p.force_cfg)) p.force_cfg = -1;
    op.cfg = conv_plan(p);
    const int K = p.ksize * p.ksize * p.Cin;
    info.m = p.M; info.n = ntot; info.k = K;
    info.flops = 2.0 * p.M * (double)ntot * K;
    // algorithmic bytes: each distinct input element once, weights once, outputs once, residual once
    const bool shared_src = p.nseg == 1 || d.seg[0].src_coff == d.seg[1].src_coff;
    info.bytes = dtype_bytes(dt) * p.H * p.W * p.Cin * (shared_src ? 1 : p.nseg) + dtype_bytes(dt) * ntot * K + 4.0 * ntot + out_bytes +
                 (p.res ? dtype_bytes(p.res_dtype) * p.M * ntot : 0.0);
  } else if (d.kind == kOpStem) {
    const SegDesc& sd = d.seg[0];
    const Buffer& db = e->bufs[sd.dst_buf];
    StemParams& p = op.sp;
    const int odt = act_dtype_of(db.d.dtype);
    p.dtype = odt;
    p.dst_lo = lo_plane(db.d);
    p.src = static_cast<const float*>(src.ptr);
    p.w = reinterpret_cast<const float*>(blob + sd.w_off);
    p.wt = reinterpret_cast<const float*>(blob + op.wt_off);
    p.bias = reinterpret_cast<const float*>(blob + sd.b_off);
    p.dst = static_cast<char*>(db.ptr) + (size_t)sd.dst_coff * dtype_size(odt);
    p.H = (int)d.in_h; p.W = (int)d.in_w; p.Ho = (int)d.out_h; p.Wo = (int)d.out_w;
    p.Co = (int)sd.n_count; p.dst_ld = (int)db.d.c;
    info.m = p.Ho * p.Wo; info.n = p.Co; info.k = 27;
    info.flops = 2.0 * info.m * info.n * 27;
    info.bytes = 4.0 * 3 * p.H * p.W + dtype_bytes(odt) * info.m * p.Co;
  } else if (d.kind == kOpSppfPool) {
    PoolParams& p = op.pp;
    const int dt = act_dtype_of(src.d.dtype);
    p.dtype = dt;
    p.buf = src.ptr;
    p.lo = lo_plane(src.d);
    p.H = (int)d.in_h; p.W = (int)d.in_w; p.C = (int)d.cin; p.ld = (int)src.d.c; p.coff = (int)d.seg[0].src_coff;
    info.bytes = dtype_bytes(dt) * p.H * p.W * p.C * 4;
  } else {   // kOpQuant
    const Buffer& db = e->bufs[d.seg[0].dst_buf];
    QuantParams& p = op.qp;
    p.src = static_cast<const half_t*>(src.ptr);
    p.dst = static_cast<signed char*>(db.ptr);
    p.n = (size_t)src.d.h * src.d.w * src.d.c;
    p.inv_scale = 1.0f / db.d.scale;
    info.bytes = 3.0 * p.n;
  }
  return UNINA_OK;
}

// Op b's work now runs inside op `at`'s launch, whose info is `a` (`how`: "fused into" / "dual launch with"): a takes over
// b's flops and bytes, b names that launch. (a's kernel and geometry are its launch's: launch_info.)
void absorb_info(unina_op_info* a, unina_op_info* b, const char* how, size_t at) {
  a->flops += b->flops;
  a->bytes += b->bytes;
  b->flops = 0;
  b->bytes = 0;
  b->grid = 0;
  snprintf(b->kernel, sizeof b->kernel, "(%s op %zu)", how, at);
}

// Fused conv pair led by op `i` (conv_pair.hip), with the SPPF pool in front when fuse_pre.
int plan_pair(unina_engine* e, size_t i) {
  const char* blob = static_cast<const char*>(e->d_blob);
  PlannedOp& op = e->ops[i];
  const OpDesc& a = e->ops[i + op.fuse_pre].d;
  PlannedOp& zb = e->ops[op.group_last];
  const OpDesc& z = zb.d;
  const Buffer& src = e->bufs[a.src_buf];
  const Buffer& mid = e->bufs[a.seg[0].dst_buf];
  const Buffer& out = e->bufs[z.seg[0].dst_buf];
  PairParams& f = op.pr;
  memset(&f, 0, sizeof f);
  f.dtype = act_dtype_of(src.d.dtype);
  const size_t esz = dtype_size(f.dtype);
  f.src = static_cast<const char*>(src.ptr) + a.seg[0].src_coff * esz;
  f.src_ld = (int)src.d.c;
  f.c0 = (int)a.cin; f.c1 = (int)a.seg[0].n_count; f.c2 = (int)z.seg[0].n_count;
  f.H = (int)a.in_h; f.W = (int)a.in_w;
  f.dst = static_cast<char*>(mid.ptr) + a.seg[0].dst_coff * esz;
  f.dst_ld = (int)mid.d.c;
  f.dst2 = static_cast<char*>(out.ptr) + z.seg[0].dst_coff * esz;
  f.dst2_ld = (int)out.d.c;
  f.up2 = (z.seg[0].flags & kSegUp2) ? 1 : 0;
  f.src_lo = lo_plane(src.d); f.dst_lo = lo_plane(mid.d); f.dst2_lo = lo_plane(out.d);
  f.pool = op.fuse_pre;
  f.wstream = reinterpret_cast<const unsigned char*>(blob + op.stream_off);
  f.bias = reinterpret_cast<const float*>(blob + op.fbias_off);
  f.zeros = e->d_zeros;
  if (!pair_layout(&f)) return fail(e, UNINA_ERR_UNSUPPORTED, "op %zu: fused conv pair does not fit", i);
  if (!e->fuse) return UNINA_OK;
  if (op.fuse_pre) {   // the pool op is the group's head: the infos of cv2 move onto it (the pool's own traffic is not counted)
    unina_op_info& ai = e->ops[i + 1].info;
    op.info.m = ai.m; op.info.n = ai.n;
    op.info.flops = op.info.bytes = 0;
    absorb_info(&op.info, &ai, "fused into", i);
    op.info.bytes -= dtype_bytes(f.dtype) * f.H * f.W * 3 * (f.c0 / 4);   // the pooled maps are formed in LDS
  }
  absorb_info(&op.info, &zb.info, "fused into", i);
  op.info.bytes -= dtype_bytes(f.dtype) * f.H * f.W * f.c1;     // the second conv reads the first's output from LDS
  op.info.k = 0;
  snprintf(op.info.name, sizeof op.info.name, "%.40s+%.40s", a.name, z.name);
  return UNINA_OK;
}

// Fused DetectionHead led by op `i` (head_fused.hip).
int plan_head(unina_engine* e, size_t i) {
  const char* blob = static_cast<const char*>(e->d_blob);
  PlannedOp& op = e->ops[i];
  const OpDesc& a = op.d;
  const OpDesc& z = e->ops[op.group_last].d;
  const Buffer& src = e->bufs[a.src_buf];
  HeadParams& f = op.hp;
  memset(&f, 0, sizeof f);
  f.src = static_cast<const half_t*>(src.ptr) + a.seg[0].src_coff;
  f.src_ld = (int)src.d.c;
  f.C = (int)a.cin;
  f.H = (int)a.in_h;
  f.W = (int)a.in_w;
  f.out_cls = static_cast<float*>(e->bufs[z.seg[0].dst_buf].ptr);
  f.out_reg = static_cast<float*>(e->bufs[z.seg[1].dst_buf].ptr);
  f.n_cls = (int)z.seg[0].n_count;
  f.n_reg = (int)z.seg[1].n_count;
  f.wstream = reinterpret_cast<const unsigned char*>(blob + op.stream_off);
  f.bias = reinterpret_cast<const float*>(blob + op.fbias_off);
  f.zeros = e->d_zeros;
  if (!head_layout(&f)) return fail(e, UNINA_ERR_UNSUPPORTED, "op %zu: fused head does not fit", i);
  if (!e->fuse) return UNINA_OK;
  unina_op_info& info = op.info;
  double wbytes = 0;
  for (int k = (int)i; k <= op.group_last; ++k) {
    wbytes += 2.0 * e->ops[k].info.n * e->ops[k].info.k + 4.0 * e->ops[k].info.n;
    if (k > (int)i) absorb_info(&info, &e->ops[k].info, "fused into", i);
  }
  info.bytes = 2.0 * f.H * f.W * f.C + wbytes + 4.0 * f.H * f.W * (f.n_cls + f.n_reg);
  info.n = f.n_cls + f.n_reg;
  info.k = 0;
  snprintf(info.name, sizeof info.name, "%.*s[head]", (int)(strchr(a.name, '.') ? strchr(a.name, '.') - a.name : 60), a.name);
  return UNINA_OK;
}

// Fused C3k2 block led by op `i` (c3k2_fused.hip), with its pre-conv, tail conv and QUANT store where the matcher found them.
int plan_c3k2(unina_engine* e, size_t i) {
  const char* blob = static_cast<const char*>(e->d_blob);
  PlannedOp& op = e->ops[i];
  const OpDesc& a = e->ops[i + op.fuse_pre].d;   // the block's cv1|cv2
  const OpDesc& z = e->ops[op.group_last].d;
  const OpDesc& in = op.d;                       // the op whose input the kernel reads (the pre-conv, or cv1|cv2 itself)
  const Buffer& src = e->bufs[in.src_buf];
  const Buffer& dst = e->bufs[z.seg[0].dst_buf];
  C3k2Params& f = op.fp;
  memset(&f, 0, sizeof f);
  f.dtype = act_dtype_of(src.d.dtype);
  const size_t fesz = dtype_size(f.dtype);
  const double fb = dtype_bytes(f.dtype);
  f.src = static_cast<const char*>(src.ptr) + in.seg[0].src_coff * fesz;
  f.src_ld = (int)src.d.c;
  if (op.fuse_pre) {
    f.cpre = (int)in.cin;
    f.preH = (int)in.in_h;
    f.preW = (int)in.in_w;
    f.cx = (int)in.seg[0].n_count;
    const Buffer& xb = e->bufs[a.src_buf];   // the rest of the block's input (a concat's other part) still comes from HBM
    f.src2 = static_cast<const char*>(xb.ptr) + (a.seg[0].src_coff + f.cx) * fesz;
    f.src2_ld = (int)xb.d.c;
    f.src2_lo = lo_plane(xb.d);
  }
  f.src_lo = lo_plane(src.d);
  f.dst_lo = lo_plane(dst.d);
  f.Cin = (int)a.cin;
  f.H = (int)a.in_h;
  f.W = (int)a.in_w;
  f.dst = static_cast<char*>(dst.ptr) + z.seg[0].dst_coff * fesz;
  f.dst_ld = (int)dst.d.c;
  for (int b = 0; b < op.nb; ++b) {   // int8: scale of each bottleneck's shortcut tensor (the 3x3's residual buffer)
    const OpDesc& c2 = e->ops[i + op.fuse_pre + 2 + 2 * b].d;
    f.res_scale[b] = c2.res_buf >= 0 ? e->bufs[c2.res_buf].d.scale : 1.0f;
  }
  f.wstream = reinterpret_cast<const unsigned char*>(blob + op.stream_off);
  f.bias = reinterpret_cast<const float*>(blob + op.fbias_off);
  f.zeros = e->d_zeros;
  f.hid = op.hid;
  f.nb = op.nb;
  if (op.tail_op >= 0) {
    const SegDesc& ts = e->ops[op.tail_op].d.seg[0];
    const Buffer& tb = e->bufs[ts.dst_buf];
    f.tail = op.tail_kind;
    f.dst2 = static_cast<char*>(tb.ptr) + ts.dst_coff * (op.tail_kind == 3 ? 2 : fesz);
    f.dst2_ld = (int)tb.d.c;
    f.dst2_lo = lo_plane(tb.d);
  }
  if (op.quant_op >= 0) {
    const Buffer& qb = e->bufs[e->ops[op.quant_op].d.seg[0].dst_buf];
    f.dst_q = static_cast<signed char*>(qb.ptr);
    f.dst_q_ld = (int)qb.d.c;
    f.q_inv = 1.0f / qb.d.scale;   // as the QUANT op's own parameter
  }
  if (!c3k2_layout(&f)) return fail(e, UNINA_ERR_UNSUPPORTED, "op %zu: fused C3k2 block does not fit", i);
  if (!e->fuse) return UNINA_OK;
  unina_op_info& info = op.info;
  double wbytes = 0;
  const int last_op = op.tail_op >= 0 ? op.tail_op : op.group_last;
  for (int k = (int)i; k <= last_op; ++k) {
    wbytes += fb * e->ops[k].info.n * e->ops[k].info.k + 4.0 * e->ops[k].info.n;
    if (k > (int)i) absorb_info(&info, &e->ops[k].info, "fused into", i);
  }
  if (op.quant_op >= 0) absorb_info(&info, &e->ops[op.quant_op].info, "fused into", i);
  info.bytes = (f.cpre ? fb * (f.preH * f.preW * f.cpre + f.H * f.W * (f.Cin - f.cx)) : fb * f.H * f.W * f.Cin) + wbytes + fb * f.H * f.W * 2 * f.hid +   // input once, weights once, output once
               (f.tail ? fb * (f.tail == 1 ? 4 : 1) * f.H * f.W * f.hid : 0.0);            // (+ the tail conv's output)
  info.n = 2 * f.hid;
  info.k = 0;
  snprintf(info.name, sizeof info.name, "%.*s[c3k2 x%d]", (int)(strchr(a.name, '+') ? strchr(a.name, '+') - a.name - 4 : 60), a.name, f.nb);
  return UNINA_OK;
}

// May an op that reads `r` and writes `w` move across ops [lo, hi] (to either side of them)? None of them may write what it
// reads, or read or write what it writes. Their regions are taken as they stand, so pairs already made count.
bool may_cross(const unina_engine* e, size_t lo, size_t hi, const std::vector<Region>& r, const std::vector<Region>& w) {
  std::vector<Region> rk, wk;
  for (size_t k = lo; k <= hi; ++k) {
    op_regions(e, k, &rk, &wk);
    for (const Region& x : wk) {
      for (const Region& y : r)
        if (overlaps(x, y)) return false;
      for (const Region& y : w)
        if (overlaps(x, y)) return false;
    }
    for (const Region& x : rk)
      for (const Region& y : w)
        if (overlaps(x, y)) return false;
  }
  return true;
}

// Dual launches: pair independent convs of one kernel family (the P3 / P4 head layers) into one grid each. The later
// op moves to the earlier one's position, so nothing between them may feed it or touch what it writes.
void plan_duals(unina_engine* e) {
  for (auto& op : e->ops) {
    op.dual_with = op.dual_kind = -1;
    op.dual_absorbed = false;
  }
  if (!e->fuse || getenv("UNINA_NO_DUAL")) return;
  const size_t n = e->ops.size();
  std::vector<Region> ra, wa, rb, wb;
  // a fused C3k2 block and the fused head that does not depend on it (pan_c3k2_2 and head_p2): block_dual.hip
  for (size_t i = 0; i < n; ++i) {
    PlannedOp& a = e->ops[i];
    if (a.fuse_role != 1 || a.fuse_kind != 1 || a.dual_with >= 0) continue;
    for (size_t j = i + 1; j < n; ++j) {
      PlannedOp& b = e->ops[j];
      if (b.fuse_role != 1 || b.fuse_kind != 2 || b.dual_absorbed || !block_dual_match(a.fp, b.hp)) continue;
      op_regions(e, j, &rb, &wb);
      if (!may_cross(e, i, j - 1, rb, wb)) continue;
      a.dual_with = (int)j;
      b.dual_absorbed = true;
      absorb_info(&a.info, &b.info, "dual launch with", i);
      break;
    }
  }
  for (size_t i = 0; i < n; ++i) {
    PlannedOp& a = e->ops[i];
    if (a.d.kind != kOpConv || a.fuse_role || a.dual_absorbed || a.dual_with >= 0 || a.cp.force_cfg >= 0) continue;
    for (size_t j = i + 1; j < n; ++j) {
      PlannedOp& b = e->ops[j];
      if (b.d.kind != kOpConv || b.fuse_role || b.dual_absorbed || b.dual_with >= 0 || b.cp.force_cfg >= 0) continue;
      const int kind = conv_dual_match(a.cp, b.cp);
      if (kind < 0) continue;
      op_regions(e, j, &rb, &wb);
      if (may_cross(e, i, j - 1, rb, wb)) {
        a.dual_with = (int)j;
        a.dual_kind = kind;
        b.dual_absorbed = true;
        absorb_info(&a.info, &b.info, "dual launch with", i);
        break;
      }
      // the other direction: the EARLIER op sinks to the later one's position (an INT8 engine's P3 output conv
      // waits for the P4 head's): nothing in between may read what it writes or write what it reads / writes
      const int kind2 = conv_dual_match(b.cp, a.cp);
      if (kind2 < 0) continue;
      op_regions(e, i, &ra, &wa);
      if (!may_cross(e, i + 1, j, ra, wa)) continue;
      b.dual_with = (int)i;
      b.dual_kind = kind2;
      a.dual_absorbed = true;
      absorb_info(&b.info, &a.info, "dual launch with", j);
      break;
    }
  }
}

enum LaunchForm { kNoLaunch, kLaunchConv, kLaunchConvDual, kLaunchStem, kLaunchPool, kLaunchQuant, kLaunchC3k2, kLaunchHead, kLaunchPair,
                  kLaunchBlockDual, kLaunchBad };
// The launch op i would make on its own.
LaunchForm own_form(const PlannedOp& op) {
  switch (op.d.kind) {
    case kOpConv: return kLaunchConv;
    case kOpStem: return kLaunchStem;
    case kOpSppfPool: return kLaunchPool;
    case kOpQuant: return kLaunchQuant;
    default: return kLaunchBad;
  }
}

// The launch of the fused group op i leads (fuse_role 1).
LaunchForm group_form(const PlannedOp& op) { return op.fuse_kind == 4 ? kLaunchPair : (op.fuse_kind == 2 ? kLaunchHead : kLaunchC3k2); }

// Which launch op i makes: its own, its fused group's, a dual launch it leads, or none (it runs inside another op's).
LaunchForm launch_form(const unina_engine* e, size_t i) {
  const PlannedOp& op = e->ops[i];
  if (op.dual_absorbed || (e->fuse && op.fuse_role == 2)) return kNoLaunch;
  if (e->fuse && op.fuse_role == 1) return op.dual_with >= 0 ? kLaunchBlockDual : group_form(op);
  return op.dual_with >= 0 ? kLaunchConvDual : own_form(op);
}

// One launch: its descriptor and the argument values it passes (copies of the planned parameters, finalised by the family's
// desc function). args points into the object itself, hence no copies.
struct OpLaunch {
  LaunchDesc d{};           // d.func == nullptr: nothing to launch
  int cfg = -1;             // kLaunchConv: the tile configuration
  ConvParams cp[2];         // conv (A, and B of a dual launch)
  C3k2Params fp;
  HeadParams hp;
  PairParams pr;
  StemParams sp;
  PoolParams pp;
  QuantParams qp;
  int split = 0;            // dual launches: the kernel's third argument
  void* args[3] = {};
  OpLaunch() = default;
  OpLaunch(const OpLaunch&) = delete;
};
constexpr auto kNoEdit = [](OpLaunch&) {};

// Fills `l` with op i's launch as `f` (launch_form, or a single conv / block for the autotuner and the debug entry points):
// copies the parameters, lets `edit` change them (a forced configuration, debug stamps), then builds the descriptor.
template <typename Edit = decltype(kNoEdit)>
hipError_t op_launch(const unina_engine* e, size_t i, LaunchForm f, OpLaunch* l, Edit edit = kNoEdit) {
  const PlannedOp& op = e->ops[i];
  switch (f) {
    case kNoLaunch: return hipSuccess;
    case kLaunchConv: l->cp[0] = op.cp; l->cfg = op.cfg; break;
    case kLaunchConvDual: l->cp[0] = op.cp; l->cp[1] = e->ops[op.dual_with].cp; break;
    case kLaunchStem: l->sp = op.sp; break;
    case kLaunchPool: l->pp = op.pp; break;
    case kLaunchQuant: l->qp = op.qp; break;
    case kLaunchC3k2: l->fp = op.fp; break;
    case kLaunchHead: l->hp = op.hp; break;
    case kLaunchPair: l->pr = op.pr; break;
    case kLaunchBlockDual: l->fp = op.fp; l->hp = e->ops[op.dual_with].hp; break;
    default: return hipErrorInvalidValue;
  }
  edit(*l);
  void** a = l->args;
  switch (f) {
    case kLaunchConv: a[0] = &l->cp[0]; return conv_desc(l->cp[0], l->cfg, &l->d);
    case kLaunchConvDual:
      a[0] = &l->cp[0]; a[1] = &l->cp[1]; a[2] = &l->split;
      return conv_dual_desc(op.dual_kind, l->cp[0], l->cp[1], &l->d, &l->split);
    case kLaunchStem: a[0] = &l->sp; return stem_desc(l->sp, &l->d);
    case kLaunchPool: a[0] = &l->pp; return sppf_pool_desc(l->pp, &l->d);
    case kLaunchQuant: a[0] = &l->qp; return quant_desc(l->qp, &l->d);
    case kLaunchC3k2: a[0] = &l->fp; return c3k2_desc(l->fp, &l->d);
    case kLaunchHead: a[0] = &l->hp; return head_desc(l->hp, &l->d);
    case kLaunchPair: a[0] = &l->pr; return pair_desc(l->pr, &l->d);
    default: a[0] = &l->fp; a[1] = &l->hp; a[2] = &l->split; return block_dual_desc(l->fp, l->hp, &l->d, &l->split);
  }
}

template <typename Edit = decltype(kNoEdit)>
hipError_t launch_op_as(const unina_engine* e, size_t i, hipStream_t s, LaunchForm f, Edit edit = kNoEdit) {
  OpLaunch l;
  const hipError_t err = op_launch(e, i, f, &l, edit);
  return err != hipSuccess || !l.d.func ? err : launch_desc(l.d, l.args, s);
}

// What differs from one frame call to the next besides the thresholds and the outputs. It travels by argument from the entry point
// to the launch; the engine and its plan hold nothing of it, before or after.
struct FrameCall {
  const CameraSource* region = nullptr;   // what the stems read; nullptr: the bound "images" tensor
  const unina_letterbox* lb = nullptr;    // the region letterboxed into the network input; nullptr: stretched
  float pad = 0.f;                        // letterbox: r = g = b outside the inner rectangle
  bool map_boxes = false;                 // letterbox: the post-process maps the kept records to camera pixels (PostParams::map_*)
  unsigned int* done_flag = nullptr;      // the last post-process block stores done_value there (infer_sync); nullptr: nothing is signalled
  unsigned int done_value = 0;
};

// The stem parameters of a call: the planned ones, reading the call's region as the kind it is for this stem's input size
StemParams call_stem(StemParams sp, const FrameCall& call) {
  if (const CameraSource* c = call.region)
    sp.cam = launch_source(*c, frame_kind(c->format, c->w, c->h, sp.W, sp.H, call.lb), sp.W, sp.H, call.lb, call.pad);
  return sp;
}

// Ops that read the caller's "images" tensor (the stem) stay OUTSIDE the captured graph: a camera pipeline hands
// over a different input buffer every frame, and re-binding must not cost a re-capture.
bool is_eager(const unina_engine* e, size_t i) { return (int)e->ops[i].d.src_buf == e->images_buf; }

// Op i as planned; in a frame call, an eager stem with the call's parameters
hipError_t launch_op(const unina_engine* e, size_t i, hipStream_t s, const FrameCall& call = {}) {
  const LaunchForm f = launch_form(e, i);
  const bool stem = f == kLaunchStem && is_eager(e, i);
  return launch_op_as(e, i, s, f, [&](OpLaunch& l) { if (stem) l.sp = call_stem(l.sp, call); });
}

// The op info's kernel, grid and block: those of op i's launch as `f`.
void launch_info(unina_engine* e, size_t i, LaunchForm f) {
  OpLaunch l;
  if (op_launch(e, i, f, &l) != hipSuccess || !l.d.func) return;
  unina_op_info& info = e->ops[i].info;
  snprintf(info.kernel, sizeof info.kernel, "%s", l.d.name);
  info.grid = (int)(l.d.grid.x * l.d.grid.y * l.d.grid.z);
  info.block = (int)l.d.block.x;
}

// Does op j launch in a frame whose post-process is `pp`? Not if it runs inside another op's launch, nor if the decode launch
// computes it (a head's output conv folded into the two-launch form; a dual launch only when both its convs are).
bool launches_in_frame(const unina_engine* e, size_t j, const PostParams& pp) {
  auto folded = [&](int k) {
    for (int h = 0; h < 3; ++h)
      if (pp.mode == kPostSplit && e->fold_op[h] == k && pp.h1[h] != nullptr) return true;
    return false;
  };
  const LaunchForm f = launch_form(e, j);
  return f != kNoLaunch && !(folded((int)j) && (f != kLaunchConvDual || folded(e->ops[j].dual_with)));
}

// (Re)computes kernel parameters from the current buffer addresses. Element types are properties of the BUFFERS
// (fp16 / fp32 / int8 NHWC): a conv runs in the type of its source buffer and converts to the type of each
// destination buffer in its epilogue, so fp16, fp32 and mixed int8/fp16 engines share one planner. Fused groups get the
// parameters of their one-launch form, and op infos describe what actually runs.
int plan(unina_engine* e) {
  for (size_t i = 0; i < e->ops.size(); ++i) {
    const int rc = plan_op(e, i);
    if (rc != UNINA_OK) return rc;
    launch_info(e, i, own_form(e->ops[i]));
  }
  for (size_t i = 0; i < e->ops.size(); ++i) {
    const PlannedOp& op = e->ops[i];
    if (op.fuse_role != 1) continue;
    const int rc = op.fuse_kind == 4 ? plan_pair(e, i) : (op.fuse_kind == 2 ? plan_head(e, i) : plan_c3k2(e, i));
    if (rc != UNINA_OK) return rc;
    if (e->fuse) launch_info(e, i, group_form(op));
  }
  plan_duals(e);
  find_fold_ops(e);
  for (size_t i = 0; i < e->ops.size(); ++i)   // what runs (an op a dual launch absorbs keeps its own block)
    if (launch_form(e, i) != kNoLaunch) launch_info(e, i, launch_form(e, i));
  e->plan_dirty = false;
  drop_graph(e);
  return UNINA_OK;
}

int launch_all(unina_engine* e, hipStream_t s, int which = 0 /*0 all, 1 eager only, 2 graph part only*/, const FrameCall& call = {}) {
  for (size_t i = 0; i < e->ops.size(); ++i) {
    if ((which == 1 && !is_eager(e, i)) || (which == 2 && is_eager(e, i))) continue;
    hipError_t err = launch_op(e, i, s, call);
    if (err != hipSuccess) return fail(e, UNINA_ERR_HIP, "op %zu (%s): %s", i, e->ops[i].d.name, hipGetErrorString(err));
  }
  return UNINA_OK;
}

// Captures the graph part of the forward as a plain chain on a stream that lives for the capture. (Independent branches as parallel graph
// paths -- heads | PAN path on side streams with event edges -- were implemented and measured in round 1: 1 821 / 2 503
// frames/s with 2 / 3 paths against 5 837 as a chain; removed.)
int capture(unina_engine* e) {
  drop_graph(e);
  CaptureStream cs;
  HIPCHK(e, cs.begin());
  int rc = UNINA_OK;
  for (size_t j = 0; j < e->ops.size() && rc == UNINA_OK; ++j) {
    if (is_eager(e, j)) continue;
    const hipError_t err = launch_op(e, j, cs.s);
    if (err != hipSuccess) rc = fail(e, UNINA_ERR_HIP, "op %zu (%s): %s", j, e->ops[j].d.name, hipGetErrorString(err));
  }
  const hipError_t end = cs.end(&e->graph);
  if (rc != UNINA_OK) return rc;
  if (end != hipSuccess) return fail(e, UNINA_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(end));
  HIPCHK(e, hipGraphInstantiate(&e->exec, e->graph, nullptr, nullptr, 0));
  return UNINA_OK;
}

// Before anything is launched: the engine's device current, something for the stems to read (the bound "images" tensor, unless the
// call brings a camera region) and the plan up to date
int make_ready(unina_engine* e, const FrameCall& call = {}) {
  HIPCHK(e, hipSetDevice(e->device));
  if (!call.region && !e->bufs[e->images_buf].ptr) return fail(e, UNINA_ERR_STATE, "tensor 'images' is not bound");
  bool stem = !call.region;
  for (size_t k = 0; k < e->ops.size() && !stem; ++k) stem = is_eager(e, k) && e->ops[k].d.kind == kOpStem;
  if (!stem) return fail(e, UNINA_ERR_STATE, "no stem op reads the input tensor");
  return e->plan_dirty ? plan(e) : UNINA_OK;
}

// The raw-head forward of a ready engine: the eager stems, then the captured graph of the rest (or every op, without graphs)
int enqueue_forward(unina_engine* e, const FrameCall& call, hipStream_t stream) {
  if (!e->use_graph) return launch_all(e, stream, 0, call);
  if (!e->exec) {
    int rc = capture(e);
    if (rc != UNINA_OK) return rc;
  }
  int rc = launch_all(e, stream, 1, call);
  if (rc != UNINA_OK) return rc;
  HIPCHK(e, hipGraphLaunch(e->exec, stream));
  return UNINA_OK;
}

// ---- fusable C3k2 groups (model.py:76-110) -------------------------------------------------------------------------
// The exporter lowers a C3k2 block to  [cv1|cv2 (1x1, two slices)] -> n x [b.cv1 (1x1), b.cv2 (3x3, +residual)] ->
// [cv3 (1x1 over the concat buffer)]. This recognises that shape in the op table (structurally: buffers, slices and
// residual wiring must match exactly, and no op outside the group may read the group's intermediates), packs the
// group's weights into the stage stream of c3k2_fused.hip and appends it to the (host copy of the) blob.
bool is_plain_conv(const OpDesc& d, uint32_t k, uint32_t nseg, bool int8 = false) {
  if (d.kind != kOpConv || d.ksize != k || d.stride != 1 || !d.relu || d.nseg != nseg) return false;
  for (uint32_t s = 0; s < nseg; ++s)
    if (d.seg[s].flags || (d.seg[s].m_off != 0) != int8 || d.seg[s].n_pad != d.seg[s].n_count) return false;
  return true;
}

// Conv op `o` as one step of a packed block stream: `padded` counts the stored rows (n_pad) instead of the live ones,
// `i8` adds the int8 multipliers and output scales.
C3k2Conv pack_conv(const unina_engine* e, const std::vector<char>& blob, const OpDesc& o, bool padded, bool i8) {
  C3k2Conv cv;
  memset(&cv, 0, sizeof cv);
  for (uint32_t s = 0; s < o.nseg; ++s) {
    const SegDesc& sg = o.seg[s];
    cv.w[s] = reinterpret_cast<const unsigned char*>(blob.data() + sg.w_off);
    cv.bias[s] = reinterpret_cast<const float*>(blob.data() + sg.b_off);
    cv.n[s] = (int)(padded ? sg.n_pad : sg.n_count);
    if (i8) {
      cv.mult[s] = reinterpret_cast<const float*>(blob.data() + sg.m_off);
      cv.out_inv[s] = 1.0f / e->bufs[sg.dst_buf].d.scale;   // as plan() computes ConvSeg::out_inv_scale
    }
  }
  cv.K = (int)(o.ksize * o.ksize * o.cin);
  return cv;
}

// Appends `bytes` bytes at the blob's next 256-byte boundary; returns their offset.
uint64_t append_aligned(std::vector<char>* blob, const void* p, size_t bytes) {
  blob->resize((blob->size() + 255) & ~(size_t)255);
  const uint64_t off = blob->size();
  blob->insert(blob->end(), static_cast<const char*>(p), static_cast<const char*>(p) + bytes);
  return off;
}

// A fused group's packed weight stream and biases, appended to the blob for the group's first op.
void append_stream(std::vector<char>* blob, const std::vector<unsigned char>& stream, const std::vector<float>& bias, PlannedOp* head) {
  head->stream_off = append_aligned(blob, stream.data(), stream.size());
  head->fbias_off = append_aligned(blob, bias.data(), bias.size() * sizeof(float));
}

void find_c3k2_groups(unina_engine* e, std::vector<char>* blob) {
  const size_t n = e->ops.size();
  for (size_t i = 0; i + 3 < n; ++i) {
    const OpDesc& a = e->ops[i].d;
    // fp16 block, or (INT8 engines) a block whose input, output and intermediates are all int8 code tensors
    const uint32_t bdt = e->bufs[a.src_buf].d.dtype;
    if (bdt != kBufF16Nhwc && bdt != kBufI8Nhwc && bdt != kBufS16Nhwc) continue;
    const bool i8 = bdt == kBufI8Nhwc;
    const int dt = i8 ? kI8 : (bdt == kBufS16Nhwc ? kS16 : kF16);
    const uint32_t al = i8 ? 16 : 8;   // channels per 16-byte chunk
    if (!is_plain_conv(a, 1, 2, i8) || a.res_buf >= 0) continue;
    const uint32_t h = a.seg[0].n_count;
    if (a.seg[1].n_count != h || a.seg[0].src_coff != a.seg[1].src_coff) continue;
    if (a.seg[0].src_coff % al || e->bufs[a.src_buf].d.c % al) continue;
    // bottlenecks
    uint32_t cur_buf = a.seg[0].dst_buf, cur_coff = a.seg[0].dst_coff;
    size_t j = i + 1;
    int nb = 0;
    std::vector<uint32_t> inter = {a.seg[0].dst_buf, a.seg[1].dst_buf};
    while (j + 1 < n && nb < 2) {
      const OpDesc& c1 = e->ops[j].d;
      const OpDesc& c2 = e->ops[j + 1].d;
      if (!is_plain_conv(c1, 1, 1, i8) || !is_plain_conv(c2, 3, 1, i8)) break;
      if (c1.res_buf >= 0 || c1.cin != h || c1.seg[0].n_count != h || c1.src_buf != cur_buf || c1.seg[0].src_coff != cur_coff) break;
      if (c2.cin != h || c2.seg[0].n_count != h || c2.src_buf != c1.seg[0].dst_buf || c2.seg[0].src_coff != c1.seg[0].dst_coff) break;
      if (c2.res_buf != (int)cur_buf || c2.res_coff != (int)cur_coff) break;
      inter.push_back(c1.seg[0].dst_buf);
      inter.push_back(c2.seg[0].dst_buf);
      cur_buf = c2.seg[0].dst_buf;
      cur_coff = c2.seg[0].dst_coff;
      j += 2;
      ++nb;
    }
    if (nb < 1 || j >= n) continue;
    const OpDesc& z = e->ops[j].d;  // cv3 over [last bottleneck | cv2]
    if (!is_plain_conv(z, 1, 1, i8) || z.res_buf >= 0 || z.cin != 2 * h || z.seg[0].n_count != 2 * h) continue;
    if (z.src_buf != cur_buf || z.src_buf != a.seg[1].dst_buf || cur_coff != z.seg[0].src_coff || a.seg[1].dst_coff != cur_coff + h) continue;
    if (e->bufs[z.seg[0].dst_buf].d.dtype != bdt || z.seg[0].dst_coff % al || e->bufs[z.seg[0].dst_buf].d.c % al) continue;
    if (a.in_h != z.out_h || a.in_w != z.out_w) continue;
    if (!c3k2_supported((int)h, nb, (int)a.cin, 0, dt)) continue;
    // A 1x1 ConvBlock 2h -> h on cv3's output that becomes the block kernel's last step (tail kind 1-3), with the slice
    // flags, int8 multipliers and destination type that tail kind takes.
    auto is_tail = [&](const OpDesc& t, uint32_t flags, bool mult, uint32_t dst_dtype, int kind) {
      const SegDesc& ts = t.seg[0];
      const BufferDesc& tb = e->bufs[ts.dst_buf].d;
      const uint32_t tal = dst_dtype == kBufI8Nhwc ? 16 : 8;
      return t.kind == kOpConv && t.ksize == 1 && t.stride == 1 && t.relu && t.nseg == 1 && t.res_buf < 0 && ts.flags == flags &&
             (ts.m_off != 0) == mult && ts.n_pad == ts.n_count && t.cin == 2 * h && ts.n_count == h && t.src_buf == z.seg[0].dst_buf &&
             ts.src_coff == z.seg[0].dst_coff && tb.dtype == dst_dtype && ts.dst_coff % tal == 0 && tb.c % tal == 0 &&
             ts.dst_buf != z.seg[0].dst_buf && t.in_h == z.out_h && t.in_w == z.out_w && c3k2_supported((int)h, nb, (int)a.cin, kind, dt);
    };
    int tail_kind = 0;
    if (j + 1 < n) {
      const OpDesc& t = e->ops[j + 1].d;
      // 1: an FPN block's lateral conv (model.py:256,259: ConvBlock 1x1, 2h -> h) whose store does the nearest x2 upsample
      if (!i8 && is_tail(t, kSegUp2, false, bdt, 1)) tail_kind = 1;
      // 2: a plain 1x1 ConvBlock on the block's output (stage3_c3k2 -> sppf.cv1, model.py:215-216), fp16 or int8
      else if (is_tail(t, 0, i8, bdt, 2)) tail_kind = 2;
      // 3 (INT8 engines): an int8 FPN block whose lateral (int8 conv) writes the fp16 concat buffer of a narrow fp16 block
      else if (i8 && is_tail(t, kSegUp2, true, kBufF16Nhwc, 3)) tail_kind = 3;
    }
    const size_t jt = tail_kind ? j + 1 : j;   // last op of the group incl. the tail
    // INT8 engines: an fp16 block whose output gets an int8 twin from the QUANT op that follows (mixed readers)
    int quant_op = -1;
    if (!i8 && dt == kF16 && jt + 1 < n) {
      const OpDesc& qd = e->ops[jt + 1].d;
      if (qd.kind == kOpQuant && qd.src_buf == z.seg[0].dst_buf && z.seg[0].dst_coff == 0 && e->bufs[z.seg[0].dst_buf].d.c == 2 * h &&
          qd.nseg == 1 && qd.seg[0].dst_coff == 0 && e->bufs[qd.seg[0].dst_buf].d.dtype == kBufI8Nhwc &&
          e->bufs[qd.seg[0].dst_buf].d.c == 2 * h && !e->ops[jt + 1].fuse_role)
        quant_op = (int)(jt + 1);
    }
    // the 3x3 / stride-2 ConvBlock that produces the block's input (stage1_conv -> stage1_block) as a first step, when the
    // block is its only reader (the input tensor then never exists in HBM) and a class exists
    size_t i0 = i;   // first op of the group
    if (i > 0 && !e->ops[i - 1].fuse_role) {
      const OpDesc& pz = e->ops[i - 1].d;
      const uint32_t cx = pz.seg[0].n_count;   // the pre-conv writes the FIRST cx channels of the block's input (all of it, or
                                               // the down-sampling half of a PAN concat)
      const bool ok = pz.kind == kOpConv && pz.ksize == 3 && pz.stride == 2 && pz.relu && pz.nseg == 1 && pz.res_buf < 0 && !pz.seg[0].flags &&
                      (pz.seg[0].m_off != 0) == i8 && pz.seg[0].n_pad == pz.seg[0].n_count && pz.seg[0].dst_buf == a.src_buf &&
                      pz.seg[0].dst_coff == a.seg[0].src_coff && cx <= a.cin && cx % al == 0 &&
                      e->bufs[pz.src_buf].d.dtype == bdt && pz.seg[0].src_coff % al == 0 && e->bufs[pz.src_buf].d.c % al == 0 &&
                      pz.out_h == a.in_h && pz.out_w == a.in_w && pz.src_buf != a.src_buf &&
                      c3k2_supported((int)h, nb, (int)a.cin, tail_kind, dt, (int)pz.cin, (int)cx) &&
                      !(e->bufs[a.src_buf].d.flags & (kBufInput | kBufOutput)) &&
                      // its output must be private to the group: nothing else reads or writes those channels
                      !touched_outside(e, Region{(int)a.src_buf, (int)pz.seg[0].dst_coff, (int)(pz.seg[0].dst_coff + cx)}, i - 1, j);
      if (ok) i0 = i - 1;
    }
    const OpDesc& first = e->ops[i0].d;
    // the group's intermediates must be private to it, and must not be its own input or output
    bool priv = true;
    for (uint32_t b : inter)
      priv = priv && e->bufs[b].d.dtype == bdt &&   // (an INT8 engine's fp16 conv may still write an int8 buffer)
             b != first.src_buf && b != z.seg[0].dst_buf && !(e->bufs[b].d.flags & (kBufInput | kBufOutput)) &&
             !touched_outside(e, whole((int)b), i0, j);
    if (!priv) continue;
    // pack
    std::vector<C3k2Conv> convs;
    for (size_t k = i0; k <= jt; ++k) convs.push_back(pack_conv(e, *blob, e->ops[k].d, false, i8));
    std::vector<unsigned char> stream;
    std::vector<float> bias;
    if (!c3k2_pack((int)h, nb, (int)a.cin, tail_kind, convs.data(), &stream, &bias, dt, i0 < i ? (int)first.cin : 0,
                   i0 < i ? (int)first.seg[0].n_count : 0)) continue;
    PlannedOp& head = e->ops[i0];
    append_stream(blob, stream, bias, &head);
    head.fuse_role = 1;
    head.fuse_kind = 1;
    head.fuse_pre = i0 < i ? 1 : 0;
    head.group_last = (int)j;
    head.hid = (int)h;
    head.nb = nb;
    head.tail_op = jt > j ? (int)jt : -1;
    head.tail_kind = tail_kind;
    head.quant_op = quant_op;
    if (quant_op >= 0) e->ops[quant_op].fuse_role = 2;
    for (size_t k = i0 + 1; k <= jt; ++k) e->ops[k].fuse_role = 2;
    ++e->n_groups;
    i = jt;
  }
}

// Two consecutive 1x1 ConvBlocks outside any block group (sppf.cv2 -> lateral_p3, whose store does the x2 upsample):
// one launch when conv_pair.hip has a class for the channel counts. fp16 or all-int8.
void find_pair_groups(unina_engine* e, std::vector<char>* blob) {
  const size_t n = e->ops.size();
  for (size_t i = 0; i + 1 < n; ++i) {
    if (e->ops[i].fuse_role || e->ops[i + 1].fuse_role) continue;
    const OpDesc& a = e->ops[i].d;
    const OpDesc& z = e->ops[i + 1].d;
    if (a.kind != kOpConv || z.kind != kOpConv) continue;
    // SPPF: the pool op right in front (x -> [p1 | p2 | p3] next to x in the same buffer) whose 4-way concat `a` reads can
    // run inside the pair's launch when nothing else reads the pooled maps
    int pool = 0;
    if (i > 0 && !e->ops[i - 1].fuse_role && e->ops[i - 1].d.kind == kOpSppfPool) {
      const OpDesc& pl = e->ops[i - 1].d;
      const Region pooled{(int)pl.src_buf, (int)(pl.seg[0].src_coff + pl.cin), (int)(pl.seg[0].src_coff + 4 * pl.cin)};
      if (pl.src_buf == a.src_buf && pl.seg[0].src_coff == a.seg[0].src_coff && a.cin == 4 * pl.cin && !touched_outside(e, pooled, i - 1, i))
        pool = 1;
    }
    const uint32_t bdt = e->bufs[a.src_buf].d.dtype;
    if (bdt != kBufF16Nhwc && bdt != kBufI8Nhwc && bdt != kBufS16Nhwc) continue;
    const bool i8 = bdt == kBufI8Nhwc;
    const uint32_t al = i8 ? 16 : 8;
    if (!is_plain_conv(a, 1, 1, i8) || a.res_buf >= 0) continue;
    if (z.ksize != 1 || z.stride != 1 || !z.relu || z.nseg != 1 || z.res_buf >= 0 || (z.seg[0].flags & ~(uint32_t)kSegUp2) ||
        (z.seg[0].m_off != 0) != i8 || z.seg[0].n_pad != z.seg[0].n_count) continue;
    if (z.src_buf != a.seg[0].dst_buf || z.seg[0].src_coff != a.seg[0].dst_coff || z.cin != a.seg[0].n_count) continue;
    if (e->bufs[a.seg[0].dst_buf].d.dtype != bdt || e->bufs[z.seg[0].dst_buf].d.dtype != bdt) continue;
    if (a.seg[0].src_coff % al || e->bufs[a.src_buf].d.c % al || a.seg[0].dst_coff % al || e->bufs[a.seg[0].dst_buf].d.c % al ||
        z.seg[0].dst_coff % al || e->bufs[z.seg[0].dst_buf].d.c % al) continue;
    if (z.seg[0].dst_buf == a.seg[0].dst_buf || z.seg[0].dst_buf == a.src_buf || a.seg[0].dst_buf == a.src_buf) continue;
    const int dt = i8 ? kI8 : (bdt == kBufS16Nhwc ? kS16 : kF16), up2 = (z.seg[0].flags & kSegUp2) ? 1 : 0;
    if (pool && !pair_supported(dt, (int)a.cin, (int)a.seg[0].n_count, (int)z.seg[0].n_count, up2, 1)) pool = 0;
    if (!pair_supported(dt, (int)a.cin, (int)a.seg[0].n_count, (int)z.seg[0].n_count, up2, pool)) continue;
    const C3k2Conv cv[2] = {pack_conv(e, *blob, a, false, i8), pack_conv(e, *blob, z, false, i8)};
    std::vector<unsigned char> stream;
    std::vector<float> bias;
    block_pack(cv, 2, &stream, &bias, dt);
    PlannedOp& head = e->ops[i - pool];
    append_stream(blob, stream, bias, &head);
    head.fuse_role = 1;
    head.fuse_kind = 4;
    head.fuse_pre = pool;            // 1: this op is the SPPF pool, the conv pair are the next two ops
    head.group_last = (int)(i + 1);
    if (pool) e->ops[i].fuse_role = 2;
    e->ops[i + 1].fuse_role = 2;
    ++e->n_groups;
    ++i;
  }
}

// A DetectionHead (model.py:274-303) in the exporter's table: [cls.0|reg.0 3x3, same input, two slices of h0] ->
// [cls.1|reg.1 3x3, slice i reads h0's slice i, writes h1's slice i] -> [cls.2|reg.2 1x1 without ReLU into the two
// fp32 planar outputs]. Fused when the channel width has a head_fused.hip class and h0 / h1 are private.
void find_head_groups(unina_engine* e, std::vector<char>* blob) {
  const size_t n = e->ops.size();
  for (size_t i = 0; i + 2 < n; ++i) {
    const OpDesc& a = e->ops[i].d;
    const OpDesc& b = e->ops[i + 1].d;
    const OpDesc& c = e->ops[i + 2].d;
    if (e->ops[i].fuse_role || e->ops[i + 1].fuse_role || e->ops[i + 2].fuse_role) continue;
    if (!is_plain_conv(a, 3, 2) || !is_plain_conv(b, 3, 2) || a.res_buf >= 0 || b.res_buf >= 0) continue;
    const uint32_t C = a.cin;
    if (a.seg[0].n_count != C || a.seg[1].n_count != C || a.seg[0].src_coff != a.seg[1].src_coff) continue;
    const uint32_t h0 = a.seg[0].dst_buf;
    if (a.seg[1].dst_buf != h0 || a.seg[0].dst_coff != 0 || a.seg[1].dst_coff != C || e->bufs[h0].d.c != 2 * C) continue;
    if (b.cin != C || b.src_buf != h0 || b.seg[0].src_coff != 0 || b.seg[1].src_coff != C || b.seg[0].n_count != C || b.seg[1].n_count != C) continue;
    const uint32_t h1 = b.seg[0].dst_buf;
    if (b.seg[1].dst_buf != h1 || b.seg[0].dst_coff != 0 || b.seg[1].dst_coff != C || e->bufs[h1].d.c != 2 * C || h1 == h0) continue;
    if (c.kind != kOpConv || c.ksize != 1 || c.stride != 1 || c.relu || c.nseg != 2 || c.res_buf >= 0 || c.cin != C || c.src_buf != h1) continue;
    if (c.seg[0].src_coff != 0 || c.seg[1].src_coff != C) continue;
    bool ok = true;
    for (int s = 0; s < 2; ++s)
      ok = ok && (c.seg[s].flags == kSegPlanarF32) && !c.seg[s].m_off && c.seg[s].n_pad == 16 && c.seg[s].n_count <= 16 &&
           c.seg[s].dst_coff == 0 && e->bufs[c.seg[s].dst_buf].d.dtype == kBufF32Planar;
    if (!ok || e->bufs[a.src_buf].d.dtype != kBufF16Nhwc || !head_supported((int)C)) continue;
    if (a.in_h != c.out_h || a.in_w != c.out_w) continue;
    for (uint32_t hb : {h0, h1})
      ok = ok && e->bufs[hb].d.dtype == kBufF16Nhwc && hb != a.src_buf && !(e->bufs[hb].d.flags & (kBufInput | kBufOutput)) &&
           !touched_outside(e, whole((int)hb), i, i + 2);
    if (!ok) continue;
    const C3k2Conv convs[3] = {pack_conv(e, *blob, a, true, false), pack_conv(e, *blob, b, true, false), pack_conv(e, *blob, c, true, false)};
    std::vector<unsigned char> stream;
    std::vector<float> bias;
    block_pack(convs, 3, &stream, &bias);
    PlannedOp& head = e->ops[i];
    append_stream(blob, stream, bias, &head);
    head.fuse_role = 1;
    head.fuse_kind = 2;
    head.group_last = (int)i + 2;
    head.hid = (int)C;
    e->ops[i + 1].fuse_role = e->ops[i + 2].fuse_role = 2;
    ++e->n_groups;
    i += 2;
  }
}

// ---- full-frame graph ------------------------------------------------------------------------------------------------
hipError_t last_captured_node(hipStream_t st, hipGraphNode_t* node) {
  hipStreamCaptureStatus status;
  unsigned long long id = 0;
  hipGraph_t g = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t ndeps = 0;
  hipError_t err = hipStreamGetCaptureInfo_v2(st, &status, &id, &g, &deps, &ndeps);
  if (err != hipSuccess) return err;
  if (status != hipStreamCaptureStatusActive || ndeps != 1) return hipErrorInvalidValue;
  *node = deps[0];
  return hipSuccess;
}

int capture_full(unina_engine* e, const FrameCall& call, const PostParams& pp) {
  if (e->fexec) (void)hipGraphExecDestroy(e->fexec);
  if (e->fgraph) (void)hipGraphDestroy(e->fgraph);
  e->fexec = nullptr;
  e->fgraph = nullptr;
  e->stem_node = e->post_node = e->post_node2 = nullptr;
  e->stem_op = -1;
  CaptureStream cs;
  HIPCHK(e, cs.begin());
  hipStream_t st = cs.s;
  hipError_t err = hipSuccess;
  int rc = UNINA_OK;
  for (size_t j = 0; j < e->ops.size() && err == hipSuccess; ++j) {
    if (!launches_in_frame(e, j, pp)) continue;
    err = launch_op(e, j, st, call);
    if (err != hipSuccess) {
      rc = fail(e, UNINA_ERR_HIP, "op %zu (%s): %s", j, e->ops[j].d.name, hipGetErrorString(err));
      break;
    }
    if (is_eager(e, j) && e->ops[j].d.kind == kOpStem && e->stem_op < 0) {
      err = last_captured_node(st, &e->stem_node);
      e->stem_op = (int)j;
    }
  }
  LaunchDesc pd[2];
  const int npost = postprocess_desc(pp, pd);
  if (npost < 1) err = hipErrorInvalidValue;
  for (int k = 0; k < npost && err == hipSuccess; ++k) {
    PostParams copy = pp;
    void* args[] = {&copy};
    err = launch_desc(pd[k], args, st);
    if (err == hipSuccess) err = last_captured_node(st, k == 0 ? &e->post_node : &e->post_node2);
  }
  hipError_t end = cs.end(&e->fgraph);
  if (rc != UNINA_OK) return rc;
  if (err != hipSuccess) return fail(e, UNINA_ERR_HIP, "full-frame graph capture: %s", hipGetErrorString(err));
  if (end != hipSuccess) return fail(e, UNINA_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(end));
  if (e->stem_op < 0 || !e->stem_node || !e->post_node) return fail(e, UNINA_ERR_STATE, "full-frame graph: stem / post-process node not found");
  HIPCHK(e, hipGraphInstantiate(&e->fexec, e->fgraph, nullptr, nullptr, 0));
  e->f_stem = call_stem(e->ops[e->stem_op].sp, call);
  e->f_post = pp;
  return UNINA_OK;
}

template <typename P>
hipError_t set_node(hipGraphExec_t exec, hipGraphNode_t node, const LaunchDesc& d, const P& params) {
  P copy = params;
  void* args[] = {&copy};
  hipKernelNodeParams np;
  memset(&np, 0, sizeof np);
  np.func = const_cast<void*>(d.func);
  np.gridDim = d.grid;
  np.blockDim = d.block;
  np.sharedMemBytes = d.shmem;
  np.kernelParams = args;
  return hipGraphExecKernelNodeSetParams(exec, node, &np);
}

// One graph launch for the whole frame; re-points the stem / post-process nodes when this call's parameters differ from the last
// ones launched.
int launch_full(unina_engine* e, const FrameCall& call, const PostParams& pp, hipStream_t stream) {
  if (!e->fexec) {
    int rc = capture_full(e, call, pp);
    if (rc != UNINA_OK) return rc;
  } else {
    const StemParams sp = call_stem(e->ops[e->stem_op].sp, call);
    if (memcmp(&sp, &e->f_stem, sizeof sp)) {
      LaunchDesc d;
      HIPCHK(e, stem_desc(sp, &d));
      HIPCHK(e, set_node(e->fexec, e->stem_node, d, sp));
      e->f_stem = sp;
    }
    if (memcmp(&pp, &e->f_post, sizeof pp)) {
      LaunchDesc d[2];
      const int npost = postprocess_desc(pp, d);
      if (npost < 1 || (npost == 2) != (e->post_node2 != nullptr)) return fail(e, UNINA_ERR_STATE, "post-process launch shape changed");
      HIPCHK(e, set_node(e->fexec, e->post_node, d[0], pp));
      if (npost == 2) HIPCHK(e, set_node(e->fexec, e->post_node2, d[1], pp));
      e->f_post = pp;
    }
  }
  HIPCHK(e, hipGraphLaunch(e->fexec, stream));
  return UNINA_OK;
}

// Mean duration of op `i` measured INSIDE the frame sequence: every repetition replays ops 0..i-1 first, so the op
// finds the caches as it does in a real frame (weights cold in L2, inputs just written). Timing back-to-back repeats
// of one launch instead keeps its weights L2-resident and ranks weight-heavy configurations wrongly (measured: a
// configuration that re-reads 2.4 MB of weights from 25 workgroup columns won the warm timing at 13.4 us and ran
// 20.8 us in the frame). `launch` issues op i (so that the autotuner can substitute a candidate configuration).
template <typename F>
int time_in_sequence(unina_engine* e, size_t i, int iters, hipStream_t stream, hipEvent_t a, hipEvent_t b, F launch, float* ms_out) {
  float total = 0.f;
  for (int it = 0; it < iters; ++it) {
    for (size_t k = 0; k < i; ++k) {
      hipError_t err = launch_op(e, k, stream);
      if (err != hipSuccess) return fail(e, UNINA_ERR_HIP, "op %zu (%s): %s", k, e->ops[k].d.name, hipGetErrorString(err));
    }
    HIPCHK(e, hipEventRecord(a, stream));
    HIPCHK(e, launch());
    HIPCHK(e, hipEventRecord(b, stream));
    HIPCHK(e, hipEventSynchronize(b));
    float ms = 0.f;
    HIPCHK(e, hipEventElapsedTime(&ms, a, b));
    total += ms;
  }
  *ms_out = total / (float)iters;
  return UNINA_OK;
}

int find_buffer(const unina_engine* e, const char* name) {
  for (size_t i = 0; i < e->bufs.size(); ++i)
    if (!strncmp(e->bufs[i].d.name, name, sizeof e->bufs[i].d.name)) return (int)i;
  return -1;
}

float half_bits_to_float(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000) << 16;
  uint32_t exp = (h >> 10) & 0x1F, man = h & 0x3FF, bits;
  if (exp == 0) {
    if (man == 0) bits = sign;
    else {
      int sh = 0;
      while (!(man & 0x400)) { man <<= 1; ++sh; }
      man &= 0x3FF;
      bits = sign | ((uint32_t)(127 - 15 - sh + 1) << 23) | (man << 13);
    }
  } else if (exp == 31) bits = sign | 0x7F800000u | (man << 13);
  else bits = sign | ((exp + 112) << 23) | (man << 13);
  float f;
  memcpy(&f, &bits, 4);
  return f;
}

int fill_post_params(unina_engine* e, PostParams* pp, const FrameCall& call, float conf, float iou, float q, GpuDetection* d_out,
                     int* d_count, int* d_cand_count, bool fold = false) {
  memset(pp, 0, sizeof *pp);
  for (int i = 0; i < 3; ++i) {
    const Buffer& c = e->bufs[e->out_buf[2 * i]];
    const Buffer& r = e->bufs[e->out_buf[2 * i + 1]];
    pp->cls[i] = static_cast<const float*>(c.ptr);
    pp->reg[i] = static_cast<const float*>(r.ptr);
    pp->gw[i] = (int)c.d.w;
    pp->gh[i] = (int)c.d.h;
    pp->stride[i] = (int)e->h.strides[i];
  }
  pp->num_classes = (int)e->h.num_classes;
  pp->conf_thr = conf;
  pp->iou_thr = iou;
  pp->conformal_q = q;
  pp->cand = e->d_cand;
  pp->block_count = e->d_block_count;
  pp->ticket = e->d_ticket;
  pp->mode = e->post_split ? kPostSplit : kPostOneLaunch;
  if (pp->mode == kPostSplit) {
    post_bind_workspace(pp, e->d_post_ws, e->d_cand);
    for (int h = 0; h < 3 && fold; ++h) {
      if (e->fold_op[h] < 0) continue;
      const ConvParams& c = e->ops[e->fold_op[h]].cp;
      pp->h1[h] = c.src;
      pp->h1_lo[h] = c.dtype == kS16 ? c.src_lo : 0;
      pp->h1_ld[h] = c.src_ld;
      pp->h1_c[h] = c.Cin;
      for (int k = 0; k < 2; ++k) {
        pp->h1_coff[h][k] = c.seg[k].src_coff;
        pp->w2[h][k] = static_cast<const unsigned char*>(c.seg[k].w_lane);
        pp->b2[h][k] = c.seg[k].bias;
      }
    }
    if (!post_plan_blocks(pp)) {     // does not fit the block table: everything in one launch
      pp->mode = kPostOneLaunch;
      pp->ws_box = nullptr;
      for (int h = 0; h < 3; ++h) pp->h1[h] = nullptr;
    }
  }
  pp->out = d_out;
  pp->out_count = d_count;
  pp->out_candidates = d_cand_count;
  pp->stamps = getenv("UNINA_POST_STAMPS") ? reinterpret_cast<long long*>(e->d_result->pad_stamps) : nullptr;
  pp->done_flag = call.done_flag;
  pp->done_value = call.done_value;
  if (call.map_boxes && call.lb) {
    pp->map_boxes = 1;
    pp->map_left = (float)call.lb->left;
    pp->map_top = (float)call.lb->top;
    pp->map_sx = (float)call.region->w / (float)call.lb->new_w;
    pp->map_sy = (float)call.region->h / (float)call.lb->new_h;
  }
  return UNINA_OK;
}

// One frame: forward + post-process into d_out / d_count, as one launch of the full-frame graph or as the raw-head forward and the
// post-process behind it. The body of every inference entry point; `call` says what this frame reads and whom it signals.
int enqueue_frame(unina_engine* e, const FrameCall& call, float conf, float iou, float q, GpuDetection* d_out, int* d_count,
                  hipStream_t stream) {
  if (!d_out || !d_count) return UNINA_ERR_ARG;
  int rc = make_ready(e, call);
  if (rc != UNINA_OK) return rc;
  const bool full = e->full_graph && e->use_graph;
  PostParams pp;
  fill_post_params(e, &pp, call, conf, iou, q, d_out, d_count, &e->d_result->candidates, /*fold=*/full);
  if (full) return launch_full(e, call, pp, stream);
  rc = enqueue_forward(e, call, stream);
  if (rc != UNINA_OK) return rc;
  HIPCHK(e, postprocess_launch(pp, stream));
  return UNINA_OK;
}

// Bytes of a conv slice's weight blocks in the blob (engine_validate.h: validate_engine has held them inside the blob).
uint64_t weight_bytes(const unina_engine* e, const OpDesc& d, const SegDesc& sd) { return conv_weight_bytes(d, sd, e->bufs[d.src_buf].d.dtype); }

// Host side of loading an engine file: reads and validates it, appends the lane-order weight twins, the stem transpose and
// the fused groups' streams to `blob` and sets e->fuse. No device is touched (unina_debug_fusable_groups runs exactly this).
// On error: the code, with the message in g_load_error.
int load_host(const char* path, unina_engine* e, std::vector<char>* blob_out) {
  FILE* f = fopen(path, "rb");
  if (!f) return fail(nullptr, UNINA_ERR_IO, "cannot open %s", path);
  auto bail = [&](int code, const char* msg) {
    g_load_error = msg;
    if (f) fclose(f);
    return code;
  };
  auto refused = [&](const Verdict& v) { return bail(v.code, v.msg); };
  std::vector<char>& blob = *blob_out;
  // Every check that depends on the file alone is validate_engine's (engine_validate.h). Above that call nothing is allocated
  // from a field of the file but the two tables, which read_engine_tables sizes after it has capped their lengths, and
  // nothing is indexed or dereferenced through one.
  EngineTables t;
  Verdict v = read_engine_tables([&](void* dst, size_t bytes) { return bytes == 0 || fread(dst, bytes, 1, f) == 1; }, &t);
  if (!v.ok()) return refused(v);
  const long tables_end = ftell(f);
  if (tables_end < 0 || fseek(f, 0, SEEK_END)) return bail(UNINA_ERR_IO, "cannot seek in the engine file");
  const long file_end = ftell(f);
  if (file_end < tables_end || fseek(f, tables_end, SEEK_SET)) return bail(UNINA_ERR_IO, "cannot seek in the engine file");
  v = validate_engine(t.h, t.bufs.data(), t.ops.data(), (uint64_t)(file_end - tables_end));
  if (!v.ok()) return refused(v);
  e->h = t.h;
  e->bufs.resize(t.bufs.size());
  for (size_t i = 0; i < t.bufs.size(); ++i) e->bufs[i].d = t.bufs[i];
  e->ops.resize(t.ops.size());
  for (size_t i = 0; i < t.ops.size(); ++i) {
    e->ops[i].d = t.ops[i];
    e->ops[i].d.name[sizeof e->ops[i].d.name - 1] = 0;
  }
  blob.resize(e->h.blob_bytes);   // (no more than the file holds: validate_engine)
  if (e->h.blob_bytes && fread(blob.data(), 1, blob.size(), f) != blob.size()) return bail(UNINA_ERR_IO, "cannot read the weight blob");
  fclose(f);
  f = nullptr;

  for (size_t i = 0; i < e->bufs.size(); ++i) {
    e->bufs[i].bytes = buffer_bytes(e->bufs[i].d);
    if (e->bufs[i].d.flags & kBufInput) e->images_buf = (int)i;
  }
  for (int i = 0; i < 6; ++i) e->out_buf[i] = find_buffer(e, kHeadOutputs[i]);
  for (size_t i = 0; i < e->ops.size(); ++i)   // graph (A)'s P4 before SPPF: what the mining path pools (unina_mine*)
    if (e->ops[i].d.kind == kOpConv && e->ops[i].d.nseg == 1 && !strcmp(e->ops[i].d.name, "backbone.stage3_c3k2.cv3")) e->embed_op = (int)i;

  // convs: a LANE-order twin of every slice's weight blocks (kernels.h weight_block_to_lane_order) for the kernels that take
  // weights straight into registers (conv3x3_regq / conv3x3_ws / the decode launch's output convs); the file's order stays
  // what the LDS-DMA kernels copy into LDS
  for (auto& op : e->ops) {
    if (op.d.kind != kOpConv) continue;
    for (uint32_t s = 0; s < op.d.nseg; ++s) {
      const SegDesc& sd = op.d.seg[s];
      const uint64_t wbytes = weight_bytes(e, op.d, sd);
      if (wbytes == 0 || wbytes % 1024) continue;
      blob.resize((blob.size() + 255) & ~(size_t)255);
      op.w_lane_off[s] = blob.size();
      blob.resize(blob.size() + wbytes);
      for (uint64_t b = 0; b < wbytes; b += 1024)
        weight_block_to_lane_order(reinterpret_cast<const unsigned char*>(blob.data()) + sd.w_off + b,
                                   reinterpret_cast<unsigned char*>(blob.data()) + op.w_lane_off[s] + b);
    }
  }

  // stem: a [27][Co] transposed copy of its weights (wave-uniform scalar loads in stem_conv_kernel)
  for (auto& op : e->ops) {
    if (op.d.kind != kOpStem) continue;
    const SegDesc& sd = op.d.seg[0];
    const uint32_t co = sd.n_count;
    std::vector<float> wt((size_t)27 * co);
    const float* w = reinterpret_cast<const float*>(blob.data() + sd.w_off);
    for (uint32_t c = 0; c < co; ++c)
      for (int k = 0; k < 27; ++k) wt[(size_t)k * co + c] = w[(size_t)c * 27 + k];
    op.wt_off = append_aligned(&blob, wt.data(), wt.size() * sizeof(float));
  }
  // fusable groups: their packed weight streams are appended to the blob before upload. The matchers accept all-fp16
  // groups (in an INT8 engine: the carved-out P2 head, train.py:779) and, for C3k2 blocks, all-int8 groups
  if (e->h.precision == kFp16 || e->h.precision == kInt8 || e->h.precision == kSplit16) {
    find_c3k2_groups(e, &blob);
    find_head_groups(e, &blob);
    find_pair_groups(e, &blob);
    const char* fz = getenv("UNINA_FUSE");
    e->fuse = e->n_groups > 0 && !(fz && fz[0] == '0');
  }
  return UNINA_OK;
}

// Device side of loading: uploads the blob, allocates the activation arena and the post-process workspace, initialises
// the kernel families. On error: the code, with the message in g_load_error.
int load_device(unina_engine* e, const std::vector<char>& blob) {
  hipError_t err;
#define LOADCHK(call) \
  if ((err = (call)) != hipSuccess) return fail(nullptr, UNINA_ERR_HIP, "%s: %s", #call, hipGetErrorString(err));
  LOADCHK(hipSetDevice(e->device));
  LOADCHK(hipMalloc(&e->d_blob, blob.size() ? blob.size() : 16));
  LOADCHK(hipMemcpy(e->d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice));
  size_t arena = 0;
  for (auto& b : e->bufs)
    if (!(b.d.flags & kBufInput)) arena += (b.bytes + 255) & ~(size_t)255;
  LOADCHK(kernels_init());
  LOADCHK(hipMalloc(&e->d_zeros, 256));
  LOADCHK(hipMemset(e->d_zeros, 0, 256));
  LOADCHK(hipMalloc(&e->d_arena, arena ? arena : 256));
  LOADCHK(hipMemset(e->d_arena, 0, arena ? arena : 256));
  size_t off = 0;
  for (auto& b : e->bufs) {
    if (b.d.flags & kBufInput) continue;
    b.owned = static_cast<char*>(e->d_arena) + off;
    b.ptr = b.owned;
    off += (b.bytes + 255) & ~(size_t)255;
  }
  int gw[3], gh[3];
  for (int i = 0; i < 3; ++i) {
    gw[i] = (int)e->bufs[e->out_buf[2 * i]].d.w;
    gh[i] = (int)e->bufs[e->out_buf[2 * i]].d.h;
  }
  e->post_blocks = post_num_blocks(gw, gh);
  if (e->post_blocks > kPostBlock) return fail(nullptr, UNINA_ERR_UNSUPPORTED, "input too large for the post-process workspace");
  {  // candidate segments: post_blocks x 1024 records (one-launch form) or up to 1024 workgroups x 256 (split form)
    const size_t recs = (size_t)e->post_blocks * kPostBlock > (size_t)1024 * kPost2Block ? (size_t)e->post_blocks * kPostBlock : (size_t)1024 * kPost2Block;
    LOADCHK(hipMalloc(&e->d_cand, sizeof(GpuDetection) * recs));
    LOADCHK(hipMalloc(&e->d_block_count, sizeof(int) * (size_t)(e->post_blocks > 1024 ? e->post_blocks : 1024)));
  }
  LOADCHK(hipMalloc(&e->d_ticket, sizeof(unsigned int)));
  LOADCHK(hipMemset(e->d_ticket, 0, sizeof(unsigned int)));
  LOADCHK(hipMalloc(&e->d_post_ws, post_workspace_bytes()));
  LOADCHK(hipMemset(e->d_post_ws, 0, post_workspace_bytes()));
  LOADCHK(hipMalloc(&e->d_result, sizeof(DeviceResult)));
  LOADCHK(hipMemset(e->d_result, 0, sizeof(DeviceResult)));
  LOADCHK(hipHostMalloc(&e->h_result, sizeof(DeviceResult), hipHostMallocMapped));
  memset(e->h_result, 0, sizeof(DeviceResult));
  if (hipHostGetDevicePointer(reinterpret_cast<void**>(&e->h_result_dev), e->h_result, 0) != hipSuccess) {
    e->h_result_dev = nullptr;
    (void)hipGetLastError();
  }
  LOADCHK(hipDeviceSynchronize());
#undef LOADCHK
  return UNINA_OK;
}
}  // namespace

extern "C" {

#ifndef UNINA_SOURCE_HASH
#define UNINA_SOURCE_HASH "unhashed"
#endif
// "... src:<hash of the sources this binary was built from>" (build.py source_hash(); tests compare it with the tree's)
const char* unina_version(void) { return "unina_mi355 0.3.0 gfx950 src:" UNINA_SOURCE_HASH; }

const char* unina_last_error(const unina_engine_t* e) { return e ? e->err.c_str() : g_load_error.c_str(); }

int unina_load_engine(const char* path, int device_id, unina_engine_t** out) {
  if (!path || !out) return fail(nullptr, UNINA_ERR_ARG, "unina_load_engine: null argument");
  *out = nullptr;
  unina_engine* e = new unina_engine();
  e->device = device_id;
  std::vector<char> blob;
  int rc = load_host(path, e, &blob);
  if (rc == UNINA_OK) rc = load_device(e, blob);
  if (rc != UNINA_OK) {
    unina_unload_engine(e);
    return rc;
  }
  const char* ng = getenv("UNINA_NO_GRAPH");
  e->use_graph = !(ng && ng[0] == '1');
  if (const char* fg = getenv("UNINA_FULL_GRAPH")) e->full_graph = fg[0] != '0';
  if (const char* ps = getenv("UNINA_POST_SPLIT")) e->post_split = ps[0] != '0';
  if (const char* pf = getenv("UNINA_POST_FOLD")) e->fold_heads = pf[0] != '0';
  e->plan_dirty = true;
  *out = e;
  return UNINA_OK;
}

void unina_unload_engine(unina_engine_t* e) {
  if (!e) return;
  if (e->t_calls) fprintf(stderr, "unina_infer host split over %ld calls: submit (params + hipGraphLaunch) %.2f us, wait for the completion word %.2f us, record copy %.2f us\n", e->t_calls, e->t_submit_us / e->t_calls, e->t_wait_us / e->t_calls, e->t_copy_us / e->t_calls);
  (void)hipSetDevice(e->device);
  drop_graph(e);
  void* dev[] = {e->d_blob, e->d_arena, e->d_zeros, e->d_cand, e->d_block_count, e->d_ticket, e->d_post_ws, e->d_result, e->d_mine_ws, e->d_tile_slots, e->d_calib_tab};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  if (e->h_result) (void)hipHostFree(e->h_result);
  delete e;
}

int unina_engine_input_dims(const unina_engine_t* e, int* width, int* height, int* num_classes) {
  if (!e) return UNINA_ERR_ARG;
  if (width) *width = (int)e->h.in_w;
  if (height) *height = (int)e->h.in_h;
  if (num_classes) *num_classes = (int)e->h.num_classes;
  return UNINA_OK;
}

int unina_set_tensor_address(unina_engine_t* e, const char* name, void* device_ptr) {
  if (!e || !name) return UNINA_ERR_ARG;
  const int i = find_buffer(e, name);
  if (i < 0 || !(e->bufs[i].d.flags & (kBufInput | kBufOutput))) return fail(e, UNINA_ERR_ARG, "unknown I/O tensor '%s'", name);
  if (!device_ptr && (e->bufs[i].d.flags & kBufOutput)) device_ptr = e->bufs[i].owned;  // NULL = back to the engine-owned buffer
  if (((uintptr_t)device_ptr) & 15) return fail(e, UNINA_ERR_ARG, "tensor '%s': address must be 16-byte aligned", name);
  if (e->bufs[i].ptr != device_ptr) {
    e->bufs[i].ptr = device_ptr;
    if (i == e->images_buf && !e->plan_dirty) {
      for (size_t k = 0; k < e->ops.size(); ++k)  // only the eager (stem) ops read it: patch them, keep the graph
        if (is_eager(e, k)) e->ops[k].sp.src = static_cast<const float*>(device_ptr);
    } else {
      e->plan_dirty = true;
    }
  }
  return UNINA_OK;
}

int unina_tensor_address(const unina_engine_t* e, const char* name, void** device_ptr, size_t* num_floats) {
  if (!e || !name) return UNINA_ERR_ARG;
  const int i = find_buffer(e, name);
  if (i < 0 || !(e->bufs[i].d.flags & (kBufInput | kBufOutput))) return UNINA_ERR_ARG;
  if (device_ptr) *device_ptr = e->bufs[i].ptr;
  if (num_floats) *num_floats = (size_t)e->bufs[i].d.h * e->bufs[i].d.w * e->bufs[i].d.c;
  return UNINA_OK;
}

int unina_enqueue(unina_engine_t* e, hipStream_t stream) {
  if (!e) return UNINA_ERR_ARG;
  const int rc = make_ready(e);
  return rc != UNINA_OK ? rc : enqueue_forward(e, FrameCall{}, stream);
}

int unina_postprocess_async(unina_engine_t* e, float conf, float iou, float q, GpuDetection* d_out, int* d_out_count,
                            hipStream_t stream) {
  if (!e || !d_out || !d_out_count) return UNINA_ERR_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  PostParams pp;
  fill_post_params(e, &pp, FrameCall{}, conf, iou, q, d_out, d_out_count, &e->d_result->candidates);
  HIPCHK(e, postprocess_launch(pp, stream));
  return UNINA_OK;
}

int unina_infer_async(unina_engine_t* e, const float* d_images, float conf, float iou, float q, GpuDetection* d_out,
                      int* d_out_count, hipStream_t stream) {
  if (!e) return UNINA_ERR_ARG;
  if (d_images) {
    int rc = unina_set_tensor_address(e, "images", const_cast<float*>(d_images));
    if (rc != UNINA_OK) return rc;
  }
  return enqueue_frame(e, FrameCall{}, conf, iou, q, d_out, d_out_count, stream);
}

}  // extern "C"

namespace {
// The synchronous delivery of unina_infer and every synchronous camera call: `enqueue(d_out, d_count, done_flag, done_value)` enqueues
// the work whose LAST post-process launch writes the records and the count there and then stores done_value to done_flag (nullptr:
// the host waits for the stream instead).
template <typename Enqueue>
int infer_sync(unina_engine* e, Enqueue enqueue, GpuDetection* out, int* out_count, hipStream_t stream) {
  // The post-process writes its compacted output (write-only: count + n records) straight into the pinned, device-mapped
  // host block: no D2H copy command (a blit-kernel launch of its own, and all 1024 slots) on the latency path.
  // UNINA_HOST_RESULT=0 restores the device buffer + copy.
  static const bool host_result = !(getenv("UNINA_HOST_RESULT") && getenv("UNINA_HOST_RESULT")[0] == '0');
  // ... and the host does not wait for the stream either: the last block stores this call's sequence number behind the
  // records (system-scope release) and the host spins on that word -- the runtime's completion signal of the frame graph
  // arrives microseconds later. UNINA_HOST_POLL=0 waits with hipStreamSynchronize instead.
  static const bool host_poll = !(getenv("UNINA_HOST_POLL") && getenv("UNINA_HOST_POLL")[0] == '0');
  bool copied = false;
  if (host_result && e->h_result_dev) {
    unsigned int seq = 0;
    if (host_poll) seq = ++e->result_seq ? e->result_seq : ++e->result_seq;   // never 0
    static const bool timing = getenv("UNINA_TIMING") != nullptr;
    const auto ta = std::chrono::steady_clock::now();
    int rc = enqueue(e->h_result_dev->det, &e->h_result_dev->count, host_poll ? &e->h_result_dev->seq : nullptr, seq);
    if (rc != UNINA_OK) return rc;
    const auto tb = std::chrono::steady_clock::now();
    if (host_poll) {
      volatile unsigned int* flag = &e->h_result->seq;
      const auto t0 = std::chrono::steady_clock::now();
      bool seen = false;
      for (unsigned long it = 1;; ++it) {
        if (*flag == seq) { seen = true; break; }
        __builtin_ia32_pause();
        if ((it & 0xFFFFF) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;
      }
      std::atomic_thread_fence(std::memory_order_acquire);
      if (!seen) HIPCHK(e, hipStreamSynchronize(stream));   // (a faulted launch reports here)
    } else {
      HIPCHK(e, hipStreamSynchronize(stream));
    }
    if (timing) {
      const auto tc = std::chrono::steady_clock::now();
      const int n0 = e->h_result->count;
      if (n0 >= 0 && n0 <= MAX_DETECTIONS) {
        memcpy(out, e->h_result->det, sizeof(GpuDetection) * (size_t)n0);
        copied = true;
      }
      const auto td = std::chrono::steady_clock::now();
      e->t_submit_us += std::chrono::duration<double, std::micro>(tb - ta).count();
      e->t_wait_us += std::chrono::duration<double, std::micro>(tc - tb).count();
      e->t_copy_us += std::chrono::duration<double, std::micro>(td - tc).count();
      ++e->t_calls;
    }
  } else {
    int rc = enqueue(e->d_result->det, &e->d_result->count, nullptr, 0u);
    if (rc != UNINA_OK) return rc;
    HIPCHK(e, hipMemcpyAsync(e->h_result, e->d_result, sizeof(DeviceResult), hipMemcpyDeviceToHost, stream));
    HIPCHK(e, hipStreamSynchronize(stream));
  }
  int n = e->h_result->count;
  if (n < 0 || n > MAX_DETECTIONS) return fail(e, UNINA_ERR_STATE, "post-process returned count %d", n);
  if (!copied) memcpy(out, e->h_result->det, sizeof(GpuDetection) * (size_t)n);   // (the UNINA_TIMING branch has copied them already)
  *out_count = n;
  return UNINA_OK;
}

// One frame as `call` describes it, delivered to the host (infer_sync, whose completion word joins the call) or left on the stream
int run_frame(unina_engine* e, FrameCall call, bool async, float conf, float iou, float q, GpuDetection* out, int* out_count, hipStream_t stream) {
  if (async) return enqueue_frame(e, call, conf, iou, q, out, out_count, stream);
  return infer_sync(e, [&](GpuDetection* d_out, int* d_count, unsigned int* done_flag, unsigned int done_value) {
    call.done_flag = done_flag;
    call.done_value = done_value;
    return enqueue_frame(e, call, conf, iou, q, d_out, d_count, stream);
  }, out, out_count, stream);
}
}  // namespace

extern "C" {

int unina_infer(unina_engine_t* e, const float* d_images, float conf, float iou, float q, GpuDetection* out,
                int* out_count, hipStream_t stream) {
  if (!e || !out || !out_count) return UNINA_ERR_ARG;
  if (d_images) {
    int rc = unina_set_tensor_address(e, "images", const_cast<float*>(d_images));
    if (rc != UNINA_OK) return rc;
  }
  return run_frame(e, FrameCall{}, false, conf, iou, q, out, out_count, stream);
}

// ---- data mining (active_learning.py:31-99, 234-305): scores and embedding behind the raw-head forward ----
static int embed_channels(const unina_engine* e) {
  const SegDesc& sg = e->ops[e->embed_op].d.seg[0];
  // a narrower model embedded at the file's width keeps its own channels first (export.py, statedict.widen_state_dict)
  const uint32_t own = e->h.model_base_channels ? 8 * e->h.model_base_channels : sg.n_count;
  return (int)(own < sg.n_count ? own : sg.n_count);
}

int unina_embedding_dim(const unina_engine_t* e) {
  if (!e) return -UNINA_ERR_ARG;
  if (e->embed_op < 0) return -UNINA_ERR_UNSUPPORTED;
  return embed_channels(e);
}

// Fills the launch parameters from the current buffer addresses; embed: also the pooled slice (checked here, per call:
// fusion can be switched at run time). The workspace is allocated on first use: [partials | 8 scores | embedding] (the last
// two are unina_mine's staging).
static int fill_mine_params(unina_engine* e, MineParams* mp, bool embed, float** stage) {
  memset(mp, 0, sizeof *mp);
  for (int i = 0; i < 3; ++i) {
    const Buffer& c = e->bufs[e->out_buf[2 * i]];
    if (!c.ptr) return fail(e, UNINA_ERR_STATE, "head tensor '%s' has no address", c.d.name);
    mp->cls[i] = static_cast<const float*>(c.ptr);
    mp->cells[i] = (int)(c.d.h * c.d.w);
  }
  mp->num_classes = (int)e->h.num_classes;
  MineParams all = *mp;   // the workspace is sized for a call WITH the embedding, whatever this one asks for
  if (e->embed_op >= 0) {
    const PlannedOp& op = e->ops[e->embed_op];
    const SegDesc& sg = op.d.seg[0];
    const Buffer& b = e->bufs[sg.dst_buf];
    all.hw = (int)(b.d.h * b.d.w);
    all.ctot = (int)b.d.c;
    all.coff = (int)sg.dst_coff;
    all.c = embed_channels(e);
    all.act = act_dtype_of(b.d.dtype);
    all.scale = b.d.scale;
    all.lo_off = lo_plane(b.d);
    if (embed) {
      if (all.act < 0 || all.c < kGapChunk || all.c % kGapChunk || all.coff % kGapChunk || all.ctot % kGapChunk || all.c > kGapMaxChannels)
        return fail(e, UNINA_ERR_UNSUPPORTED, "embedding: slice [%d, %d) of '%s' does not fit the pool kernel's 8-channel chunks", all.coff, all.coff + all.c, b.d.name);
      // the slice must be written to memory by whatever launches the op now: its own conv, or a fused C3k2 block whose OUTPUT
      // it is (a block's output is always stored; only the tensors between its first conv and cv3 stay in LDS)
      if (e->fuse && op.fuse_role == 2) {
        bool stored = false;
        for (const PlannedOp& g : e->ops) stored = stored || (g.fuse_role == 1 && g.fuse_kind == 1 && g.group_last == e->embed_op);
        if (!stored) return fail(e, UNINA_ERR_UNSUPPORTED, "embedding: '%s' is internal to a fused launch and never written (unina_set_fusion(e, 0) writes it)", op.d.name);
      }
      all.src = b.ptr;
    }
  } else if (embed) {
    return fail(e, UNINA_ERR_UNSUPPORTED, "embedding: this engine has no 'backbone.stage3_c3k2.cv3' (graph (B) models have no .backbone; the reference's extract_backbone_embeddings takes another route for them, which is not covered)");
  }
  mine_plan(&all);
  const size_t part = (mine_workspace_floats(all) + 3) & ~(size_t)3;
  if (!e->d_mine_ws) HIPCHK(e, hipMalloc(&e->d_mine_ws, sizeof(float) * (part + UNINA_MINE_SCORES + (size_t)(all.c > 0 ? all.c : 1))));
  *mp = all;
  mp->score_partial = e->d_mine_ws;
  mp->gap_partial = e->d_mine_ws + (((size_t)2 * all.blk0[3] + 3) & ~(size_t)3);
  if (stage) *stage = e->d_mine_ws + part;
  return UNINA_OK;
}

int unina_mine_heads_async(unina_engine_t* e, float* d_scores8, hipStream_t stream) {
  if (!e) return UNINA_ERR_ARG;
  if (!d_scores8 || ((uintptr_t)d_scores8 & 3)) return fail(e, UNINA_ERR_ARG, "unina_mine_heads_async: null / misaligned score pointer");
  HIPCHK(e, hipSetDevice(e->device));
  MineParams mp;
  int rc = fill_mine_params(e, &mp, false, nullptr);
  if (rc != UNINA_OK) return rc;
  mp.scores = d_scores8;
  HIPCHK(e, mine_launch(mp, stream));
  return UNINA_OK;
}

int unina_mine_async(unina_engine_t* e, const float* d_images, float* d_scores8, float* d_embed, hipStream_t stream) {
  if (!e) return UNINA_ERR_ARG;
  if (!d_scores8 || ((uintptr_t)d_scores8 & 3) || ((uintptr_t)d_embed & 3)) return fail(e, UNINA_ERR_ARG, "unina_mine_async: null / misaligned result pointer");
  HIPCHK(e, hipSetDevice(e->device));
  MineParams mp;
  int rc = fill_mine_params(e, &mp, d_embed != nullptr, nullptr);   // before any launch: an unsupported engine enqueues nothing
  if (rc != UNINA_OK) return rc;
  if (d_images) {
    rc = unina_set_tensor_address(e, "images", const_cast<float*>(d_images));
    if (rc != UNINA_OK) return rc;
  }
  rc = unina_enqueue(e, stream);   // the raw-head forward: all six fp32 planes are written
  if (rc != UNINA_OK) return rc;
  mp.scores = d_scores8;
  mp.embed = d_embed;
  HIPCHK(e, mine_launch(mp, stream));
  return UNINA_OK;
}

int unina_mine(unina_engine_t* e, const float* d_images, float* scores8, float* embed, hipStream_t stream) {
  if (!e) return UNINA_ERR_ARG;
  if (!scores8) return fail(e, UNINA_ERR_ARG, "unina_mine: null score pointer");
  HIPCHK(e, hipSetDevice(e->device));
  MineParams mp;
  float* stage = nullptr;
  int rc = fill_mine_params(e, &mp, embed != nullptr, &stage);
  if (rc != UNINA_OK) return rc;
  rc = unina_mine_async(e, d_images, stage, embed ? stage + UNINA_MINE_SCORES : nullptr, stream);
  if (rc != UNINA_OK) return rc;
  HIPCHK(e, hipStreamSynchronize(stream));
  HIPCHK(e, hipMemcpy(scores8, stage, sizeof(float) * UNINA_MINE_SCORES, hipMemcpyDeviceToHost));
  if (embed) HIPCHK(e, hipMemcpy(embed, stage + UNINA_MINE_SCORES, sizeof(float) * (size_t)mp.c, hipMemcpyDeviceToHost));
  return UNINA_OK;
}

// ---- INT8 calibration (qat.py:171-220): |x| value-count tables of the fp16 activation buffers, behind the raw-head forward ----
static bool is_calib_buffer(const Buffer& b) { return b.d.dtype == kBufF16Nhwc; }

int unina_calib_buffer_count(const unina_engine_t* e) {
  if (!e) return -UNINA_ERR_ARG;
  int n = 0;
  for (const Buffer& b : e->bufs) n += is_calib_buffer(b);
  return n;
}

int unina_calib_buffer_name(const unina_engine_t* e, int i, char* name, size_t cap) {
  if (!e || !name || cap == 0 || i < 0) return UNINA_ERR_ARG;
  for (const Buffer& b : e->bufs) {
    if (!is_calib_buffer(b) || i--) continue;
    const size_t len = strnlen(b.d.name, sizeof b.d.name);
    if (len + 1 > cap) return UNINA_ERR_ARG;
    memcpy(name, b.d.name, len);
    name[len] = 0;
    return UNINA_OK;
  }
  return UNINA_ERR_ARG;
}

// What every calibration call checks before it enqueues anything -- the engine first (a caller sizes its table from
// unina_calib_buffer_count, which is 0 for an fp32 / STRICT engine), then the table pointer -- and the descriptor table (built
// once per handle).
static int calib_prepare(unina_engine* e, const char* who, uint32_t* d_counts) {
  if (e->h.precision != kFp16) return fail(e, UNINA_ERR_UNSUPPORTED, "%s: calibration runs on the fp16 engine (this one has precision %u)", who, e->h.precision);
  if (unina_fusion_groups(e) > 0)
    return fail(e, UNINA_ERR_STATE, "%s: %d fused launches do not write their internal buffers; call unina_set_fusion(e, 0) first", who, unina_fusion_groups(e));
  if (!d_counts || ((uintptr_t)d_counts & 15)) return fail(e, UNINA_ERR_ARG, "%s: null / misaligned table pointer", who);
  if (e->d_calib_tab) return UNINA_OK;
  std::vector<CalibDesc> tab;
  for (size_t i = 0; i < e->bufs.size(); ++i) {
    const Buffer& b = e->bufs[i];
    if (!is_calib_buffer(b)) continue;
    if (!b.ptr || ((uintptr_t)b.ptr & 15)) return fail(e, UNINA_ERR_STATE, "%s: buffer '%s' has no 16-byte aligned address", who, b.d.name);
    tab.push_back(CalibDesc{b.ptr, (unsigned long long)b.d.h * b.d.w * b.d.c, (unsigned)tab.size(), 0, 0, 0});
    e->calib_bufs.push_back((int)i);
  }
  if (tab.empty()) return fail(e, UNINA_ERR_UNSUPPORTED, "%s: the engine has no fp16 activation buffer", who);
  e->calib_grid = calib_plan(tab.data(), (int)tab.size());
  if (!e->calib_grid) return fail(e, UNINA_ERR_HIP, "%s: calib_plan failed (device query)", who);
  HIPCHK(e, hipMalloc(&e->d_calib_tab, sizeof(CalibDesc) * tab.size()));
  HIPCHK(e, hipMemcpy(e->d_calib_tab, tab.data(), sizeof(CalibDesc) * tab.size(), hipMemcpyHostToDevice));
  return UNINA_OK;
}

static int calib_enqueue(unina_engine* e, uint32_t* d_counts, hipStream_t stream) {
  const int count = (int)e->calib_bufs.size();
  HIPCHK(e, hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * (size_t)count * UNINA_CALIB_BINS, stream));
  HIPCHK(e, calib_launch_table(e->d_calib_tab, count, e->calib_grid, d_counts, stream));
  return UNINA_OK;
}

int unina_calib_buffers_async(unina_engine_t* e, uint32_t* d_counts, hipStream_t stream) {
  if (!e) return UNINA_ERR_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  const int rc = calib_prepare(e, "unina_calib_buffers_async", d_counts);
  return rc != UNINA_OK ? rc : calib_enqueue(e, d_counts, stream);
}

int unina_calib_async(unina_engine_t* e, const float* d_images, uint32_t* d_counts, hipStream_t stream) {
  if (!e) return UNINA_ERR_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  int rc = calib_prepare(e, "unina_calib_async", d_counts);   // before any launch: a refused call enqueues nothing
  if (rc != UNINA_OK) return rc;
  if (d_images) {
    rc = unina_set_tensor_address(e, "images", const_cast<float*>(d_images));
    if (rc != UNINA_OK) return rc;
  }
  rc = unina_enqueue(e, stream);   // the raw-head forward, unfused: every activation buffer is written
  if (rc != UNINA_OK) return rc;
  return calib_enqueue(e, d_counts, stream);
}

// `n_calls` serial unina_infer calls over a ring of `n_ring` input frames, each timed on the host's steady clock from entry to
// return (detections copied out): the latency a C / C++ caller of this ABI sees, without a binding layer's per-call cost
// (the ctypes path adds ~12 us). lat_us[n_calls].
int unina_serial_latency(unina_engine_t* e, const float* const* d_frames, int n_ring, int n_calls, float conf, float iou, float q,
                         double* lat_us, hipStream_t stream) {
  if (!e || !d_frames || !lat_us || n_ring < 1 || n_calls < 1) return UNINA_ERR_ARG;
  std::vector<GpuDetection> out(MAX_DETECTIONS);
  int n = 0;
  for (int i = 0; i < n_calls; ++i) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = unina_infer(e, d_frames[i % n_ring], conf, iou, q, out.data(), &n, stream);
    lat_us[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (rc != UNINA_OK) return rc;
  }
  return UNINA_OK;
}

// ---- camera frames: every entry point describes its frame as a unina_frame and its call as a FrameCall ----
// The frame of a format-named entry point (GpuBufferHandle::format, perception_node.cpp:357-368)
static unina_frame bgra_frame(const uint8_t* d_bgra, int w, int h, int pitch) { return {UNINA_FMT_BGRA, w, h, {d_bgra, nullptr}, {pitch, 0}}; }
static unina_frame nv12_frame(const uint8_t* d_y, const uint8_t* d_uv, int w, int h, int y_pitch, int uv_pitch) {
  return {UNINA_FMT_NV12, w, h, {d_y, d_uv}, {y_pitch, uv_pitch}};
}

// What every camera call checks before its own arguments: the pointers, the result alignment of the asynchronous forms (the
// synchronous ones hand the post-process a buffer of the engine's) and the frame geometry of the format (frame_defect)
static int check_frame_call(unina_engine* e, const char* who, const unina_frame* f, const NormParams* norm, bool async, const GpuDetection* out,
                            const int* out_count) {
  if (!e) return UNINA_ERR_ARG;
  if (!norm || !out || !out_count) return fail(e, UNINA_ERR_ARG, "%s: null norm / result pointer", who);
  if (async && ((uintptr_t)out & 15)) return fail(e, UNINA_ERR_ARG, "%s: misaligned result pointer", who);
  const char* why = frame_defect(f);
  if (!why) return UNINA_OK;
  if (f) return fail(e, UNINA_ERR_ARG, "%s: %s (format %d, %d x %d, pitch %d / %d)", who, why, f->format, f->width, f->height, f->pitch[0], f->pitch[1]);
  return fail(e, UNINA_ERR_ARG, "%s: %s", who, why);
}

// Camera frame -> detections: unina_infer with the pre-process (camera_source.h: colour conversion, optional half-pixel-centre
// bilinear resize, normalise) computed inside the stem kernel instead of written to an fp32 tensor by one launch and read back by
// the next (BGRA: 4 B/px in instead of 12 B/px out + 12 B/px in, one launch less). The same functions, so the detections are those
// of the two-step form bit for bit (tests/test_gpu_preprocess.py, test_gpu_nv12.py, test_gpu_frame_formats.py).
static int infer_plain(unina_engine* e, const char* who, const unina_frame* f, const NormParams* norm, float conf, float iou, float q, bool async,
                       GpuDetection* out, int* out_count, hipStream_t stream) {
  const int rc = check_frame_call(e, who, f, norm, async, out, out_count);
  if (rc != UNINA_OK) return rc;
  const CameraSource c = frame_source(*f, *norm);
  FrameCall call;
  call.region = &c;
  return run_frame(e, call, async, conf, iou, q, out, out_count, stream);
}

// Letterboxed (include/unina_mi355.h at unina_letterbox_geometry). Nothing is enqueued before the last check has passed.
static int infer_letterbox(unina_engine* e, const char* who, const unina_frame* f, const NormParams* norm, float conf, float iou, float q,
                           float pad_value, int map_boxes, bool async, GpuDetection* out, int* out_count, hipStream_t stream) {
  const int rc = check_frame_call(e, who, f, norm, async, out, out_count);
  if (rc != UNINA_OK) return rc;
  if (map_boxes != 0 && map_boxes != 1) return fail(e, UNINA_ERR_ARG, "%s: map_boxes must be 0 or 1, got %d", who, map_boxes);
  unina_letterbox lb;
  if (unina_letterbox_geometry(f->width, f->height, (int)e->h.in_w, (int)e->h.in_h, &lb) != UNINA_OK)
    return fail(e, UNINA_ERR_ARG, "%s: bad frame size %d x %d", who, f->width, f->height);
  const CameraSource c = frame_source(*f, *norm);
  FrameCall call;
  call.region = &c;
  call.lb = &lb;
  call.pad = pad_value;
  call.map_boxes = map_boxes != 0;
  return run_frame(e, call, async, conf, iou, q, out, out_count, stream);
}

int unina_infer_bgra(unina_engine_t* e, const uint8_t* d_bgra, int src_width, int src_height, int src_pitch,
                     const NormParams* norm, float conf, float iou, float q, GpuDetection* out, int* out_count,
                     hipStream_t stream) {
  const unina_frame f = bgra_frame(d_bgra, src_width, src_height, src_pitch);
  return infer_plain(e, "unina_infer_bgra", &f, norm, conf, iou, q, false, out, out_count, stream);
}

int unina_infer_nv12(unina_engine_t* e, const uint8_t* d_y, const uint8_t* d_uv, int src_width, int src_height, int y_pitch,
                     int uv_pitch, const NormParams* norm, float conf, float iou, float q, GpuDetection* out, int* out_count,
                     hipStream_t stream) {
  const unina_frame f = nv12_frame(d_y, d_uv, src_width, src_height, y_pitch, uv_pitch);
  return infer_plain(e, "unina_infer_nv12", &f, norm, conf, iou, q, false, out, out_count, stream);
}

int unina_infer_frame(unina_engine_t* e, const unina_frame* frame, const NormParams* norm, float conf, float iou, float q,
                      GpuDetection* out, int* out_count, hipStream_t stream) {
  return infer_plain(e, "unina_infer_frame", frame, norm, conf, iou, q, false, out, out_count, stream);
}

int unina_infer_frame_async(unina_engine_t* e, const unina_frame* frame, const NormParams* norm, float conf, float iou, float q,
                            GpuDetection* d_out, int* d_out_count, hipStream_t stream) {
  return infer_plain(e, "unina_infer_frame_async", frame, norm, conf, iou, q, true, d_out, d_out_count, stream);
}

int unina_infer_letterbox_bgra(unina_engine_t* e, const uint8_t* d_bgra, int src_width, int src_height, int src_pitch,
                               const NormParams* norm, float conf, float iou, float q, float pad_value, int map_boxes,
                               GpuDetection* out, int* out_count, hipStream_t stream) {
  const unina_frame f = bgra_frame(d_bgra, src_width, src_height, src_pitch);
  return infer_letterbox(e, "unina_infer_letterbox_bgra", &f, norm, conf, iou, q, pad_value, map_boxes, false, out, out_count, stream);
}

int unina_infer_letterbox_bgra_async(unina_engine_t* e, const uint8_t* d_bgra, int src_width, int src_height, int src_pitch,
                                     const NormParams* norm, float conf, float iou, float q, float pad_value, int map_boxes,
                                     GpuDetection* d_out, int* d_out_count, hipStream_t stream) {
  const unina_frame f = bgra_frame(d_bgra, src_width, src_height, src_pitch);
  return infer_letterbox(e, "unina_infer_letterbox_bgra_async", &f, norm, conf, iou, q, pad_value, map_boxes, true, d_out, d_out_count, stream);
}

int unina_infer_letterbox_nv12(unina_engine_t* e, const uint8_t* d_y, const uint8_t* d_uv, int src_width, int src_height, int y_pitch,
                               int uv_pitch, const NormParams* norm, float conf, float iou, float q, float pad_value, int map_boxes,
                               GpuDetection* out, int* out_count, hipStream_t stream) {
  const unina_frame f = nv12_frame(d_y, d_uv, src_width, src_height, y_pitch, uv_pitch);
  return infer_letterbox(e, "unina_infer_letterbox_nv12", &f, norm, conf, iou, q, pad_value, map_boxes, false, out, out_count, stream);
}

int unina_infer_letterbox_nv12_async(unina_engine_t* e, const uint8_t* d_y, const uint8_t* d_uv, int src_width, int src_height,
                                     int y_pitch, int uv_pitch, const NormParams* norm, float conf, float iou, float q, float pad_value,
                                     int map_boxes, GpuDetection* d_out, int* d_out_count, hipStream_t stream) {
  const unina_frame f = nv12_frame(d_y, d_uv, src_width, src_height, y_pitch, uv_pitch);
  return infer_letterbox(e, "unina_infer_letterbox_nv12_async", &f, norm, conf, iou, q, pad_value, map_boxes, true, d_out, d_out_count, stream);
}

int unina_infer_letterbox_frame(unina_engine_t* e, const unina_frame* frame, const NormParams* norm, float conf, float iou, float q,
                                float pad_value, int map_boxes, GpuDetection* out, int* out_count, hipStream_t stream) {
  return infer_letterbox(e, "unina_infer_letterbox_frame", frame, norm, conf, iou, q, pad_value, map_boxes, false, out, out_count, stream);
}

int unina_infer_letterbox_frame_async(unina_engine_t* e, const unina_frame* frame, const NormParams* norm, float conf, float iou, float q,
                                      float pad_value, int map_boxes, GpuDetection* d_out, int* d_out_count, hipStream_t stream) {
  return infer_letterbox(e, "unina_infer_letterbox_frame_async", frame, norm, conf, iou, q, pad_value, map_boxes, true, d_out, d_out_count, stream);
}

// ---- sliced inference (auto_labeler.py:124-199, 255-271): T frame graphs into T device slots, one merge ----
// The overlap ratio as the reference's arithmetic sees it: Python computes int(slice * (1 - 0.2)) in double, and 0.2f widened to
// double is 0.20000000298, which turns 640 * 0.8 = 512 into 511. The float is therefore read as the shortest decimal that names
// it (0.2f -> "0.2" -> the double 0.2), which is what the caller wrote.
static double ratio_as_written(float r) {
  char buf[40];
  for (int prec = 1; prec <= 9; ++prec) {
    snprintf(buf, sizeof buf, "%.*g", prec, (double)r);
    const double d = strtod(buf, nullptr);
    if ((float)d == r) return d;
  }
  return (double)r;
}

int unina_slice_tiles(int frame_w, int frame_h, int slice_w, int slice_h, float overlap_w, float overlap_h, unina_tile* out, int cap) {
  if (frame_w <= 0 || frame_h <= 0 || slice_w <= 0 || slice_h <= 0 || cap < 0 || (cap > 0 && !out)) return -UNINA_ERR_ARG;
  if (!(overlap_w == overlap_w) || !(overlap_h == overlap_h)) return -UNINA_ERR_ARG;
  int n = 0;
  auto emit = [&](int x, int y, int w, int h) {
    if (n < cap) out[n] = unina_tile{x, y, w, h};
    ++n;
  };
  if (frame_h <= slice_h && frame_w <= slice_w) {   // "Handle small images" (:139-141): the whole frame
    emit(0, 0, frame_w, frame_h);
    return n;
  }
  const double sh = (double)slice_h * (1.0 - ratio_as_written(overlap_h)), sw = (double)slice_w * (1.0 - ratio_as_written(overlap_w));
  if (!(sh >= 1.0 && sh < 2147483648.0 && sw >= 1.0 && sw < 2147483648.0)) return -UNINA_ERR_ARG;   // (range() needs a positive step)
  const int stride_h = (int)sh, stride_w = (int)sw;
  // start / extent of the slice that range() step `pos` gives along one axis (:146-151), and whether an earlier step gave the same
  auto axis = [](int len, int slice, int stride, std::vector<int>* start, std::vector<int>* extent, std::vector<char>* first) {
    for (long long pos = 0; pos < len; pos += stride) {
      const int end = (int)(pos + slice < len ? pos + slice : len);
      const int st = end - slice > 0 ? end - slice : 0;
      bool seen = false;
      for (int s : *start) seen = seen || s == st;
      start->push_back(st);
      extent->push_back(end - st);
      first->push_back(!seen);
    }
  };
  std::vector<int> xs, xw, ys, yh;
  std::vector<char> xf, yf;
  axis(frame_h, slice_h, stride_h, &ys, &yh, &yf);
  axis(frame_w, slice_w, stride_w, &xs, &xw, &xf);
  for (size_t j = 0; j < ys.size(); ++j)
    for (size_t i = 0; i < xs.size(); ++i)
      if (yf[j] && xf[i]) emit(xs[i], ys[j], xw[i], yh[j]);   // (a slice repeats exactly when its row or its column does)
  return n;
}

// offset and scale of every tile, fp32 (include/unina_mi355.h at "sliced inference"); checks the tile list against the frame
// when frame_w > 0
static int fill_tile_maps(unina_engine* e, const char* who, const unina_tile* tiles, int n_tiles, int frame_w, int frame_h, TileGatherParams* g) {
  if (!tiles || n_tiles < 1 || n_tiles > UNINA_MAX_TILES) return fail(e, UNINA_ERR_ARG, "%s: need 1..%d tiles, got %d", who, UNINA_MAX_TILES, tiles ? n_tiles : 0);
  static_assert(UNINA_MAX_TILES == kMaxTiles64, "the gather kernel's tile table");
  for (int t = 0; t < n_tiles; ++t) {
    const unina_tile& r = tiles[t];
    if (r.w <= 0 || r.h <= 0 || r.x < 0 || r.y < 0 ||
        (frame_w > 0 && ((long long)r.x + r.w > frame_w || (long long)r.y + r.h > frame_h)))
      return fail(e, UNINA_ERR_ARG, "%s: tile %d (x %d, y %d, %d x %d) is empty or not inside the frame", who, t, r.x, r.y, r.w, r.h);
    g->map[t] = TileMap{(float)r.w / (float)e->h.in_w, (float)r.h / (float)e->h.in_h, (float)r.x, (float)r.y};
  }
  g->n_tiles = n_tiles;
  return UNINA_OK;
}

// gather + the frame's own NMS launch on the handle's workspace; `done`: the synchronous form's completion word (or nullptr)
static int enqueue_merge(unina_engine* e, TileGatherParams* g, const GpuDetection* d_slots, const int* d_counts, float merge_iou,
                         GpuDetection* d_out, int* d_out_count, unsigned int* done, unsigned int done_value, hipStream_t stream) {
  PostParams pp;
  memset(&pp, 0, sizeof pp);
  post_bind_workspace(&pp, e->d_post_ws, e->d_cand);
  pp.mode = kPostSplit;
  pp.iou_thr = merge_iou;
  pp.eoff[2] = g->n_tiles * MAX_DETECTIONS;   // (the NMS launch sizes its enumeration-index split by eoff[2] + gw[2] * gh[2])
  pp.out = d_out;
  pp.out_count = d_out_count;
  pp.out_candidates = &e->d_result->candidates;
  pp.done_flag = done;
  pp.done_value = done_value;
  g->slots = d_slots;
  g->counts = d_counts;
  g->list = pp.list;
  HIPCHK(e, merge_tiles_launch(*g, pp, stream));
  return UNINA_OK;
}

int unina_merge_tiles_async(unina_engine_t* e, const GpuDetection* d_slots, const int* d_counts, const unina_tile* tiles, int n_tiles,
                            float merge_iou, GpuDetection* d_out, int* d_out_count, hipStream_t stream) {
  if (!e) return UNINA_ERR_ARG;
  if (!d_slots || !d_counts || !d_out || !d_out_count || ((uintptr_t)d_slots & 15) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_counts & 3))
    return fail(e, UNINA_ERR_ARG, "unina_merge_tiles_async: null / misaligned pointer");
  TileGatherParams g;
  int rc = fill_tile_maps(e, "unina_merge_tiles_async", tiles, n_tiles, 0, 0, &g);
  if (rc != UNINA_OK) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  return enqueue_merge(e, &g, d_slots, d_counts, merge_iou, d_out, d_out_count, nullptr, 0, stream);
}

// The tiled calls' body: one frame per tile into the handle's slots, one merge. The tiles' frames signal nothing: the completion
// word of the synchronous form belongs to the merge.
static int infer_tiled(unina_engine* e, const char* who, const unina_frame* f, const unina_tile* tiles, int n_tiles, const NormParams* norm,
                       float conf, float iou, float q, float merge_iou, bool async, GpuDetection* out, int* out_count, hipStream_t stream) {
  int rc = check_frame_call(e, who, f, norm, async, out, out_count);
  if (rc != UNINA_OK) return rc;
  TileGatherParams g;
  rc = fill_tile_maps(e, who, tiles, n_tiles, f->width, f->height, &g);
  if (rc != UNINA_OK) return rc;
  HIPCHK(e, hipSetDevice(e->device));
  constexpr size_t kSlotBytes = sizeof(GpuDetection) * MAX_DETECTIONS;
  if (!e->d_tile_slots) HIPCHK(e, hipMalloc(reinterpret_cast<void**>(&e->d_tile_slots), UNINA_MAX_TILES * (kSlotBytes + sizeof(int))));
  int* d_counts = reinterpret_cast<int*>(e->d_tile_slots + (size_t)UNINA_MAX_TILES * MAX_DETECTIONS);
  const CameraSource frame = frame_source(*f, *norm);
  auto enqueue = [&](GpuDetection* d_out, int* d_count, unsigned int* done_flag, unsigned int done_value) {
    for (int t = 0; t < n_tiles; ++t) {
      // (a BGRA / RGB / RGBA tile is a pointer offset; an NV12, 4:2:2 or Bayer tile is not: its origin travels to the kernel)
      const CameraSource c = frame_region(frame, tiles[t].x, tiles[t].y, tiles[t].w, tiles[t].h);
      FrameCall call;
      call.region = &c;
      const int rc = enqueue_frame(e, call, conf, iou, q, e->d_tile_slots + (size_t)t * MAX_DETECTIONS, d_counts + t, stream);
      if (rc != UNINA_OK) return rc;
    }
    return enqueue_merge(e, &g, e->d_tile_slots, d_counts, merge_iou, d_out, d_count, done_flag, done_value, stream);
  };
  return async ? enqueue(out, out_count, nullptr, 0u) : infer_sync(e, enqueue, out, out_count, stream);
}

int unina_infer_tiled_bgra_async(unina_engine_t* e, const uint8_t* d_bgra, int src_width, int src_height, int src_pitch,
                                 const unina_tile* tiles, int n_tiles, const NormParams* norm, float conf, float iou, float q,
                                 float merge_iou, GpuDetection* d_out, int* d_out_count, hipStream_t stream) {
  const unina_frame f = bgra_frame(d_bgra, src_width, src_height, src_pitch);
  return infer_tiled(e, "unina_infer_tiled_bgra", &f, tiles, n_tiles, norm, conf, iou, q, merge_iou, true, d_out, d_out_count, stream);
}

int unina_infer_tiled_bgra(unina_engine_t* e, const uint8_t* d_bgra, int src_width, int src_height, int src_pitch,
                           const unina_tile* tiles, int n_tiles, const NormParams* norm, float conf, float iou, float q,
                           float merge_iou, GpuDetection* out, int* out_count, hipStream_t stream) {
  const unina_frame f = bgra_frame(d_bgra, src_width, src_height, src_pitch);
  return infer_tiled(e, "unina_infer_tiled_bgra", &f, tiles, n_tiles, norm, conf, iou, q, merge_iou, false, out, out_count, stream);
}

// The NV12 pair: the same slots, gather and merge; only the stem's source differs (CameraSource::x0 / y0 carry the tile).
int unina_infer_tiled_nv12_async(unina_engine_t* e, const uint8_t* d_y, const uint8_t* d_uv, int src_width, int src_height,
                                 int y_pitch, int uv_pitch, const unina_tile* tiles, int n_tiles, const NormParams* norm,
                                 float conf, float iou, float q, float merge_iou, GpuDetection* d_out, int* d_out_count,
                                 hipStream_t stream) {
  const unina_frame f = nv12_frame(d_y, d_uv, src_width, src_height, y_pitch, uv_pitch);
  return infer_tiled(e, "unina_infer_tiled_nv12", &f, tiles, n_tiles, norm, conf, iou, q, merge_iou, true, d_out, d_out_count, stream);
}

int unina_infer_tiled_nv12(unina_engine_t* e, const uint8_t* d_y, const uint8_t* d_uv, int src_width, int src_height, int y_pitch,
                           int uv_pitch, const unina_tile* tiles, int n_tiles, const NormParams* norm, float conf, float iou,
                           float q, float merge_iou, GpuDetection* out, int* out_count, hipStream_t stream) {
  const unina_frame f = nv12_frame(d_y, d_uv, src_width, src_height, y_pitch, uv_pitch);
  return infer_tiled(e, "unina_infer_tiled_nv12", &f, tiles, n_tiles, norm, conf, iou, q, merge_iou, false, out, out_count, stream);
}

int unina_infer_tiled_frame_async(unina_engine_t* e, const unina_frame* frame, const unina_tile* tiles, int n_tiles, const NormParams* norm,
                                  float conf, float iou, float q, float merge_iou, GpuDetection* d_out, int* d_out_count,
                                  hipStream_t stream) {
  return infer_tiled(e, "unina_infer_tiled_frame_async", frame, tiles, n_tiles, norm, conf, iou, q, merge_iou, true, d_out, d_out_count, stream);
}

int unina_infer_tiled_frame(unina_engine_t* e, const unina_frame* frame, const unina_tile* tiles, int n_tiles, const NormParams* norm,
                            float conf, float iou, float q, float merge_iou, GpuDetection* out, int* out_count, hipStream_t stream) {
  return infer_tiled(e, "unina_infer_tiled_frame", frame, tiles, n_tiles, norm, conf, iou, q, merge_iou, false, out, out_count, stream);
}

int unina_debug_post_stamps(unina_engine_t* e, long long* out16) {
  if (!e || !out16) return UNINA_ERR_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipDeviceSynchronize());
  HIPCHK(e, hipMemcpy(out16, e->d_result->pad_stamps, sizeof(long long) * 16, hipMemcpyDeviceToHost));
  return UNINA_OK;
}

// Debug: runs conv op `op_index` once with in-kernel s_memtime stamps on (one workgroup in the middle of the grid):
// out5 = shader-clock ticks at start / prologue issued / first data usable / K loop done / stores drained.
int unina_debug_conv_stamps(unina_engine_t* e, int op_index, long long* out5, hipStream_t stream) {
  if (!e || !out5 || op_index < 0 || op_index >= (int)e->ops.size()) return UNINA_ERR_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  if (e->plan_dirty) {
    int rc = plan(e);
    if (rc != UNINA_OK) return rc;
  }
  if (e->ops[op_index].d.kind != kOpConv) return fail(e, UNINA_ERR_ARG, "op %d is not a convolution", op_index);
  long long* stamps = reinterpret_cast<long long*>(e->d_result->pad_stamps);
  HIPCHK(e, hipMemsetAsync(stamps, 0, sizeof(long long) * 8, stream));
  HIPCHK(e, launch_op_as(e, op_index, stream, kLaunchConv, [&](OpLaunch& l) { l.cp[0].stamps = stamps; }));
  HIPCHK(e, hipStreamSynchronize(stream));
  HIPCHK(e, hipMemcpy(out5, stamps, sizeof(long long) * 8, hipMemcpyDeviceToHost));  // 5 shader-clock stamps + 2 at 100 MHz + entry
  return UNINA_OK;
}

// One launch of the DUAL conv launch led by op `op_index` (fusion on: e.g. the P3 | P4 head layers) with in-kernel stamps of
// the mid workgroup of each of its two convs: out16[0..7] conv A, out16[8..15] conv B, each as unina_debug_conv_stamps.
int unina_debug_dual_stamps(unina_engine_t* e, int op_index, long long* out16, hipStream_t stream) {
  if (!e || !out16 || op_index < 0 || op_index >= (int)e->ops.size()) return UNINA_ERR_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  if (e->plan_dirty) {
    int rc = plan(e);
    if (rc != UNINA_OK) return rc;
  }
  const PlannedOp& op = e->ops[op_index];
  if (op.d.kind != kOpConv || op.fuse_role || op.dual_with < 0 || op.dual_absorbed)
    return fail(e, UNINA_ERR_ARG, "op %d does not lead a dual conv launch", op_index);
  long long* stamps = reinterpret_cast<long long*>(e->d_result->pad_stamps);
  HIPCHK(e, hipMemsetAsync(stamps, 0, sizeof(long long) * 16, stream));
  HIPCHK(e, launch_op_as(e, op_index, stream, kLaunchConvDual, [&](OpLaunch& l) {
    l.cp[0].stamps = stamps;
    l.cp[1].stamps = stamps + 8;
  }));
  HIPCHK(e, hipStreamSynchronize(stream));
  HIPCHK(e, hipMemcpy(out16, stamps, sizeof(long long) * 16, hipMemcpyDeviceToHost));
  return UNINA_OK;
}

// Debug: the fused C3k2 block led by op `op_index`, launched once as its stamped twin right after the ops in front of it (cold
// weights, as in a frame): out16[k] = shader-clock stamp of the mid workgroup after step k (block_kernels.h), [14] / [15] =
// the 100 MHz wall clock at its end / entry. Only the 40^2 blocks have twins.
int unina_debug_block_stamps(unina_engine_t* e, int op_index, long long* out16, hipStream_t stream) {
  if (!e || !out16 || op_index < 0 || op_index >= (int)e->ops.size()) return UNINA_ERR_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  if (e->plan_dirty) {
    int rc = plan(e);
    if (rc != UNINA_OK) return rc;
  }
  const PlannedOp& op = e->ops[op_index];
  if (!e->fuse || op.fuse_role != 1 || op.fuse_kind != 1) return fail(e, UNINA_ERR_ARG, "op %d does not lead a fused C3k2 block", op_index);
  for (int i = 0; i < op_index; ++i) HIPCHK(e, launch_op(e, (size_t)i, stream));
  long long* stamps = reinterpret_cast<long long*>(e->d_result->pad_stamps);
  HIPCHK(e, hipMemsetAsync(stamps, 0, sizeof(long long) * 16, stream));
  HIPCHK(e, launch_op_as(e, op_index, stream, kLaunchC3k2, [&](OpLaunch& l) { l.fp.stamps = stamps; }));
  HIPCHK(e, hipStreamSynchronize(stream));
  HIPCHK(e, hipMemcpy(out16, stamps, sizeof(long long) * 16, hipMemcpyDeviceToHost));
  return UNINA_OK;
}

namespace unina {
__global__ void debug_stamp_kernel(long long* t) { if (threadIdx.x == 0) *t = wall_clock64(); }
}
// Same launch with EVERY workgroup's start / end on the 100 MHz wall clock: out[2*i], out[2*i+1] for workgroup i in BLOCK-ID
// order (the weights-stationary pairs put conv B's workgroups first, the register-queue pairs conv A's), then the clock of a
// one-wave marker kernel enqueued right before and of one right after the launch (dispatch gaps); cap >= 2 * grid + 2
// values. Returns the grid size (> 0) or a negative error code.
int unina_debug_dual_timeline(unina_engine_t* e, int op_index, long long* out, int cap, hipStream_t stream) {
  if (!e || !out || op_index < 0 || op_index >= (int)e->ops.size()) return -UNINA_ERR_ARG;
  if (hipSetDevice(e->device) != hipSuccess) return -UNINA_ERR_HIP;
  if (e->plan_dirty) {
    int rc = plan(e);
    if (rc != UNINA_OK) return -rc;
  }
  const PlannedOp& op = e->ops[op_index];
  if (op.d.kind != kOpConv || op.fuse_role || op.dual_with < 0 || op.dual_absorbed) return -UNINA_ERR_ARG;
  // every workgroup writes wg_times[2 * blockIdx.x ..]: the buffer is sized from the grid, known BEFORE anything is launched
  int grid = 0;
  {
    OpLaunch l;
    if (op_launch(e, op_index, kLaunchConvDual, &l) != hipSuccess) return -UNINA_ERR_ARG;
    grid = (int)l.d.grid.x;
  }
  if (grid < 1 || 2 * grid + 2 > cap) return -UNINA_ERR_ARG;
  long long* d = nullptr;
  const size_t words = 18 + 2 * (size_t)grid;
  if (hipMalloc(&d, sizeof(long long) * words) != hipSuccess) return -UNINA_ERR_HIP;
  long long* marks = d + 16 + 2 * grid;
  hipError_t he = hipMemsetAsync(d, 0, sizeof(long long) * words, stream);
  if (he == hipSuccess) {
    hipLaunchKernelGGL(unina::debug_stamp_kernel, dim3(1), dim3(64), 0, stream, marks);
    he = hipGetLastError();
  }
  if (he == hipSuccess)
    he = launch_op_as(e, op_index, stream, kLaunchConvDual, [&](OpLaunch& l) {
      l.cp[0].stamps = d;
      l.cp[1].stamps = d + 8;
      l.cp[0].wg_times = l.cp[1].wg_times = d + 16;
    });
  if (he == hipSuccess) {
    hipLaunchKernelGGL(unina::debug_stamp_kernel, dim3(1), dim3(64), 0, stream, marks + 1);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = hipStreamSynchronize(stream);
  if (he == hipSuccess) he = hipMemcpy(out, d + 16, sizeof(long long) * 2 * grid, hipMemcpyDeviceToHost);
  if (he == hipSuccess) he = hipMemcpy(out + 2 * grid, marks, sizeof(long long) * 2, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  return he == hipSuccess ? grid : -UNINA_ERR_HIP;
}

int unina_op_count(const unina_engine_t* e) { return e ? (int)e->ops.size() : -1; }

int unina_get_op_info(const unina_engine_t* ce, int index, unina_op_info* info) {
  unina_engine* e = const_cast<unina_engine*>(ce);
  if (!e || !info || index < 0 || index >= (int)e->ops.size()) return UNINA_ERR_ARG;
  if (e->plan_dirty) {
    // planning needs addresses only for pointers; shapes/flops are valid regardless
    int rc = plan(e);
    if (rc != UNINA_OK) return rc;
  }
  *info = e->ops[index].info;
  return UNINA_OK;
}

// Load-time analysis alone (no device is touched): the loader's host side, checks and matchers, on the engine file.
int unina_debug_fusable_groups(const char* path) {
  if (!path) return -UNINA_ERR_ARG;
  unina_engine e;
  std::vector<char> blob;
  const int rc = load_host(path, &e, &blob);
  return rc != UNINA_OK ? -rc : e.n_groups;
}

int unina_set_fusion(unina_engine_t* e, int enable) {
  if (!e) return UNINA_ERR_ARG;
  const bool on = enable && e->n_groups > 0;
  if (on != e->fuse) {
    e->fuse = on;
    e->plan_dirty = true;
  }
  return UNINA_OK;
}

int unina_fusion_groups(const unina_engine_t* e) { return e ? (e->fuse ? e->n_groups : 0) : -1; }

int unina_conv_config_count(void) { return (int)kCfgCount; }

const char* unina_conv_config_name(int cfg) { return conv_config_name(cfg, kF16); }

int unina_set_op_config(unina_engine_t* e, int op_index, int cfg) {
  if (!e || op_index < 0 || op_index >= (int)e->ops.size()) return UNINA_ERR_ARG;
  if (e->plan_dirty) {
    int rc = plan(e);
    if (rc != UNINA_OK) return rc;
  }
  if (e->ops[op_index].d.kind != kOpConv) return fail(e, UNINA_ERR_ARG, "op %d is not a convolution", op_index);
  if (cfg >= 0 && !conv_config_valid(e->ops[op_index].cp, cfg)) return fail(e, UNINA_ERR_UNSUPPORTED, "config %d does not fit op %d", cfg, op_index);
  if (e->force_cfg.size() < e->ops.size()) e->force_cfg.assign(e->ops.size(), -1);
  e->force_cfg[op_index] = cfg;
  e->plan_dirty = true;
  return UNINA_OK;
}

// Tactic selection by timing, like the reference's TensorRT build step (export_trt.py:459-468) does on the target:
// every conv op is timed with every tile configuration that fits it and keeps the fastest. Results do not change
// (each output element accumulates its K terms in the same order under every configuration).
int unina_autotune(unina_engine_t* e, int iters, hipStream_t stream) {
  if (!e || iters < 1) return UNINA_ERR_ARG;
  int rc = make_ready(e);
  if (rc == UNINA_OK) rc = launch_all(e, stream);
  if (rc != UNINA_OK) return rc;
  if (e->force_cfg.size() < e->ops.size()) e->force_cfg.assign(e->ops.size(), -1);
  hipEvent_t a, b;
  HIPCHK(e, hipEventCreate(&a));
  HIPCHK(e, hipEventCreate(&b));
  for (size_t i = 0; i < e->ops.size(); ++i) {
    if (e->ops[i].d.kind != kOpConv || (e->fuse && e->ops[i].fuse_role) || e->ops[i].dual_with >= 0 || e->ops[i].dual_absorbed) continue;
    float best = 1e30f;
    int best_cfg = -1;
    for (int cfg = 0; cfg < (int)kCfgCount; ++cfg) {
      if (!conv_config_valid(e->ops[i].cp, cfg)) continue;
      float ms = 0.f;
      rc = time_in_sequence(e, i, iters, stream, a, b,
                            [&]() { return launch_op_as(e, i, stream, kLaunchConv, [&](OpLaunch& l) { l.cfg = cfg; }); }, &ms);
      if (rc != UNINA_OK) return rc;
      if (ms < best) {
        best = ms;
        best_cfg = cfg;
      }
    }
    e->force_cfg[i] = best_cfg;
  }
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  e->plan_dirty = true;
  return UNINA_OK;
}

int unina_profile_ops(unina_engine_t* e, int iters, float* ms_per_op, hipStream_t stream) {
  if (!e || !ms_per_op || iters < 1) return UNINA_ERR_ARG;
  int rc = make_ready(e);
  if (rc == UNINA_OK) rc = launch_all(e, stream);  // warm-up: every buffer holds real activations
  if (rc != UNINA_OK) return rc;
  hipEvent_t a, b;
  HIPCHK(e, hipEventCreate(&a));
  HIPCHK(e, hipEventCreate(&b));
  PostParams pp;   // which head output convs the frame's decode launch computes itself (they are not launched in a frame)
  fill_post_params(e, &pp, FrameCall{}, 0.5f, 0.45f, 0.1f, e->d_result->det, &e->d_result->count, &e->d_result->candidates, e->full_graph && e->use_graph);
  for (size_t i = 0; i < e->ops.size(); ++i) {
    if (!launches_in_frame(e, i, pp)) {
      ms_per_op[i] = 0.f;
      continue;
    }
    rc = time_in_sequence(e, i, iters, stream, a, b, [&]() { return launch_op(e, i, stream); }, &ms_per_op[i]);
    if (rc != UNINA_OK) return rc;
  }
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return UNINA_OK;
}

// The post-process launches of a frame, timed like unina_profile_ops (HIP events on `stream`, each repetition replays the
// whole forward first): ms2[0] = decode launch (with the folded head output convs), ms2[1] = pair tiles + scan + output
// (0 when the post-process is one launch). Thresholds as given.
int unina_profile_post(unina_engine_t* e, int iters, float conf, float iou, float q, float* ms2, hipStream_t stream) {
  if (!e || !ms2 || iters < 1) return UNINA_ERR_ARG;
  int rc0 = make_ready(e);
  if (rc0 != UNINA_OK) return rc0;
  PostParams pp;
  fill_post_params(e, &pp, FrameCall{}, conf, iou, q, e->d_result->det, &e->d_result->count, &e->d_result->candidates, true);
  LaunchDesc d[2];
  const int npost = postprocess_desc(pp, d);
  if (npost < 1) return fail(e, UNINA_ERR_STATE, "post-process launch shape");
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  ms2[0] = ms2[1] = 0.f;
  // (the events are destroyed on every path out of here)
  auto run = [&]() -> int {
    for (auto& x : ev) HIPCHK(e, hipEventCreate(&x));
    for (int it = 0; it < iters; ++it) {
      int rc = launch_all(e, stream);
      if (rc != UNINA_OK) return rc;
      for (int k = 0; k < npost; ++k) {
        PostParams copy = pp;
        void* args[] = {&copy};
        HIPCHK(e, hipEventRecord(ev[k], stream));
        HIPCHK(e, launch_desc(d[k], args, stream));
      }
      HIPCHK(e, hipEventRecord(ev[npost], stream));
      HIPCHK(e, hipEventSynchronize(ev[npost]));
      for (int k = 0; k < npost; ++k) {
        float ms = 0.f;
        HIPCHK(e, hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
        ms2[k] += ms / (float)iters;
      }
    }
    return UNINA_OK;
  };
  const int rc = run();
  for (auto& x : ev)
    if (x) (void)hipEventDestroy(x);
  return rc;
}

int unina_debug_owned_streams(void) { return g_owned_streams.load(); }

int unina_debug_folded_heads(unina_engine_t* e) {
  if (!e) return -UNINA_ERR_ARG;
  if (e->plan_dirty && plan(e) != UNINA_OK) return -UNINA_ERR_STATE;
  PostParams pp;   // exactly what unina_infer_async hands to the frame's post-process
  fill_post_params(e, &pp, FrameCall{}, 0.5f, 0.45f, 0.1f, e->d_result->det, &e->d_result->count, &e->d_result->candidates, e->full_graph && e->use_graph);
  int mask = 0;
  for (int h = 0; h < 3; ++h)
    if (pp.mode == kPostSplit && pp.h1[h] != nullptr) mask |= 1 << h;
  return mask;
}

int unina_debug_read_buffer(unina_engine_t* e, const char* name, float* host_out, size_t capacity, int* c, int* h, int* w) {
  if (!e || !name) return UNINA_ERR_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  const int i = find_buffer(e, name);
  if (i < 0) return fail(e, UNINA_ERR_ARG, "unknown buffer '%s'", name);
  const Buffer& b = e->bufs[i];
  const size_t n = (size_t)b.d.h * b.d.w * b.d.c;
  if (c) *c = (int)b.d.c;
  if (h) *h = (int)b.d.h;
  if (w) *w = (int)b.d.w;
  if (capacity < n) return fail(e, UNINA_ERR_ARG, "buffer '%s' needs %zu floats", name, n);  // dims are still reported
  HIPCHK(e, hipDeviceSynchronize());
  if (b.d.dtype == kBufI8Nhwc) {  // returned as real values (code * scale)
    std::vector<signed char> tmp(n);
    HIPCHK(e, hipMemcpy(tmp.data(), b.ptr, n, hipMemcpyDeviceToHost));
    const size_t hw = (size_t)b.d.h * b.d.w;
    for (size_t p = 0; p < hw; ++p)
      for (size_t ch = 0; ch < b.d.c; ++ch) host_out[ch * hw + p] = (float)tmp[p * b.d.c + ch] * b.d.scale;
  } else if (b.d.dtype == kBufF32Nhwc) {
    std::vector<float> tmp(n);
    HIPCHK(e, hipMemcpy(tmp.data(), b.ptr, n * 4, hipMemcpyDeviceToHost));
    const size_t hw = (size_t)b.d.h * b.d.w;
    for (size_t p = 0; p < hw; ++p)
      for (size_t ch = 0; ch < b.d.c; ++ch) host_out[ch * hw + p] = tmp[p * b.d.c + ch];
  } else if (b.d.dtype == kBufF16Nhwc) {
    std::vector<uint16_t> tmp(n);
    HIPCHK(e, hipMemcpy(tmp.data(), b.ptr, n * 2, hipMemcpyDeviceToHost));
    const size_t hw = (size_t)b.d.h * b.d.w;
    for (size_t p = 0; p < hw; ++p)
      for (size_t ch = 0; ch < b.d.c; ++ch) host_out[ch * hw + p] = half_bits_to_float(tmp[p * b.d.c + ch]);
  } else if (b.d.dtype == kBufS16Nhwc) {   // value = hi + lo
    std::vector<uint16_t> tmp(2 * n);
    HIPCHK(e, hipMemcpy(tmp.data(), b.ptr, n * 4, hipMemcpyDeviceToHost));
    const size_t hw = (size_t)b.d.h * b.d.w;
    for (size_t p = 0; p < hw; ++p)
      for (size_t ch = 0; ch < b.d.c; ++ch)
        host_out[ch * hw + p] = half_bits_to_float(tmp[p * b.d.c + ch]) + half_bits_to_float(tmp[n + p * b.d.c + ch]);
  } else {
    HIPCHK(e, hipMemcpy(host_out, b.ptr, n * 4, hipMemcpyDeviceToHost));
  }
  return UNINA_OK;
}

}  // extern "C"
