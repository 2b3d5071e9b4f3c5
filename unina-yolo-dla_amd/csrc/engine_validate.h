// engine_validate.h -- every check of a .une engine file that depends on the file alone, in plain C++ (engine_format.h, the
// public header's error codes and the standard library: no HIP, no device types), so a host compiler builds it by itself
// (tests/engine_validate_host.cpp) as it builds post_math.h, track_math.h and rectify_map.h.
//
// The kernels trust what the loader derives from the tables -- pointers, leading dimensions, channel and blob offsets --
// without a bounds check of their own, so a file is refused HERE, before anything is allocated from one of its fields, before
// anything is dereferenced through one of its offsets and long before a launch. Two steps, because the tables cannot be read
// before the header has sized them:
//   read_engine_tables   header, then the two tables, through a caller-supplied reader (a FILE in engine.hip, memory in the test)
//   validate_engine      THE validator: header + tables + the number of blob bytes the file really holds -> UNINA_OK or code + message
// Every sum of an offset and an extent is compared as `a > limit || b > limit - a`, or in 64 bits where the terms are 32-bit
// fields; products that can pass 2^64 saturate (mul_sat). tests/engine_file_cases.py states the same rules over Python integers.
#ifndef UNINA_ENGINE_VALIDATE_H
#define UNINA_ENGINE_VALIDATE_H

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#if !defined(__HIPCC__) && !defined(UNINA_NO_HIP_HEADERS)
#define UNINA_NO_HIP_HEADERS   // a host compiler: the error codes without the HIP runtime's headers
#endif
#include "../../include/unina_mi355.h"
#include "engine_format.h"

namespace unina {

struct Verdict {
  int code = UNINA_OK;
  char msg[192] = "";
  bool ok() const { return code == UNINA_OK; }
};

inline Verdict refuse(int code, const char* fmt, ...) {
  Verdict v;
  v.code = code;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(v.msg, sizeof v.msg, fmt, ap);
  va_end(ap);
  return v;
}

constexpr uint32_t kMaxTableEntries = 4096;
constexpr uint64_t kMaxBufferBytes = 1ull << 40;   // plausibility cap on one activation buffer: 4096 of them sum far below 2^64
constexpr uint32_t kMaxClasses = 16383;            // the two-launch NMS carries a class id in 14 bits (kernels.h kMaxNumClasses)
constexpr uint32_t kPoolChannels = 32;             // channels per workgroup of the SPPF pool kernels (stem_pool.hip kPoolCH)
constexpr uint64_t kPoolLdsBytes = 64 * 1024;      // ... and the LDS their three row buffers may take (sppf_pool_desc)
static const char* const kHeadOutputs[6] = {"p2_cls", "p2_reg", "p3_cls", "p3_reg", "p4_cls", "p4_reg"};

inline uint64_t mul_sat(uint64_t a, uint64_t b) {
  uint64_t r;
  return __builtin_mul_overflow(a, b, &r) ? UINT64_MAX : r;
}
// [off, off + len) lies inside [0, limit)
inline bool inside(uint64_t off, uint64_t len, uint64_t limit) { return off <= limit && len <= limit - off; }

inline bool is_act(uint32_t dtype) { return dtype == kBufF16Nhwc || dtype == kBufF32Nhwc || dtype == kBufI8Nhwc || dtype == kBufS16Nhwc; }
// bytes per element of one plane of an activation buffer (addressing: a split-fp16 buffer is two fp16 planes)
inline uint64_t plane_elem_bytes(uint32_t dtype) { return dtype == kBufF32Nhwc ? 4 : (dtype == kBufI8Nhwc ? 1 : 2); }
// bytes per value of a buffer (storage)
inline uint64_t value_bytes(uint32_t dtype) { return dtype == kBufF16Nhwc ? 2 : (dtype == kBufI8Nhwc ? 1 : 4); }
// bytes per weight of a conv, by the type of the buffer it reads (fp32 and split fp16: 4, int8: 1, fp16: 2)
inline uint64_t weight_elem_bytes(uint32_t src_dtype) {
  return (src_dtype == kBufF32Nhwc || src_dtype == kBufS16Nhwc) ? 4 : (src_dtype == kBufI8Nhwc ? 1 : 2);
}
// Bytes of a conv slice's weight blocks in the blob (saturating)
inline uint64_t conv_weight_bytes(const OpDesc& d, const SegDesc& sd, uint32_t src_dtype) {
  return mul_sat(mul_sat(mul_sat(sd.n_pad, (uint64_t)d.ksize * d.ksize), d.cin), weight_elem_bytes(src_dtype));
}
// output extent of a conv with padding k / 2 (graph.py Graph._conv); in >= 1, k in {1, 3}, stride >= 1
inline uint64_t conv_out(uint64_t in, uint64_t k, uint64_t stride) { return (in + 2 * (k / 2) - k) / stride + 1; }

inline int find_buffer_named(const BufferDesc* bufs, uint32_t n, const char* name) {
  for (uint32_t i = 0; i < n; ++i)
    if (!strncmp(bufs[i].name, name, sizeof bufs[i].name)) return (int)i;
  return -1;
}

// What must hold of the header before the tables can be read: they are sized from it.
inline Verdict header_defect(const FileHeader& h) {
  if (memcmp(h.magic, kMagic, 8)) return refuse(UNINA_ERR_FORMAT, "bad magic (not a UNINAENG file)");
  if (h.version != kVersion) return refuse(UNINA_ERR_FORMAT, "unsupported engine file version");
  if (h.precision != kFp16 && h.precision != kFp32 && h.precision != kInt8 && h.precision != kSplit16)
    return refuse(UNINA_ERR_UNSUPPORTED, "unknown engine precision");
  if (h.n_heads != 3 || h.n_buffers == 0 || h.n_buffers > kMaxTableEntries || h.n_ops == 0 || h.n_ops > kMaxTableEntries)
    return refuse(UNINA_ERR_FORMAT, "implausible table sizes");
  return Verdict();
}

struct EngineTables {
  FileHeader h;
  std::vector<BufferDesc> bufs;
  std::vector<OpDesc> ops;
};

// Header and tables through `rd(void* dst, size_t bytes) -> bool` (false: the source ended first).
template <class Read>
Verdict read_engine_tables(Read&& rd, EngineTables* t) {
  if (!rd(&t->h, sizeof t->h)) return refuse(UNINA_ERR_FORMAT, "truncated header");
  const Verdict v = header_defect(t->h);
  if (!v.ok()) return v;
  t->bufs.resize(t->h.n_buffers);
  if (!rd(t->bufs.data(), sizeof(BufferDesc) * t->bufs.size())) return refuse(UNINA_ERR_FORMAT, "truncated buffer table");
  t->ops.resize(t->h.n_ops);
  if (!rd(t->ops.data(), sizeof(OpDesc) * t->ops.size())) return refuse(UNINA_ERR_FORMAT, "truncated op table");
  return Verdict();
}

namespace validate_detail {

inline Verdict check_buffers(const FileHeader& h, const BufferDesc* bufs) {
  uint32_t n_inputs = 0;
  for (uint32_t i = 0; i < h.n_buffers; ++i) {
    const BufferDesc& b = bufs[i];
    if (b.dtype > kBufS16Nhwc) return refuse(UNINA_ERR_FORMAT, "buffer %u: unknown dtype %u", i, b.dtype);
    if (b.h == 0 || b.w == 0 || b.c == 0) return refuse(UNINA_ERR_FORMAT, "buffer %u: empty extent", i);
    if (mul_sat(mul_sat((uint64_t)b.h * b.w, b.c), value_bytes(b.dtype)) > kMaxBufferBytes)
      return refuse(UNINA_ERR_FORMAT, "buffer %u: implausible size", i);
    if (!memchr(b.name, 0, sizeof b.name)) return refuse(UNINA_ERR_FORMAT, "buffer %u: name without terminator", i);
    if (b.dtype == kBufI8Nhwc && !(std::isfinite(b.scale) && b.scale > 0.f))
      return refuse(UNINA_ERR_FORMAT, "buffer %u: int8 buffer needs a finite positive scale", i);
    if (b.flags & kBufInput) {
      ++n_inputs;
      if (b.dtype != kBufF32NchwInput || b.c != h.in_c || b.h != h.in_h || b.w != h.in_w)
        return refuse(UNINA_ERR_FORMAT, "buffer %u: the images input buffer differs from the header's input shape", i);
    }
  }
  if (n_inputs == 0) return refuse(UNINA_ERR_FORMAT, "engine file lacks the images input buffer");
  if (n_inputs > 1) return refuse(UNINA_ERR_FORMAT, "engine file has more than one images input buffer");
  // the decode launch reads num_classes planes of every cls buffer, 4 of every reg buffer, over the head's cell grid
  for (int i = 0; i < 6; ++i) {
    const int at = find_buffer_named(bufs, h.n_buffers, kHeadOutputs[i]);
    if (at < 0) return refuse(UNINA_ERR_FORMAT, "engine file lacks a head output buffer (%s)", kHeadOutputs[i]);
    const BufferDesc& b = bufs[at];
    if (b.dtype != kBufF32Planar) return refuse(UNINA_ERR_FORMAT, "head output %s is not an fp32 planar buffer", kHeadOutputs[i]);
    if (!(i & 1) && b.c != h.num_classes)
      return refuse(UNINA_ERR_FORMAT, "header num_classes differs from the channel count of a cls output buffer");
    if ((i & 1) && b.c != 4) return refuse(UNINA_ERR_FORMAT, "head output %s needs 4 channels", kHeadOutputs[i]);
    const uint64_t s = h.strides[i / 2];
    if (b.h != ((uint64_t)h.in_h + s - 1) / s || b.w != ((uint64_t)h.in_w + s - 1) / s)
      return refuse(UNINA_ERR_FORMAT, "head output %s: map size differs from the input size over its stride", kHeadOutputs[i]);
  }
  return Verdict();
}

inline bool geometry_ok(const OpDesc& d) {
  return d.out_h == conv_out(d.in_h, d.ksize, d.stride) && d.out_w == conv_out(d.in_w, d.ksize, d.stride);
}

inline Verdict check_conv(const FileHeader& h, const BufferDesc* bufs, const OpDesc& d, uint32_t i) {
  const BufferDesc& sb = bufs[d.src_buf];
  if ((d.ksize != 1 && d.ksize != 3) || (d.stride != 1 && d.stride != 2))
    return refuse(UNINA_ERR_UNSUPPORTED, "op %u: conv kernel size %u / stride %u not covered", i, d.ksize, d.stride);
  if (!is_act(sb.dtype)) return refuse(UNINA_ERR_FORMAT, "op %u: source is not an activation buffer", i);
  const uint32_t kb = sb.dtype == kBufF32Nhwc ? 16 : (sb.dtype == kBufI8Nhwc ? 64 : 32);
  if (d.cin == 0 || d.cin % kb || ((uint64_t)sb.c * plane_elem_bytes(sb.dtype)) % 16)
    return refuse(UNINA_ERR_UNSUPPORTED, "op %u (%.71s): Cin %% %u != 0", i, d.name, kb);
  if (sb.h != d.in_h || sb.w != d.in_w) return refuse(UNINA_ERR_FORMAT, "op table: source slice outside buffer (op %u: input size)", i);
  if (!geometry_ok(d)) return refuse(UNINA_ERR_FORMAT, "op %u: output size does not follow from input size, kernel and stride", i);
  uint64_t ntot = 0;
  for (uint32_t s = 0; s < d.nseg; ++s) {
    const SegDesc& sd = d.seg[s];
    const BufferDesc& db = bufs[sd.dst_buf];
    if ((uint64_t)sd.src_coff + d.cin > sb.c) return refuse(UNINA_ERR_FORMAT, "op table: source slice outside buffer (op %u)", i);
    if (((uint64_t)sd.src_coff * plane_elem_bytes(sb.dtype)) % 16)   // the kernels fetch a pixel's channels in 16-byte chunks
      return refuse(UNINA_ERR_UNSUPPORTED, "op %u: source slice is not 16-byte aligned", i);
    if (sd.n_count == 0 || sd.n_pad != (((uint64_t)sd.n_count + 15) & ~15ull))
      return refuse(UNINA_ERR_FORMAT, "op %u: n_pad is not n_count rounded up to 16", i);
    if (sd.m_off && (sd.m_off % 16 || !inside(sd.m_off, (uint64_t)sd.n_pad * 4, h.blob_bytes)))
      return refuse(UNINA_ERR_FORMAT, "op table: multiplier offset outside blob (op %u)", i);
    if (sd.w_off % 16 || sd.b_off % 16 || !inside(sd.w_off, conv_weight_bytes(d, sd, sb.dtype), h.blob_bytes) ||
        !inside(sd.b_off, (uint64_t)sd.n_pad * 4, h.blob_bytes))
      return refuse(UNINA_ERR_FORMAT, "op table: weight offset outside blob (op %u)", i);
    if (sb.dtype == kBufI8Nhwc && !sd.m_off) return refuse(UNINA_ERR_FORMAT, "op %u: int8 conv without multipliers", i);
    if (sd.flags & kSegPlanarF32) {
      if (db.dtype != kBufF32Planar) return refuse(UNINA_ERR_FORMAT, "op %u: planar slice into non-planar buffer", i);
    } else {
      const uint32_t al = db.dtype == kBufI8Nhwc ? 16 : 8;   // a 16-byte store chunk must not straddle the slice
      if (!is_act(db.dtype) || sd.n_count % al || sd.dst_coff % al || db.c % al)
        return refuse(UNINA_ERR_UNSUPPORTED, "op %u: NHWC slice needs channel counts/offsets that are multiples of %u", i, al);
      if ((db.dtype == kBufS16Nhwc) != (sb.dtype == kBufS16Nhwc))
        return refuse(UNINA_ERR_FORMAT, "op %u: split-fp16 conv into a buffer of another type", i);
    }
    const uint64_t mul = (sd.flags & kSegUp2) ? 2 : 1;
    if ((uint64_t)sd.dst_coff + sd.n_count > db.c || db.h != d.out_h * mul || db.w != d.out_w * mul)
      return refuse(UNINA_ERR_FORMAT, "op table: destination slice outside buffer (op %u)", i);
    ntot += sd.n_count;
  }
  if (d.res_buf >= 0) {
    const BufferDesc& rb = bufs[d.res_buf];
    if (!is_act(rb.dtype)) return refuse(UNINA_ERR_FORMAT, "op %u: residual is not an activation buffer", i);
    if ((rb.dtype == kBufS16Nhwc) != (sb.dtype == kBufS16Nhwc))
      return refuse(UNINA_ERR_FORMAT, "op %u: split-fp16 conv with a residual of another type", i);
    if (rb.h != d.out_h || rb.w != d.out_w || d.res_coff < 0 || (uint64_t)d.res_coff + ntot > rb.c)
      return refuse(UNINA_ERR_FORMAT, "op %u: residual slice outside buffer", i);
  }
  return Verdict();
}

inline Verdict check_stem(const FileHeader& h, const BufferDesc* bufs, const OpDesc& d, uint32_t i) {
  const BufferDesc& sb = bufs[d.src_buf];
  const SegDesc& sd = d.seg[0];
  const BufferDesc& db = bufs[sd.dst_buf];
  if (!(sb.flags & kBufInput)) return refuse(UNINA_ERR_FORMAT, "op %u: the stem reads the images input buffer only", i);
  if (d.cin != 3 || d.ksize != 3 || d.stride != 2) return refuse(UNINA_ERR_UNSUPPORTED, "op %u: the stem is a 3x3 stride-2 conv of 3 channels", i);
  if (sb.h != d.in_h || sb.w != d.in_w) return refuse(UNINA_ERR_FORMAT, "op %u: stem input size differs from the images buffer", i);
  if (!geometry_ok(d)) return refuse(UNINA_ERR_FORMAT, "op %u: output size does not follow from input size, kernel and stride", i);
  if (db.dtype != kBufF16Nhwc && db.dtype != kBufF32Nhwc && db.dtype != kBufS16Nhwc)
    return refuse(UNINA_ERR_UNSUPPORTED, "stem output must be fp16, fp32 or split fp16");
  if (sd.n_count == 0 || (uint64_t)sd.dst_coff + sd.n_count > db.c || db.h != d.out_h || db.w != d.out_w)
    return refuse(UNINA_ERR_FORMAT, "op table: destination slice outside buffer (op %u)", i);
  // fp32 [n][27] weights and [n] biases, read as floats on the host (the transposed copy) and on the device
  if (sd.w_off % 16 || sd.b_off % 16 || !inside(sd.w_off, (uint64_t)sd.n_count * 27 * 4, h.blob_bytes) ||
      !inside(sd.b_off, (uint64_t)sd.n_count * 4, h.blob_bytes))
    return refuse(UNINA_ERR_FORMAT, "stem weights out of range");
  return Verdict();
}

inline Verdict check_pool(const BufferDesc* bufs, const OpDesc& d, uint32_t i) {
  const BufferDesc& sb = bufs[d.src_buf];
  if (!is_act(sb.dtype)) return refuse(UNINA_ERR_FORMAT, "op %u: pool on a non-activation buffer", i);
  if (sb.h != d.in_h || sb.w != d.in_w) return refuse(UNINA_ERR_FORMAT, "op %u: pool size differs from its buffer", i);
  // x at [coff, coff + C), y1..y3 written behind it: 4 C channels of the buffer, in 16-byte vectors, 32 channels per workgroup
  const uint64_t esz = plane_elem_bytes(sb.dtype);
  if (d.cin == 0 || d.cin % kPoolChannels || ((uint64_t)d.seg[0].src_coff * esz) % 16 || ((uint64_t)sb.c * esz) % 16)
    return refuse(UNINA_ERR_UNSUPPORTED, "op %u: pool needs channel counts that are multiples of %u and 16-byte aligned slices", i, kPoolChannels);
  if (3ull * sb.w * kPoolChannels * (sb.dtype == kBufS16Nhwc ? 4 : esz) > kPoolLdsBytes)
    return refuse(UNINA_ERR_UNSUPPORTED, "op %u: pool row too wide for the LDS", i);
  if ((uint64_t)d.seg[0].src_coff + 4ull * d.cin > sb.c) return refuse(UNINA_ERR_FORMAT, "op %u: pool slice outside buffer", i);
  return Verdict();
}

inline Verdict check_quant(const BufferDesc* bufs, const OpDesc& d, uint32_t i) {
  const BufferDesc& sb = bufs[d.src_buf];
  const BufferDesc& db = bufs[d.seg[0].dst_buf];
  if (sb.dtype != kBufF16Nhwc || db.dtype != kBufI8Nhwc || sb.c != db.c || sb.h != db.h || sb.w != db.w)
    return refuse(UNINA_ERR_FORMAT, "op %u: QUANT needs an fp16 source and an int8 twin of the same shape", i);
  if (((uint64_t)sb.h * sb.w * sb.c) % 16)   // (below 2^40 elements: check_buffers)
    return refuse(UNINA_ERR_UNSUPPORTED, "op %u: QUANT needs an element count that is a multiple of 16", i);
  return Verdict();
}

}  // namespace validate_detail

// THE validator. `bufs` / `ops`: h.n_buffers / h.n_ops records (read_engine_tables); `blob_present`: bytes of the file behind the
// tables. UNINA_OK: every pointer, leading dimension and offset the loader derives from these tables stays inside the
// blob and the buffers they describe.
inline Verdict validate_engine(const FileHeader& h, const BufferDesc* bufs, const OpDesc* ops, uint64_t blob_present) {
  using namespace validate_detail;
  Verdict v = header_defect(h);
  if (!v.ok()) return v;
  for (int i = 0; i < 3; ++i)
    if (h.strides[i] == 0) return refuse(UNINA_ERR_FORMAT, "header: stride %d is zero", i);
  if (h.in_c != 3 || h.in_h == 0 || h.in_w == 0) return refuse(UNINA_ERR_FORMAT, "header: input must be 3 channels of a non-empty size");
  // the decode reads num_classes planes of every cls buffer; the two-launch NMS carries a class id in 14 bits
  if (h.num_classes == 0 || h.num_classes > kMaxClasses) return refuse(UNINA_ERR_UNSUPPORTED, "num_classes must be 1..16383");
  if (h.blob_bytes > blob_present) return refuse(UNINA_ERR_FORMAT, "truncated weight blob");
  v = check_buffers(h, bufs);
  if (!v.ok()) return v;
  for (uint32_t i = 0; i < h.n_ops; ++i) {
    const OpDesc& d = ops[i];
    if (d.kind != kOpConv && d.kind != kOpStem && d.kind != kOpSppfPool && d.kind != kOpQuant)
      return refuse(UNINA_ERR_UNSUPPORTED, "op %u: kind %u not executable", i, d.kind);
    if (d.src_buf >= h.n_buffers || d.nseg < 1 || d.nseg > 2 || (d.kind != kOpConv && d.nseg != 1) || d.res_buf < -1 ||
        d.res_buf >= (int32_t)h.n_buffers)
      return refuse(UNINA_ERR_FORMAT, "op table: bad buffer index (op %u)", i);
    for (uint32_t s = 0; s < d.nseg; ++s) {
      if (d.seg[s].dst_buf >= h.n_buffers) return refuse(UNINA_ERR_FORMAT, "op table: bad destination buffer (op %u)", i);
      if (bufs[d.seg[s].dst_buf].flags & kBufInput) return refuse(UNINA_ERR_FORMAT, "op %u: writes into the images input buffer", i);
    }
    v = d.kind == kOpConv ? check_conv(h, bufs, d, i)
                          : (d.kind == kOpStem ? check_stem(h, bufs, d, i) : (d.kind == kOpSppfPool ? check_pool(bufs, d, i) : check_quant(bufs, d, i)));
    if (!v.ok()) return v;
  }
  return Verdict();
}

}  // namespace unina

#endif
