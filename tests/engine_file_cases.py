"""Engine files for tests/test_engine_file_cpu.py: a reference model of what unina_load_engine must accept, the files it
must keep accepting, a corpus of damaged files with the verdict each must get, and the single-field sweep.

`defect` states the rules of csrc/engine_validate.h a second time, in Python integers over export._HDR / _BUF / _OP_HEAD /
_SEG: no sum or product here can wrap, which is the point -- the C++ compares 32- and 64-bit fields whose sums do. It is
written from the rule list (header, buffers, every op, conv, stem, pool, quant), each rule from what the kernels read and write:
a conv reads `cin` channels at `src_coff` of every pixel of its source and `n_pad * k * k * cin` weights at `w_off`, the pool
kernel reads C and writes 3 C channels behind them in 16-byte vectors, the decode launch reads num_classes / 4 planes of the
head maps, and so on. Nothing in this module loads the library or touches a device."""
import math
import struct

from unina_yolo_dla_amd import export as X

OK, FORMAT, UNSUPPORTED = 0, 2, 6        # include/unina_mi355.h: UNINA_OK, UNINA_ERR_FORMAT, UNINA_ERR_UNSUPPORTED
HEAD_OUTPUTS = ("p2_cls", "p2_reg", "p3_cls", "p3_reg", "p4_cls", "p4_reg")
ACT = (X.BUF_F16, X.BUF_F32_NHWC, X.BUF_I8, X.BUF_S16)
PLANE_ELEM = {X.BUF_F16: 2, X.BUF_F32_NHWC: 4, X.BUF_I8: 1, X.BUF_S16: 2}      # bytes per element of one plane (addressing)
VALUE_BYTES = {X.BUF_F16: 2, X.BUF_I8: 1}                                      # bytes per stored value (default 4)
WEIGHT_ELEM = {X.BUF_F16: 2, X.BUF_F32_NHWC: 4, X.BUF_I8: 1, X.BUF_S16: 4}

# ---- the layout, field by field: name -> (offset inside the record, width in bytes) -----------------------------------------
HDR_FIELDS = {"version": (8, 4), "precision": (12, 4), "in_c": (16, 4), "in_h": (20, 4), "in_w": (24, 4), "num_classes": (28, 4),
              "n_buffers": (32, 4), "n_ops": (36, 4), "n_heads": (40, 4), "strides0": (44, 4), "strides1": (48, 4), "strides2": (52, 4),
              "blob_bytes": (56, 8), "macs": (64, 8), "model_base_channels": (72, 4)}
BUF_FIELDS = {"h": (0, 4), "w": (4, 4), "c": (8, 4), "dtype": (12, 4), "flags": (16, 4), "scale": (60, 4)}
BUF_NAME_AT, BUF_NAME_LEN = 20, 40
OP_FIELDS = {"kind": (0, 4), "ksize": (4, 4), "stride": (8, 4), "relu": (12, 4), "src_buf": (16, 4), "cin": (20, 4), "res_buf": (24, 4),
             "res_coff": (28, 4), "nseg": (32, 4), "in_h": (36, 4), "in_w": (40, 4), "out_h": (44, 4), "out_w": (48, 4), "in_scale": (52, 4)}
SEG_FIELDS = {"src_coff": (0, 4), "n_count": (4, 4), "n_pad": (8, 4), "dst_buf": (12, 4), "dst_coff": (16, 4), "flags": (20, 4),
              "w_off": (24, 8), "b_off": (32, 8), "w_scale": (40, 4), "out_scale": (44, 4), "m_off": (48, 8)}
HDR, BUF, OPREC, SEG, SEG0_AT = X._HDR.size, X._BUF.size, 256, X._SEG.size, X._OP_HEAD.size
assert (HDR, BUF, SEG, SEG0_AT) == (128, 64, 64, 56)


# ---- the reference model ----------------------------------------------------------------------------------------------
def _inside(off, size, limit):
    return off + size <= limit


def _conv_out(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


def _header_defect(h):
    if h["magic"] != X.MAGIC:
        return FORMAT, "magic"
    if h["version"] != X.VERSION:
        return FORMAT, "version"
    if h["precision"] not in (X.FP16, X.INT8, X.FP32, X.SPLIT):
        return UNSUPPORTED, "precision"
    if h["n_heads"] != 3 or not 1 <= h["n_buffers"] <= 4096 or not 1 <= h["n_ops"] <= 4096:
        return FORMAT, "implausible table sizes"
    return None


def defect(raw, length=None):
    """None if the engine file `raw` (its first `length` bytes) is one unina_load_engine must accept, else (code, fragment of the
    message)."""
    raw = bytes(raw)
    return defect_of(lambda pos, n: raw[pos:pos + n], len(raw) if length is None else length)


def defect_of(read, length):
    """`defect` on a file given as read(pos, n) -> bytes and its length."""
    if length < HDR:
        return FORMAT, "truncated header"
    f = X._HDR.unpack(read(0, HDR))
    h = dict(magic=f[0], version=f[1], precision=f[2], in_c=f[3], in_h=f[4], in_w=f[5], num_classes=f[6], n_buffers=f[7], n_ops=f[8],
             n_heads=f[9], strides=f[10:13], blob_bytes=f[13])
    bad = _header_defect(h)
    if bad:
        return bad
    nb, no = h["n_buffers"], h["n_ops"]
    if HDR + BUF * nb > length:
        return FORMAT, "truncated buffer table"
    if HDR + BUF * nb + OPREC * no > length:
        return FORMAT, "truncated op table"
    braw = read(HDR, BUF * nb)
    oraw = read(HDR + BUF * nb, OPREC * no)
    blob_present = length - (HDR + BUF * nb + OPREC * no)
    for i, s in enumerate(h["strides"]):
        if s == 0:
            return FORMAT, f"stride {i} is zero"
    if h["in_c"] != 3 or h["in_h"] == 0 or h["in_w"] == 0:
        return FORMAT, "header: input"
    if not 1 <= h["num_classes"] <= 16383:
        return UNSUPPORTED, "num_classes"
    if h["blob_bytes"] > blob_present:
        return FORMAT, "truncated weight blob"
    blob = h["blob_bytes"]

    # buffers: (h, w, c, dtype, flags, name, scale)
    bufs = list(X._BUF.iter_unpack(braw))
    inputs = 0
    for bh, bw, bc, dtype, flags, name, scale in bufs:
        if dtype > X.BUF_S16:
            return FORMAT, "unknown dtype"
        if bh == 0 or bw == 0 or bc == 0:
            return FORMAT, "empty extent"
        if bh * bw * bc * VALUE_BYTES.get(dtype, 4) > 1 << 40:
            return FORMAT, "implausible size"
        if b"\0" not in name:
            return FORMAT, "name without terminator"
        if dtype == X.BUF_I8 and not (math.isfinite(scale) and scale > 0):
            return FORMAT, "finite positive scale"
        if flags & X.BUF_INPUT:
            inputs += 1
            if dtype != X.BUF_F32_NCHW_IN or (bc, bh, bw) != (h["in_c"], h["in_h"], h["in_w"]):
                return FORMAT, "images input buffer differs"
    if inputs == 0:
        return FORMAT, "lacks the images input buffer"
    if inputs > 1:
        return FORMAT, "more than one images input buffer"
    names = [b[5].split(b"\0")[0] for b in bufs]
    for i, out in enumerate(HEAD_OUTPUTS):
        if out.encode() not in names:
            return FORMAT, "lacks a head output buffer"
        bh, bw, bc, dtype = bufs[names.index(out.encode())][:4]
        if dtype != X.BUF_F32_PLANAR:
            return FORMAT, "is not an fp32 planar buffer"
        if i % 2 == 0 and bc != h["num_classes"]:
            return FORMAT, "num_classes"
        if i % 2 == 1 and bc != 4:
            return FORMAT, "needs 4 channels"
        s = h["strides"][i // 2]
        if (bh, bw) != (-(-h["in_h"] // s), -(-h["in_w"] // s)):      # graph.py: each stride-2 stage rounds up
            return FORMAT, "map size differs"

    for i in range(no):
        rec = oraw[OPREC * i:OPREC * (i + 1)]
        kind, k, stride, _relu, src_buf, cin, res_buf, res_coff, nseg, in_h, in_w, out_h, out_w, _s = X._OP_HEAD.unpack_from(rec)
        if kind not in (X.OP_CONV, X.OP_STEM, X.OP_SPPF_POOL, X.OP_QUANT):
            return UNSUPPORTED, "not executable"
        if src_buf >= nb or nseg not in (1, 2) or (kind != X.OP_CONV and nseg != 1) or not -1 <= res_buf < nb:
            return FORMAT, "bad buffer index"
        segs = [X._SEG.unpack_from(rec, SEG0_AT + SEG * s) for s in range(nseg)]
        for sg in segs:
            if sg[3] >= nb:
                return FORMAT, "bad destination buffer"
            if bufs[sg[3]][4] & X.BUF_INPUT:
                return FORMAT, "writes into the images input buffer"
        sh, sw, sc, sdt, sflags = bufs[src_buf][:5]
        geometry = k >= 1 and stride >= 1 and (out_h, out_w) == (_conv_out(in_h, k, stride), _conv_out(in_w, k, stride))
        if kind == X.OP_CONV:
            if k not in (1, 3) or stride not in (1, 2):
                return UNSUPPORTED, "not covered"
            if sdt not in ACT:
                return FORMAT, "source is not an activation buffer"
            kb = {X.BUF_F32_NHWC: 16, X.BUF_I8: 64}.get(sdt, 32)
            if cin == 0 or cin % kb or (sc * PLANE_ELEM[sdt]) % 16:
                return UNSUPPORTED, "Cin %"
            if (sh, sw) != (in_h, in_w):
                return FORMAT, "source slice outside buffer"
            if not geometry:
                return FORMAT, "output size does not follow"
            ntot = 0
            for src_coff, n_count, n_pad, dst_buf, dst_coff, flags, w_off, b_off, _ws, _os, m_off in segs:
                dh, dw, dc, ddt = bufs[dst_buf][:4]
                if src_coff + cin > sc:
                    return FORMAT, "source slice outside buffer"
                if (src_coff * PLANE_ELEM[sdt]) % 16:
                    return UNSUPPORTED, "source slice is not 16-byte aligned"
                if n_count == 0 or n_pad != -(-n_count // 16) * 16:
                    return FORMAT, "n_pad is not n_count rounded up"
                if m_off and (m_off % 16 or not _inside(m_off, n_pad * 4, blob)):
                    return FORMAT, "multiplier offset outside blob"
                if w_off % 16 or b_off % 16 or not _inside(w_off, n_pad * k * k * cin * WEIGHT_ELEM[sdt], blob) or \
                        not _inside(b_off, n_pad * 4, blob):
                    return FORMAT, "weight offset outside blob"
                if sdt == X.BUF_I8 and not m_off:
                    return FORMAT, "int8 conv without multipliers"
                if flags & X.SEG_PLANAR_F32:
                    if ddt != X.BUF_F32_PLANAR:
                        return FORMAT, "planar slice into non-planar buffer"
                else:
                    al = 16 if ddt == X.BUF_I8 else 8
                    if ddt not in ACT or n_count % al or dst_coff % al or dc % al:
                        return UNSUPPORTED, "NHWC slice needs"
                    if (ddt == X.BUF_S16) != (sdt == X.BUF_S16):
                        return FORMAT, "split-fp16 conv"
                mul = 2 if flags & X.SEG_UP2 else 1
                if dst_coff + n_count > dc or (dh, dw) != (out_h * mul, out_w * mul):
                    return FORMAT, "destination slice outside buffer"
                ntot += n_count
            if res_buf >= 0:
                rh, rw, rc, rdt = bufs[res_buf][:4]
                if rdt not in ACT:
                    return FORMAT, "residual is not an activation buffer"
                if (rdt == X.BUF_S16) != (sdt == X.BUF_S16):
                    return FORMAT, "split-fp16 conv"
                if (rh, rw) != (out_h, out_w) or res_coff < 0 or res_coff + ntot > rc:
                    return FORMAT, "residual slice outside buffer"
        elif kind == X.OP_STEM:
            src_coff, n_count, n_pad, dst_buf, dst_coff, flags, w_off, b_off, _ws, _os, m_off = segs[0]
            dh, dw, dc, ddt = bufs[dst_buf][:4]
            if not sflags & X.BUF_INPUT:
                return FORMAT, "the stem reads the images input buffer only"
            if (cin, k, stride) != (3, 3, 2):
                return UNSUPPORTED, "the stem is a 3x3 stride-2 conv"
            if (sh, sw) != (in_h, in_w):
                return FORMAT, "stem input size differs"
            if not geometry:
                return FORMAT, "output size does not follow"
            if ddt not in (X.BUF_F16, X.BUF_F32_NHWC, X.BUF_S16):
                return UNSUPPORTED, "stem output must be"
            if n_count == 0 or dst_coff + n_count > dc or (dh, dw) != (out_h, out_w):
                return FORMAT, "destination slice outside buffer"
            if w_off % 16 or b_off % 16 or not _inside(w_off, n_count * 27 * 4, blob) or not _inside(b_off, n_count * 4, blob):
                return FORMAT, "stem weights out of range"
        elif kind == X.OP_SPPF_POOL:
            src_coff = segs[0][0]
            if sdt not in ACT:
                return FORMAT, "pool on a non-activation buffer"
            if (sh, sw) != (in_h, in_w):
                return FORMAT, "pool size differs"
            esz = PLANE_ELEM[sdt]
            if cin == 0 or cin % 32 or (src_coff * esz) % 16 or (sc * esz) % 16:
                return UNSUPPORTED, "pool needs channel counts"
            if 3 * sw * 32 * (4 if sdt == X.BUF_S16 else esz) > 64 * 1024:      # three row buffers of 32 channels in LDS
                return UNSUPPORTED, "pool row too wide"
            if src_coff + 4 * cin > sc:
                return FORMAT, "pool slice outside buffer"
        else:
            dh, dw, dc, ddt = bufs[segs[0][3]][:4]
            if sdt != X.BUF_F16 or ddt != X.BUF_I8 or (sh, sw, sc) != (dh, dw, dc):
                return FORMAT, "QUANT needs"
            if (sh * sw * sc) % 16:
                return UNSUPPORTED, "multiple of 16"
    return None


# ---- a base file, parsed for the cases to find their records ----------------------------------------------------------
class Layout:
    def __init__(self, raw):
        self.raw = bytes(raw)
        f = X._HDR.unpack_from(self.raw)
        self.in_h, self.in_w, self.n_buffers, self.n_ops, self.blob_bytes = f[4], f[5], f[7], f[8], f[13]
        self.buf0 = HDR
        self.op0 = HDR + BUF * self.n_buffers
        self.prefix = self.op0 + OPREC * self.n_ops
        self.bufs = [X._BUF.unpack_from(self.raw, self.buf0 + BUF * i) for i in range(self.n_buffers)]
        self.names = [b[5].split(b"\0")[0].decode() for b in self.bufs]
        self.ops = [X._OP_HEAD.unpack_from(self.raw, self.op0 + OPREC * i) for i in range(self.n_ops)]

    def seg(self, op, s):
        return X._SEG.unpack_from(self.raw, self.op0 + OPREC * op + SEG0_AT + SEG * s)

    def hdr(self, field, value):
        off, width = HDR_FIELDS[field]
        return off, width, value

    def buf(self, i, field, value):
        off, width = BUF_FIELDS[field]
        return self.buf0 + BUF * i + off, width, value

    def op(self, i, field, value):
        off, width = OP_FIELDS[field]
        return self.op0 + OPREC * i + off, width, value & 0xFFFFFFFF

    def sg(self, i, s, field, value):
        off, width = SEG_FIELDS[field]
        return self.op0 + OPREC * i + SEG0_AT + SEG * s + off, width, value

    def first(self, pred):
        return next(i for i, o in enumerate(self.ops) if pred(i, o))

    def first_kind(self, kind):
        return self.first(lambda i, o: o[0] == kind)


def cut(length):
    """The edit that ends the file after `length` bytes."""
    return 0, 0, length


def apply(raw, edits):
    """(edited bytes, length) -- for the reference model and the child that writes real files; small files only."""
    out, length = bytearray(raw), len(raw)
    for off, width, value in edits:
        if width == 0:
            length = value
        else:
            out[off:off + width] = (value & ((1 << (8 * width)) - 1)).to_bytes(width, "little")
    return bytes(out[:length]), length


def pack_cases(base, cases):
    """The input of tests/engine_validate_host.cpp (and of engine_file_child.py): the base file and [(id, edits)]."""
    out = [b"UNEVAL01", struct.pack("<Q", len(base)), base, struct.pack("<Q", len(cases))]
    for cid, edits in cases:
        out.append(struct.pack("<II", cid, len(edits)))
        out += [struct.pack("<QIQ", off, width, value & 0xFFFFFFFFFFFFFFFF) for off, width, value in edits]
    return b"".join(out)


def defect_edited(lay, edits):
    """`defect` of the base file of `lay` under `edits`, copying the header and the tables only (the sweep's 10^4 cases)."""
    head, length, base = bytearray(lay.raw[:lay.prefix]), len(lay.raw), lay.raw
    for off, width, value in edits:
        if width == 0:
            length = value
        else:
            assert off + width <= lay.prefix
            head[off:off + width] = (value & ((1 << (8 * width)) - 1)).to_bytes(width, "little")
    n = len(head)

    def read(pos, cnt):
        if pos + cnt <= n:
            return bytes(head[pos:pos + cnt])
        return bytes(head[pos:]) + base[max(pos, n):pos + cnt]
    return defect_of(read, length)


# ---- the corpus: name -> (bases it runs on, edits(layout), code, message fragment) ------------------------------------------
def _res_conv(lay):
    return lay.first(lambda i, o: o[0] == X.OP_CONV and o[6] >= 0)


def _up2_conv(lay):
    return lay.first(lambda i, o: o[0] == X.OP_CONV and lay.seg(i, 0)[5] & X.SEG_UP2)


def _i8_conv(lay):
    return lay.first(lambda i, o: o[0] == X.OP_CONV and lay.bufs[o[4]][3] == X.BUF_I8)


def _spare_src_conv(lay):
    """A conv that reads a slice with channels to spare behind it (a concat buffer): its src_coff + 1 stays inside."""
    return lay.first(lambda i, o: o[0] == X.OP_CONV and lay.seg(i, 0)[0] + o[5] < lay.bufs[o[4]][2])


def _other_resolution(lay, op):
    """An activation buffer whose map size differs from op's output."""
    o = lay.ops[op]
    return next(i for i, b in enumerate(lay.bufs) if b[3] in ACT and (b[0], b[1]) != (o[11], o[12]))


def _second_input(lay):
    i = lay.n_buffers - 1          # the last buffer becomes a second images buffer, field for field
    assert not lay.bufs[i][4] & X.BUF_INPUT
    return [lay.buf(i, "h", lay.in_h), lay.buf(i, "w", lay.in_w), lay.buf(i, "c", 3), lay.buf(i, "dtype", X.BUF_F32_NCHW_IN),
            lay.buf(i, "flags", X.BUF_INPUT)]


def _unterminated_name(lay):
    at = lay.buf0 + BUF * (lay.n_buffers - 1) + BUF_NAME_AT
    return [(at + 8 * j, 8, 0x6161616161616161) for j in range(BUF_NAME_LEN // 8)]


ALL = ("fp16", "int8", "strict")
conv0 = lambda lay: lay.first_kind(X.OP_CONV)
stem = lambda lay: lay.first_kind(X.OP_STEM)
pool = lambda lay: lay.first_kind(X.OP_SPPF_POOL)
CORPUS = {
    # the issue's table
    "w_off_wraps": (("fp16",), lambda L: [L.sg(conv0(L), 0, "w_off", 2 ** 64 - 1024)], FORMAT, "weight offset outside blob"),
    "src_coff_wraps": (("fp16",), lambda L: [L.sg(conv0(L), 0, "src_coff", 2 ** 32 - L.ops[conv0(L)][5])], FORMAT, "source slice outside buffer"),
    "src_coff_misaligned": (("fp16",), lambda L: [L.sg(_spare_src_conv(L), 0, "src_coff", L.seg(_spare_src_conv(L), 0)[0] + 1)], UNSUPPORTED, "source slice is not 16-byte aligned"),
    "res_coff_far": (("fp16",), lambda L: [L.op(_res_conv(L), "res_coff", 1 << 20)], FORMAT, "residual slice outside buffer"),
    "res_buf_minus_2": (("fp16",), lambda L: [L.op(_res_conv(L), "res_buf", -2)], FORMAT, "bad buffer index"),
    "pool_src_coff_far": (("fp16",), lambda L: [L.sg(pool(L), 0, "src_coff", 1 << 20)], FORMAT, "pool slice outside buffer"),
    "pool_in_h_x4": (("fp16",), lambda L: [L.op(pool(L), "in_h", 4 * L.ops[pool(L)][9])], FORMAT, "pool size differs"),
    "header_in_h_128": (("fp16",), lambda L: [L.hdr("in_h", 2 * L.in_h)], FORMAT, "images input buffer differs"),
    "stem_out_h_x2": (("fp16",), lambda L: [L.op(stem(L), "out_h", 2 * L.ops[stem(L)][11])], FORMAT, "output size does not follow"),
    "stem_b_off_far": (("fp16",), lambda L: [L.sg(stem(L), 0, "b_off", 1 << 40)], FORMAT, "stem weights out of range"),
    "n_pad_zero": (("fp16",), lambda L: [L.sg(conv0(L), 0, "n_pad", 0)], FORMAT, "n_pad is not n_count rounded up"),
    "stride_zero": (("fp16",), lambda L: [L.op(conv0(L), "stride", 0)], UNSUPPORTED, "not covered"),
    "ksize_5": (("fp16",), lambda L: [L.op(conv0(L), "ksize", 5)], UNSUPPORTED, "not covered"),
    "header_stride_zero": (("fp16",), lambda L: [L.hdr("strides0", 0)], FORMAT, "stride 0 is zero"),
    "p2_reg_fp16": (("fp16",), lambda L: [L.buf(L.names.index("p2_reg"), "dtype", X.BUF_F16)], FORMAT, "is not an fp32 planar buffer"),
    "kind_9": (("fp16",), lambda L: [L.op(conv0(L), "kind", 9)], UNSUPPORTED, "not executable"),
    # found by reading
    "blob_bytes_2_60": (("fp16",), lambda L: [L.hdr("blob_bytes", 2 ** 60)], FORMAT, "truncated weight blob"),
    "dst_coff_wraps": (("fp16",), lambda L: [L.sg(conv0(L), 0, "dst_coff", 2 ** 32 - L.seg(conv0(L), 0)[1])], FORMAT, "destination slice outside buffer"),
    # out_h * 2 of an upsampling store wraps to the buffer's height in 32 bits; the geometry rule sees the op first
    "up2_out_h_wraps": (("fp16",), lambda L: [L.op(_up2_conv(L), "out_h", 2 ** 31 + L.ops[_up2_conv(L)][11])], FORMAT, "output size does not follow"),
    "images_other_size": (("fp16",), lambda L: [L.buf(L.names.index("images"), "h", L.in_h // 2)], FORMAT, "images input buffer differs"),
    "reg_c_5": (("fp16",), lambda L: [L.buf(L.names.index("p3_reg"), "c", 5)], FORMAT, "needs 4 channels"),
    "head_map_size": (("fp16",), lambda L: [L.buf(L.names.index("p4_cls"), "h", L.bufs[L.names.index("p4_cls")][0] + 1)], FORMAT, "map size differs"),
    "two_inputs": (("fp16",), _second_input, FORMAT, "more than one images input buffer"),
    "pool_nseg_2": (("fp16",), lambda L: [L.op(pool(L), "nseg", 2)], FORMAT, "bad buffer index"),
    "conv_into_input": (("fp16",), lambda L: [L.sg(conv0(L), 0, "dst_buf", L.names.index("images"))], FORMAT, "writes into the images input buffer"),
    "res_other_resolution": (("fp16",), lambda L: [L.op(_res_conv(L), "res_buf", _other_resolution(L, _res_conv(L)))], FORMAT, "residual slice outside buffer"),
    "m_off_past_blob": (ALL, lambda L: [L.sg(conv0(L), 0, "m_off", (L.blob_bytes + 15) & ~15)], FORMAT, "multiplier offset outside blob"),
    "name_unterminated": (("fp16",), _unterminated_name, FORMAT, "name without terminator"),
    "cut_mid_header": (("fp16",), lambda L: [cut(HDR // 2)], FORMAT, "truncated header"),
    "cut_mid_buffer_table": (("fp16",), lambda L: [cut(L.buf0 + BUF * 3 + 10)], FORMAT, "truncated buffer table"),
    "cut_mid_op_table": (("fp16",), lambda L: [cut(L.op0 + OPREC * 5 + 100)], FORMAT, "truncated op table"),
    "cut_first_blob_byte": (("fp16",), lambda L: [cut(L.prefix)], FORMAT, "truncated weight blob"),
    "cut_last_blob_byte": (("fp16",), lambda L: [cut(len(L.raw) - 1)], FORMAT, "truncated weight blob"),
    # int8 and split-fp16 fields
    "i8_m_off_zero": (("int8",), lambda L: [L.sg(_i8_conv(L), 0, "m_off", 0)], FORMAT, "int8 conv without multipliers"),
    "i8_scale_zero": (("int8",), lambda L: [L.buf(L.ops[_i8_conv(L)][4], "scale", 0)], FORMAT, "finite positive scale"),
    "i8_scale_nan": (("int8",), lambda L: [L.buf(L.ops[_i8_conv(L)][4], "scale", 0x7FC00000)], FORMAT, "finite positive scale"),
    "quant_onto_itself": (("int8",), lambda L: [L.sg(L.first_kind(X.OP_QUANT), 0, "dst_buf", L.ops[L.first_kind(X.OP_QUANT)][4])], FORMAT, "QUANT needs"),
    "strict_res_fp16": (("strict",), lambda L: [L.buf(L.ops[_res_conv(L)][6], "dtype", X.BUF_F16)], FORMAT, "split-fp16 conv"),
}


# ---- the sweep: every numeric field of the header and of every buffer, op and seg record ---------------------------------
# Fields no rule mentions (no kernel address, extent or launch shape depends on them): every swept value of them must be accepted.
UNRULED = {"hdr.macs", "hdr.model_base_channels", "op.relu", "op.in_scale", "seg.w_scale", "seg.out_scale",
           # ruled for int8 buffers only, which an fp16 base does not have (the corpus holds it on the int8 base)
           "buf.scale"}


def sweep(lay):
    """[(field label, (offset, width, value))]: each field set to 0, 1, v + 1, 2 v, 2^31 - 1, 2^32 - 1 and, 64-bit fields,
    2^64 - 1024 -- without the values that leave it unchanged. Seg records an op does not use (nseg = 1) are swept too."""
    out = []

    def field(label, at, width):
        v = int.from_bytes(lay.raw[at:at + width], "little")
        mask = (1 << (8 * width)) - 1
        vals = [0, 1, v + 1, 2 * v, 2 ** 31 - 1, 2 ** 32 - 1] + ([2 ** 64 - 1024] if width == 8 else [])
        for x in dict.fromkeys(x & mask for x in vals):
            if x != v:
                out.append((label, (at, width, x)))
    for name, (off, width) in HDR_FIELDS.items():
        field("hdr." + name, off, width)
    for i in range(lay.n_buffers):
        for name, (off, width) in BUF_FIELDS.items():
            field("buf." + name, lay.buf0 + BUF * i + off, width)
    for i in range(lay.n_ops):
        for name, (off, width) in OP_FIELDS.items():
            field("op." + name, lay.op0 + OPREC * i + off, width)
        for s in range(2):
            for name, (off, width) in SEG_FIELDS.items():
                field("seg." + name, lay.op0 + OPREC * i + SEG0_AT + SEG * s + off, width)
    return out


# ---- the files the exporter writes for what the suite builds ------------------------------------------------------------
PRECISIONS = {"fp16": X.FP16, "fp32": X.FP32, "strict": X.STRICT, "int8": X.INT8}


def unit_ranges(sd, g):
    """Activation ranges for an INT8 export where only the TABLES matter (the ranges set scales, never a shape, a type or an
    offset): 1.0 for every buffer."""
    return {b[0]: 1.0 for b in X.EngineBuilder(sd, g).buffers}
