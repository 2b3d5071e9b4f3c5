"""Engine builder: state_dict of graph (A) or (B) (graph.py)  ->  .une engine file for libunina_mi355.so.

Plays the role of the reference's ``export_trt.py::export_pipeline`` (export_trt.py:497-566:
ONNX export -> TensorRT build -> serialized plan) for the MI355X engine. Instead of an opaque plan
the output is an explicit table of FUSED ops over NHWC fp16 activation buffers. The table is DERIVED from graph.py's node
list (EngineBuilder._lower walks Graph.blocks; layer names, widths, strides and concat orders are written only there);
what this module adds are the fusion rules, each decided by a node's kind and users:

* BatchNorm (eval) is folded into the conv:  W' = W*g/sqrt(var+eps),  b' = beta - mean*g/sqrt(var+eps)
  (model.py:41-50; eps = 1e-5); ReLU is an epilogue flag.
* every ``torch.cat`` (model.py:110,132,257,260,264,267) becomes a shared buffer: producers write
  channel slices (offset = the channels of the concat's earlier members), the members' other users read them, so concat
  costs nothing.
* C3k2 ``cv1``/``cv2`` (same input, model.py:107-108) and the head's ``cls_branch.0``/``reg_branch.0``
  (same input, model.py:303) are merged into one implicit GEMM with two output slices; the head's
  ``.1`` and ``.2`` layers run as one two-group launch.
* the Bottleneck residual (model.py:73) is added in the 3x3 conv's epilogue, after its ReLU.
* ``Upsample`` (model.py:145-147) is folded into the lateral 1x1 conv's store (each output pixel is
  written to its 2x2 block of the FPN concat buffer).
* the SPPF pool pyramid (model.py:129-131) is ONE op producing y1,y2,y3 into the 4-way concat buffer.

Graph (A): 67 reference convs -> 50 conv ops + stem + pool = 52 ops; graph (B): 74 -> 56 + stem + pool = 58.
"""
from __future__ import annotations

import math
import os
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from .graph import Graph, OUTPUT_NAMES, STRIDES

MAGIC = b"UNINAENG"
VERSION = 3
FP16, INT8, FP32, SPLIT = 0, 1, 2, 3
STRICT = SPLIT            # the precision mode that meets the north-star tolerance on every detection at fp16-MFMA speed
BUF_F16, BUF_F32_PLANAR, BUF_F32_NCHW_IN, BUF_I8, BUF_F32_NHWC, BUF_S16 = 0, 1, 2, 3, 4, 5
BUF_INPUT, BUF_OUTPUT = 1, 2
OP_CONV, OP_STEM, OP_SPPF_POOL, OP_UPSAMPLE, OP_QUANT = 1, 2, 3, 4, 5
SEG_UP2, SEG_PLANAR_F32 = 1, 2
BN_EPS = 1e-5

_HDR = struct.Struct("<8sII3II2II3IQQI52x")   # last word: base_channels of a narrower embedded model (0 = none)
_BUF = struct.Struct("<3III40sf")
_SEG = struct.Struct("<6IQQffQ8x")
_OP_HEAD = struct.Struct("<4I2I2iI4If")
assert _HDR.size == 128 and _BUF.size == 64 and _SEG.size == 64 and _OP_HEAD.size == 56


@dataclass
class View:
    buf: int
    coff: int
    c: int


@dataclass
class Seg:
    module: str               # reference module path whose weights this slice carries
    src_coff: int
    n_count: int
    dst: View
    flags: int = 0
    w_off: int = 0
    b_off: int = 0
    n_pad: int = 0
    # raw parameters (filled by the emitters, serialised by EngineBuilder._finalize)
    w_raw: Optional[np.ndarray] = None      # [n, K] fp64, K = (kh,kw,cin), UNFOLDED conv weight
    fold: Optional[np.ndarray] = None       # [n] fp64: gamma/sqrt(var+eps) (1 for convs without BN)
    bias: Optional[np.ndarray] = None       # [n] fp64: beta - mean*fold (or the conv bias)
    bn: bool = True
    m_off: int = 0                          # int8 convs: blob offset of the per-channel multiplier
    w_scale: float = 1.0


@dataclass
class Op:
    kind: int
    name: str
    src_buf: int
    cin: int
    k: int = 1
    s: int = 1
    relu: int = 1
    res: Optional[View] = None
    in_hw: Tuple[int, int] = (0, 0)
    out_hw: Tuple[int, int] = (0, 0)
    segs: List[Seg] = field(default_factory=list)


_SWZ_G = (0, 2, 3, 1)


def pack_weights(wk: np.ndarray) -> np.ndarray:
    """[n_pad][K] fp16 or fp32 (K = (kh,kw,cin), n_pad % 16 == 0) -> the LDS image the conv kernel DMA-loads:
    1-KiB blocks [n_pad/16][K/kb], each 64 slots x 16 bytes with slot(r, c) = 4*r + (c ^ G[r>>2]), G = (0,2,3,1)
    (conv_igemm.hip: conflict-free ds_read_b128 fragment reads). A 16-byte chunk is 8 halfs / 4 floats, so a block
    spans kb = 32 (fp16) or 16 (fp32) values of k."""
    n_pad, K = wk.shape
    ce = 16 // wk.dtype.itemsize
    kb = 4 * ce
    assert n_pad % 16 == 0 and K % kb == 0, (n_pad, K)
    blk = wk.reshape(n_pad // 16, 16, K // kb, 4, ce).transpose(0, 2, 1, 3, 4)       # [nsub][kblk][r][c][ce]
    out = np.empty_like(blk)
    for r in range(16):
        for c in range(4):
            out[:, :, r, c ^ _SWZ_G[r >> 2]] = blk[:, :, r, c]
    return np.ascontiguousarray(out).reshape(-1)


def pack_weights_split(hi: np.ndarray, lo: np.ndarray) -> np.ndarray:
    """SPLIT engines: two [n_pad][K] fp16 matrices (w = hi + lo) -> pairs of 1-KiB fragment blocks [n_pad/16][K/32][hi | lo],
    each block in pack_weights' image: the kernels fetch a k block's hi and lo fragments from adjacent blocks."""
    n_pad, K = hi.shape
    nblk = (n_pad // 16) * (K // 32)
    out = np.empty((nblk, 2, 512), dtype=np.float16)
    out[:, 0] = pack_weights(hi).reshape(nblk, 512)
    out[:, 1] = pack_weights(lo).reshape(nblk, 512)
    return out.reshape(-1)


def unpack_weights_split(packed: np.ndarray, n_pad: int, K: int) -> np.ndarray:
    """Inverse of pack_weights_split: the fp32 values hi + lo, [n_pad][K] (tests / emulator)."""
    blk = packed.reshape(-1, 2, 512)
    hi = unpack_weights(np.ascontiguousarray(blk[:, 0]).reshape(-1), n_pad, K)
    lo = unpack_weights(np.ascontiguousarray(blk[:, 1]).reshape(-1), n_pad, K)
    return hi.astype(np.float32) + lo.astype(np.float32)


def unpack_weights(packed: np.ndarray, n_pad: int, K: int) -> np.ndarray:
    """Inverse of pack_weights (tests / emulator)."""
    ce = 16 // packed.dtype.itemsize
    blk = packed.reshape(n_pad // 16, K // (4 * ce), 16, 4, ce)
    out = np.empty_like(blk)
    for r in range(16):
        for c in range(4):
            out[:, :, r, c] = blk[:, :, r, c ^ _SWZ_G[r >> 2]]
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3, 4)).reshape(n_pad, K)


def bn_terms(sd: Dict[str, np.ndarray], module: str):
    """ConvBlock -> (W [O,C,k,k] fp64 unfolded, f [O] = gamma/sqrt(var+eps), b' [O] = beta - mean*f)."""
    w = sd[f"{module}.conv.weight"].astype(np.float64)
    g = sd[f"{module}.bn.weight"].astype(np.float64)
    b = sd[f"{module}.bn.bias"].astype(np.float64)
    m = sd[f"{module}.bn.running_mean"].astype(np.float64)
    v = sd[f"{module}.bn.running_var"].astype(np.float64)
    f = g / np.sqrt(v + BN_EPS)
    return w, f, b - m * f


def fold_bn(sd: Dict[str, np.ndarray], module: str):
    """ConvBlock -> (W' [O,C,k,k] fp64, b' [O] fp64)."""
    w, f, b = bn_terms(sd, module)
    return w * f[:, None, None, None], b


# FP16 carve-outs of the reference's QAT recipe (train.py:779, qat.py:700-753): module-path prefixes kept in float
INT8_CARVE_OUT = ("backbone.stem", "backbone.stage1_conv", "head_p2",      # graph (A) module paths
                  "stem", "stage1_conv")                                  # graph (B) (qat.py) module paths


def quantize_sym(x: np.ndarray, scale: float) -> np.ndarray:
    """Per-tensor symmetric int8: clamp(round_half_even(x / scale), -127, 127)   (qat.py:91-126: num_bits=8, axis=None)."""
    return np.clip(np.rint(x / scale), -127, 127).astype(np.int8)


class EngineBuilder:
    def __init__(self, sd: Dict[str, np.ndarray], graph: Optional[Graph] = None, precision: int = FP16,
                 amax: Optional[Dict[str, float]] = None, weight_amax: Optional[Dict[str, float]] = None):
        """precision: FP16 (fp16 weights + activations, v_mfma_f32_16x16x32_f16), FP32 (fp32 everywhere,
        v_mfma_f32_16x16x4_f32: meets the north-star tolerance outright at 1/16 of the fp16 matrix rate), SPLIT (= STRICT:
        every folded weight and every stored activation is an fp16 PAIR hi + lo -- ~22 mantissa bits -- and a conv is three
        fp16 MFMAs per k block, hi*hi + hi*lo + lo*hi, into one fp32 accumulator: the tolerance of FP32 at the fp16 rate), or INT8
        (per-tensor symmetric int8 activations AND weights as in qat.py:91-126, v_mfma_i32_16x16x64_i8, with the
        reference's FP16 carve-outs; needs `amax`: buffer name -> calibrated |activation| maximum, see calibrate() or,
        for a QAT checkpoint, amax_from_qat()). `weight_amax`: optional conv module -> weight range from a checkpoint's
        `_weight_quantizer._amax` (default: max |W| of the conv, which is what a max calibrator stores)."""
        if precision not in (FP16, FP32, INT8, SPLIT):
            raise NotImplementedError("precision must be FP16, FP32, INT8 or SPLIT")
        if precision == INT8 and amax is None:
            raise ValueError("INT8 needs calibrated activation ranges (amax): run export.calibrate() first")
        self.sd = sd
        self.precision = precision
        self.amax = amax
        self.weight_amax = weight_amax or {}
        self.wdtype = np.float32 if precision == FP32 else np.float16
        self.act_dtype = BUF_F32_NHWC if precision == FP32 else (BUF_S16 if precision == SPLIT else BUF_F16)
        self.g = graph or Graph()
        self.narrow_base_channels = 0
        if self.g.base_channels % 32:
            # the kernels' K block is 32 channels: a narrower model (model.py:331-333 base_channels=16) is embedded, exactly,
            # in the same topology at the next supported width (statedict.widen_state_dict: zero channels)
            from .statedict import widen_state_dict
            if self.g.base_channels <= 0:
                raise NotImplementedError("base_channels must be positive")
            self.narrow_base_channels = self.g.base_channels
            wide = self.g.base_channels * 32 // math.gcd(self.g.base_channels, 32)
            self.sd, self.g = widen_state_dict(sd, self.g, wide)
        self.buffers: List[list] = []   # [name, h, w, c, dtype, flags, scale]
        self.ops: List[Op] = []
        self.blob = bytearray()
        self._lower()
        if precision == INT8:
            self._quantize_pass()
        self._finalize()

    # ---- tables -------------------------------------------------------------------------------
    def buf(self, name: str, h: int, w: int, c: int, dtype: Optional[int] = None, flags: int = 0) -> int:
        self.buffers.append([name, h, w, c, self.act_dtype if dtype is None else dtype, flags, 1.0])
        return len(self.buffers) - 1

    def view(self, name: str, h: int, w: int, c: int) -> View:
        return View(self.buf(name, h, w, c), 0, c)

    def _hw(self, buf: int) -> Tuple[int, int]:
        return self.buffers[buf][1], self.buffers[buf][2]

    def _blob_add(self, arr: np.ndarray) -> int:
        pad = (-len(self.blob)) % 256
        self.blob += b"\0" * pad
        off = len(self.blob)
        self.blob += arr.tobytes()
        return off

    # ---- where a node's tensor lives: self.at[node index] = View -------------------------------------
    def _share(self, name: str, members: List[int]) -> int:
        """One buffer holding several nodes' tensors side by side, in the listed order: a concat (its producers write
        channel slices, its members' other users read them) or the merged outputs of sibling convs."""
        nodes = [self.g.nodes[i] for i in members]
        b = self.buf(name, nodes[0].h, nodes[0].w, sum(n.c for n in nodes))
        off = 0
        for n in nodes:
            assert n.idx not in self.at, n.name
            self.at[n.idx] = View(b, off, n.c)
            off += n.c
        return b

    def _cat(self, i: int):
        n = self.g.nodes[i]
        self.at[i] = View(self._share(n.name, n.srcs), 0, n.c)

    def _own(self, i: int, name: str):
        """A buffer of its own for node i, unless a concat already holds it."""
        n = self.g.nodes[i]
        if i not in self.at:
            self.at[i] = self.view(name, n.h, n.w, n.c)

    # ---- op emitters ---------------------------------------------------------------------------
    def _conv(self, idxs):
        """Sibling conv nodes (inputs in one buffer, same geometry) -> one launch, one output slice each. A conv whose only
        user is an `add` (Bottleneck shortcut) or an `up2` stores that node's tensor: the shortcut is the op's `res`,
        added after the ReLU; the upsample is the SEG_UP2 store into the slice the `up2` owns in its concat."""
        nodes = self.g.nodes
        first = nodes[idxs[0]]
        if first.srcs[0] < 0:
            return self._stem(first)
        cin, k, s, bn = first.cin, first.k, first.s, first.kind == "conv"
        src_buf = self.at[first.srcs[0]].buf
        op = Op(OP_CONV, "+".join(nodes[i].name for i in idxs), src_buf, cin, k, s, int(bn), None,
                self._hw(src_buf), (first.h, first.w))
        for n in (nodes[i] for i in idxs):
            module, src, out, flags = n.name, self.at[n.srcs[0]], n, 0
            assert (src.buf, n.kind, n.cin, n.k, n.s, n.h, n.w) == (src_buf, first.kind, cin, k, s, first.h, first.w), module
            users = [nodes[u] for u in n.users]
            if [u.kind for u in users] == ["add"]:
                out = users[0]
                op.res = self.at[next(x for x in out.srcs if x != n.idx)]
            elif [u.kind for u in users] == ["up2"]:
                out, flags = users[0], SEG_UP2
            self._own(out.idx, out.name)
            dst = self.at[out.idx]
            if self.buffers[dst.buf][4] == BUF_F32_PLANAR:
                flags |= SEG_PLANAR_F32
            if bn:
                w, f, b = bn_terms(self.sd, module)
            else:
                w = self.sd[f"{module}.weight"].astype(np.float64)
                b = self.sd[f"{module}.bias"].astype(np.float64)
                f = np.ones_like(b)
            assert w.shape == (n.c, cin, k, k), (module, w.shape, n.c, cin, k)
            assert self._hw(dst.buf) == (out.h, out.w) and dst.c == n.c, (module, self._hw(dst.buf), dst.c)
            seg = Seg(module, src.coff, n.c, dst, flags, n_pad=-(-n.c // 16) * 16)
            seg.w_raw = np.transpose(w, (0, 2, 3, 1)).reshape(n.c, k * k * cin)      # [O][(kh,kw,C)]
            seg.fold, seg.bias, seg.bn = f, b, bn
            op.segs.append(seg)
        self.ops.append(op)

    def _stem(self, n):
        """The conv that reads the network input: its own op kind, folded fp32 weights [O][(c,kh,kw)]."""
        images = self.at[-1].buf
        self._own(n.idx, n.name)
        w, b = fold_bn(self.sd, n.name)
        op = Op(OP_STEM, n.name, images, n.cin, n.k, n.s, 1, None, self._hw(images), (n.h, n.w))
        seg = Seg(n.name, 0, n.c, self.at[n.idx], 0, n_pad=n.c)
        seg.w_raw, seg.fold, seg.bias = w.reshape(n.c, -1), np.ones(n.c), b
        op.segs.append(seg)
        self.ops.append(op)

    # ---- lowering rules, one per graph.Block kind -------------------------------------------------------
    def conv(self, blk):
        self._conv(blk.nodes)

    def c3k2(self, blk):
        """C3k2 (model.py:76-110) -> 2 + 2n launches: cv1+cv2, per Bottleneck cv1 and cv2(+shortcut), cv3."""
        cv1, cv2, *bottlenecks, cat, cv3 = blk.nodes
        self._own(cv3, blk.label or blk.name)
        self._cat(cat)
        self._conv([cv1, cv2])
        for i in bottlenecks:
            if self.g.nodes[i].kind == "conv":
                self._conv([i])
        self._conv([cv3])

    def head(self, blk):
        """DetectionHead (model.py:274-303; qat.py:411-440) -> 3 launches (both branches per launch)."""
        pairs = list(zip(blk.nodes[:3], blk.nodes[3:]))                  # (cls.i, reg.i)
        for j, pair in enumerate(pairs[:-1]):                            # the .2 pair writes the outputs
            self._share(f"{blk.name}.h{j}", pair)
        for pair in pairs:
            self._conv(pair)

    def sppf(self, blk):
        """SPPF_DLA (model.py:113-132; qat.py:328-345): cv1 -> ONE pool op (y1,y2,y3) -> cv2 over the 4-way concat."""
        cv1, *pools, cat, cv2 = blk.nodes
        src = self.at[self.g.nodes[cv1].srcs[0]]
        if src.c == self.buffers[src.buf][3]:
            # buffer ORDER is part of the engine file (the activation arena is laid out in it), and the two graphs' SPPFs
            # have always differed in it: one that reads a buffer of its own (graph B) gets its destination first, like a
            # C3k2; one that reads a concat slice (graph A: the pre-SPPF P4 also feeds the PAN) gets it after its concat
            self._own(cv2, blk.name)
        self._cat(cat)
        self._conv([cv1])
        x, y, p = self.at[cv1], [self.at[i] for i in pools], self.g.nodes[pools[0]]
        pool = Op(OP_SPPF_POOL, f"{blk.name}.pool1+pool2+pool3", x.buf, x.c, p.k, p.s, 0, None, (p.h, p.w), (p.h, p.w))
        pool.segs.append(Seg(f"{blk.name}.pool", x.coff, sum(v.c for v in y), View(x.buf, y[0].coff, sum(v.c for v in y))))
        self.ops.append(pool)
        self._own(cv2, blk.name)
        self._conv([cv2])

    def _lower(self):
        """Graph -> buffers + fused ops. The network's input, outputs and network-level concats get their buffers first (a
        concat's members are produced long before it); then every block, in forward order, by the rule of its kind."""
        g = self.g
        self.at: Dict[int, View] = {-1: View(self.buf("images", g.in_h, g.in_w, 3, BUF_F32_NCHW_IN, BUF_INPUT), 0, 3)}
        for name, n in zip(OUTPUT_NAMES, (g.nodes[i] for i in g.outputs)):
            self.at[n.idx] = View(self.buf(name, n.h, n.w, n.c, BUF_F32_PLANAR, BUF_OUTPUT), 0, n.c)
        inner = {i for blk in g.blocks for i in blk.nodes}
        for n in g.nodes:
            if n.kind == "cat" and n.idx not in inner:
                self._cat(n.idx)
        for blk in g.blocks:
            getattr(self, blk.kind)(blk)

    # ---- INT8 pass (generic over the op table) ----------------------------------------------------
    def _quantize_pass(self):
        """Decides, per op, int8 or fp16 execution and, per buffer, int8 or fp16 storage.

        * an op runs in int8 iff it is a BN conv of a module outside the reference's FP16 carve-outs
          (train.py:779) whose Cin is a multiple of the int8 MFMA block (64). The head's output convs are plain
          nn.Conv2d in the reference's QAT graph (qat.py:416,421: unquantised) -> fp16.
        * precision is a per-layer builder choice, as in the reference's TensorRT build (export_trt.py:432-441 sets
          the INT8 flag without precision constraints, so the builder keeps a layer in float where that is faster):
          a C3k2 block whose bottlenecks cannot be int8 (hidden width 32 < one int8 MFMA block) runs in fp16 as a
          whole -- alternating types inside it costs more than int8 saves and loses the one-launch block kernel --
          and so does a conv that shares a multi-writer concat buffer with fp16 readers (an int8 twin of a buffer
          that is written in several places would need several QUANT passes).
        * a buffer is int8 iff every op that reads it as an INPUT is int8 (the SPPF pool is type-agnostic); a
          buffer with mixed readers stays fp16 and gets an int8 twin filled by one QUANT op.
        * scales: activations s = amax/127 per BUFFER (a concat buffer has one scale: its consumer conv has one
          input quantizer, qat.py:245-248); weights s_w = max|W|/127 per conv on the UNFOLDED weight (BN stays a
          float per-channel multiplier, qat.py:225-260)."""
        def seg_q(seg):
            return seg.bn and not any(seg.module.startswith(c) for c in INT8_CARVE_OUT)
        self.op_int8 = [op.kind == OP_CONV and op.cin % 64 == 0 and all(seg_q(sg) for sg in op.segs) for op in self.ops]
        nbuf = len(self.buffers)
        readers = {b: [] for b in range(nbuf)}
        writers = {b: set() for b in range(nbuf)}
        for i, op in enumerate(self.ops):
            if op.kind == OP_CONV:
                readers[op.src_buf].append(i)
            for sg in op.segs:
                writers[sg.dst.buf].add(i)
        narrow = {sg.module.split(".bottlenecks.")[0] + "." for op in self.ops if op.kind == OP_CONV and op.cin % 64
                  for sg in op.segs if ".bottlenecks." in sg.module and seg_q(sg)}
        for i, op in enumerate(self.ops):
            if self.op_int8[i] and any(sg.module.startswith(n) for sg in op.segs for n in narrow):
                self.op_int8[i] = False
        changed = True
        while changed:
            changed = False
            for b in range(nbuf):
                qs = [self.op_int8[i] for i in readers[b]]
                if len(writers[b]) > 1 and any(qs) and not all(qs):
                    for i in readers[b]:
                        self.op_int8[i] = False
                    changed = True
        new_ops: List[Op] = []
        twin_of: Dict[int, int] = {}
        for b in range(nbuf):
            name, h, w, c, dtype, flags, _ = self.buffers[b]
            if dtype != BUF_F16 or not readers[b]:
                continue
            qs = [self.op_int8[i] for i in readers[b]]
            if all(qs):
                self.buffers[b][4] = BUF_I8
                self.buffers[b][6] = self._scale_of(name)
            elif any(qs):                                   # mixed readers: int8 twin
                t = self.buf(name + ".q8", h, w, c, BUF_I8)
                self.buffers[t][6] = self._scale_of(name)
                twin_of[b] = t
        # re-point int8 readers to the twins and schedule the QUANT ops after the last writer of the original
        for b, t in twin_of.items():
            for i in readers[b]:
                if self.op_int8[i]:
                    self.ops[i].src_buf = t
        last_writer = {}
        for i, op in enumerate(self.ops):
            for sg in op.segs:
                if sg.dst.buf in twin_of:
                    last_writer[sg.dst.buf] = i
        out_ops, out_q = [], []
        for i, op in enumerate(self.ops):
            out_ops.append(op)
            out_q.append(self.op_int8[i])
            for b, t in twin_of.items():
                if last_writer.get(b) == i:
                    name, h, w, c = self.buffers[b][:4]
                    q = Op(OP_QUANT, f"quant({name})", b, c, 1, 1, 0, None, (h, w), (h, w))
                    q.segs.append(Seg("quant", 0, c, View(t, 0, c)))
                    out_ops.append(q)
                    out_q.append(False)
        self.ops, self.op_int8 = out_ops, out_q

    def _scale_of(self, buffer_name: str) -> float:
        if buffer_name not in self.amax:
            raise KeyError(f"no calibrated range for buffer '{buffer_name}'")
        return max(float(self.amax[buffer_name]), 1e-8) / 127.0

    # ---- blob -----------------------------------------------------------------------------------
    def _finalize(self):
        for i, op in enumerate(self.ops):
            if op.kind == OP_STEM:
                sg = op.segs[0]
                sg.w_off = self._blob_add(sg.w_raw.astype(np.float32))
                sg.b_off = self._blob_add(sg.bias.astype(np.float32))
            if op.kind != OP_CONV:
                continue
            int8 = self.precision == INT8 and self.op_int8[i]
            in_scale = self.buffers[op.src_buf][6]
            for sg in op.segs:
                K = sg.w_raw.shape[1]
                bk = np.zeros((sg.n_pad,), dtype=np.float32)
                bk[:sg.n_count] = sg.bias.astype(np.float32)
                if int8:
                    sg.w_scale = max(float(self.weight_amax.get(sg.module, np.abs(sg.w_raw).max())), 1e-12) / 127.0
                    wk = np.zeros((sg.n_pad, K), dtype=np.int8)
                    wk[:sg.n_count] = quantize_sym(sg.w_raw, sg.w_scale)
                    mk = np.zeros((sg.n_pad,), dtype=np.float32)
                    mk[:sg.n_count] = (in_scale * sg.w_scale * sg.fold).astype(np.float32)
                    sg.w_off = self._blob_add(pack_weights(wk))
                    sg.m_off = self._blob_add(mk)
                elif self.precision == SPLIT:
                    wf = sg.w_raw * sg.fold[:, None]                                     # fp64 folded weights
                    hi = np.zeros((sg.n_pad, K), dtype=np.float16)
                    lo = np.zeros((sg.n_pad, K), dtype=np.float16)
                    hi[:sg.n_count] = wf.astype(np.float16)
                    lo[:sg.n_count] = (wf - hi[:sg.n_count].astype(np.float64)).astype(np.float16)
                    sg.w_off = self._blob_add(pack_weights_split(hi, lo))
                else:
                    wk = np.zeros((sg.n_pad, K), dtype=self.wdtype)
                    wk[:sg.n_count] = (sg.w_raw * sg.fold[:, None]).astype(self.wdtype)
                    sg.w_off = self._blob_add(pack_weights(wk))
                sg.b_off = self._blob_add(bk)

    # ---- serialisation --------------------------------------------------------------------------
    def tobytes(self) -> bytes:
        g = self.g
        out = bytearray()
        out += _HDR.pack(MAGIC, VERSION, self.precision, 3, g.in_h, g.in_w, g.num_classes, len(self.buffers), len(self.ops),
                         3, *STRIDES, len(self.blob), g.macs(), self.narrow_base_channels)
        for name, h, w, c, dtype, flags, scale in self.buffers:
            out += _BUF.pack(h, w, c, dtype, flags, name.encode()[:39], scale)
        for op in self.ops:
            rec = bytearray(_OP_HEAD.pack(op.kind, op.k, op.s, op.relu, op.src_buf, op.cin,
                                          op.res.buf if op.res else -1, op.res.coff if op.res else 0,
                                          len(op.segs), op.in_hw[0], op.in_hw[1], op.out_hw[0], op.out_hw[1],
                                          float(self.buffers[op.src_buf][6])))
            for i in range(2):
                if i < len(op.segs):
                    s = op.segs[i]
                    rec += _SEG.pack(s.src_coff, s.n_count, s.n_pad, s.dst.buf, s.dst.coff, s.flags,
                                     s.w_off, s.b_off, s.w_scale, float(self.buffers[s.dst.buf][6]), s.m_off)
                else:
                    rec += b"\0" * _SEG.size
            rec += op.name.encode()[:71].ljust(72, b"\0")
            assert len(rec) == 256
            out += rec
        out += self.blob
        return bytes(out)

    def save(self, path: str) -> None:
        with open(path, "wb") as f:
            f.write(self.tobytes())


class HistogramCalibrator:
    """Per-tensor |x| histogram + range selection, the role of pytorch-quantization's ``HistogramCalibrator`` that the
    reference configures for activations AND weights (qat.py:91-126: ``QuantDescriptor(num_bits=8, calib_method="histogram",
    axis=None)``; its docstring calls it "Histogram (Entropy) calibration"). That library is not available here and the
    reference holds no calibrated value, so this is the build's OWN restatement of the published algorithm (parity
    unpinned): 2048 bins of |x| whose range grows by whole bins when a later batch exceeds it; then one of
      * ``entropy``    -- the threshold (from bin 128 on) whose 128-level re-quantised distribution has the smallest
                          KL divergence from the clipped original (the TensorRT-style entropy calibration);
      * ``mse``        -- the threshold whose int8 fake-quantisation of the bin centres has the smallest count-weighted
                          squared error;
      * ``percentile`` -- the |x| below which `percentile` percent of the values lie."""

    def __init__(self, num_bins: int = 2048):
        self.num_bins = num_bins
        self.hist: Optional[np.ndarray] = None
        self.edges: Optional[np.ndarray] = None

    def collect(self, x: np.ndarray) -> None:
        self._fold(np.abs(np.asarray(x, dtype=np.float32)).reshape(-1), None)

    def collect_counts(self, counts: np.ndarray) -> None:
        """Folds one frame given as its |x| value-count table (CALIB_BINS entries: how many elements carry each 15-bit
        fp16 pattern, Engine.calib_counts / unina_abs_histogram_f16) exactly as `collect` folds the frame's tensor: the
        values are the fp16 numbers of the non-empty patterns as float32, each weighted by its count, through the same
        np.histogram calls, restart and growth rules. Counts are integers below 2^53, so the float64 weighted sums are
        exact and hist / edges come out bit-identical. A non-finite pattern (Inf / NaN, 0x7c00 and above) with a count
        raises ValueError."""
        a, w = pattern_values(counts)
        self._fold(a, w)

    def _fold(self, a: np.ndarray, weights: Optional[np.ndarray]) -> None:
        """a: |x| values, float32, flat; weights: None (every value once) or a float64 count per value."""
        amax = float(a.max()) if a.size else 0.0
        if self.hist is not None and self.edges[-1] <= 1e-6 and amax > self.edges[-1]:
            # everything seen so far was (numerically) zero -- a dead buffer on the first frames: its range (0, 1e-8) must not be
            # GROWN by whole bins (1e12 of them for an ordinary activation); start over from this batch, the zeros go to bin 0
            zeros = float(self.hist.sum())
            self.hist = None
        else:
            zeros = 0.0
        if self.hist is None:
            amax = max(amax, 1e-8)
            self.hist, self.edges = np.histogram(a, bins=self.num_bins, range=(0.0, amax), weights=weights)
            self.hist = self.hist.astype(np.float64)
            self.hist[0] += zeros
            return
        if amax > self.edges[-1]:                      # grow the range by whole bins of the same width
            width = self.edges[1] - self.edges[0]
            extra = int(np.ceil((amax - self.edges[-1]) / width))
            self.edges = np.concatenate([self.edges, self.edges[-1] + width * np.arange(1, extra + 1)])
            self.hist = np.concatenate([self.hist, np.zeros(extra)])
        h, _ = np.histogram(a, bins=self.edges, weights=weights)
        self.hist += h

    # -- range selection ------------------------------------------------------------------------------
    def amax(self, method: str = "entropy", percentile: float = 99.99, start_bin: int = 128, stride: int = 1) -> float:
        if self.hist is None:
            raise ValueError("no data collected")
        if method == "percentile":
            cdf = np.cumsum(self.hist) / self.hist.sum()
            idx = int(np.searchsorted(cdf, percentile / 100.0))
            return float(self.edges[min(idx + 1, len(self.edges) - 1)])
        if method == "mse":
            return self._mse(start_bin, stride)
        if method == "entropy":
            return self._entropy(start_bin, stride)
        raise ValueError(f"unknown calibration method {method!r}")

    def _mse(self, start_bin: int, stride: int) -> float:
        centers = (self.edges[1:] + self.edges[:-1]) / 2
        counts = self.hist
        best, arg = None, len(centers) - 1
        for i in range(min(start_bin, len(centers) - 1), len(centers), stride):
            amax = centers[i]
            q = np.clip(np.rint(centers * (127.0 / amax)), -127, 127) * (amax / 127.0)
            mse = float((((q - centers) ** 2) * counts).mean())
            if best is None or mse < best:
                best, arg = mse, i
        return float(centers[arg])

    def _entropy(self, start_bin: int, stride: int) -> float:
        bins = self.hist.copy()
        bins[0] = bins[1]
        nbins = 128                                                  # 1 << (num_bits - 1): positive int8 levels
        stop = len(bins)
        if stop <= start_bin:
            return float(self.edges[-1])
        csum = np.concatenate([[0.0], np.cumsum(bins)])
        total = csum[-1]
        best, arg = None, stop
        for i in range(start_bin, stop + 1, stride):
            # reference: the first i bins with everything beyond folded into the last one
            ref = bins[:i].copy()
            ref[-1] += total - csum[i]
            # candidate: the first i bins merged into 128 levels; a level's mass is spread evenly over its NON-EMPTY bins
            level = (np.arange(i) * nbins) // i
            nz = bins[:i] > 0
            mass = np.bincount(level, weights=bins[:i], minlength=nbins)
            cnt = np.bincount(level, weights=nz.astype(np.float64), minlength=nbins)
            per = np.divide(mass, cnt, out=np.zeros(nbins), where=cnt > 0)
            cand = np.where(nz, per[level], 0.0)
            p = ref / ref.sum()
            qsum = cand.sum()
            if qsum <= 0:
                continue
            q = cand / qsum
            m = p > 0
            if np.any(m & (q <= 0)):
                continue                                             # infinite divergence
            kl = float(np.sum(p[m] * np.log(p[m] / q[m])))
            if best is None or kl <= best:                           # ties: the LAST (largest) threshold, as the library's argmin over the reversed list
                best, arg = kl, i
        return float(self.edges[arg])


CALIB_BINS = 32768                 # include/unina_mi355.h UNINA_CALIB_BINS: fp16 patterns with the sign bit dropped
_FIRST_NON_FINITE = 0x7c00         # +Inf; every pattern above it is a NaN


def pattern_values(counts: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """One |x| value-count table -> (the fp16 numbers of its non-empty patterns as float32, ascending; their counts as
    float64). ValueError for a table of another length or one that counts an Inf / NaN pattern."""
    c = np.asarray(counts).reshape(-1)
    if c.size != CALIB_BINS:
        raise ValueError(f"a value-count table has {CALIB_BINS} entries, got {c.size}")
    nz = np.flatnonzero(c)
    if nz.size and nz[-1] >= _FIRST_NON_FINITE:
        raise ValueError(f"the table counts {int(c[_FIRST_NON_FINITE:].sum())} non-finite fp16 values (Inf / NaN): the buffer cannot be calibrated")
    return nz.astype(np.uint16).view(np.float16).astype(np.float32), c[nz].astype(np.float64)


def calibrate(named_buffers_per_frame, percentile: Optional[float] = None, method: Optional[str] = None) -> Dict[str, float]:
    """The build's own activation calibrator (the reference's lives in NVIDIA pytorch-quantization, qat.py:129-220,
    which is not available: parity unpinned). Input: an iterable of {buffer name: ndarray} (one dict per
    calibration frame, e.g. Engine.read_buffer() of an fp16/fp32 engine, or tests/emulate.py on CPU). Output:
    {buffer name: amax}.
      method None / "max" : max |x| over all frames (with `percentile`: the max over frames of that per-frame percentile --
                            round 1's calibrator);
      "entropy" | "mse" | "percentile" : per-buffer |x| histogram over ALL frames (HistogramCalibrator above -- what the
                            reference configures, qat.py:91-126), then that range selection (`percentile` defaults to 99.99)."""
    if method in (None, "max"):
        amax: Dict[str, float] = {}
        for named in named_buffers_per_frame:
            for name, arr in named.items():
                a = np.abs(np.asarray(arr, dtype=np.float32))
                v = float(a.max()) if percentile is None else float(np.percentile(a, percentile))
                amax[name] = max(amax.get(name, 0.0), v)
        return amax
    cals: Dict[str, HistogramCalibrator] = {}
    for named in named_buffers_per_frame:
        for name, arr in named.items():
            cals.setdefault(name, HistogramCalibrator()).collect(arr)
    return {name: c.amax(method, 99.99 if percentile is None else percentile) for name, c in cals.items()}


def calibrate_all(named_buffers_per_frame, specs) -> Dict[str, Dict[str, float]]:
    """One pass over the calibration frames, several range selections: specs = {label: (method, percentile | None)}.
    Returns {label: {buffer name: amax}} (tools/int8_drift.py compares them)."""
    cals: Dict[str, HistogramCalibrator] = {}
    mx: Dict[str, float] = {}
    for named in named_buffers_per_frame:
        for name, arr in named.items():
            cals.setdefault(name, HistogramCalibrator()).collect(arr)
            mx[name] = max(mx.get(name, 0.0), float(np.abs(np.asarray(arr)).max()))
    out = {}
    for label, (method, pct) in specs.items():
        out[label] = dict(mx) if method == "max" else {n: c.amax(method, 99.99 if pct is None else pct) for n, c in cals.items()}
    return out


def _table_max(counts: np.ndarray) -> float:
    a, _w = pattern_values(counts)
    return float(a[-1]) if a.size else 0.0


def calibrate_counts(tables_per_frame, names, percentile: Optional[float] = None, method: Optional[str] = None) -> Dict[str, float]:
    """`calibrate` on |x| value-count tables: tables_per_frame is an iterable of [len(names), CALIB_BINS] integer arrays
    (one per calibration frame, Engine.calib_counts), names the buffer of each row. Same ranges as `calibrate` on the
    tensors the tables were counted from, float for float (HistogramCalibrator.collect_counts).
      method None / "max" : the value of the largest non-empty pattern over all frames. With a `percentile` it is NOT
                            offered: np.percentile's interpolation over the raw tensor is not reproduced from a table
                            (ValueError; engine.calibrate_amax computes that one);
      "entropy" | "mse" | "percentile" : as `calibrate`."""
    names = list(names)
    if method in (None, "max"):
        if percentile is not None:
            raise ValueError('method "max" with a per-frame percentile needs the raw tensors (np.percentile interpolates between '
                             "elements): use engine.calibrate_amax for it")
        amax: Dict[str, float] = {}
        for tables in tables_per_frame:
            for name, row in zip(names, _rows(tables, names)):
                amax[name] = max(amax.get(name, 0.0), _table_max(row))
        return amax
    cals: Dict[str, HistogramCalibrator] = {}
    for tables in tables_per_frame:
        for name, row in zip(names, _rows(tables, names)):
            cals.setdefault(name, HistogramCalibrator()).collect_counts(row)
    return {name: c.amax(method, 99.99 if percentile is None else percentile) for name, c in cals.items()}


def calibrate_counts_all(tables_per_frame, names, specs) -> Dict[str, Dict[str, float]]:
    """`calibrate_all` on value-count tables: one pass, several range selections, specs = {label: (method, percentile | None)}."""
    names = list(names)
    cals: Dict[str, HistogramCalibrator] = {}
    mx: Dict[str, float] = {}
    for tables in tables_per_frame:
        for name, row in zip(names, _rows(tables, names)):
            cals.setdefault(name, HistogramCalibrator()).collect_counts(row)
            mx[name] = max(mx.get(name, 0.0), _table_max(row))
    out = {}
    for label, (method, pct) in specs.items():
        out[label] = dict(mx) if method == "max" else {n: c.amax(method, 99.99 if pct is None else pct) for n, c in cals.items()}
    return out


def _rows(tables, names):
    t = np.asarray(tables)
    if t.shape != (len(names), CALIB_BINS):
        raise ValueError(f"expected tables of shape {(len(names), CALIB_BINS)}, got {t.shape}")
    return t


def export_engine(sd: Dict[str, np.ndarray], path: str, graph: Optional[Graph] = None,
                  precision: int = FP16, amax: Optional[Dict[str, float]] = None,
                  weight_amax: Optional[Dict[str, float]] = None) -> EngineBuilder:
    """state_dict (reference key names) -> engine file. Returns the builder (op table for inspection)."""
    b = EngineBuilder(sd, graph, precision, amax, weight_amax)
    b.save(path)
    return b


def amax_from_qat(sd: Dict[str, np.ndarray], graph: Graph, quant: dict,
                  fallback: Optional[Dict[str, float]] = None) -> Dict[str, float]:
    """Activation ranges for an INT8 engine taken from a QAT checkpoint's own quantizers (statedict.from_qat_checkpoint):
    the reference puts ONE input quantizer on every QuantConv2d (qat.py:109-124, 245-248), the engine keeps ONE scale per
    activation buffer (a concat buffer feeds one conv, sibling convs such as C3k2's cv1 / cv2 share their input), so a
    buffer takes the LARGEST range of the convs that read it (no clipping that the checkpoint's quantizers would not do).
    Buffers no checkpoint quantizer speaks for (e.g. a residual-only tensor) come from `fallback` (a calibrate() result)."""
    b = EngineBuilder(sd, graph)                         # fp16 table: which conv module reads which buffer
    out: Dict[str, float] = dict(fallback or {})
    seen = set()
    for op in b.ops:
        if op.kind != OP_CONV:
            continue
        name = b.buffers[op.src_buf][0]
        for sg in op.segs:
            a = quant.get("input_amax", {}).get(sg.module)
            if a is not None:
                out[name] = max(a, out[name]) if name in seen else a
                seen.add(name)
    return out


def export_qat_checkpoint(ck: Dict[str, np.ndarray], path: str, in_h: int = 640, in_w: int = 640, num_classes: int = 4,
                          base_channels: int = 32, fallback_amax: Optional[Dict[str, float]] = None) -> EngineBuilder:
    """A `UNINA_YOLO_DLA_QAT` checkpoint (qat.py key names, quantizer `_amax` entries included) -> INT8 engine file of
    graph (B), using the checkpoint's own activation / weight ranges; without quantizer entries (a float checkpoint of
    the QAT topology) -> fp16 engine."""
    from . import statedict
    weights, quant = statedict.from_qat_checkpoint(ck)
    g = Graph(num_classes=num_classes, base_channels=base_channels, in_h=in_h, in_w=in_w, variant="B")
    if not quant["input_amax"]:
        return export_engine(weights, path, g, FP16)
    amax = amax_from_qat(weights, g, quant, fallback_amax)
    return export_engine(weights, path, g, INT8, amax, quant["weight_amax"])


def read_engine_header(path: str) -> dict:
    with open(path, "rb") as f:
        raw = f.read(_HDR.size)
    (magic, version, precision, in_c, in_h, in_w, nc, n_buf, n_ops, n_heads, s0, s1, s2, blob, macs, model_bc) = _HDR.unpack(raw)
    if magic != MAGIC:
        raise ValueError("not a UNINAENG file")
    return dict(version=version, precision=precision, in_c=in_c, in_h=in_h, in_w=in_w, num_classes=nc,
                n_buffers=n_buf, n_ops=n_ops, n_heads=n_heads, strides=(s0, s1, s2), blob_bytes=blob, macs=macs,
                model_base_channels=model_bc)


# ---- command line: weights file -> engine file (export_trt.py's `python export_trt.py --weights ... --output ...`) ----
PRECISIONS = {"fp16": FP16, "strict": STRICT, "fp32": FP32, "int8": INT8}
CALIBRATORS = ("max", "entropy", "mse", "percentile")


def load_weights(path: str) -> Dict[str, np.ndarray]:
    """A .unsd file (statedict.py), or a .pt / .pth checkpoint read with torch's weights-only (non-executing) loader: a
    state_dict, or a dict holding one under "state_dict" / "model"; a `module.` prefix, BatchNorm counters and quantizer
    entries are dropped (statedict.from_qat_checkpoint's name rules)."""
    from . import statedict
    if path.lower().endswith(".unsd"):
        return statedict.load(path)
    import torch
    ck = torch.load(path, map_location="cpu", weights_only=True)
    for key in ("state_dict", "model"):
        if isinstance(ck, dict) and isinstance(ck.get(key), dict):
            ck = ck[key]
    weights, _quant = statedict.from_qat_checkpoint({k: v.numpy() for k, v in ck.items() if hasattr(v, "numpy")})
    return weights


def graph_for(sd: Dict[str, np.ndarray], in_h: int, in_w: int) -> Graph:
    """The Graph a state_dict belongs to, read off its own tensors: variant by key names, width from the stem, class count
    from a cls head's output conv, lite_p2 from the P2 stage being one ConvBlock."""
    from . import statedict
    variant = statedict.detect_variant(sd)
    stem = "backbone.stem.conv.weight" if variant == "A" else "stem.conv.weight"
    cls = "head_p3.cls_branch.2.weight" if variant == "A" else "head_p3_cls.2.weight"
    if cls not in sd:
        raise ValueError(f"state_dict has no {cls!r}")
    return Graph(num_classes=int(sd[cls].shape[0]), base_channels=int(sd[stem].shape[0]),
                 lite_p2=variant == "A" and "backbone.stage1_block.conv.weight" in sd, in_h=in_h, in_w=in_w, variant=variant)


def cli_parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m unina_yolo_dla_amd.export",
                                 description="weights file -> .une engine file for libunina_mi355.so")
    ap.add_argument("--weights", required=True, help=".unsd (statedict.py), or a .pt / .pth state_dict (loaded weights-only)")
    ap.add_argument("--out", required=True, help="engine file to write (.une)")
    ap.add_argument("--precision", default="fp16", choices=sorted(PRECISIONS))
    ap.add_argument("--size", type=int, nargs=2, default=(640, 640), metavar=("H", "W"), help="network input size")
    ap.add_argument("--calib-dir", help="int8: folder of calibration images (or .npy frames), read as mine.load_frame does")
    ap.add_argument("--calib-frames", type=int, default=30, help="int8: number of frames taken from --calib-dir (sorted order)")
    ap.add_argument("--calibrator", default="entropy", choices=CALIBRATORS, help="int8: range selection")
    ap.add_argument("--percentile", type=float, default=None, help='int8, --calibrator percentile: default 99.99')
    ap.add_argument("--device", type=int, default=0, help="int8: GPU the calibration runs on")
    return ap


def main(argv=None) -> int:
    ap = cli_parser()
    args = ap.parse_args(argv)
    precision = PRECISIONS[args.precision]
    if precision == INT8 and not args.calib_dir:
        ap.error("--precision int8 needs --calib-dir")
    if precision != INT8 and args.calib_dir:
        ap.error("--calib-dir is only used with --precision int8")
    if args.percentile is not None and args.calibrator != "percentile":
        ap.error("--percentile goes with --calibrator percentile")
    if args.calib_frames < 1:
        ap.error("--calib-frames must be at least 1")
    try:
        sd = load_weights(args.weights)
        g = graph_for(sd, args.size[0], args.size[1])
    except (OSError, ValueError, KeyError) as e:
        ap.error(f"{args.weights}: {e}")
    amax = None
    if precision == INT8:
        from . import mine
        files = mine.list_files(args.calib_dir)[:args.calib_frames] if os.path.isdir(args.calib_dir) else []
        if not files:
            ap.error(f"--calib-dir {args.calib_dir}: no images")
        import torch  # noqa: F401  (first: the engine library then shares the HIP runtime that torch has loaded)
        from . import engine
        frames = (mine.load_frame(p, g.in_w, g.in_h)[None] for p in files)
        amax = engine.calibrate_amax_device(sd, g, frames, device=args.device, percentile=args.percentile,
                                            method=None if args.calibrator == "max" else args.calibrator)
        print(f"calibrated {len(amax)} buffers on {len(files)} frames ({args.calibrator})")
    b = export_engine(sd, args.out, g, precision, amax)
    print(f"wrote {args.out}: {args.precision}, {g.in_h}x{g.in_w}, graph ({g.variant}), {len(b.ops)} ops")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
