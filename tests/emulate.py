"""Test-only emulator of the ENGINE's arithmetic: executes the exporter's fused op table with torch CPU math,
rounding exactly where the HIP kernels do (folded fp16 weights, every NHWC buffer write; int8 engines: integer dot
products, per-channel float multiplier, round-half-even requantisation). It checks, independently of the kernels:
(1) the op table (fusions, concat slices, residual/upsample folding, int8 pass) computes graph (A); (2) the fp16
engine's deviation from the fp32 oracle is the fp16 FORMAT's rounding noise, not a kernel error; (3) the int8
engine's integer arithmetic bit for bit."""
import numpy as np
import torch
import torch.nn.functional as F

from unina_yolo_dla_amd import export


def split16(t):
    """fp32 tensor -> (hi, lo) fp16 pair as fp32 tensors: hi = fp16(t), lo = fp16(t - hi) (the SPLIT engine's storage format)."""
    hi = t.float().half().float()
    lo = (t.float() - hi).half().float()
    return hi, lo


def run_op_table(builder: "export.EngineBuilder", x: np.ndarray, fp16: bool = True, teacher: dict = None,
                 precise_w=None, precise_a=None, builder32: "export.EngineBuilder" = None, split: bool = False):
    """x: [1,3,H,W] fp32. Returns ({output name: [C,H,W] fp32}, {buffer name: [C,H,W] fp32}).
    int8 buffers are returned as their integer codes (multiply by the buffer scale to dequantise).

    teacher = {buffer name: stored values (codes for int8 buffers) read back from the ENGINE after a per-op forward}:
    every op then reads the engine's own buffers and writes into a separate set, so the returned buffers hold each
    op's emulated output GIVEN THE ENGINE'S INPUTS -- a per-op comparison that rounding flips cannot snowball through
    (deep in an int8 network a handful of +-1 input codes moves a third of the outputs by one code).

    Error-budget switches (tools/fp16_error_budget.py): ops whose index is in `precise_w` take their weights from
    `builder32` (an FP32 builder of the same state_dict: same op order, fp32 folded weights) instead of the fp16 blob;
    ops in `precise_a` store their output without the fp16 rounding. Everything else is unchanged, so the head error
    of such a run against the fp32 oracle is the contribution of the roundings left switched on.

    A SPLIT builder (or split=True with an FP32 builder): the SPLIT precision mode's arithmetic -- every folded weight and every stored
    activation is an fp16 pair hi + lo, a conv is the three fp16 products hi*hi + lo*hi + hi*lo accumulated in fp32
    (the lo*lo term is dropped), the stem and the epilogues are fp32."""
    precise_w = precise_w or ()
    precise_a = precise_a or ()
    blob32 = bytes(builder32.blob) if builder32 is not None else None
    cur_op = [0]
    prec = builder.precision
    split = split or prec == export.SPLIT
    wdt = {export.FP16: "<f2", export.FP32: "<f4", export.INT8: "<f2", export.SPLIT: "<f2"}[prec]
    blob = bytes(builder.blob)
    bdtype = [b[4] for b in builder.buffers]
    bscale = [b[6] for b in builder.buffers]
    bufs = {i: torch.zeros((c, h, w), dtype=torch.float64 if prec == export.INT8 else torch.float32)
            for i, (name, h, w, c, *_rest) in enumerate(builder.buffers)}
    img = next(i for i, b in enumerate(builder.buffers) if b[5] & export.BUF_INPUT)
    bufs[img] = torch.from_numpy(np.ascontiguousarray(x[0])).to(bufs[img].dtype)
    wr = bufs
    if teacher is not None:
        for i, b in enumerate(builder.buffers):
            if i != img and b[0] in teacher:
                bufs[i] = torch.from_numpy(np.ascontiguousarray(teacher[b[0]])).to(bufs[i].dtype)
        wr = {i: t.clone() for i, t in bufs.items()}

    def store(dst_buf, y):
        """round y (real values) the way a kernel writing into buffer `dst_buf` does"""
        d = bdtype[dst_buf]
        if d == export.BUF_I8:
            # the engine's reciprocal: 1.0f / (the fp32 scale of the engine file), engine.hip plan()
            inv = np.float32(1.0) / np.float32(bscale[dst_buf])
            return torch.clamp(torch.round(y.float() * inv), -127, 127).to(y.dtype)
        if d == export.BUF_F16 and fp16 and cur_op[0] not in precise_a:
            return y.half().to(y.dtype)
        if split and d in (export.BUF_F32_NHWC, export.BUF_S16):
            hi, lo = split16(y)
            return (hi + lo).to(y.dtype)
        return y.float().to(y.dtype)

    def real(buf_idx, t):
        """real values held by (a slice of) buffer buf_idx"""
        return t * bscale[buf_idx] if bdtype[buf_idx] == export.BUF_I8 else t

    for oi, op in enumerate(builder.ops):
        src = bufs[op.src_buf]
        cur_op[0] = oi
        if op.kind == export.OP_STEM:
            s = op.segs[0]
            w = torch.from_numpy(np.frombuffer(blob, dtype="<f4", count=s.n_count * 27, offset=s.w_off).reshape(s.n_count, 3, 3, 3).copy())
            b = torch.from_numpy(np.frombuffer(blob, dtype="<f4", count=s.n_count, offset=s.b_off).copy())
            y = F.relu(F.conv2d(src[None].float(), w, b, stride=2, padding=1))[0].to(src.dtype)
            wr[s.dst.buf][s.dst.coff:s.dst.coff + s.n_count] = store(s.dst.buf, y)
        elif op.kind == export.OP_SPPF_POOL:
            s = op.segs[0]
            c = op.cin
            t = src[s.src_coff:s.src_coff + c][None]
            for i in range(1, 4):
                t = F.max_pool2d(t, 5, 1, 2)
                wr[op.src_buf][s.src_coff + i * c:s.src_coff + (i + 1) * c] = t[0]
        elif op.kind == export.OP_QUANT:
            s = op.segs[0]
            wr[s.dst.buf][s.dst.coff:s.dst.coff + s.n_count] = store(s.dst.buf, src[:s.n_count])
        elif op.kind == export.OP_CONV:
            k = op.k
            int8 = prec == export.INT8 and builder.op_int8[oi]
            for s in op.segs:
                K = k * k * op.cin
                xin = src[s.src_coff:s.src_coff + op.cin][None]
                b = torch.from_numpy(np.frombuffer(blob, dtype="<f4", count=s.n_count, offset=s.b_off).copy())
                if int8:
                    w = np.frombuffer(blob, dtype="i1", count=s.n_pad * K, offset=s.w_off)
                    w = export.unpack_weights(w, s.n_pad, K).reshape(s.n_pad, k, k, op.cin)[:s.n_count]
                    w = torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2).contiguous()
                    mult = torch.from_numpy(np.frombuffer(blob, dtype="<f4", count=s.n_count, offset=s.m_off).copy())
                    acc = F.conv2d(xin.double(), w, None, stride=op.s, padding=k // 2)[0]          # exact integers
                    # kernel: fmaf(acc, mult, bias) -> one fp32 rounding; the product is exact in fp64 (|acc| < 2^26)
                    y = (acc * mult.double()[:, None, None] + b.double()[:, None, None]).float().double()
                elif oi in precise_w:
                    s32 = builder32.ops[oi].segs[op.segs.index(s)]
                    w = np.frombuffer(blob32, dtype="<f4", count=s.n_pad * K, offset=s32.w_off)
                    w = export.unpack_weights(w, s.n_pad, K).reshape(s.n_pad, k, k, op.cin)[:s.n_count]
                    w = torch.from_numpy(w.astype(np.float32)).permute(0, 3, 1, 2).contiguous()
                    y = F.conv2d(real(op.src_buf, xin).float(), w, b, stride=op.s, padding=k // 2)[0].to(src.dtype)
                elif split:
                    if prec == export.SPLIT:
                        w = np.frombuffer(blob, dtype="<f2", count=2 * s.n_pad * K, offset=s.w_off)
                        w = export.unpack_weights_split(w, s.n_pad, K).reshape(s.n_pad, k, k, op.cin)[:s.n_count]
                    else:
                        w = np.frombuffer(blob, dtype="<f4", count=s.n_pad * K, offset=s.w_off)
                        w = export.unpack_weights(w, s.n_pad, K).reshape(s.n_pad, k, k, op.cin)[:s.n_count]
                    w = torch.from_numpy(w.astype(np.float32)).permute(0, 3, 1, 2).contiguous()
                    wh, wl = split16(w)
                    xh, xl = split16(xin)
                    y = (F.conv2d(xh, wl, None, stride=op.s, padding=k // 2) + F.conv2d(xl, wh, None, stride=op.s, padding=k // 2)
                         + F.conv2d(xh, wh, b, stride=op.s, padding=k // 2))[0].to(src.dtype)
                else:
                    w = np.frombuffer(blob, dtype=wdt, count=s.n_pad * K, offset=s.w_off)
                    w = export.unpack_weights(w, s.n_pad, K).reshape(s.n_pad, k, k, op.cin)[:s.n_count]
                    w = torch.from_numpy(w.astype(np.float32)).permute(0, 3, 1, 2).contiguous()
                    y = F.conv2d(real(op.src_buf, xin).float(), w, b, stride=op.s, padding=k // 2)[0].to(src.dtype)
                if op.relu:
                    y = F.relu(y)
                if op.res is not None:
                    r = bufs[op.res.buf][op.res.coff:op.res.coff + s.n_count]
                    if bdtype[op.res.buf] == export.BUF_I8:      # kernel: fmaf(code, s_res, y)
                        y = (y.double() + r.double() * float(np.float32(bscale[op.res.buf]))).float().to(y.dtype)
                    else:
                        y = (y.float() + r.float()).to(y.dtype)
                if s.flags & export.SEG_PLANAR_F32:
                    wr[s.dst.buf][s.dst.coff:s.dst.coff + s.n_count] = y.float().to(y.dtype)
                    continue
                y = store(s.dst.buf, y)
                if s.flags & export.SEG_UP2:
                    y = y.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
                wr[s.dst.buf][s.dst.coff:s.dst.coff + s.n_count] = y
        else:
            raise NotImplementedError(op.kind)
    named = {builder.buffers[i][0]: t.float().numpy() for i, t in wr.items()}
    outs = {n: named[n] for n in ("p2_cls", "p2_reg", "p3_cls", "p3_reg", "p4_cls", "p4_reg")}
    return outs, named


def dequantised(builder: "export.EngineBuilder", named: dict) -> dict:
    """{buffer name: real-valued ndarray} (int8 buffers multiplied by their scale)."""
    out = {}
    for name, h, w, c, dtype, flags, scale in builder.buffers:
        out[name] = named[name] * scale if dtype == export.BUF_I8 else named[name]
    return out


def engine_buffers(builder: "export.EngineBuilder", read_buffer) -> dict:
    """{buffer name: stored values} of an engine after a per-op (unfused) forward, int8 buffers as codes: the `teacher`
    of run_op_table and per_op_bounds. Every buffer but the input image: fp16, int8, fp32 NHWC, split pairs (hi + lo) and the
    planar fp32 head outputs. read_buffer(name) returns real values (code * scale), as Engine.read_buffer does."""
    out = {}
    for name, h, w, c, dtype, flags, scale in builder.buffers:
        if dtype != export.BUF_F32_NCHW_IN and not (flags & export.BUF_INPUT):
            v = read_buffer(name)
            out[name] = np.rint(v / np.float32(scale)) if dtype == export.BUF_I8 else v
    return out


def per_op_mismatch(builder: "export.EngineBuilder", teacher: dict, named: dict) -> dict:
    """Per activation buffer: (fraction of int8 codes that differ | fraction of fp16 values off by more than 2 fp16
    ulp, worst difference in codes | in units of the 2-ulp tolerance) between the engine and the teacher-forced emulation."""
    out = {}
    for name, h, w, c, dtype, flags, scale in builder.buffers:
        if name not in teacher:
            continue
        a, b = np.asarray(teacher[name], np.float64), np.asarray(named[name], np.float64)
        if dtype == export.BUF_I8:
            d = np.abs(a - b)
            out[name] = (float((d > 0.5).mean()), float(d.max()))
        else:
            tol = 2.0 ** -9 * np.maximum(np.abs(a), np.abs(b)) + 1e-4
            d = np.abs(a - b) / tol
            out[name] = (float((d > 1.0).mean()), float(d.max()))
    return out


# ---- the exact per-op reference and its rounding bound -------------------------------------------------------------
# Every op of the table, evaluated in float64 on the SAME stored inputs the engine (or the emulator) read, with the
# bound its arithmetic allows -- derived, not measured:
#   * round_nearest(a) is within half an ulp of the destination format of a;
#   * an fp32 accumulation of K terms is within K * 2^-24 * S of the exact sum, S = the sum of the absolute terms;
#     the bias, the shortcut (two additions for a split pair) and the fma of an int8 epilogue are at most 4 more terms.
# A stored value `got` passes when |got - y| <= tol; no element is exempt.
MUTANTS = ("drop_tap", "edge_pad", "res_before_relu", "up2_last_col", "bias_neighbour")


def ulp16(a):
    """Spacing of fp16 at magnitude a (subnormal spacing 2^-24 below 2^-14)."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(a), 2.0 ** -14))) - 10)


def ulp32(a):
    """Spacing of fp32 at magnitude a."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(a), 2.0 ** -126))) - 23)


def _is_f32(a):
    """True where the float64 value a is an fp32 number: an fp32 operation whose exact result is a returns a, unrounded."""
    return a.astype(np.float32).astype(np.float64) == a


def _seg_params(builder, blob, op, oi, s):
    """Folded weights of one segment AS STORED in the blob -> (list of float64 [n, cin, k, k] planes -- one, or (hi, lo) for
    a split engine --, bias [n] float64, multiplier [n] float64 or None)."""
    prec, k = builder.precision, op.k
    K = k * k * op.cin
    bias = np.frombuffer(blob, dtype="<f4", count=s.n_count, offset=s.b_off).astype(np.float64)

    def planes(w):
        return torch.from_numpy(w.reshape(s.n_pad, k, k, op.cin)[:s.n_count].astype(np.float64)).permute(0, 3, 1, 2).contiguous()

    if prec == export.INT8 and builder.op_int8[oi]:
        w = export.unpack_weights(np.frombuffer(blob, dtype="i1", count=s.n_pad * K, offset=s.w_off), s.n_pad, K)
        mult = np.frombuffer(blob, dtype="<f4", count=s.n_count, offset=s.m_off).astype(np.float64)
        return [planes(w)], bias, mult
    if prec == export.SPLIT:
        blk = np.frombuffer(blob, dtype="<f2", count=2 * s.n_pad * K, offset=s.w_off).reshape(-1, 2, 512)
        return [planes(export.unpack_weights(np.ascontiguousarray(blk[:, i]).reshape(-1), s.n_pad, K)) for i in (0, 1)], bias, None
    wdt = "<f4" if prec == export.FP32 else "<f2"
    return [planes(export.unpack_weights(np.frombuffer(blob, dtype=wdt, count=s.n_pad * K, offset=s.w_off), s.n_pad, K))], bias, None


def _conv64(x, w, stride, k, edge_pad=False):
    """float64 conv, zero padding k // 2 (edge_pad: the LEFT border replicates the first column instead -- a mutant)."""
    if edge_pad and k == 3:
        xp = F.pad(x, (1, 1, 1, 1))
        xp[..., 0] = xp[..., 1]
        return F.conv2d(xp, w, None, stride=stride)[0]
    return F.conv2d(x, w, None, stride=stride, padding=k // 2)[0]


def per_op_bounds(builder: "export.EngineBuilder", x: np.ndarray, teacher: dict, mutate: dict = None, only_op=None):
    """One record per written buffer slice of every op (every segment; the three pooled maps of the SPPF as one slice), each op
    evaluated in float64 on the buffers of `teacher` (what run_op_table(teacher=...) reads; x is the input image):
      op, seg, name, kernel-independent; buf, c0, c1: the slice [c0:c1] of buffer `buf`;
      dest: "f16" | "f32" | "s16" | "i8" | "pool" (the destination's storage), terms: K = k*k*cin (3K for a split conv);
      y: the exact value; S: the sum of absolute terms conv(|x|, |w|) + |bias| (+ |shortcut|), through the same ReLU / add /
         up2 structure;
      int8 destinations also: t = the pre-rounding value y / s_out (float64), slack = how far the engine's fp32 t may be from it.
    mutate = {"op": index, "kind": one of MUTANTS}: that op's y (and t) is computed WRONG in that way (tests of the check itself);
    only_op: an op index or a collection of them -- evaluate those ops alone."""
    prec = builder.precision
    blob = bytes(builder.blob)
    names = [b[0] for b in builder.buffers]
    bdtype = [b[4] for b in builder.buffers]
    scale32 = [np.float32(b[6]) for b in builder.buffers]
    dest_of = {export.BUF_F16: "f16", export.BUF_F32_NHWC: "f32", export.BUF_F32_PLANAR: "f32", export.BUF_S16: "s16", export.BUF_I8: "i8"}

    def stored(i):
        if builder.buffers[i][5] & export.BUF_INPUT:
            return torch.from_numpy(np.ascontiguousarray(x[0]).astype(np.float64))
        return torch.from_numpy(np.ascontiguousarray(teacher[names[i]]).astype(np.float64))

    def to_i8(rec, y1, y2, inv, exact_acc, S):
        """int8 destination: t = y2 * inv; the engine's fp32 t is off by at most half an ulp per INEXACT fp32 step (fma, shortcut
        fma, the multiply), each taken at the largest magnitude it passes through -- under 4 ulp32(M), M = max(|y1|, |y2|) * inv
        and |t| -- plus, for an fp32-accumulated conv, the accumulation's share (terms + 4) * 2^-24 * S * inv. Where every step is
        exact in fp32 the engine's t IS t: no slack, the code must be the half-even one."""
        t = y2 * inv
        M = np.maximum(np.maximum(np.abs(y1), np.abs(y2)) * inv, np.abs(t))
        if exact_acc:
            slack = np.where(_is_f32(y1) & _is_f32(y2) & _is_f32(t), 0.0, 4.0 * ulp32(M))
        else:
            slack = 4.0 * ulp32(M) + (rec["terms"] + 4) * 2.0 ** -24 * S * inv
        rec.update(y=y2, S=S, t=t, slack=slack)

    if isinstance(only_op, int):
        only_op = (only_op,)
    out = []
    for oi, op in enumerate(builder.ops):
        if only_op is not None and oi not in only_op:
            continue
        mut = mutate["kind"] if mutate is not None and mutate["op"] == oi else None
        src = stored(op.src_buf)
        for si, s in enumerate(op.segs):
            dst = s.dst.buf
            rec = dict(op=oi, seg=si, name=op.name, kind=op.kind, buf=names[dst], c0=s.dst.coff, c1=s.dst.coff + s.n_count,
                       dest=dest_of[bdtype[dst]], terms=op.k * op.k * op.cin, relu=bool(op.relu), res=op.res is not None,
                       up2=bool(s.flags & export.SEG_UP2))
            inv = float(np.float32(1.0) / scale32[dst])
            if op.kind == export.OP_SPPF_POOL:
                c = op.cin
                t = src[s.src_coff:s.src_coff + c][None]
                maps = []
                for _ in range(3):                      # 5 / 9 / 13 clipped windows (max_pool2d pads with -inf)
                    t = F.max_pool2d(t, 5, 1, 2)
                    maps.append(t[0])
                rec.update(dest="pool", y=torch.cat(maps).numpy(), S=None)
            elif op.kind == export.OP_QUANT:
                v = src[:s.n_count].numpy()
                rec["terms"] = 0
                to_i8(rec, v, v, inv, True, np.abs(v))
            elif op.kind == export.OP_STEM:
                w = torch.from_numpy(np.frombuffer(blob, dtype="<f4", count=s.n_count * 27, offset=s.w_off).reshape(s.n_count, 3, 3, 3).astype(np.float64))
                b = np.frombuffer(blob, dtype="<f4", count=s.n_count, offset=s.b_off).astype(np.float64)
                if mut == "drop_tap":
                    w = w.clone()
                    w[:, 0, 0, 0] = 0
                y = (F.conv2d(src[None], w, None, stride=2, padding=1)[0].numpy() + b[:, None, None]).clip(min=0)
                S = F.conv2d(src[None].abs(), w.abs(), None, stride=2, padding=1)[0].numpy() + np.abs(b)[:, None, None]
                rec.update(y=y, S=S, terms=27)
                if rec["dest"] == "i8":
                    to_i8(rec, y, y, inv, False, S)
            elif op.kind == export.OP_CONV:
                int8 = prec == export.INT8 and builder.op_int8[oi]
                planes, b, mult = _seg_params(builder, blob, op, oi, s)
                xin = src[s.src_coff:s.src_coff + op.cin][None]
                bm = b.copy()
                if mut == "bias_neighbour":
                    bm[0] = b[1]
                wy = [p.clone() for p in planes]
                if mut == "drop_tap":
                    for p in wy:
                        p[:, 0, 0, 0] = 0
                ep = mut == "edge_pad"
                if len(planes) == 2:                    # split: hi*hi + lo*hi + hi*lo = (hi + lo) * w_hi + hi * w_lo; lo*lo is not computed
                    xh, xl = (torch.from_numpy(np.ascontiguousarray(v.numpy()).astype(np.float64)) for v in split16(xin.float()))
                    acc = _conv64(xh + xl, wy[0], op.s, op.k, ep) + _conv64(xh, wy[1], op.s, op.k, ep)
                    S = _conv64(xh.abs() + xl.abs(), planes[0].abs(), op.s, op.k) + _conv64(xh.abs(), planes[1].abs(), op.s, op.k)
                    rec["terms"] = 3 * rec["terms"]
                else:
                    acc = _conv64(xin, wy[0], op.s, op.k, ep)
                    S = _conv64(xin.abs(), planes[0].abs(), op.s, op.k)
                acc, S = acc.numpy(), S.numpy()
                if mult is not None:                    # int8 conv: acc is the exact integer, y1 = fma(acc, mult, bias)
                    y1 = acc * mult[:, None, None] + bm[:, None, None]
                    S = S * np.abs(mult)[:, None, None] + np.abs(b)[:, None, None]
                else:
                    y1 = acc + bm[:, None, None]
                    S = S + np.abs(b)[:, None, None]
                r = None
                if op.res is not None:
                    r = stored(op.res.buf)[op.res.coff:op.res.coff + s.n_count].numpy()
                    if bdtype[op.res.buf] == export.BUF_I8:
                        r = r * float(scale32[op.res.buf])
                    S = S + np.abs(r)
                if mut == "res_before_relu" and r is not None:
                    y1 = y2 = np.maximum(y1 + r, 0)
                else:
                    if op.relu:
                        y1 = np.maximum(y1, 0)
                    y2 = y1 + r if r is not None else y1
                if s.flags & export.SEG_UP2:
                    y1, y2, S = (np.repeat(np.repeat(a, 2, axis=1), 2, axis=2) for a in (y1, y2, S))
                    if mut == "up2_last_col":           # the last column duplicates the pixel one to the LEFT of its own
                        y1, y2 = y1.copy(), y2.copy()
                        y1[:, :, -1], y2[:, :, -1] = y1[:, :, -3], y2[:, :, -3]
                rec.update(y=y2, S=S)
                if rec["dest"] == "i8":
                    to_i8(rec, y1, y2, inv, int8, S)
            else:
                raise NotImplementedError(op.kind)
            out.append(rec)
    return out


def as_stored(rec):
    """rec's y rounded to its destination the way the documented epilogue does (the mutants' `engine output`)."""
    y = rec["y"]
    if rec["dest"] == "f16":
        return y.astype(np.float32).astype(np.float16).astype(np.float64)
    if rec["dest"] == "s16":
        hi, lo = split16(torch.from_numpy(y.astype(np.float32)))
        return (hi + lo).numpy().astype(np.float64)
    if rec["dest"] == "i8":
        return np.clip(np.rint(rec["t"].astype(np.float32)), -127, 127).astype(np.float64)
    return y.astype(np.float32).astype(np.float64)


def check_slice(rec, got):
    """One slice of stored values against its record. Returns dict(n, violations, worst = the largest error / bound (float
    destinations), first = (channel, row, column, got, want, bound) of the first offender or None, mismatches, cap (int8:
    codes that differ from the half-even code of t, and the number of elements whose t is within its slack of a tie))."""
    got = np.asarray(got, np.float64)
    y = rec["y"]
    assert got.shape == y.shape, (rec["name"], rec["buf"], got.shape, y.shape)
    res = dict(n=int(y.size), worst=0.0, mismatches=0, cap=0)
    if rec["dest"] == "pool":
        bad, want, tol = got != y, y, np.zeros_like(y)
    elif rec["dest"] == "i8":
        t, slack = rec["t"], rec["slack"]
        want = np.clip(np.rint(t), -127, 127)
        lo = np.clip(np.ceil(t - slack - 0.5), -127, 127)
        hi = np.clip(np.floor(t + slack + 0.5), -127, 127)
        tie = (slack > 0) & (lo < hi)
        bad = (got != want) & ~(tie & (np.abs(got - want) == 1) & (got >= lo) & (got <= hi))
        res.update(mismatches=int((got != want).sum()), cap=int(tie.sum()))
        tol = slack
    else:
        S, n = rec["S"], rec["terms"]
        tol = (n + 4) * 2.0 ** -24 * S
        if rec["dest"] == "f16":
            tol = tol + 0.5 * ulp16(np.maximum(np.abs(got), np.abs(y)))
        elif rec["dest"] == "s16":
            tol = tol + 2.0 ** -22 * np.abs(y) + 2.0 ** -25
        tol = np.where(S == 0, 0.0, tol)       # nothing but zeros entered the sum: the result is exactly 0 in any format
        err = np.abs(got - y)
        bad = ~(err <= tol)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
        res["worst"] = float(np.nanmax(ratio)) if ratio.size else 0.0
        want = y
    res["violations"] = int(bad.sum())
    res["first"] = None
    if res["violations"]:
        c, yy, xx = (int(v) for v in np.argwhere(bad)[0])
        res["first"] = (c, yy, xx, float(got[c, yy, xx]), float(want[c, yy, xx]), float(tol[c, yy, xx]))
    return res


def check_per_op(records, named: dict, ops=None):
    """Every record (of the ops in `ops`, default all) against the stored buffers `named` ({buffer name: [C,H,W]}, int8 as
    codes). Returns (list of failures as printable strings, worst error / bound, {buffer: (int8 mismatches, tie cap)})."""
    fails, worst, ties = [], 0.0, {}
    for rec in records:
        if ops is not None and rec["op"] not in ops:
            continue
        c0, c1 = rec["c0"], rec["c1"]
        if rec["dest"] == "pool":
            c1 = c0 + rec["y"].shape[0]
        r = check_slice(rec, np.asarray(named[rec["buf"]])[c0:c1])
        worst = max(worst, r["worst"])
        if rec["dest"] == "i8":
            m, cap = ties.get(rec["buf"], (0, 0))
            ties[rec["buf"]] = (m + r["mismatches"], cap + r["cap"])
            if r["mismatches"] > r["cap"]:
                fails.append(f"op {rec['op']} {rec['name']} seg {rec['seg']} -> {rec['buf']}[{c0}:{c1}]: {r['mismatches']} mismatching codes > tie cap {r['cap']}")
        if r["violations"]:
            c, yy, xx, g, w, tol = r["first"]
            fails.append(f"op {rec['op']} {rec['name']} seg {rec['seg']} -> {rec['buf']}[{c0}:{c1}] ({rec['dest']}): {r['violations']} of {r['n']} "
                         f"outside the bound, worst error/bound {r['worst']:.3g}; first at (c={c0 + c}, y={yy}, x={xx}): got {g!r}, want {w!r}, bound {tol:.3g}")
    return fails, worst, ties


# the sizes and topologies the per-op bound is held at (tests/test_gpu_per_op.py on the kernels, tests/test_per_op_bound_cpu.py
# on this emulator): P2 / P3 / P4 maps of 4x4 / 2x2 / 1x1 (every map smaller than every tile), a one-row P4 map, odd maps whose
# widths are no multiple of 4 or 8, and partial tiles in both directions on every level. Graph (B)'s stride-32 map: 1x1, one
# row of three, 3x5 (odd both ways, partial tiles on every level)
PER_OP_SIZES = ((16, 16), (16, 48), (80, 112), (96, 160))
PER_OP_TOPOLOGIES = (("B-32x32", dict(variant="B", in_h=32, in_w=32)), ("B-32x96", dict(variant="B", in_h=32, in_w=96)),
                     ("B-96x160", dict(variant="B", in_h=96, in_w=160)),
                     ("lite_p2", dict(lite_p2=True, in_h=80, in_w=112)), ("base16", dict(base_channels=16, in_h=80, in_w=112)),
                     ("classes1", dict(num_classes=1, in_h=80, in_w=112)), ("classes7", dict(num_classes=7, in_h=80, in_w=112)),
                     ("classes20", dict(num_classes=20, in_h=80, in_w=112)))


# ---- the frame as launched (fusion on): which ops can be held teacher-forced on the frame's OWN buffers ----------------
# With fusion on, a fused group keeps its intermediates in LDS: their buffers are not written, so most ops of the table have
# no stored input or output to be checked against. What stays checkable is every op whose source, shortcut and destination
# slices all reach memory in that frame: the launches outside any group (the P3 / P4 head layers among them, which then run
# as dual launches) and the convs at a group's edge. Group membership is read from op_infos(): the engine names an absorbed
# op's kernel "(fused into op N)" / "(dual launch with op N)" (engine.hip absorb_info).
def launched_groups(infos):
    """op_infos() of an engine with fusion on -> ({leader: [ops fused into its launch]}, {leader: [ops sharing its dual launch]})."""
    import re
    groups, duals = {}, {}
    for i, o in enumerate(infos):
        m = re.fullmatch(r"\((fused into|dual launch with) op (\d+)\)", o["kernel"])
        if m:
            (groups if m.group(1) == "fused into" else duals).setdefault(int(m.group(2)), []).append(i)
    return groups, duals


def launched_kernel(infos, oi):
    """The kernel that computes op oi in the frame: its own, or that of the launch that absorbed it."""
    import re
    k = infos[oi]["kernel"]
    m = re.fullmatch(r"\((?:fused into|dual launch with) op (\d+)\)", k)
    return launched_kernel(infos, int(m.group(1))) if m else k


def op_reads(op):
    """[(buffer index, c0, c1)] of the slices op reads: per segment its source slice and its shortcut slice."""
    if op.kind == export.OP_QUANT:
        out = [(op.src_buf, 0, op.segs[0].n_count)]
    elif op.kind == export.OP_STEM:
        out = [(op.src_buf, 0, op.cin)]
    else:
        out = [(op.src_buf, s.src_coff, s.src_coff + op.cin) for s in op.segs]
    if op.res is not None:
        out += [(op.res.buf, op.res.coff, op.res.coff + s.n_count) for s in op.segs]
    return out


def op_writes(op):
    return [(s.dst.buf, s.dst.coff, s.dst.coff + s.n_count) for s in op.segs]


def written_when_launched(builder, infos):
    """{buffer name: bool mask over its channels} -- what the frame with fusion on writes to memory (the input image counts as
    written). An op outside every fused group writes its slices. Inside a group (engine.hip op_regions): a slice reaches memory
    when an op outside the group reads it or it is a network output -- a block's cv3, its tail conv and its int8 twin, a head's
    planes; the pre-conv's and the bottlenecks' tensors stay in LDS --, and both convs of a conv pair store theirs (the pooled
    maps of an SPPF pool inside the pair do not)."""
    groups, _ = launched_groups(infos)
    leader = {m: L for L, ms in groups.items() for m in ms}
    leader.update({L: L for L in groups})
    mask = [np.zeros(b[3], dtype=bool) for b in builder.buffers]
    for i, b in enumerate(builder.buffers):
        if b[5] & export.BUF_INPUT:
            mask[i][:] = True
    reads = [op_reads(op) for op in builder.ops]
    for oi, op in enumerate(builder.ops):
        L = leader.get(oi)
        for (buf, c0, c1) in op_writes(op):
            if L is None:
                w = True
            elif infos[L]["kernel"].startswith("conv_pair"):
                w = op.kind == export.OP_CONV
            else:
                inside = {L, *groups[L]}
                w = bool(builder.buffers[buf][5] & export.BUF_OUTPUT) or any(
                    rb == buf and r0 < c1 and c0 < r1 for k, rs in enumerate(reads) if k not in inside for (rb, r0, r1) in rs)
            if w:
                mask[buf][c0:c1] = True
    return {b[0]: m for b, m in zip(builder.buffers, mask)}


def launched_ops(builder, infos, written=None):
    """Indices of the ops whose source, shortcut and destination slices are all written by the frame with fusion on: the ops
    per_op_bounds(only_op=...) can evaluate on that frame's own buffers."""
    written = written_when_launched(builder, infos) if written is None else written
    names = [b[0] for b in builder.buffers]
    return [oi for oi, op in enumerate(builder.ops)
            if all(written[names[buf]][c0:c1].all() for (buf, c0, c1) in op_reads(op) + op_writes(op))]


def head_ops(builder, levels=("p3", "p4")):
    """{level: [op index of the .0, .1 and .2 layer pair]} -- the op whose two slices carry head_<level>.cls_branch.<j> and
    head_<level>.reg_branch.<j> (graph.py's names)."""
    out = {}
    for lv in levels:
        out[lv] = []
        for j in range(3):
            want = {f"head_{lv}.cls_branch.{j}", f"head_{lv}.reg_branch.{j}"}
            hit = [oi for oi, op in enumerate(builder.ops) if {s.module for s in op.segs} == want]
            assert len(hit) == 1, (lv, j, hit)
            out[lv].append(hit[0])
    return out
