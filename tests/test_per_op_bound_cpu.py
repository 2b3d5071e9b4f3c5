"""The per-op rounding bound (tests/emulate.py per_op_bounds / check_slice) has teeth, shown without a GPU:
(1) the emulator -- fp32 torch convolutions, a summation order of its own -- stays inside the bound on every element of every
op at every precision, size and topology the GPU test uses (the bound is not too tight for a correct implementation);
(2) every mutant of one op -- a dropped tap, a replicated border, a shortcut added before the ReLU, an upsample that copies
the wrong neighbour, a neighbour's bias, half-away rounding, a clamp at 128 -- is flagged (it is not too loose for a wrong one),
on graph (A) and, in the int8 table, on the ops only graph (B) has."""
import numpy as np
import pytest
import torch

import emulate as E

PRECISIONS = ("fp16", "fp32", "strict", "int8")
_cache = {}


def _prec(export, name):
    return {"fp16": export.FP16, "fp32": export.FP32, "strict": export.STRICT, "int8": export.INT8}[name]


def _amax(pkg, sd, g, scale=1.0):
    from unina_yolo_dla_amd import export
    b16 = export.EngineBuilder(sd, g)
    amax = export.calibrate(E.run_op_table(b16, pkg.rng.frame(5000 + i, g.in_h, g.in_w))[1] for i in range(2))
    return {k: v * scale for k, v in amax.items()}


def _free_run(pkg, sd, precision, amax_scale=1.0, **gkw):
    """(builder, frame, the free-running emulation's buffers, the float64 records on those buffers), computed once."""
    from unina_yolo_dla_amd import export
    key = (precision, amax_scale, tuple(sorted(gkw.items())))
    if key not in _cache:
        torch.set_num_threads(4)
        g = pkg.graph.Graph(**gkw)
        if sd is None:
            sd = pkg.synth.make_state_dict(7, g)
        p = _prec(export, precision)
        b = export.EngineBuilder(sd, g, p, _amax(pkg, sd, g, amax_scale) if p == export.INT8 else None)
        x = pkg.rng.frame(1234, g.in_h, g.in_w)
        named = E.run_op_table(b, x)[1]
        _cache[key] = (b, x, named, E.per_op_bounds(b, x, named))
    return _cache[key]


def _hold(b, recs, named, label):
    fails, worst, ties = E.check_per_op(recs, named)
    n = sum(r["y"].size for r in recs)
    print(f"{label}: {len(recs)} slices, {n} elements, worst error/bound {worst:.3f}, int8 mismatches / tie cap "
          f"{sum(m for m, _ in ties.values())} / {sum(c for _, c in ties.values())}")
    assert not fails, "\n".join(fails[:8])
    assert worst <= 1.0
    written = {(r["buf"], c) for r in recs for c in range(r["c0"], r["c0"] + r["y"].shape[0])}
    for name, h, w, c, dtype, flags, scale in b.buffers:          # every channel of every buffer is some op's output
        if not flags & 1:
            assert all((name, ch) in written for ch in range(c)), name


@pytest.mark.parametrize("size", E.PER_OP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("precision", PRECISIONS)
def test_emulator_stays_within_the_bound(pkg, sd7, precision, size):
    b, x, named, recs = _free_run(pkg, sd7, precision, in_h=size[0], in_w=size[1])
    _hold(b, recs, named, f"{precision} {size[0]}x{size[1]}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("topology", E.PER_OP_TOPOLOGIES, ids=lambda t: t[0])
def test_emulator_stays_within_the_bound_on_other_topologies(pkg, precision, topology):
    b, x, named, recs = _free_run(pkg, None, precision, **topology[1])
    _hold(b, recs, named, f"{precision} {topology[0]}")


@pytest.mark.parametrize("size", ((80, 112), (96, 160)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_emulator_stays_within_the_bound_when_int8_saturates(pkg, sd7, size):
    b, x, named, recs = _free_run(pkg, sd7, "int8", 0.5, in_h=size[0], in_w=size[1])
    _hold(b, recs, named, f"int8, ranges halved, {size[0]}x{size[1]}")
    from unina_yolo_dla_amd import export
    i8 = [bb[0] for bb in b.buffers if bb[4] == export.BUF_I8]
    assert sum(np.abs(named[n]).max() == 127 for n in i8) >= len(i8) / 2      # the clamp really runs


# ---- mutants: one op of the 80x112 table computed wrong, its output rounded as the epilogue rounds -> flagged ----
def _targets(b, want):
    """First backbone op and first neck op for which want(op, index) holds."""
    out = []
    for prefix in ("backbone.", "neck."):
        hit = [i for i, op in enumerate(b.ops) if op.name.startswith(prefix) and want(op, i)]
        assert hit, prefix
        out.append(hit[0])
    return out


def _flagged(b, x, named, recs, oi, kind):
    good = [r for r in recs if r["op"] == oi]
    wrong = E.per_op_bounds(b, x, named, mutate=dict(op=oi, kind=kind), only_op=oi)
    res = [E.check_slice(g, E.as_stored(w)) for g, w in zip(good, wrong)]
    # (the unmutated evaluation, rounded the same way, passes: what is flagged is the mutation, not the rounding)
    assert all(E.check_slice(g, E.as_stored(g))["violations"] == 0 for g in good)
    return sum(r["violations"] for r in res), res


@pytest.mark.parametrize("precision", ("fp16", "fp32", "strict"))
@pytest.mark.parametrize("kind", E.MUTANTS)
def test_float_mutants_are_flagged(pkg, sd7, precision, kind):
    from unina_yolo_dla_amd import export
    b, x, named, recs = _free_run(pkg, sd7, precision, in_h=80, in_w=112)
    conv = lambda op: op.kind == export.OP_CONV
    if kind in ("drop_tap", "edge_pad"):
        ops = _targets(b, lambda op, i: conv(op) and op.k == 3)
    elif kind == "bias_neighbour":
        ops = _targets(b, lambda op, i: conv(op))
    elif kind == "res_before_relu":
        ops = _targets(b, lambda op, i: conv(op) and op.res is not None)
    else:                                   # the x2 upsample lives in the neck's two lateral convs only
        ops = [i for i, op in enumerate(b.ops) if conv(op) and any(s.flags & export.SEG_UP2 for s in op.segs)]
        assert len(ops) == 2
    for oi in ops:
        n, _ = _flagged(b, x, named, recs, oi, kind)
        print(precision, kind, b.ops[oi].name, "flagged elements:", n)
        assert n > 0, (kind, b.ops[oi].name)


def test_stem_tap_mutant_is_flagged(pkg, sd7):
    b, x, named, recs = _free_run(pkg, sd7, "fp16", in_h=80, in_w=112)
    assert _flagged(b, x, named, recs, 0, "drop_tap")[0] > 0


@pytest.mark.parametrize("kind", ("drop_tap", "edge_pad", "res_before_relu", "up2_last_col", "bias_neighbour"))
def test_int8_conv_mutants_are_flagged(pkg, sd7, kind):
    """The same mutants on int8 convs (integer accumulators, requantising epilogue), backbone and neck."""
    from unina_yolo_dla_amd import export
    b, x, named, recs = _free_run(pkg, sd7, "int8", in_h=80, in_w=112)
    q = lambda op, i: op.kind == export.OP_CONV and b.op_int8[i]
    if kind in ("drop_tap", "edge_pad"):
        ops = _targets(b, lambda op, i: q(op, i) and op.k == 3)
    elif kind == "bias_neighbour":
        ops = _targets(b, q)
    elif kind == "res_before_relu":
        ops = _targets(b, lambda op, i: q(op, i) and op.res is not None)
    else:
        ops = [i for i, op in enumerate(b.ops) if q(op, i) and any(s.flags & export.SEG_UP2 for s in op.segs)]
        assert len(ops) == 2
    for oi in ops:
        n, _ = _flagged(b, x, named, recs, oi, kind)
        assert n > 0, (kind, b.ops[oi].name)


@pytest.mark.parametrize("kind", ("drop_tap", "edge_pad", "up2_last_col", "res_before_relu"))
def test_int8_mutants_on_graph_b_are_flagged(pkg, kind):
    """The ops graph (A) never instantiates, in the int8 engine of graph (B) at 96x160 (stride-32 map 3x5): the 3x3 int8 conv that
    writes the stride-32 map, the lateral conv that upsamples FROM it (the third FPN level), and every conv with a shortcut --
    picked by those properties, not by name."""
    from unina_yolo_dla_amd import export
    b, x, named, recs = _free_run(pkg, None, "int8", variant="B", in_h=96, in_w=160)
    hw = lambda buf: tuple(b.buffers[buf][1:3])
    s32 = (96 // 32, 160 // 32)
    q = lambda i: b.ops[i].kind == export.OP_CONV and b.op_int8[i]
    up2 = [i for i, op in enumerate(b.ops) if q(i) and any(s.flags & export.SEG_UP2 for s in op.segs)]
    assert len(up2) == 3                                         # graph (A) has two
    if kind in ("drop_tap", "edge_pad"):
        ops = [i for i, op in enumerate(b.ops) if q(i) and op.k == 3 and all(hw(s.dst.buf) == s32 for s in op.segs)]
        assert len(ops) == 1 and b.ops[ops[0]].s == 2, ops       # the stage's stride-2 conv, reading a 6x10 map
    elif kind == "up2_last_col":
        ops = [i for i in up2 if hw(b.ops[i].src_buf) == s32]
        assert len(ops) == 1, ops
    else:
        ops = [i for i, op in enumerate(b.ops) if q(i) and op.res is not None]
        assert ops                                               # every block's bottleneck that runs in int8, the third FPN block's too
    for oi in ops:
        n, _ = _flagged(b, x, named, recs, oi, kind)
        print("int8 B-96x160", kind, b.ops[oi].name, "flagged elements:", n)
        assert n > 0, (kind, b.ops[oi].name)


def _requantised(rec, how):
    t = rec["t"].astype(np.float32).astype(np.float64)
    if how == "half_away":
        return np.clip(np.sign(t) * np.floor(np.abs(t) + 0.5), -127, 127)
    return np.clip(np.rint(t), -128, 128)                                  # "clamp128"


def test_int8_clamp_at_128_is_flagged(pkg, sd7):
    """Ranges halved, so values beyond +-127.5 steps exist: a clamp at +-128 stores a code the bound never admits."""
    from unina_yolo_dla_amd import export
    b, x, named, recs = _free_run(pkg, sd7, "int8", 0.5, in_h=80, in_w=112)
    first = {r["op"]: r for r in reversed(recs)}
    sat = lambda op, i: (op.kind == export.OP_CONV and b.op_int8[i] and first[i]["dest"] == "i8"
                         and np.abs(first[i]["t"]).max() > 128.5)              # the op really saturates
    for oi in _targets(b, sat):
        rec = first[oi]
        assert E.check_slice(rec, _requantised(rec, "clamp128"))["violations"] > 0
        assert E.check_slice(rec, E.as_stored(rec))["violations"] == 0


def test_int8_round_half_away_exceeds_the_tie_cap_on_exact_ties(pkg, sd7):
    """Inputs built to contain exact ties: a backbone and a neck int8 conv whose multiplier is made 1/32 of the output step with
    no bias (t = acc / 32, every fp32 step exact), and the QUANT op fed fp16 values (n + 1/2) * step with a power-of-two step.
    Where the arithmetic is exact there is no slack: half-away codes differ from the half-even ones on every tie with an even
    n, none of them is excused, and their number exceeds the tie cap."""
    from unina_yolo_dla_amd import export
    b, x, named, _ = _free_run(pkg, sd7, "int8", in_h=80, in_w=112)
    plain = lambda op, i: (op.kind == export.OP_CONV and b.op_int8[i] and op.res is None and b.buffers[op.segs[0].dst.buf][4] == export.BUF_I8)
    saved_blob, saved_scales = bytes(b.blob), [bb[6] for bb in b.buffers]
    try:
        for oi in _targets(b, plain):
            op = b.ops[oi]
            s = op.segs[0]
            b.buffers[s.dst.buf][6] = 2.0 ** -3
            b.blob[s.m_off:s.m_off + 4 * s.n_pad] = np.full(s.n_pad, 2.0 ** -8, "<f4").tobytes()
            b.blob[s.b_off:s.b_off + 4 * s.n_pad] = np.zeros(s.n_pad, "<f4").tobytes()
            rec = E.per_op_bounds(b, x, named, only_op=oi)[0]
            ties = (np.abs(rec["t"]) % 1 == 0.5) & (np.abs(rec["t"]) < 127)
            print(b.ops[oi].name, "exact ties:", int(ties.sum()))
            assert ties.sum() > 20 and (rec["slack"][ties] == 0).all()
            ok = E.check_slice(rec, E.as_stored(rec))
            bad = E.check_slice(rec, _requantised(rec, "half_away"))
            assert ok["violations"] == 0 and ok["mismatches"] == 0
            assert bad["violations"] > 0 and bad["mismatches"] > bad["cap"], (b.ops[oi].name, bad)
        oi = next(i for i, op in enumerate(b.ops) if op.kind == export.OP_QUANT)
        op = b.ops[oi]
        b.buffers[op.segs[0].dst.buf][6] = 2.0 ** -4
        src = b.buffers[op.src_buf][0]
        forced = dict(named)
        n = np.arange(named[src].size, dtype=np.float64).reshape(named[src].shape) % 255 - 127.5      # -127.5 ... 126.5
        forced[src] = (n * 2.0 ** -4).astype(np.float16).astype(np.float32)
        assert np.array_equal(forced[src].astype(np.float64), n * 2.0 ** -4)
        rec = E.per_op_bounds(b, x, forced, only_op=oi)[0]
        assert (rec["slack"] == 0).all()
        ok = E.check_slice(rec, E.as_stored(rec))
        bad = E.check_slice(rec, _requantised(rec, "half_away"))
        assert ok["violations"] == 0 and bad["violations"] > 0 and bad["mismatches"] > bad["cap"], bad
    finally:
        b.blob[:] = saved_blob
        for bb, sc in zip(b.buffers, saved_scales):
            bb[6] = sc
