"""Shared by tests/test_gpu_launched_heads.py, tests/test_launched_heads_cpu.py and their child processes: the checks of the P3 /
P4 head path of the frame AS LAUNCHED (fusion on: dual launches of the 3x3 layers, output convs folded into the decode launch),
and -- run as a script -- the same checks in a fresh process, because UNINA_DUAL_WS and UNINA_POST_FOLD are read once per process.

  python tests/launched_heads_child.py bound <precision> <HxW> [<HxW> ...]     hold_launched_frame at every size; exit code 0 = held
  python tests/launched_heads_child.py decode <precision> <out.npz> <HxW> ...  the records of infer(x, 0, 1, q) for q in DECODE_QS,
                                                                                and which heads the decode launch folds
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

# 80x112 and 96x160: partial tiles on every level, but no P3 map there has 16 rows and no P4 map 8 -- the last rows of the pair's
# 16 x 16 | 8 x 16 tiles (the last patch row of conv3x3_wsc_body, which feeds the ky = 2 taps of the tile's last row alone) would
# never be computed. 144x144: P3 18 x 18 and P4 9 x 9, a full tile and a partial one in both directions.
SIZES = ((80, 112), (96, 160), (144, 144))
DECODE_SIZES = ((16, 16), (16, 48), (80, 112))
DECODE_QS = (0.0, 0.1)
IDS = lambda s: f"{s[0]}x{s[1]}"

# The dual launch of the P3 | P4 head layers per precision (conv_igemm.hip kDual): the kernel op_infos() must name, and the
# single tile configurations whose bodies it instantiates (conv3x3_wsc_body<T, TH, CIN, NCHUNK, NW>), P3's then P4's, by the
# names the engine gives them in that precision's row of the configuration table.
DUAL = {
    "fp16": ("conv_dual_head3x3_ws<", ("conv3x3_ws<f16,16x16,128/2,4w>", "conv3x3_ws<f16,8x16,256/4,4w>")),
    "int8": ("conv_dual_head3x3_ws_i8<", ("conv3x3_ws<i8,16x16,128/2,4w>", "conv3x3_ws<i8,8x16,256/4,4w>")),
    "strict": ("conv_dual_head3x3_ws_s16<", ("conv3x3_ws<s16,16x16,128/4,4w>", "conv3x3_ws<s16,8x16,256/4,4w>")),
    "fp16-small": ("conv_dual_head3x3_ws_small<", ("conv3x3_ws<f16,8x16,128/2,4w>", "conv3x3_ws<f16,4x16,256/4,4w>")),
}
# UNINA_DUAL_WS=0: the register-queue pairs
DUAL_REGQ = {"fp16": "conv_dual_head3x3<", "int8": "conv_dual_head3x3_i8<", "strict": "conv_dual_head3x3_s16<"}

# Graph (A)'s fused groups as (first op, last op) by graph.py's names -- the stand-in for op_infos() where there is no engine
# (tests/test_launched_heads_cpu.py); the GPU test holds the engine's own op_infos() to this list at 80x112.
GROUPS_A = (
    ("c3k2_fused", "backbone.stage1_conv", "backbone.stage1_block.cv3"),
    ("c3k2_fused", "backbone.stage2_c3k2.cv1+backbone.stage2_c3k2.cv2", "backbone.stage2_c3k2.cv3"),
    ("c3k2_fused", "backbone.stage3_c3k2.cv1+backbone.stage3_c3k2.cv2", "backbone.sppf.cv1"),
    ("conv_pair", "backbone.sppf.pool1+pool2+pool3", "neck.lateral_p3"),          # (STRICT: from backbone.sppf.cv2, the pool is a launch of its own)
    ("c3k2_fused", "neck.fpn_c3k2_1.cv1+neck.fpn_c3k2_1.cv2", "neck.lateral_p2"),
    ("c3k2_fused", "neck.fpn_c3k2_2.cv1+neck.fpn_c3k2_2.cv2", "neck.fpn_c3k2_2.cv3"),
    ("c3k2_fused", "neck.down1", "neck.pan_c3k2_1.cv3"),
    ("c3k2_fused", "neck.down2", "neck.pan_c3k2_2.cv3"),
    ("head_fused", "head_p2.cls_branch.0+head_p2.reg_branch.0", "head_p2.cls_branch.2+head_p2.reg_branch.2"),   # (fp16 engines only)
)
# ... and the ops that are then held on the launched frame's own buffers (emulate.launched_ops), besides the six head ops of
# P3 / P4: the stem, the two stage convs that lead into a block, and the three convs at a group's end with both ends in memory
STRICT_PAIR_FIRST = "backbone.sppf.cv2"
EDGE_OPS_A = ("backbone.stem", "backbone.stage2_conv", "backbone.stage3_conv", "backbone.sppf.cv1", "neck.lateral_p3", "neck.lateral_p2")


def stand_in_infos(builder, strict):
    """op_infos() as an engine with fusion on would report it for graph (A), from GROUPS_A (STRICT engines have no head kernel)."""
    names = [op.name for op in builder.ops]
    infos = [dict(name=n, kernel="own") for n in names]
    for kind, first, last in GROUPS_A[:-1] if strict else GROUPS_A:
        if strict and kind == "conv_pair":
            first = STRICT_PAIR_FIRST
        a, z = names.index(first), names.index(last)
        infos[a]["kernel"] = kind + "<...>"
        for k in range(a + 1, z + 1):
            infos[k]["kernel"] = f"(fused into op {a})"
    return infos


def expected_ops_a(builder, strict):
    import emulate as E
    names = [op.name for op in builder.ops]
    ops = {names.index(n) for n in EDGE_OPS_A} | {oi for lv in E.head_ops(builder).values() for oi in lv}
    if strict:     # no split-fp16 head kernel: the P2 head's ops are launches; the pool's maps are in memory, so sppf.cv2 is held too
        ops |= set(E.head_ops(builder, ("p2",))["p2"]) | {names.index("backbone.sppf.pool1+pool2+pool3"), names.index(STRICT_PAIR_FIRST)}
    return sorted(ops)


def smallest_half_height_size(limit=8192):
    """The smallest legal input (H, W multiples of 16, by pixel count) at which conv_dual_match picks the half-height pair: the
    grids of the full-height pair together exceed 256 workgroups. conv_grid: (ceil(Ho / th) * ceil(Wo / tw)) M tiles times
    n_tiles = sum over the two slices of ceil(n_pad / 64) N tiles. P3 (Ho, Wo) = (H / 8, W / 8), 16 x 16 tiles, two slices of
    128 channels: 4 N tiles; P4 (H / 16, W / 16), 8 x 16 tiles, two slices of 256: 8 N tiles."""
    up = lambda a, b: -(-a // b)
    best = None
    for h in range(16, limit + 1, 16):
        if best and h * 16 >= best[0]:
            break
        for w in range(16, limit + 1, 16):
            if best and h * w >= best[0]:
                break
            ga = up(h // 8, 16) * up(w // 8, 16) * 4
            gb = up(h // 16, 8) * up(w // 16, 16) * 8
            if ga + gb > 256:
                best = (h * w, h, w, ga, gb)
                break
    return best[1:]


def _buffers_of(builder, ops):
    return sorted({builder.buffers[s.dst.buf][0] for oi in ops for s in builder.ops[oi].segs})


def hold_launched_frame(pkg, sd7, torch, tmp_path, precision, size, dual_prefix, check_groups=False):
    """Section 1: one forward with fusion on, every op whose slices all reach memory held to its float64 bound on the frame's own
    buffers. Returns (checked ops, worst error / bound)."""
    import emulate as E
    from test_gpu_per_op import _amax, _hold, _make, _teacher
    from test_gpu_parity import WRITTEN_WHEN_FUSED
    g = pkg.graph.Graph(in_h=size[0], in_w=size[1])
    b, e, _ = _make(pkg, sd7, g, precision, tmp_path, _amax(pkg, sd7, size) if precision == "int8" else None)
    try:
        assert e.set_fusion(True) > 0
        infos = e.op_infos()
        assert len(infos) == len(b.ops)
        heads = E.head_ops(b)
        # not vacuous (a): the four 3x3 layers run as the pair kernel this precision selects, P3's op leading P4's
        for j in (0, 1):
            for lv in ("p3", "p4"):
                k = E.launched_kernel(infos, heads[lv][j])
                assert k.startswith(dual_prefix) and "stamped" not in k, (lv, j, k)
            pair = {oi if "(dual" not in infos[oi]["kernel"] else int(infos[oi]["kernel"].split()[-1][:-1]) for oi in (heads["p3"][j], heads["p4"][j])}
            assert len(pair) == 1, (j, pair)                       # P3's and P4's layer j are ONE launch
        written = E.written_when_launched(b, infos)
        for name, (c0, c1) in WRITTEN_WHEN_FUSED.items():
            if name in written:
                want = np.zeros(len(written[name]), dtype=bool)
                want[c0:c1] = True
                # (a STRICT engine's SPPF pool is a launch of its own: it writes the pooled maps too)
                assert np.array_equal(written[name], want) if precision != "strict" else written[name][want].all(), name
        ops = E.launched_ops(b, infos, written)
        # not vacuous (b): all six head ops of each level are among them
        assert {oi for lv in heads.values() for oi in lv} <= set(ops), (heads, ops)
        if check_groups and precision != "int8":
            groups, _ = E.launched_groups(infos)
            assert groups == E.launched_groups(stand_in_infos(b, precision == "strict"))[0], [(b.ops[k].name, b.ops[v[-1]].name) for k, v in groups.items()]
            assert ops == expected_ops_a(b, precision == "strict"), [b.ops[oi].name for oi in ops]
        # not vacuous (c): every slice taken as written really is -- it changes with the frame
        e.forward(torch.from_numpy(pkg.rng.frame(4321, *size)).cuda())
        other = E.engine_buffers(b, e.read_buffer)
        x = pkg.rng.frame(1234, *size)
        teacher = _teacher(b, e, torch.from_numpy(x).cuda())
        for oi in ops:
            for s in b.ops[oi].segs:
                name = b.buffers[s.dst.buf][0]
                c0, c1 = s.dst.coff, s.dst.coff + s.n_count
                assert teacher[name][c0:c1].tobytes() != other[name][c0:c1].tobytes(), (b.ops[oi].name, name)
        recs = _hold(b, x, teacher, f"launched frame, {precision} {IDS(size)}, {dual_prefix[:-1]}, {len(ops)} ops", ops=ops)
        assert {r["op"] for r in recs} == set(ops)
        return ops
    finally:
        e.close()


def find_config(e, op_index, kernel):
    """Forces on op `op_index` the tile configuration whose kernel the engine names `kernel`; returns its index (None: no
    configuration that fits the op carries that name)."""
    for cfg in range(len(e.conv_configs())):
        if e.set_op_config(op_index, cfg):
            if e.op_infos()[op_index]["kernel"] == kernel:
                return cfg
            e.set_op_config(op_index, -1)
    return None


def force_twins(e, b, twins):
    """The four 3x3 head ops of P3 / P4 forced to the single configurations `twins` = (P3's, P4's); returns the forced ops."""
    import emulate as E
    heads = E.head_ops(b)
    forced = []
    for lv, kernel in zip(("p3", "p4"), twins):
        for oi in heads[lv][:2]:
            cfg = find_config(e, oi, kernel)
            assert cfg is not None, (b.ops[oi].name, kernel)
            if "<f16," in kernel:
                assert e.conv_configs()[cfg] == kernel
            forced.append(oi)
    return forced


def head_buffers(e, b):
    """The hidden buffers behind layer 0 and layer 1 and the four head planes of P3 / P4, as bytes."""
    import emulate as E
    heads = E.head_ops(b)
    names = _buffers_of(b, [oi for lv in heads.values() for oi in lv])
    assert len(names) == 8, names
    return {n: e.read_buffer(n).tobytes() for n in names}


def exact_twin(pkg, sd7, torch, tmp_path, precision, size, key=None, fused_upstream=False):
    """Section 2: the per-op table with the four 3x3 head ops forced to the single configurations of the pair's bodies, against
    the frame as launched. Returns {buffer: equal?} over the eight buffers (and, under "upstream", whether the heads' inputs were
    the same bytes in both runs). fused_upstream: fusion stays on in the first run too (a forced configuration alone takes an op
    out of its pair), so both runs read the block kernels' outputs."""
    import emulate as E
    from test_gpu_per_op import _amax, _make
    prefix, twins = DUAL[key or precision]
    g = pkg.graph.Graph(in_h=size[0], in_w=size[1])
    b, e, _ = _make(pkg, sd7, g, precision, tmp_path, _amax(pkg, sd7, size) if precision == "int8" else None)
    try:
        xd = torch.from_numpy(pkg.rng.frame(1234, *size)).cuda()
        heads = E.head_ops(b)
        inputs = sorted({b.buffers[b.ops[heads[lv][0]].src_buf][0] for lv in heads})
        if fused_upstream:
            assert e.set_fusion(True) > 0
        else:
            assert e.set_fusion(False) == 0
        forced = force_twins(e, b, twins)
        infos = e.op_infos()
        assert [infos[oi]["kernel"] for oi in forced] == [twins[0]] * 2 + [twins[1]] * 2
        e.forward(xd)
        single = head_buffers(e, b)
        single_in = {n: e.read_buffer(n).tobytes() for n in inputs}
        for oi in forced:
            assert e.set_op_config(oi, -1)
        assert e.set_fusion(True) > 0
        infos = e.op_infos()
        for oi in forced:
            assert E.launched_kernel(infos, oi).startswith(prefix), (b.ops[oi].name, E.launched_kernel(infos, oi))
        e.forward(xd)
        dual = head_buffers(e, b)
        out = {n: single[n] == dual[n] for n in single}
        out["upstream"] = all(single_in[n] == e.read_buffer(n).tobytes() for n in inputs)
        return out
    finally:
        e.close()


def n_cells(size):
    return sum((size[0] // s) * (size[1] // s) for s in (4, 8, 16))


def decode_records(pkg, sd7, torch, precision, sizes):
    """{"HxW_q": records of infer(x, 0, 1, q) as launched, "HxW_folded": the heads the decode launch folds}."""
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine
    out = {}
    for size in sizes:
        e = Engine.from_state_dict(sd7, pkg.graph.Graph(in_h=size[0], in_w=size[1]),
                                   precision={"fp16": export.FP16, "strict": export.STRICT}[precision])
        try:
            xd = torch.from_numpy(pkg.rng.frame(1234, *size)).cuda()
            out[f"{IDS(size)}_folded"] = np.array(e.folded_heads())
            for q in DECODE_QS:
                out[f"{IDS(size)}_{q}"] = e.infer(xd, 0.0, 1.0, q)
        finally:
            e.close()
    return out


def main(argv):
    import tempfile
    import pathlib
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import unina_yolo_dla_amd as pkg
    sd7 = pkg.synth.make_state_dict(7, pkg.graph.Graph())
    mode, precision = argv[0], argv[1]
    parse = lambda s: tuple(int(v) for v in s.split("x"))
    if mode == "bound":
        prefix = DUAL_REGQ[precision] if os.environ.get("UNINA_DUAL_WS") == "0" else DUAL[precision][0]
        for size in map(parse, argv[2:]):
            with tempfile.TemporaryDirectory() as tmp:
                hold_launched_frame(pkg, sd7, torch, pathlib.Path(tmp), precision, size, prefix)
    elif mode == "decode":
        np.savez(argv[2], **decode_records(pkg, sd7, torch, precision, [parse(s) for s in argv[3:]]))
    else:
        raise SystemExit(f"unknown mode {mode!r}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
