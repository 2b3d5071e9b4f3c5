"""Every element of every op's output against a float64 evaluation of that op on the ENGINE'S OWN inputs (teacher-forced,
tests/emulate.py per_op_bounds), held to the bound the arithmetic allows -- no fraction, no exempt element.
The other forward checks are sized for a whole tensor or compare one form of the engine with another; a wrong tap at the
pixels of a partial tile, in code every form shares, passes all of them. Sizes: the smallest legal input (every map smaller
than every tile), a one-row map, odd maps, partial tiles on every level. Topologies (emulate.PER_OP_TOPOLOGIES): graph (B) with a
stride-32 map of 1x1, 1x3 and 3x5, the lite P2 stage, a 16-channel model, 1 / 7 / 20 classes -- in all four precisions, under
every tile configuration and as the frame launches them."""
import numpy as np
import pytest

import emulate as E

pytestmark = pytest.mark.gpu

SIZES = E.PER_OP_SIZES
TOPOLOGY = {t[0]: t for t in E.PER_OP_TOPOLOGIES}
IDS = lambda s: f"{s[0]}x{s[1]}"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_amax_cache = {}
_topology_cache = {}


def _amax(pkg, sd, key, scale=1.0, graph=None):
    """Calibrated int8 ranges of state dict `sd`, cached under `key`: a size (h, w) -- graph (A) at that size --, or a topology's
    label with its `graph` (base16 at 80x112 is not graph (A) at 80x112)."""
    from unina_yolo_dla_amd.engine import calibrate_amax
    if key not in _amax_cache:
        g = pkg.graph.Graph(in_h=key[0], in_w=key[1]) if graph is None else graph
        _amax_cache[key] = calibrate_amax(sd, g, [pkg.rng.frame(5000 + i, g.in_h, g.in_w) for i in range(2)])
    return {k: v * scale for k, v in _amax_cache[key].items()}


def _topology(pkg, topology):
    """(label, graph, its seed-7 state dict) of one entry of emulate.PER_OP_TOPOLOGIES."""
    label, kw = topology
    if label not in _topology_cache:
        g = pkg.graph.Graph(**kw)
        _topology_cache[label] = (g, pkg.synth.make_state_dict(7, g))
    return (label, *_topology_cache[label])


def _make_topology(pkg, topology, precision, tmp_path, amax_scale=1.0):
    """_make for a topology, its int8 ranges calibrated on that topology: (label, graph, builder, engine, path)."""
    label, g, sd = _topology(pkg, topology)
    b, e, path = _make(pkg, sd, g, precision, tmp_path, _amax(pkg, sd, label, amax_scale, g) if precision == "int8" else None)
    return label, g, b, e, path


def _make(pkg, sd, g, precision, tmp_path, amax=None):
    """(builder, engine loaded from the file the builder wrote, that file's path)"""
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine
    p = {"fp16": export.FP16, "fp32": export.FP32, "strict": export.STRICT, "int8": export.INT8}[precision]
    b = export.EngineBuilder(sd, g, p, amax)
    path = str(tmp_path / "e.une")
    b.save(path)
    return b, Engine(path), path


def _teacher(b, e, xd):
    """One forward, every buffer read back; the heads forward() returns are the planar output buffers."""
    heads = e.forward(xd)
    teacher = E.engine_buffers(b, e.read_buffer)
    for k, v in heads.items():
        assert np.array_equal(v, teacher[k]), k
    return teacher


def _hold(b, x, teacher, label, ops=None):
    recs = E.per_op_bounds(b, x, teacher, only_op=ops)
    fails, worst, ties = E.check_per_op(recs, teacher)
    print(f"per-op bound: {label}: {len(recs)} slices, {sum(r['y'].size for r in recs)} elements, worst error/bound {worst:.3f}")
    for buf, (m, cap) in ties.items():
        if m or cap:
            print(f"per-op bound: {label}: int8 {buf}: {m} codes off the half-even code of the float64 t, tie cap {cap}")
    assert not fails, "\n".join(fails[:8])
    assert worst <= 1.0
    return recs


@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("precision", ["fp16", "fp32", "strict", "int8"])
def test_per_op_table_every_buffer(pkg, sd7, torch_cuda, tmp_path, precision, size):
    g = pkg.graph.Graph(in_h=size[0], in_w=size[1])
    b, e, _ = _make(pkg, sd7, g, precision, tmp_path, _amax(pkg, sd7, size) if precision == "int8" else None)
    try:
        assert e.set_fusion(False) == 0
        assert len(e.op_infos()) == len(b.ops)
        x = pkg.rng.frame(1234, *size)
        teacher = _teacher(b, e, torch_cuda.from_numpy(x).cuda())
        recs = _hold(b, x, teacher, f"{precision} {IDS(size)}")
        assert {r["buf"] for r in recs} == set(teacher)          # every buffer is some op's output and was checked
    finally:
        e.close()


@pytest.mark.parametrize("size", [(80, 112), (96, 160)], ids=IDS)
def test_per_op_table_int8_with_saturation(pkg, sd7, torch_cuda, tmp_path, size):
    """Calibrated ranges halved: the clamp at +-127 really runs (with the max calibrator a frame of the calibration
    distribution almost never clips)."""
    from unina_yolo_dla_amd import export
    g = pkg.graph.Graph(in_h=size[0], in_w=size[1])
    b, e, _ = _make(pkg, sd7, g, "int8", tmp_path, _amax(pkg, sd7, size, 0.5))
    try:
        e.set_fusion(False)
        x = pkg.rng.frame(1234, *size)
        teacher = _teacher(b, e, torch_cuda.from_numpy(x).cuda())
        i8 = [bb[0] for bb in b.buffers if bb[4] == export.BUF_I8]
        assert sum(np.abs(teacher[n]).max() == 127 for n in i8) >= len(i8) / 2
        assert all(np.abs(teacher[n]).max() <= 127 for n in i8)
        _hold(b, x, teacher, f"int8, ranges halved, {IDS(size)}")
    finally:
        e.close()


def test_per_op_table_int8_with_saturation_graph_b(pkg, torch_cuda, tmp_path):
    """The same on graph (B) at 96x160: the clamp runs on the ops graph (A) never instantiates (the stride-32 stage, the third
    FPN level)."""
    from unina_yolo_dla_amd import export
    label, g, b, e, _ = _make_topology(pkg, TOPOLOGY["B-96x160"], "int8", tmp_path, 0.5)
    try:
        e.set_fusion(False)
        x = pkg.rng.frame(1234, g.in_h, g.in_w)
        teacher = _teacher(b, e, torch_cuda.from_numpy(x).cuda())
        i8 = [bb[0] for bb in b.buffers if bb[4] == export.BUF_I8]
        assert sum(np.abs(teacher[n]).max() == 127 for n in i8) >= len(i8) / 2
        assert all(np.abs(teacher[n]).max() <= 127 for n in i8)
        only_b = [b.ops[oi].segs[0].dst.buf for oi in _ops_graph_a_lacks(pkg, b, g)]
        assert any(b.buffers[i][4] == export.BUF_I8 and np.abs(teacher[b.buffers[i][0]]).max() == 127 for i in only_b)
        _hold(b, x, teacher, f"int8, ranges halved, {label}")
    finally:
        e.close()


def _op_shape(b, op):
    """What an op computes, without its name: kind, kernel, stride, input channels, per slice (channels, x2 upsample), output map."""
    from unina_yolo_dla_amd import export
    return (op.kind, op.k, op.s, op.cin, tuple((s.n_count, bool(s.flags & export.SEG_UP2)) for s in op.segs),
            tuple(b.buffers[op.segs[0].dst.buf][1:3]))


def _ops_graph_a_lacks(pkg, b, g):
    """Indices of the ops of graph (B)'s table `b` whose shape (_op_shape) no op of graph (A) at the same input size has: the
    stride-32 stage, the lateral conv out of it and the FPN level it feeds."""
    from unina_yolo_dla_amd import export
    ga = pkg.graph.Graph(num_classes=g.num_classes, base_channels=g.base_channels, in_h=g.in_h, in_w=g.in_w)
    a = export.EngineBuilder(pkg.synth.make_state_dict(7, ga), ga)
    have = {_op_shape(a, op) for op in a.ops}
    out = [oi for oi, op in enumerate(b.ops) if op.kind in (export.OP_CONV, export.OP_SPPF_POOL) and _op_shape(b, op) not in have]
    s32 = (g.in_h // 32, g.in_w // 32)
    assert any(tuple(b.buffers[b.ops[oi].segs[0].dst.buf][1:3]) == s32 for oi in out)       # the stride-32 map is among them
    return out


# (STRICT at 80x112 only: the smallest of these sizes, every level has a partial tile; the split-fp16 rows are the table's most irregular)
# A size stands for graph (A) at that size; graph (B) at 96x160 (a 3x5 stride-32 map) and at 32x32 (every map smaller than every tile)
TILE_CASES = [(p, s) for p in ("fp16", "int8") for s in ((80, 112), (96, 160))] + [("strict", (80, 112))] + \
             [("fp16", "B-96x160"), ("int8", "B-96x160"), ("int8", "B-32x32")]
TILE_ID = lambda s: s if isinstance(s, str) else IDS(s)


@pytest.mark.parametrize("precision,size", TILE_CASES, ids=[f"{p}-{TILE_ID(s)}" for p, s in TILE_CASES])
def test_every_tile_configuration_within_the_bound(pkg, sd7, torch_cuda, tmp_path, precision, size):
    """Each tile configuration forced on every op that accepts it, then the autotuner's choice: the outputs of those ops
    against float64 (test_tile_configs_and_autotune_are_bit_identical compares them with the default configuration only).
    STRICT engines: the heads under every forced configuration also stay within the 5e-5 of the default configuration's that
    test_frame_as_launched_equals_per_op_table allows a strict frame (the configurations differ in fp32 summation order).
    Graph (A): at least 6 configurations fit some op. Graph (B): the configurations that fit an op graph (A) lacks are counted
    and printed, and there is at least one."""
    if isinstance(size, str):
        label, g, b, e, _ = _make_topology(pkg, TOPOLOGY[size], precision, tmp_path)
        only_b = set(_ops_graph_a_lacks(pkg, b, g))
    else:
        g, label, only_b = pkg.graph.Graph(in_h=size[0], in_w=size[1]), IDS(size), None
        b, e, _ = _make(pkg, sd7, g, precision, tmp_path, _amax(pkg, sd7, size) if precision == "int8" else None)
    try:
        e.set_fusion(False)
        x = pkg.rng.frame(1234, g.in_h, g.in_w)
        xd = torch_cuda.from_numpy(x).cuda()
        infos = e.op_infos()
        names = e.conv_configs()
        default = {k: v.copy() for k, v in e.forward(xd).items()} if precision == "strict" else None
        tried = tried_only_b = 0
        for cfg in range(len(names)):
            applied = [i for i, o in enumerate(infos) if o["kind"] == 1 and e.set_op_config(i, cfg)]
            if not applied:
                continue
            tried += 1
            tried_only_b += bool(only_b and only_b & set(applied))
            teacher = _teacher(b, e, xd)
            _hold(b, x, teacher, f"{precision} {label} config {cfg} {names[cfg]} on {len(applied)} ops", ops=applied)
            for k in default or ():
                np.testing.assert_allclose(teacher[k], default[k], atol=5e-5, rtol=0, err_msg=f"config {cfg} {k}")
            for i in applied:
                e.set_op_config(i, -1)
        if only_b is None:
            assert tried >= 6
        else:
            print(f"per-op bound: {precision} {label}: {tried} configurations fit some op, {tried_only_b} of them one of the "
                  f"{len(only_b)} ops graph (A) lacks: {sorted(b.ops[oi].name for oi in only_b)}")
            assert tried_only_b > 0
        e.autotune(xd, iters=3)
        _hold(b, x, _teacher(b, e, xd), f"{precision} {label} autotuned")
    finally:
        e.close()


@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("precision", ["fp16", "int8", "strict"])
def test_frame_as_launched_equals_per_op_table(pkg, sd7, torch_cuda, tmp_path, precision, size):
    """The fused frame at the new sizes, by the existing contracts: fp16 block outputs and the P2 head bit for bit, P3 / P4
    heads per same_head; int8 bit for bit; STRICT within fp32 noise. No launch census at sizes where a group may fall back:
    only that the engine fuses what the loader's host-side planner says is fusable."""
    from test_gpu_parity import BLOCK_OUTPUTS, written, same_head
    g = pkg.graph.Graph(in_h=size[0], in_w=size[1])
    b, e, path = _make(pkg, sd7, g, precision, tmp_path, _amax(pkg, sd7, size) if precision == "int8" else None)
    try:
        groups = e.set_fusion(True)
        assert groups == e.L.unina_fusion_groups(e.h) == e.L.unina_debug_fusable_groups(path.encode())
        xd = torch_cuda.from_numpy(pkg.rng.frame(1234, *size)).cuda()
        fused = {k: v.copy() for k, v in e.forward(xd).items()}
        names = [bb[0] for bb in b.buffers]
        if precision == "fp16":
            bufs = BLOCK_OUTPUTS
        elif precision == "int8":
            bufs = tuple(n for n in ("neck.cat_fpn1", "neck.cat_pan1", "neck.cat_pan2", "p3_out", "p4_out", "backbone.sppf.cat",
                                     "neck.cat_fpn2", "p2_fused", "p2_fused.q8") if n in names)
            assert len(bufs) == 9
        else:
            bufs = ("p2_fused", "p3_out", "p4_out", "backbone.sppf", "neck.cat_fpn1", "neck.cat_fpn2")
        fbuf = {n: e.read_buffer(n) for n in bufs}
        assert e.set_fusion(False) == 0
        plain = e.forward(xd)
        for k in plain:
            if precision == "fp16":
                same_head(fused[k], plain[k], k)
            elif precision == "int8":
                assert np.array_equal(fused[k], plain[k]), k
            else:
                np.testing.assert_allclose(fused[k], plain[k], atol=5e-5, rtol=0, err_msg=k)
        for n in bufs:
            want = e.read_buffer(n)
            if precision == "strict":
                np.testing.assert_allclose(fbuf[n], want, atol=2e-5 * max(1.0, float(np.abs(want).max())), rtol=0, err_msg=n)
            else:
                assert np.array_equal(written(n, fbuf[n]), written(n, want)), n
        print(f"per-op bound: {precision} {IDS(size)}: {groups} fused groups, frame as launched = per-op table")
    finally:
        e.close()




@pytest.mark.parametrize("topology", E.PER_OP_TOPOLOGIES, ids=lambda t: t[0])
@pytest.mark.parametrize("precision", ["fp16", "fp32", "strict", "int8"])
def test_per_op_table_other_topologies(pkg, torch_cuda, tmp_path, precision, topology):
    """Graph (B) down to a 1x1 stride-32 map (and one row of three, and 3x5), the lite P2 stage, a 16-channel model embedded at
    width 32 (its zero channels read exactly 0: a slice whose terms are all zero has a bound of 0; an int8 destination stores
    the code 0 there), 1 / 7 / 20 classes (output rows padded to 16). int8 ranges are calibrated on the topology itself."""
    label, g, b, e, _ = _make_topology(pkg, topology, precision, tmp_path)
    try:
        e.set_fusion(False)
        assert len(e.op_infos()) == len(b.ops)
        x = pkg.rng.frame(1234, g.in_h, g.in_w)
        teacher = _teacher(b, e, torch_cuda.from_numpy(x).cuda())
        recs = _hold(b, x, teacher, f"{precision} {label}")
        assert {r["buf"] for r in recs} == set(teacher)          # every buffer is some op's output and was checked
        if label == "base16":
            dead = [(r, np.flatnonzero((r["S"] == 0).all(axis=(1, 2)))) for r in recs if r["S"] is not None]
            assert sum(len(ch) for _, ch in dead) > 100
            for r, ch in dead:
                stored = teacher[r["buf"]][r["c0"]:r["c1"]][ch]           # (int8 buffers: the stored codes)
                assert not stored.any() and (r["dest"] != "i8" or (stored == 0).all()), r["name"]
            assert precision != "int8" or sum(len(ch) for r, ch in dead if r["dest"] == "i8") > 100
        if label.startswith("classes"):
            assert teacher["p4_cls"].shape[0] == g.num_classes
    finally:
        e.close()


FRAME_TOPOLOGIES = [TOPOLOGY[k] for k in ("B-32x32", "B-32x96", "B-96x160", "lite_p2", "base16")]


def _observable(b, infos, fused_only):
    """{buffer name: channel mask} of what the frame with fusion on stores (emulate.written_when_launched), the input image
    left out; fused_only: of that, what the ops inside fused groups store -- the block outputs."""
    from unina_yolo_dla_amd import export
    mask = E.written_when_launched(b, infos)
    if fused_only:
        groups, _ = E.launched_groups(infos)
        keep = {bb[0]: np.zeros(bb[3], dtype=bool) for bb in b.buffers}
        for oi in {*groups, *(m for ms in groups.values() for m in ms)}:
            for buf, c0, c1 in E.op_writes(b.ops[oi]):
                keep[b.buffers[buf][0]][c0:c1] = True
        mask = {n: m & keep[n] for n, m in mask.items()}
    inputs = {bb[0] for bb in b.buffers if bb[5] & export.BUF_INPUT or bb[4] == export.BUF_F32_NCHW_IN}
    return {n: m for n, m in mask.items() if m.any() and n not in inputs}


@pytest.mark.parametrize("topology", FRAME_TOPOLOGIES, ids=lambda t: t[0])
@pytest.mark.parametrize("precision", ["fp16", "int8", "strict"])
def test_frame_as_launched_equals_per_op_table_other_topologies(pkg, torch_cuda, tmp_path, precision, topology):
    """test_frame_as_launched_equals_per_op_table on graph (B), the lite P2 stage and the 16-channel model, by the same
    contracts: int8 heads and every buffer the frame stores bit for bit; fp16 heads per same_head and what the fused groups
    store (the block outputs) bit for bit; STRICT heads within 5e-5 and what the fused groups store within fp32 noise. The
    buffers are not listed by hand: emulate.written_when_launched says what the frame stores, and where test_gpu_parity's
    `written` knows a buffer it must name the same channels. Then the launched frame's own buffers against float64, for every
    op whose slices all reach memory in that frame (the method of tests/test_gpu_launched_heads.py)."""
    from test_gpu_parity import WRITTEN_WHEN_FUSED, written, same_head
    label, g, b, e, path = _make_topology(pkg, topology, precision, tmp_path)
    try:
        groups = e.set_fusion(True)
        assert groups == e.L.unina_fusion_groups(e.h) == e.L.unina_debug_fusable_groups(path.encode())
        if (label, precision) == ("B-96x160", "int8"):
            assert groups > 0                                      # (the comparison cannot pass because nothing fused)
        infos = e.op_infos()
        assert len(E.launched_groups(infos)[0]) == groups
        stored = E.written_when_launched(b, infos)
        bufs = _observable(b, infos, fused_only=precision != "int8")
        assert len(bufs) >= min(groups, 1)                         # a frame that fuses stores something a fused group wrote
        through_written = [n for n in bufs if written(n, stored[n]).all()]     # `written` keeps of them only what the frame stores
        assert set(bufs) & set(WRITTEN_WHEN_FUSED) <= set(through_written)
        e.forward(torch_cuda.from_numpy(pkg.rng.frame(4321, g.in_h, g.in_w)).cuda())
        other = E.engine_buffers(b, e.read_buffer)
        x = pkg.rng.frame(1234, g.in_h, g.in_w)
        xd = torch_cuda.from_numpy(x).cuda()
        launched = _teacher(b, e, xd)
        fused = {k: launched[k].copy() for k in pkg.graph.OUTPUT_NAMES}
        fbuf = {n: e.read_buffer(n) for n in bufs}
        ops = E.launched_ops(b, infos, stored)
        for oi in ops:                                             # every slice taken as stored changes with the frame
            for buf, c0, c1 in E.op_writes(b.ops[oi]):
                n = b.buffers[buf][0]
                assert launched[n][c0:c1].tobytes() != other[n][c0:c1].tobytes(), (b.ops[oi].name, n)
        assert e.set_fusion(False) == 0
        plain = e.forward(xd)
        assert set(plain) == set(fused)
        for k in plain:
            if precision == "fp16":
                same_head(fused[k], plain[k], k)
            elif precision == "int8":
                assert np.array_equal(fused[k], plain[k]), k
            else:
                np.testing.assert_allclose(fused[k], plain[k], atol=5e-5, rtol=0, err_msg=k)
        for n, m in bufs.items():
            want = e.read_buffer(n)
            if precision == "strict":
                np.testing.assert_allclose(fbuf[n][m], want[m], atol=2e-5 * max(1.0, float(np.abs(want).max())), rtol=0, err_msg=n)
            else:
                assert np.array_equal(fbuf[n][m], want[m]), n
                if n in through_written:
                    assert np.array_equal(written(n, fbuf[n]), written(n, want)), n
        print(f"per-op bound: {precision} {label}: {groups} fused groups, {len(bufs)} buffers, frame as launched = per-op table")
        if (label, precision) == ("B-96x160", "int8"):
            assert ops
        recs = _hold(b, x, launched, f"launched frame, {precision} {label}, {len(ops)} ops", ops=ops)
        assert {r["op"] for r in recs} == set(ops)
    finally:
        e.close()
