"""Every element of every op's output against a float64 evaluation of that op on the ENGINE'S OWN inputs (teacher-forced,
tests/emulate.py per_op_bounds), held to the bound the arithmetic allows -- no fraction, no exempt element.
The other forward checks are sized for a whole tensor or compare one form of the engine with another; a wrong tap at the
pixels of a partial tile, in code every form shares, passes all of them. Sizes: the smallest legal input (every map smaller
than every tile), a one-row map, odd maps, partial tiles on every level."""
import numpy as np
import pytest

import emulate as E

pytestmark = pytest.mark.gpu

SIZES = E.PER_OP_SIZES
IDS = lambda s: f"{s[0]}x{s[1]}"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_amax_cache = {}


def _amax(pkg, sd7, size, scale=1.0):
    from unina_yolo_dla_amd.engine import calibrate_amax
    if size not in _amax_cache:
        g = pkg.graph.Graph(in_h=size[0], in_w=size[1])
        _amax_cache[size] = calibrate_amax(sd7, g, [pkg.rng.frame(5000 + i, *size) for i in range(2)])
    return {k: v * scale for k, v in _amax_cache[size].items()}


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


# (STRICT at 80x112 only: the smallest of these sizes, every level has a partial tile; the split-fp16 rows are the table's most irregular)
TILE_CASES = [(p, s) for p in ("fp16", "int8") for s in ((80, 112), (96, 160))] + [("strict", (80, 112))]


@pytest.mark.parametrize("precision,size", TILE_CASES, ids=[f"{p}-{IDS(s)}" for p, s in TILE_CASES])
def test_every_tile_configuration_within_the_bound(pkg, sd7, torch_cuda, tmp_path, precision, size):
    """Each tile configuration forced on every op that accepts it, then the autotuner's choice: the outputs of those ops
    against float64 (test_tile_configs_and_autotune_are_bit_identical compares them with the default configuration only).
    STRICT engines: the heads under every forced configuration also stay within the 5e-5 of the default configuration's that
    test_frame_as_launched_equals_per_op_table allows a strict frame (the configurations differ in fp32 summation order)."""
    g = pkg.graph.Graph(in_h=size[0], in_w=size[1])
    b, e, _ = _make(pkg, sd7, g, precision, tmp_path, _amax(pkg, sd7, size) if precision == "int8" else None)
    try:
        e.set_fusion(False)
        x = pkg.rng.frame(1234, *size)
        xd = torch_cuda.from_numpy(x).cuda()
        infos = e.op_infos()
        names = e.conv_configs()
        default = {k: v.copy() for k, v in e.forward(xd).items()} if precision == "strict" else None
        tried = 0
        for cfg in range(len(names)):
            applied = [i for i, o in enumerate(infos) if o["kind"] == 1 and e.set_op_config(i, cfg)]
            if not applied:
                continue
            tried += 1
            teacher = _teacher(b, e, xd)
            _hold(b, x, teacher, f"{precision} {IDS(size)} config {cfg} {names[cfg]} on {len(applied)} ops", ops=applied)
            for k in default or ():
                np.testing.assert_allclose(teacher[k], default[k], atol=5e-5, rtol=0, err_msg=f"config {cfg} {k}")
            for i in applied:
                e.set_op_config(i, -1)
        assert tried >= 6
        e.autotune(xd, iters=3)
        _hold(b, x, _teacher(b, e, xd), f"{precision} {IDS(size)} autotuned")
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
@pytest.mark.parametrize("precision", ["fp16", "strict"])
def test_per_op_table_other_topologies(pkg, torch_cuda, tmp_path, precision, topology):
    """Graph (B) down to a 1x1 stride-32 map, the lite P2 stage, a 16-channel model embedded at width 32 (its zero channels
    read exactly 0: a slice whose terms are all zero has a bound of 0), 1 / 7 / 20 classes (output rows padded to 16)."""
    label, kw = topology
    g = pkg.graph.Graph(**kw)
    sd = pkg.synth.make_state_dict(7, g)
    b, e, _ = _make(pkg, sd, g, precision, tmp_path)
    try:
        e.set_fusion(False)
        x = pkg.rng.frame(1234, g.in_h, g.in_w)
        teacher = _teacher(b, e, torch_cuda.from_numpy(x).cuda())
        recs = _hold(b, x, teacher, f"{precision} {label}")
        if label == "base16":
            dead = [(r, np.flatnonzero((r["S"] == 0).all(axis=(1, 2)))) for r in recs if r["S"] is not None]
            assert sum(len(ch) for _, ch in dead) > 100
            for r, ch in dead:
                assert not teacher[r["buf"]][r["c0"]:r["c1"]][ch].any(), r["name"]
        if label.startswith("classes"):
            assert teacher["p4_cls"].shape[0] == kw["num_classes"]
    finally:
        e.close()
