"""Class counts above 16 (-m gpu). num_classes comes from the engine file; 16 is where the kernels change shape:
  - the P2 head runs as ONE fused launch only while each output branch fits one 16-row tile (nc <= 16; engine.hip
    head_layout), from 17 classes on it is three per-op launches;
  - the heads' output convs fold into the decode launch only while each branch has <= 16 channels (find_fold_ops);
    above that every head is decoded from its fp32 planes, and the cls 1x1 conv is a planar segment of several 16-row
    subtiles whose last N tile can straddle into the reg segment (conv_igemm.hip);
  - the two-launch NMS carries the class id next to the enumeration index in one word (postprocess.hip pack_ce): ids
    from 128 on, id 255 (the padding dummy's -1 in an 8-bit field) and ids c / c + 256 are where a narrow field breaks.
Heads are held to the tolerances of test_gpu_parity.py / test_gpu_strict.py; the post-process on identical inputs is
exact in all three forms (two launches, one launch, the seven-function stepwise API)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import CLS_RMS, HEAD_ATOL, REG_RMS, same_head
from test_gpu_strict import STRICT_HEAD_ATOL

pytestmark = pytest.mark.gpu

STRIDES = (4, 8, 16)
CLS_SCALE = 10.0            # cls head multiplier of test_other_class_counts' 7-class case


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _sd(pkg, nc, hw=(256, 256)):
    g = pkg.graph.Graph(num_classes=nc, in_h=hw[0], in_w=hw[1])
    sd = pkg.synth.make_state_dict(7, g, head_scales={n: (CLS_SCALE if n.endswith("cls") else 2.0) for n in pkg.graph.OUTPUT_NAMES})
    return g, sd


def _rms(a):
    return float(np.sqrt((a.astype(np.float64) ** 2).mean()))


def required_ids(nc):
    """0, 127 (the last id an 8-bit field holds), nc - 1, and where they exist 128, 254, 255 (= -1 in 8 bits), 256."""
    return sorted({0, 127 if nc > 127 else nc // 2, nc - 1} | {i for i in (128, 254, 255, 256) if i < nc})


def synth_heads(nc, h, w, seed, dense=False):
    """Head planes [p2_cls, p2_reg, p3_cls, ...] whose decode outcome is planted: every cell below 1e-3 confidence
    except the hot ones, and every hot confidence distinct by far more than an ulp of expf (so the order is exact).
      sparse: an isolated small box of every required id, a 3x3 block of one class with large boxes per required id
              (heavy same-class overlap: the NMS keeps about one of nine), adjacent large boxes of classes c and c + 256
              (IoU ~0.8: both must survive), and random small boxes of random classes;
      dense:  every cell hot (more than MAX_DETECTIONS candidates: the top-1024 selection), classes cycling through all
              ids with the required ones first, small boxes of random sizes.
    Returns (heads, planted pairs [(class c, class c + 256)])."""
    rng = np.random.default_rng(seed)
    grids = [(h // s, w // s) for s in STRIDES]
    cls = [rng.normal(-9.0, 0.5, (nc, gh, gw)).astype(np.float32) for gh, gw in grids]
    reg = [rng.uniform(0.3, 1.2, (4, gh, gw)).astype(np.float32) for gh, gw in grids]
    hot = []                                                   # (head, y, x, class, reg size or None)
    ids = required_ids(nc)
    pairs = []
    if dense:
        order = ids + [k for k in range(nc) if k not in ids]
        i = 0
        for hd, (gh, gw) in enumerate(grids):
            for y in range(gh):
                for x in range(gw):
                    hot.append((hd, y, x, order[i % nc], None))
                    i += 1
    else:
        # left half of the frame: isolated small boxes of every required id (P2) and the same-class blocks (P3)
        gh2, gw2 = grids[0]
        cells = rng.permutation(gh2 * (gw2 // 2))[:len(ids) + 40]
        for j, c in enumerate(cells):
            y, x = divmod(int(c), gw2 // 2)
            hot.append((0, y, x, ids[j] if j < len(ids) else int(rng.integers(0, nc)), None))
        gh3, gw3 = grids[1]
        for j, k in enumerate(ids):
            y0, x0 = 1 + 4 * (j // 3), 1 + 5 * (j % 3)        # 3x3 blocks, 4-5 cells apart (boxes 6 cells wide)
            for dy in range(3):
                for dx in range(3):
                    hot.append((1, y0 + dy, x0 + dx, k, 3.0))
        # right of x = 150 px: aliasing pairs on P4, boxes 3 strides either side, neighbours one stride apart
        gh4, gw4 = grids[2]
        for j, c in enumerate(k for k in (0, 1, nc - 257) if 0 <= k < nc - 256):
            y, x = 2 + 5 * j, gw4 - 3
            hot.append((2, y, x, c, 3.0))
            hot.append((2, y, x + 1, c + 256, 3.0))
            pairs.append((c, c + 256))
    n = len(hot)
    rank = rng.permutation(n)
    if dense:                                                  # the required ids among the 1024 kept: the highest confidences
        for j in range(len(ids)):
            k = int(np.flatnonzero(rank == n - 1 - j)[0])
            rank[j], rank[k] = rank[k], rank[j]
    conf = 0.55 + 0.44 * (rank + 0.5) / n                      # distinct, >= 0.44 / n apart
    logit = np.log(conf / (1.0 - conf)).astype(np.float32)
    for (hd, y, x, k, size), lg in zip(hot, logit):
        cls[hd][k, y, x] = lg
        if size is not None:
            reg[hd][:, y, x] = size
    heads = []
    for c, r in zip(cls, reg):
        heads += [c, r]
    return heads, pairs


def check_same_records(got, want, nc, ordered=True):
    """Record for record: count, boxes bit for bit, class ids, confidences within 2e-7 (GPU expf vs glibc expf),
    valid = 1 / _pad = 0, every class id inside [0, nc). ordered: the planted confidences are far apart, so the output
    order must be the oracle's; otherwise an ulp may swap equal-looking neighbours and the records compare as sets."""
    assert len(got) == len(want), (len(got), len(want))
    assert np.all((got["class_id"] >= 0) & (got["class_id"] < nc)), np.unique(got["class_id"])
    assert np.all(got["valid"] == 1) and np.all(got["_pad"] == 0)
    assert np.all(np.diff(got["confidence"]) <= 0)
    if len(want) == 0:
        return
    if ordered:
        ka = kb = np.arange(len(want))
    else:
        ka = np.lexsort((got["y2"], got["x2"], got["y1"], got["x1"], got["class_id"]))
        kb = np.lexsort((want["y2"], want["x2"], want["y1"], want["x1"], want["class_id"]))
    np.testing.assert_allclose(got["confidence"][ka], want["confidence"][kb], atol=2e-7, rtol=0)
    for f in ("x1", "y1", "x2", "y2", "class_id"):
        assert np.array_equal(got[f][ka], want[f][kb]), (f, got[f][ka][got[f][ka] != want[f][kb]][:8],
                                                          want[f][kb][got[f][ka] != want[f][kb]][:8])


def _stepwise(L, torch, heads, nc, conf, iou, q):
    """perception_node.cpp:627-656 call sequence through the seven gpu_postprocess.h symbols."""
    from unina_yolo_dla_amd.engine import DET_DTYPE
    dev = [torch.from_numpy(hh).cuda() for hh in heads]
    dets = torch.zeros(1024 * 8, dtype=torch.int32, device="cuda")
    assert L.init_postprocess_resources() == 0
    try:
        stream = torch.cuda.current_stream().cuda_stream
        assert L.reset_detection_counter(stream) == 0
        for i, s in enumerate(STRIDES):
            c, r = dev[2 * i], dev[2 * i + 1]
            assert L.decode_yolo_head(c.data_ptr(), r.data_ptr(), dets.data_ptr(), c.shape[2], c.shape[1], s, nc,
                                      conf, q, stream) == 0
        n = C.c_int(-1)
        assert L.get_detection_count(C.byref(n), stream) == 0
        torch.cuda.synchronize()
        ncand = n.value
        assert L.run_gpu_nms(dets.data_ptr(), ncand, iou, stream) == 0
        host = np.zeros(1024, dtype=DET_DTYPE)
        valid = C.c_int(-1)
        assert L.copy_valid_detections_to_host(dets.data_ptr(), host.ctypes.data, ncand, C.byref(valid), stream) == 0
        return host[:valid.value].copy(), ncand
    finally:
        L.cleanup_postprocess_resources()


# ---- (a) heads against the fp32 oracle, the fp16 emulation and the per-op table ----
@pytest.mark.parametrize("nc", [16, 17, 80, 300])
def test_fp16_heads_at_class_count(pkg, oracle_mod, torch_cuda, nc):
    from emulate import run_op_table
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine
    g, sd = _sd(pkg, nc)
    osd = oracle_mod.StateDict(sd)
    e = Engine.from_state_dict(sd, g)
    try:
        # which path ran: the fused P2 head is one of the 9 groups up to 16 classes and drops out from 17 on
        assert e.L.unina_fusion_groups(e.h) == (9 if nc <= 16 else 8)
        x = pkg.rng.frame(1234, 256, 256)
        xd = torch_cuda.from_numpy(x).cuda()
        heads = {k: v.copy() for k, v in e.forward(xd).items()}
        o = oracle_mod.forward(osd, x, num_classes=nc)
        emu, _ = run_op_table(export.EngineBuilder(sd, g), x, fp16=True)
        for n in pkg.graph.OUTPUT_NAMES:
            assert heads[n].shape == o[n].shape and heads[n].shape[0] == (nc if n.endswith("cls") else 4)
            err = heads[n] - o[n]
            assert np.abs(err).max() < HEAD_ATOL, (n, float(np.abs(err).max()))
            assert _rms(err) < (CLS_RMS if n.endswith("cls") else REG_RMS), (n, _rms(err))
            e_gpu, e_emu, e_x = _rms(err), _rms(emu[n] - o[n]), _rms(heads[n] - emu[n])
            assert e_gpu < 1.2 * e_emu + 1e-5, (n, e_gpu, e_emu)      # no worse than the fp16 emulation
            assert e_x < 1.2 * max(e_gpu, e_emu), (n, e_x, e_gpu, e_emu)
        assert e.set_fusion(False) == 0
        plain = e.forward(xd)
        for k in plain:
            same_head(heads[k], plain[k], k)
    finally:
        e.close()
        osd.close()


@pytest.mark.parametrize("precision,atol", [("fp32", 2e-4), ("strict", STRICT_HEAD_ATOL)])
def test_precise_heads_at_80_classes(pkg, oracle_mod, torch_cuda, precision, atol):
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine
    g, sd = _sd(pkg, 80)
    osd = oracle_mod.StateDict(sd)
    e = Engine.from_state_dict(sd, g, precision=export.FP32 if precision == "fp32" else export.STRICT)
    try:
        x = pkg.rng.frame(1234, 256, 256)
        heads = e.forward(torch_cuda.from_numpy(x).cuda())
        o = oracle_mod.forward(osd, x, num_classes=80)
        for n in pkg.graph.OUTPUT_NAMES:
            np.testing.assert_allclose(heads[n], o[n], atol=atol, rtol=0, err_msg=n)
    finally:
        e.close()
        osd.close()


# ---- (b) post-process on identical inputs: exact in every form ----
@pytest.mark.parametrize("nc", [16, 17, 80, 128, 129, 256, 300])
def test_postprocess_exact_at_class_count(pkg, oracle_mod, torch_cuda, monkeypatch, nc):
    """Planted head planes (synth_heads) through the two-launch default, the one-launch form (UNINA_POST_SPLIT=0) and the
    stepwise API, each against the oracle record for record. (UNINA_POST_FOLD changes nothing here: a decode from planes
    never folds; the folded decode is compared end to end below.)"""
    from unina_yolo_dla_amd.engine import Engine, load_library
    g, sd = _sd(pkg, nc)
    cases = [(synth_heads(nc, 256, 256, 100 + nc), 0.5, 0.45, 0.1), (synth_heads(nc, 256, 256, 200 + nc), 0.5, 0.6, 0.0),
             (synth_heads(nc, 256, 256, 300 + nc, dense=True), 0.5, 0.45, 0.1)]
    ids = required_ids(nc)
    wants = []
    for (heads, pairs), conf, iou, q in cases:
        want, ncand = oracle_mod.postprocess(heads, conf, iou, q)
        wants.append((want, ncand))
        assert set(ids) <= set(want["class_id"].tolist()), (ids, np.unique(want["class_id"]))
        if nc > 128:
            assert (want["class_id"] >= 128).any()
        if ncand <= 1024:
            assert len(want) < ncand - 2 * len(ids)            # the NMS really suppresses (the same-class blocks)
            for c, c2 in pairs:                                # ... but never across classes c and c + 256
                assert ((want["class_id"] == c) & (want["x1"] > 150)).sum() == 1, c
                assert ((want["class_id"] == c2) & (want["x1"] > 150)).sum() == 1, c2
        else:
            assert ncand > 4000 and 1000 < len(want) <= 1024, (ncand, len(want))   # (the top 1024, a few suppressed)
    assert any(p for (_, p), *_ in cases) == (nc > 256)

    def run(label):
        e = Engine.from_state_dict(sd, g)
        try:
            for ((heads, _), conf, iou, q), (want, ncand) in zip(cases, wants):
                for n, hh in zip(pkg.graph.OUTPUT_NAMES, heads):
                    e.outputs[n].copy_(torch_cuda.from_numpy(hh)[None])
                got = e.postprocess(conf, iou, q)
                try:
                    check_same_records(got, want, nc)
                except AssertionError as ex:
                    raise AssertionError(f"{label}, conf {conf} iou {iou} q {q}, {ncand} candidates: {ex}") from None
        finally:
            e.close()

    run("two launches")
    monkeypatch.setenv("UNINA_POST_SPLIT", "0")
    run("one launch")
    for ((heads, _), conf, iou, q), (want, ncand) in zip(cases, wants):
        if ncand > 1024:       # (the stepwise API keeps the first 1024 in enumeration order, like the reference)
            continue
        got, n = _stepwise(load_library(), torch_cuda, heads, nc, conf, iou, q)
        assert n == ncand
        check_same_records(got, want, nc)


# ---- (c) end to end on the engine's own heads ----
@pytest.mark.parametrize("nc,thr", [(16, 0.3), (80, 0.65), (300, 0.9)])     # (~500-750 candidates each)
def test_infer_matches_postprocess_of_own_heads(pkg, oracle_mod, torch_cuda, monkeypatch, nc, thr):
    """unina_infer (one frame graph: forward + two-launch post-process; at 16 classes with the P3 / P4 output convs
    folded into the decode launch) against the oracle's post-process of the heads forward() downloads for the same
    frame: the same detections exactly. (Not against the fp32 oracle's detections: at large nc, argmax flips between
    nearly equal class logits would make that a test of luck; the heads are held to the oracle above.)"""
    from unina_yolo_dla_amd.engine import Engine
    g, sd = _sd(pkg, nc)
    x = pkg.rng.frame(1234, 256, 256)

    def run():
        e = Engine.from_state_dict(sd, g)
        try:
            xd = torch_cuda.from_numpy(x).cuda()
            got = e.infer(xd, thr, 0.45, 0.1)
            heads = e.forward(xd)
            want, ncand = oracle_mod.postprocess([heads[n] for n in pkg.graph.OUTPUT_NAMES], thr, 0.45, 0.1)
            assert 100 < ncand < 1024 and len(want) < ncand, (ncand, len(want))
            check_same_records(got, want, nc, ordered=False)
            return got
        finally:
            e.close()

    folded = run()
    if nc <= 16:
        monkeypatch.setenv("UNINA_POST_FOLD", "0")
        assert run().tobytes() == folded.tobytes()


# ---- (d) tile configurations at 80 classes ----
@pytest.mark.parametrize("precision", ["fp16", "int8"])
def test_tile_configs_at_80_classes(pkg, torch_cuda, precision):
    """test_tile_configs_and_autotune_are_bit_identical at 80 classes: the cls output conv is a planar segment of five
    16-row subtiles (n_pad 80) next to the 16-row reg segment, so a 64-wide N tile straddles the two. Every accepted
    config on every conv op, then the autotuner: bit-identical heads but for the chunked conv3x3_ws<f16 rule."""
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine, EngineError, calibrate_amax
    g, sd = _sd(pkg, 80)
    x = torch_cuda.from_numpy(pkg.rng.frame(1234, 256, 256)).cuda()
    if precision == "int8":
        try:
            amax = calibrate_amax(sd, g, [pkg.rng.frame(5000 + i, 256, 256) for i in range(2)])
            e = Engine.from_state_dict(sd, g, precision=export.INT8, amax=amax)
        except EngineError as ex:      # a refusal must be a clean UNSUPPORTED with a message
            assert "[UNSUPPORTED]" in str(ex) and str(ex).split("]")[-1].strip(), str(ex)
            return
    else:
        e = Engine.from_state_dict(sd, g)
    try:
        fused = {k: v.copy() for k, v in e.forward(x).items()}
        e.set_fusion(False)
        base = {k: v.copy() for k, v in e.forward(x).items()}
        for k in base:
            if precision == "fp16":
                np.testing.assert_allclose(fused[k], base[k], atol=5e-3, rtol=0, err_msg=f"fusion {k}")
            else:
                assert np.array_equal(fused[k], base[k]), ("fusion", k)
        infos = e.op_infos()
        heads_out = [i for i, o in enumerate(infos) if o["kind"] == 1 and o["name"].endswith((".2", "cls.2", "reg.2"))]
        ncfg = len(e.conv_configs())
        tried, on_heads = 0, 0
        for cfg in range(ncfg):
            applied = [i for i, o in enumerate(infos) if o["kind"] == 1 and e.set_op_config(i, cfg)]
            if not applied:
                continue
            tried += 1
            on_heads += len(set(applied) & set(heads_out))
            out = e.forward(x)
            chunked = "conv3x3_ws<f16" in e.conv_configs()[cfg]
            for k in base:
                if chunked:
                    np.testing.assert_allclose(out[k], base[k], atol=5e-3, rtol=0, err_msg=f"{e.conv_configs()[cfg]} {k}")
                else:
                    assert np.array_equal(out[k], base[k]), (e.conv_configs()[cfg], k)
            for i in applied:
                e.set_op_config(i, -1)
        assert tried >= 6 and on_heads >= 3, (tried, on_heads)
        e.autotune(x, iters=3)
        out = e.forward(x)
        chunked = any("conv3x3_ws<f16" in o["kernel"] for o in e.op_infos())
        for k in base:
            if chunked:
                np.testing.assert_allclose(out[k], base[k], atol=5e-3, rtol=0, err_msg=f"autotune {k}")
            else:
                assert np.array_equal(out[k], base[k]), ("autotune", k)
    finally:
        e.close()
