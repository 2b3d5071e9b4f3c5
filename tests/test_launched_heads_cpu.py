"""The host side of tests/test_gpu_launched_heads.py, without a GPU: the op selection of its section 1 on graph (A)'s fused groups
(run_op_table stands in for the engine), the configuration names of section 2, the oracle half of section 4, and that the
selection keeps the teeth of the per-op bound on the ops it exists for: the mutants of tests/test_per_op_bound_cpu.py on a P3 and a
P4 head op are rejected by the check section 1 runs."""
import numpy as np
import pytest

import emulate as E
import launched_heads_child as LH
from test_per_op_bound_cpu import _free_run

SIZE = (80, 112)


def _selection(pkg, sd7, precision):
    b, x, named, recs = _free_run(pkg, sd7, precision, in_h=SIZE[0], in_w=SIZE[1])
    infos = LH.stand_in_infos(b, precision == "strict")
    return b, x, named, recs, infos, E.launched_ops(b, infos)


@pytest.mark.parametrize("precision", ("fp16", "strict"))
def test_ops_held_on_the_launched_frame(pkg, sd7, tmp_path, precision):
    """Graph (A)'s fused groups (GROUPS_A: as many as the loader's host side finds in the engine file) leave in memory both ends of
    exactly: the stem, stage2_conv, stage3_conv, sppf.cv1, lateral_p3, lateral_p2, the three ops of the P3 head and of the P4 head
    (STRICT: of the P2 head too, there is no split-fp16 head kernel, and the SPPF pool with sppf.cv2 behind it, the pool being a
    launch of its own there) -- and the written slices are test_gpu_parity's."""
    from unina_yolo_dla_amd import build, engine
    from test_gpu_parity import WRITTEN_WHEN_FUSED
    b, x, named, recs, infos, ops = _selection(pkg, sd7, precision)
    groups, duals = E.launched_groups(infos)
    build.build_native()
    path = str(tmp_path / "e.une")
    b.save(path)
    assert len(groups) == engine.load_library().unina_debug_fusable_groups(path.encode()) == (8 if precision == "strict" else 9)
    assert ops == LH.expected_ops_a(b, precision == "strict")
    heads = E.head_ops(b)
    assert all(len(v) == 3 for v in heads.values()) and {oi for v in heads.values() for oi in v} <= set(ops)
    assert [b.ops[oi].k for oi in heads["p3"]] == [3, 3, 1] and [b.ops[oi].cin for oi in heads["p4"]] == [256, 256, 256]
    written = E.written_when_launched(b, infos)
    for name, (c0, c1) in WRITTEN_WHEN_FUSED.items():
        if name in written:
            assert written[name][c0:c1].all(), name
            assert written[name].sum() == len(written[name][c0:c1]) or (precision == "strict" and name == "backbone.sppf.cat"), name
    # the emulator's own buffers pass the check section 1 runs on the selected ops
    sel = [r for r in recs if r["op"] in ops]
    fails, worst, _ = E.check_per_op(sel, named)
    assert not fails and worst <= 1.0 and {r["op"] for r in sel} == set(ops)


def test_forced_configuration_names_exist(pkg):
    """Section 2 looks its single configurations up by name: the fp16 ones are rows of unina_conv_config_name, and every name
    (the int8 / split-fp16 rows, the pair kernels' own) is a string of the built library."""
    from unina_yolo_dla_amd import build, engine
    build.build_native()
    lib = engine.load_library()
    names = [lib.unina_conv_config_name(i).decode() for i in range(lib.unina_conv_config_count())]
    # one name per enumerator of ConvConfig as kernels.h states it, and no two configurations share one: a name is built from its
    # row's tile, so two equal names would be one tile in two slots. The rows here are the fp16 ones, so the slots that exist for
    # split fp16 alone (kCfgWsS*) are empty, "n/a" -- those and no others.
    import os, re
    header = open(os.path.join(build.CSRC, "kernels.h")).read()
    body = re.search(r"enum ConvConfig : int \{(.*?)\};", header, re.S).group(1)
    enum = [t.split("=")[0].strip() for t in re.sub(r"//[^\n]*", "", body).split(",") if t.strip()]
    assert enum[-1] == "kCfgCount" and len(set(enum)) == len(enum)
    assert len(names) == len(enum) - 1
    assert [e for e, n in zip(enum, names) if n == "n/a"] == [e for e in enum if e.startswith("kCfgWsS")] != []
    kernels = [n for n in names if n != "n/a"]
    assert len(set(kernels)) == len(kernels), sorted(n for n in set(kernels) if kernels.count(n) > 1)
    for key in ("fp16", "fp16-small"):
        for n in LH.DUAL[key][1]:
            assert names.count(n) == 1, n
    blob = open(engine.LIB_PATH, "rb").read()
    for prefix, twins in LH.DUAL.values():
        for s in (prefix, *twins):
            assert s.encode() in blob, s
    for s in LH.DUAL_REGQ.values():
        assert s.encode() in blob, s


def test_half_height_pair_threshold():
    h, w, ga, gb = LH.smallest_half_height_size()
    assert (h, w, ga, gb) == (2704, 16, 88, 176)
    up = lambda a, b: -(-a // b)
    assert (4 + 8) * up(2704 - 16, 128) == 252                   # one step shorter: 21 tile rows, not more than 256 workgroups
    assert 4 * up(4112, 128) + 8 * up(4112, 256) == 268 and 16 * 4112 > 2704 * 16      # the smallest WIDE frame is larger


@pytest.mark.parametrize("size", LH.DECODE_SIZES, ids=LH.IDS)
def test_oracle_keeps_every_cell(pkg, oracle_mod, oracle_sd7, size):
    """conf_thr = 0 passes every cell (a sigmoid is positive), iou_thr = 1 suppresses nothing (IoU < 1 with the + 1e-6 in the
    denominator): the oracle returns exactly one record per cell, 21 / 63 / 735 <= MAX_DETECTIONS."""
    from unina_yolo_dla_amd.engine import MAX_DETECTIONS
    o = oracle_mod.forward(oracle_sd7, pkg.rng.frame(1234, *size))
    ncell = LH.n_cells(size)
    assert ncell == {(16, 16): 21, (16, 48): 63, (80, 112): 735}[size] <= MAX_DETECTIONS
    for q in LH.DECODE_QS:
        dets, ncand = oracle_mod.postprocess([o[n] for n in pkg.graph.OUTPUT_NAMES], 0.0, 1.0, q)
        assert len(dets) == ncand == ncell, (q, len(dets), ncand)
        assert len(set(map(tuple, dets[["x1", "y1", "x2", "y2"]].tolist()))) == ncell     # the box is a key: no two cells share one


@pytest.mark.parametrize("precision", ("fp16", "strict"))
@pytest.mark.parametrize("kind", ("drop_tap", "edge_pad", "bias_neighbour"))
def test_head_mutants_are_rejected_by_the_launched_frame_check(pkg, sd7, precision, kind):
    """One P3 and one P4 head op (P3's second 3x3 layer, P4's first) computed wrong -- a dropped tap, a replicated border, a
    neighbour's bias -- and stored as the epilogue rounds: section 1's check, restricted to the head ops, fails, on that op alone."""
    b, x, named, recs, infos, ops = _selection(pkg, sd7, precision)
    heads = E.head_ops(b)
    head_set = {oi for v in heads.values() for oi in v}
    sel = [r for r in recs if r["op"] in head_set]
    assert not E.check_per_op(sel, named)[0]
    for lv in ("p3", "p4"):
        oi = heads[lv][1 if lv == "p3" else 0]
        assert oi in ops
        wrong = E.per_op_bounds(b, x, named, mutate=dict(op=oi, kind=kind), only_op=oi)
        mutated = {k: v.copy() for k, v in named.items()}
        for r in wrong:
            mutated[r["buf"]][r["c0"]:r["c1"]] = E.as_stored(r)
        fails, worst, _ = E.check_per_op(sel, mutated)
        print(precision, kind, b.ops[oi].name, "failures:", len(fails), "worst error/bound", worst)
        assert fails and all(f"op {oi} " in f for f in fails), (kind, b.ops[oi].name)
