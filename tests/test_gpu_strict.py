"""GPU parity of the STRICT precision mode (export.SPLIT: fp16 hi/lo pairs, three fp16 MFMAs per k block) -- the ONE engine
that has to meet both north-star clauses (BASELINE.json): IoU >= 0.999 and |score delta| < 1e-3 against the fp32 forward of
model.py:347-365 on EVERY detection, at >= 100x the host-CPU frame rate (the rate is bench.py --precision strict's business)."""
import numpy as np
import pytest

from conftest import load_golden
from detcmp import compare

pytestmark = pytest.mark.gpu

STRICT_HEAD_ATOL = 2e-4     # |logit error| of a head tensor (cls std 2.0, calibrated logits up to ~8); measured ~2e-5
SEEDS = tuple(range(1234, 1246))   # 12 frames


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def strict640(pkg, sd7, torch_cuda):
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine
    e = Engine.from_state_dict(sd7, precision=export.STRICT)
    yield e
    e.close()


@pytest.fixture(scope="module")
def strict64(pkg, sd7, torch_cuda):
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine
    e = Engine.from_state_dict(sd7, pkg.graph.Graph(in_h=64, in_w=64), precision=export.STRICT)
    yield e
    e.close()


PAIRS = {
    "backbone.stem": "backbone.stem", "backbone.stage1_conv": "backbone.stage1_conv",
    "backbone.stage1_block.cat": "backbone.stage1_block.cat", "backbone.stage2_conv": "backbone.stage2_conv",
    "backbone.stage3_conv": "backbone.stage3_conv", "backbone.sppf.cat": "backbone.sppf.cat",
    "backbone.sppf": "backbone.sppf.cv2", "neck.cat_fpn1": "neck.cat_fpn1", "neck.cat_fpn2": "neck.cat_fpn2",
    "neck.cat_pan1": "neck.cat_pan1", "neck.cat_pan2": "neck.cat_pan2", "p2_fused": "neck.fpn_c3k2_2.cv3",
    "p3_out": "neck.pan_c3k2_1.cv3", "p4_out": "neck.pan_c3k2_2.cv3",
}


@pytest.mark.parametrize("size", [64, 96])
def test_strict_every_buffer_vs_oracle(pkg, sd7, oracle_mod, oracle_sd7, torch_cuda, size):
    """Per-op table (fusion off: every buffer is written) against the fp32 oracle, buffer by buffer: an fp16 pair carries ~22
    mantissa bits, so the bound is fp32-like (1e-4 of the tensor's scale), 100x tighter than the fp16 engine's."""
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine
    e = Engine.from_state_dict(sd7, pkg.graph.Graph(in_h=size, in_w=size), precision=export.STRICT)
    try:
        e.set_fusion(False)
        x = pkg.rng.frame(1234, size, size)
        heads = e.forward(torch_cuda.from_numpy(x).cuda())
        ref = oracle_mod.forward(oracle_sd7, x, keep_all=True)
        for name in pkg.graph.OUTPUT_NAMES:
            np.testing.assert_allclose(heads[name], ref[name], atol=STRICT_HEAD_ATOL, rtol=0, err_msg=name)
        for bname, oname in PAIRS.items():
            got, want = e.read_buffer(bname), ref[oname]
            assert got.shape == want.shape, (bname, got.shape, want.shape)
            np.testing.assert_allclose(got, want, atol=1e-4 * max(1.0, float(np.abs(want).max())), rtol=0, err_msg=bname)
    finally:
        e.close()


@pytest.mark.parametrize("size", [64, 96, 640])
def test_strict_fused_equals_per_op_within_fp32_noise(pkg, sd7, torch_cuda, size, tmp_path):
    """The frame as launched (fused C3k2 blocks, the conv pair, paired head launches) against the per-op table of the same
    engine, heads and block outputs; 96^2 puts partial tiles on every level. Kernel families of the split mode may order
    their fp32 sums differently (no bit-identity contract here): fp32 rounding noise only."""
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine
    path = str(tmp_path / "s.une")
    e = Engine.from_state_dict(sd7, pkg.graph.Graph(in_h=size, in_w=size), path=path, precision=export.STRICT)
    try:
        assert e.set_fusion(True) >= 8                            # 7 C3k2 blocks + the SPPF / lateral pair
        assert e.L.unina_fusion_groups(e.h) == e.L.unina_debug_fusable_groups(path.encode())   # the hook is the loader's host side
        kernels = " ".join(o["kernel"] for o in e.op_infos())
        assert "c3k2_fused<s16" in kernels and "conv_pair<s16" in kernels and "conv_dual_head3x3_ws_s16" in kernels, kernels
        x = torch_cuda.from_numpy(pkg.rng.frame(1234, size, size)).cuda()
        fused = e.forward(x)
        # (cat_pan1 / cat_pan2 are left out: their down-sampled halves live only inside the fused PAN blocks)
        outs = ("p2_fused", "p3_out", "p4_out", "backbone.sppf", "neck.cat_fpn1", "neck.cat_fpn2")
        fbuf = {b: e.read_buffer(b) for b in outs}
        e.set_fusion(False)
        plain = e.forward(x)
        for name in pkg.graph.OUTPUT_NAMES:
            np.testing.assert_allclose(fused[name], plain[name], atol=5e-5, rtol=0, err_msg=name)
        for b in outs:
            want = e.read_buffer(b)
            np.testing.assert_allclose(fbuf[b], want, atol=2e-5 * max(1.0, float(np.abs(want).max())), rtol=0, err_msg=b)
    finally:
        e.close()


def test_strict_heads_vs_reference_fixture(pkg, strict640, torch_cuda):
    gold = load_golden("frame640_seed1234.npz")
    heads = strict640.forward(torch_cuda.from_numpy(pkg.rng.frame(1234, 640, 640)).cuda())
    for name in pkg.graph.OUTPUT_NAMES:
        err = np.abs(heads[name] - gold[f"head/{name}"]).max()
        assert err < STRICT_HEAD_ATOL, (name, float(err))


@pytest.mark.parametrize("q", [0.1, 0.0])
def test_strict_engine_meets_north_star_tolerance_on_every_detection(pkg, strict640, oracle_mod, oracle_sd7, torch_cuda, q):
    """BASELINE.json: every matched box IoU >= 0.999 and |score delta| < 1e-3 vs the fp32 forward -- asserted by
    detcmp.compare on EVERY detection of 12 frames (oracle), and against the detections the reference's own model.py +
    postprocess.hpp produced (fixture frame640_seed1234.npz)."""
    gold = load_golden("frame640_seed1234.npz")
    total = 0
    worst_ds, worst_iou = 0.0, 1.0
    for seed in SEEDS:
        x = pkg.rng.frame(seed, 640, 640)
        got = strict640.infer(torch_cuda.from_numpy(x).cuda(), 0.5, 0.45, q)
        o = oracle_mod.forward(oracle_sd7, x)
        want, _ = oracle_mod.postprocess([o[n] for n in pkg.graph.OUTPUT_NAMES], 0.5, 0.45, q)
        stats = compare(got, want, 0.5, min_iou=0.999, score_tol=1e-3, max_unmatched_frac=0.005)
        assert stats["matched"] >= len(want) - 2, stats
        total += stats["matched"]
        worst_ds, worst_iou = max(worst_ds, stats["max_dscore"]), min(worst_iou, stats["min_iou"])
        if seed == 1234:
            ref = gold[f"ref_dets_q{q}"]
            want = np.zeros(len(ref), dtype=got.dtype)
            for f in ref.dtype.names:
                want[f] = ref[f]
            stats = compare(got, want, 0.5, min_iou=0.999, score_tol=1e-3, max_unmatched_frac=0.005)
            assert stats["matched"] >= len(want) - 2, stats
    assert total > 4000
    # the measured distance is two orders of magnitude inside the tolerance (CPU emulation: 5.5e-6 / 0.99999)
    assert worst_ds < 1e-4 and worst_iou > 0.9999, (worst_ds, worst_iou)


def test_strict_1280_p2_head_config(pkg, sd7, torch_cuda):
    """BASELINE configs[4] (1280x1280, P2 grid 320x320) on the STRICT engine: the reference's sampled head values within
    fp32-like bounds, and its detections (model.py + postprocess.hpp, fixture) inside the north-star tolerance, every one."""
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine
    gold = load_golden("frame1280_seed1234.npz")
    e = Engine.from_state_dict(sd7, pkg.graph.Graph(in_h=1280, in_w=1280), precision=export.STRICT)
    try:
        x = torch_cuda.from_numpy(pkg.rng.frame(1234, 1280, 1280)).cuda()
        heads = e.forward(x)
        for name in pkg.graph.OUTPUT_NAMES:
            flat = heads[name].reshape(-1)
            np.testing.assert_allclose(flat[gold[f"idx/{name}"]], gold[f"vals/{name}"], atol=STRICT_HEAD_ATOL, rtol=0, err_msg=name)
        np.testing.assert_allclose(heads["p4_cls"], gold["head/p4_cls"], atol=STRICT_HEAD_ATOL, rtol=0)
        got = e.infer(x, 0.6, 0.45, 0.1)
        ref = gold["ref_dets_conf0.6_q0.1"]
        want = np.zeros(len(ref), dtype=got.dtype)
        for f in ref.dtype.names:
            want[f] = ref[f]
        stats = compare(got, want, 0.6, min_iou=0.999, score_tol=1e-3, max_unmatched_frac=0.005)
        assert stats["matched"] >= len(want) - 2 and stats["max_dscore"] < 1e-4, stats
    finally:
        e.close()


def test_strict_graph_b_and_lite_p2_variants(pkg, torch_cuda, oracle_mod):
    """The other layer tables on the STRICT engine (blocks without a split class simply stay on the per-op kernels): graph (B)
    (qat.py's topology) and the lite_p2 variant of graph (A), heads against the fp32 oracle."""
    from unina_yolo_dla_amd import export
    from unina_yolo_dla_amd.engine import Engine
    x = pkg.rng.frame(1234, 128, 128)
    for kw in (dict(variant="B"), dict(lite_p2=True)):
        g = pkg.graph.Graph(in_h=128, in_w=128, **kw)
        sd = pkg.synth.make_state_dict(7, g)
        osd = oracle_mod.StateDict(sd)
        ref = oracle_mod.forward(osd, x, **kw)
        osd.close()
        e = Engine.from_state_dict(sd, g, precision=export.STRICT)
        try:
            heads = e.forward(torch_cuda.from_numpy(x).cuda())
            for name in pkg.graph.OUTPUT_NAMES:
                np.testing.assert_allclose(heads[name], ref[name], atol=STRICT_HEAD_ATOL, rtol=0, err_msg=f"{kw} {name}")
        finally:
            e.close()
