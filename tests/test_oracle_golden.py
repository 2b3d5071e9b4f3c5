"""Pins the CPU oracle (oracle/*.c) against fixtures produced by the reference itself
(tests/golden/make_golden.py: model.py imported as-is; postprocess.hpp compiled as-is)."""
import numpy as np
import pytest

from conftest import load_golden

FWD_ATOL = 1e-4   # fp32 vs torch/oneDNN fp32: summation-order noise only (measured 2e-5 on logits of magnitude ~8 at 640^2)


def test_graph_matches_survey(pkg):
    g = pkg.graph.Graph()
    assert len(g.convs()) == 67
    assert g.macs() == 17_832_345_600
    assert pkg.graph.Graph(in_h=1280, in_w=1280).macs() == 4 * 17_832_345_600
    shapes = g.param_shapes()
    assert len(shapes) == 317                                 # 378 reference keys - 61 num_batches_tracked
    assert shapes["backbone.stem.conv.weight"] == (32, 3, 3, 3)
    assert shapes["head_p4.reg_branch.2.bias"] == (4,)
    nparams = sum(int(np.prod(s)) for k, s in shapes.items() if "running" not in k)
    assert nparams == 5_004_344                               # model.py __main__ parameter count


def test_rng_is_pure_and_stable(pkg):
    a = pkg.rng.normal(7, "x", 1000)
    b = pkg.rng.normal(7, "x", 2000)[:1000]
    assert np.array_equal(a, b)
    assert not np.array_equal(a, pkg.rng.normal(8, "x", 1000))
    # known-answer: guards the generator the committed goldens depend on
    assert pkg.rng.frame(1234, 16, 16).reshape(-1)[:3].tolist() == pytest.approx(
        [float(v) for v in pkg.rng.normal(1234, "frame", 3).astype(np.float32)])
    z = pkg.rng.normal(1, "stat", 200_000)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01


def test_forward_mini64_every_module(pkg, oracle_mod, oracle_sd7):
    gold = load_golden("mini64_seed1234.npz")
    x = pkg.rng.frame(1234, 64, 64)
    out = oracle_mod.forward(oracle_sd7, x, keep_all=True)
    for name in pkg.graph.OUTPUT_NAMES:
        np.testing.assert_allclose(out[name], gold[f"head/{name}"], atol=FWD_ATOL, rtol=0)
    checked = 0
    for key in gold.files:
        if not key.startswith("tap/"):
            continue
        name = key[4:]
        oname = name + ".add" if name.split(".")[-2:-1] == ["bottlenecks"] else name
        assert oname in out, name
        ref = gold[key].astype(np.float32)              # stored as fp16
        np.testing.assert_allclose(out[oname], ref, atol=2e-3, rtol=2e-3, err_msg=name)
        checked += 1
    assert checked >= 70


def test_forward_640_heads_and_checksums(pkg, oracle_mod, oracle_sd7):
    gold = load_golden("frame640_seed1234.npz")
    x = pkg.rng.frame(1234, 640, 640)
    out = oracle_mod.forward(oracle_sd7, x, keep_all=True)
    for name in pkg.graph.OUTPUT_NAMES:
        np.testing.assert_allclose(out[name], gold[f"head/{name}"], atol=FWD_ATOL, rtol=0, err_msg=name)
    for i, name in enumerate(gold["tap_names"]):
        name = str(name)
        oname = name + ".add" if name.split(".")[-2:-1] == ["bottlenecks"] else name
        t = out[oname].reshape(-1)
        mean, amax = gold["tap_stats"][i]
        assert abs(t.astype(np.float64).mean() - mean) < 1e-5 + 1e-5 * abs(mean), name
        assert abs(np.abs(t).max() - amax) < 1e-4 * max(1.0, amax), name
        np.testing.assert_allclose(t[gold["tap_idx"][i]], gold["tap_vals"][i], atol=FWD_ATOL, rtol=1e-5, err_msg=name)


def test_forward_lite_p2(pkg, oracle_mod):
    gold = load_golden("lite_p2_64_seed1234.npz")
    g = pkg.graph.Graph(lite_p2=True, in_h=64, in_w=64)
    sd = oracle_mod.StateDict(pkg.synth.make_state_dict(7, g))
    out = oracle_mod.forward(sd, pkg.rng.frame(1234, 64, 64), lite_p2=True)
    for name in pkg.graph.OUTPUT_NAMES:
        np.testing.assert_allclose(out[name], gold[f"head/{name}"], atol=FWD_ATOL, rtol=0)
    sd.close()


def _heads_640(pkg, *_):
    """The REFERENCE model's own head tensors (committed fixture): decode/NMS tests are exact functions of these."""
    gold = load_golden("frame640_seed1234.npz")
    return [gold[f"head/{n}"] for n in pkg.graph.OUTPUT_NAMES]


@pytest.mark.parametrize("q", [0.1, 0.0])
def test_postprocess_cpu_header_semantics_match_reference_fixture(pkg, oracle_mod, oracle_sd7, q):
    """Oracle run with postprocess.hpp semantics == detections the compiled reference header produced."""
    gold = load_golden("frame640_seed1234.npz")
    ref = gold[f"ref_dets_q{q}"]
    heads = _heads_640(pkg, oracle_mod, oracle_sd7)
    dets, ncand = oracle_mod.postprocess(heads, 0.5, 0.45, q, sem=oracle_mod.semantics("cpu_header"))
    assert ncand == int(gold[f"ref_ncand_q{q}"])
    assert len(dets) == len(ref)
    assert np.array_equal(dets["class_id"], ref["class_id"])
    for f in ("x1", "y1", "x2", "y2"):
        np.testing.assert_allclose(dets[f], ref[f], atol=1e-4, rtol=0)      # same inputs; only libm expf/FMA contraction may differ
    np.testing.assert_allclose(dets["confidence"], ref["confidence"], atol=2e-6, rtol=0)


def test_postprocess_live_reference_header_bit_exact(pkg, oracle_mod, oracle_sd7):
    """The restatement must agree bit for bit with the compiled reference header on identical head tensors: with the
    header's output stored by tests/golden/make_golden_ref_post.py everywhere, and with the live header as well where
    oracle/_ref was built (the reference tree is present)."""
    heads = _heads_640(pkg, oracle_mod, oracle_sd7)
    gold = load_golden("ref_post_frame640_seed1234.npz")
    for conf, iou, q in [(0.5, 0.45, 0.1), (0.3, 0.2, 0.0), (0.2, 0.6, 0.25)]:
        a, na = oracle_mod.postprocess(heads, conf, iou, q, sem=oracle_mod.semantics("cpu_header"))
        tag = f"conf{conf}_iou{iou}_q{q}"
        refs = [("stored", gold[f"dets_{tag}"], int(gold[f"ncand_{tag}"]))]
        if oracle_mod.have_ref():
            refs.append(("live", *oracle_mod.ref_postprocess(heads, conf, iou, q)))
        for src, b, nb in refs:
            assert na == nb and len(a) == len(b), (src, conf, iou, q)
            assert np.array_equal(a["confidence"], b["confidence"]), (src, conf, iou, q)
            # records with EQUAL confidence may be permuted: the reference's std::sort is unstable
            # (postprocess.hpp:46-49), the oracle's order is the stable one of SURVEY App. D.
            ka = np.lexsort((a["y2"], a["x2"], a["y1"], a["x1"], a["class_id"], -a["confidence"]))
            kb = np.lexsort((b["y2"], b["x2"], b["y1"], b["x1"], b["class_id"], -b["confidence"]))
            for f in ("x1", "y1", "x2", "y2", "confidence", "class_id"):
                assert np.array_equal(a[f][ka], b[f][kb]), (src, conf, iou, q, f)


def test_postprocess_engine_semantics_properties(pkg, oracle_mod, oracle_sd7):
    """Engine semantics = GPU-file thresholds + deterministic order: sorted, capped, idempotent."""
    heads = _heads_640(pkg, oracle_mod, oracle_sd7)
    dets, ncand = oracle_mod.postprocess(heads, 0.5, 0.45, 0.1)
    assert 0 < len(dets) <= min(ncand, 1024)
    assert np.all(np.diff(dets["confidence"]) <= 0)
    assert np.all(dets["valid"] == 1) and np.all(dets["_pad"] == 0)
    # very low threshold: all 33600 cells are candidates -> cap at the 1024 best
    dets, ncand = oracle_mod.postprocess(heads, 0.0, 0.45, 0.1)
    assert ncand == 33600 and len(dets) <= 1024
    # threshold above every score: empty
    dets, ncand = oracle_mod.postprocess(heads, 0.9999999, 0.45, 0.1)
    assert ncand == 0 and len(dets) == 0


def test_iou_and_sigmoid_scalars(oracle_mod):
    import ctypes as C
    L = oracle_mod.lib()
    a = oracle_mod.Det(0, 0, 10, 10, 0.9, 0, 1, 0)
    b = oracle_mod.Det(5, 5, 15, 15, 0.8, 0, 1, 0)
    c = oracle_mod.Det(10, 0, 20, 10, 0.8, 0, 1, 0)          # touching edge: early-out 0 (postprocess.hpp:34)
    assert L.uo_iou(C.byref(a), C.byref(b), 0.0) == pytest.approx(25.0 / 175.0, rel=1e-6)
    assert L.uo_iou(C.byref(a), C.byref(c), 0.0) == 0.0
    assert L.uo_iou(C.byref(a), C.byref(b), 1e-6) < L.uo_iou(C.byref(a), C.byref(b), 0.0) + 1e-9
    assert L.uo_sigmoid(0.0) == 0.5
    assert L.uo_sigmoid(-3.5) == pytest.approx(1 / (1 + np.exp(3.5)), rel=1e-6)
