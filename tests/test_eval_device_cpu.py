"""Host side of the on-device evaluation (csrc/evalmatch.hip, include/unina_mi355.h "evaluation"), no GPU: the host metric
pinned to the reference's SmallObjectMetric, the AP definition on a hand-worked case, the numpy twin of the kernel's threshold
waves against conformal_quantile's matcher, and the argument checks of the unina_eval_* entry points."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    g = load_golden("evalmatch_seed1234.npz")
    n = len(g["counts"])
    return {"n": n, "counts": g["counts"], "geom": g["geom"], "names": [str(s) for s in g["names"]],
            "dets": [g[f"dets/{i:02d}"] for i in range(n)], "labels": [g[f"labels/{i:02d}"] for i in range(n)],
            "rows": [g[f"rows/{i:02d}"] for i in range(n)]}


def test_small_object_metric_reproduces_the_reference_counts(pkg, gold):
    """tests/golden/make_golden_evalmatch.py ran data_loader.SmallObjectMetric on these rows and labels (float64 tensors):
    the numpy mirror adds the same tp / fp / fn for every image, the edge cases among them."""
    from unina_yolo_dla_amd import metrics
    assert gold["n"] >= 40 and max(len(l) for l in gold["labels"]) > 64 and gold["counts"].sum(axis=0).min() >= 20
    for name in ("no_small_label", "no_detection", "two_for_one", "best_taken", "side_15", "iou_half"):
        assert name in gold["names"]
    for i in range(gold["n"]):
        m = metrics.SmallObjectMetric(size_threshold=15, iou_threshold=0.5, image_size=640)
        m.update([gold["rows"][i]], [gold["labels"][i]])
        got = [m.true_positives, m.false_positives, m.false_negatives]
        assert got == gold["counts"][i].tolist(), (gold["names"][i], got, gold["counts"][i])


def test_stored_rows_are_what_evaluate_builds_from_the_records(pkg, gold):
    """The rows the reference was fed are evaluate()'s chain on the stored records: fp32 rescale, predictions.json records,
    normalised rows (so a test that starts from the records checks against the same reference counts)."""
    from unina_yolo_dla_amd import metrics
    for i in range(gold["n"]):
        w, h, nw, nh = (int(v) for v in gold["geom"][i])
        d = gold["dets"][i]
        s = d.copy()
        s["x1"], s["x2"], s["y1"], s["y2"] = d["x1"] * (w / nw), d["x2"] * (w / nw), d["y1"] * (h / nh), d["y2"] * (h / nh)
        rows = metrics.coco_to_metric_rows(metrics.detections_to_coco(s, "x"), w, h)
        assert rows.tobytes() == gold["rows"][i].tobytes(), gold["names"][i]


def test_mean_average_precision_hand_worked(pkg):
    """Two classes, five detections. Class 0 (2 labels) at IoU 0.5: TP, FP, TP by confidence -> recall .5, .5, 1, precision
    1, 1/2, 2/3, monotone 1, 2/3, 2/3; the 51 recall points 0 .. 0.50 read 1, the 50 points 0.51 .. 1 read 2/3:
    AP = (51 + 50 * 2/3) / 101. At the nine higher thresholds only the first is a TP: recall never passes .5, AP = 51/101.
    Class 1 (1 label): FP then TP at thresholds 0.5 .. 0.7 -> precision 1/2 everywhere, AP = 1/2; nothing above -> 0.
    Classes 2 and 3 have no labels and do not enter the mean."""
    from unina_yolo_dla_amd import metrics
    rows = np.array([(0.9, 0, 0x3ff), (0.8, 0, 0), (0.7, 0, 0x1), (0.6, 1, 0), (0.5, 1, 0x1f)], dtype=metrics.AP_ROW_DTYPE)
    got = metrics.mean_average_precision(rows[::-1], [2, 1, 0, 0])          # row order does not matter
    ap0 = (51 + 50 * 2 / 3) / 101
    assert got["map50"] == pytest.approx((ap0 + 0.5) / 2, abs=1e-12)
    assert got["map50_95"] == pytest.approx(((ap0 + 9 * 51 / 101) / 10 + (5 * 0.5) / 10) / 2, abs=1e-12)
    assert metrics.mean_average_precision(rows, {0: 2, 1: 1}) == got
    assert metrics.mean_average_precision(rows, [0, 0, 0, 0]) == {"map50": 0.0, "map50_95": 0.0}
    # a class with labels and no detection contributes an AP of 0
    assert metrics.mean_average_precision(rows, [2, 1, 3, 0])["map50"] == pytest.approx((ap0 + 0.5) / 3, abs=1e-12)


def _conformal_matches(metrics, dets, labels, imgsz):
    """Which detections (in matching order) conformal_quantile matches: the function itself, fed one detection prefix at a
    time (a prefix's matches do not depend on what follows it)."""
    order = np.argsort(-dets["confidence"], kind="stable")
    flags, seen = [], 0
    for k in range(len(dets)):
        try:
            n = metrics.conformal_quantile([dets[order[:k + 1]]], [labels], 0.1, imgsz)["num_calibration_samples"]
        except ValueError:                                # no match yet
            n = 0
        flags.append(n > seen)
        seen = n
    return np.array(flags, dtype=bool)


def test_ap_rows_bit0_is_the_conformal_matcher(pkg, gold):
    from unina_yolo_dla_amd import metrics
    total = 0
    for i in range(gold["n"]):
        dets, labels = gold["dets"][i], gold["labels"][i]
        rows = metrics.ap_rows_numpy(dets, labels, 640)
        assert len(rows) == len(dets)
        order = np.argsort(-dets["confidence"], kind="stable")
        assert np.array_equal(rows["confidence"], dets["confidence"][order]) and np.array_equal(rows["class_id"], dets["class_id"][order])
        want = _conformal_matches(metrics, dets, labels, 640)
        assert np.array_equal((rows["tp_mask"] & 1).astype(bool), want), gold["names"][i]
        total += int((rows["tp_mask"] & 1).sum())
    assert total >= 100


@pytest.fixture(scope="module")
def lib(pkg):
    from unina_yolo_dla_amd import build, engine
    build.build_native()
    return engine.load_library()


def test_eval_symbols_and_argument_checks_without_a_gpu(lib):
    """Every unina_eval_* symbol is exported; create is host-only; update / read refuse bad arguments with UNINA_ERR_ARG
    before any HIP call (the pointers below are never dereferenced by a refused call)."""
    from unina_yolo_dla_amd import engine
    ARG = 4
    for name in ("unina_eval_create", "unina_eval_destroy", "unina_eval_reset_async", "unina_eval_update_async", "unina_eval_read"):
        assert hasattr(lib, name) and name in engine.ABI_SYMBOLS
    assert C.sizeof(engine.EvalParams) == 48 and engine.EVAL_ROW_DTYPE.itemsize == 12
    assert C.sizeof(engine.EvalResult) == 48 + 8 * engine.EVAL_MAX_CLASSES
    h = C.c_void_p()
    assert lib.unina_eval_create(0, 4, 16, 16, None) == ARG
    for nc in (0, -1, engine.EVAL_MAX_CLASSES + 1):
        assert lib.unina_eval_create(0, nc, 16, 16, C.byref(h)) == ARG and not h.value
    assert lib.unina_eval_create(-1, 4, 16, 16, C.byref(h)) == ARG and not h.value
    assert lib.unina_eval_create(0, 4, 16, 16, C.byref(h)) == 0 and h.value
    try:
        p = engine.EvalParams(1.0, 1.0, 1.0, 1.0, 640, 640, 640, 15.0, 0.5)
        fake = 0x1000                                   # aligned, non-null, never touched
        upd = lambda ev, dets, cnt, lab, m, par, what: lib.unina_eval_update_async(ev, dets, cnt, lab, m, par, what, None)   # noqa: E731
        assert upd(None, fake, fake, fake, 1, C.byref(p), 1) == ARG
        assert upd(h, None, fake, fake, 1, C.byref(p), 1) == ARG
        assert upd(h, fake, None, fake, 1, C.byref(p), 1) == ARG
        assert upd(h, fake, fake, fake, 1, None, 1) == ARG
        assert upd(h, fake, fake, None, 1, C.byref(p), 1) == ARG                 # labels announced, none given
        assert upd(h, fake, fake, fake, -1, C.byref(p), 1) == ARG
        assert upd(h, fake, fake, fake, engine.EVAL_MAX_LABELS + 1, C.byref(p), 1) == ARG     # 257 labels
        assert upd(h, fake, fake, fake, 1, C.byref(p), 0) == ARG
        assert upd(h, fake, fake, fake, 1, C.byref(p), 8) == ARG
        assert upd(h, fake + 2, fake, fake, 1, C.byref(p), 1) == ARG             # misaligned records
        assert upd(h, fake, fake, fake + 4, 1, C.byref(p), 1) == ARG             # misaligned labels
        for bad in (engine.EvalParams(1, 1, 1, 1, 0, 640, 640, 15.0, 0.5), engine.EvalParams(1, 1, 1, 1, 640, 640, 0, 15.0, 0.5),
                    engine.EvalParams(1, 1, 1, 1, 640, 640, 640, 15.0, 0.0)):
            assert upd(h, fake, fake, fake, 1, C.byref(bad), 1) == ARG
        res = engine.EvalResult()
        assert lib.unina_eval_read(None, C.byref(res), None, 0, None, 0, None) == ARG
        assert lib.unina_eval_read(h, None, None, 0, None, 0, None) == ARG
        assert lib.unina_eval_read(h, C.byref(res), None, 4, None, 0, None) == ARG
        assert lib.unina_eval_read(h, C.byref(res), None, 0, None, 4, None) == ARG
        assert lib.unina_eval_reset_async(None, None) == ARG
    finally:
        lib.unina_eval_destroy(h)
    lib.unina_eval_destroy(None)                        # a no-op


def test_evaluate_default_result_keys_are_unchanged(pkg, tmp_path):
    """Without the new switches evaluate() returns exactly the old keys; map_metrics adds the two AP numbers on the host path
    (the numpy twin), from the low-confidence pass, whether or not the conformal quantile is asked for."""
    from unina_yolo_dla_amd import evaluate as ev, metrics
    from unina_yolo_dla_amd.engine import DET_DTYPE
    (tmp_path / "images").mkdir()
    (tmp_path / "labels").mkdir()
    np.save(tmp_path / "images" / "a.npy", np.zeros((3, 64, 64), dtype=np.float32))
    (tmp_path / "labels" / "a.txt").write_text("0 0.25 0.25 0.125 0.125\n1 0.75 0.75 0.25 0.25\n")
    dets = np.zeros(3, dtype=DET_DTYPE)
    dets[0] = (12, 12, 20, 20, 0.9, 0, 1, 0)            # the first label exactly
    dets[1] = (40, 40, 56, 57, 0.8, 1, 1, 0)            # the second at IoU 16*16 / (16*17) = 0.941: matched up to 0.90
    dets[2] = (2, 2, 6, 6, 0.7, 1, 1, 0)
    detect = lambda frame, conf, iou, q: dets.copy()    # noqa: E731
    plain = ev.evaluate(detect, str(tmp_path), 64, 0.5, 0.45, 0.0, None, None, 0.1)
    assert set(plain) == {"images", "predictions", "small_object", "conformal"}
    res = ev.evaluate(detect, str(tmp_path), 64, 0.5, 0.45, 0.0, None, None, None, map_metrics=True)
    assert res["conformal"] is None and res["small_object"] == plain["small_object"]
    # class 0: AP 1 at all ten thresholds; class 1: TP then FP -> AP 1 at 0.50 .. 0.90, 0 at 0.95
    assert res["map50"] == pytest.approx(1.0) and res["map50_95"] == pytest.approx((1.0 + 0.9) / 2)
    rows = metrics.ap_rows_numpy(dets, np.array([[0, .25, .25, .125, .125], [1, .75, .75, .25, .25]]), 64)
    assert rows["tp_mask"].tolist() == [0x3ff, 0x1ff, 0]
