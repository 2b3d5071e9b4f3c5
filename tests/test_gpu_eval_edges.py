"""The evaluation stage at its edges (-m gpu): the constructed cases of tests/eval_cases.py through csrc/evalmatch.hip. What the
cases hold and why none can pass on an empty or indifferent input is proved on the CPU by tests/test_eval_cases_cpu.py.

Which piece of the kernel a family pins:
    ties         wave_best's lowest-index rule across lanes whose order is not the index order (lane l owns l, l + 64, ...),
                 inside one lane's slots, in the last xor step; two- and four-way, in the threshold waves and in wave 0
    seams        box_iou_xyxy's fp32 / double distinction in all 16 edge combinations, edges bit-equal to the record's, the
                 fp32 scale through cx, cy != 1 and sx, sy that round; IoU exactly on 0.5 / 0.75 / iou_threshold and one ulp
                 below; sides of exactly size_threshold pixels
    order        sorts_before with NaN, +-inf, +-0.0 and all-equal confidences; the strides of the ranking and row loops
                 (kEvalBlock = 704) and of the match bits (k & 63, k / 64); a count word outside [0, 1024]
    flags        each subset of `what` writes its own outputs and nothing else; evaluate()'s interleaving on one handle
    classes      num_classes 1 and 256, label classes beside and outside the range, fractional ones; boxes that are no boxes
    capacity     lists exactly full and one short, the boundary inside and between updates, reset after overflow, two handles,
                 a side stream
    dense        1024 records on 256 labels of one class: every lane slot holds a candidate and is consumed
No tolerance anywhere: counters, scores (float64 bits, in order), rows and label_counts are compared as bytes with the host
metrics, and every comparison also checks overflow and guard_intact. One workgroup per call."""
import numpy as np
import pytest

import eval_cases as ec
from records import assert_records_equal, det_buffer

pytestmark = pytest.mark.gpu

CAP = 2048          # list capacity where the test is not about capacity: above every case's counts


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def engine(pkg):
    from unina_yolo_dla_amd import engine
    return engine


def eval_params(engine, case):
    _, _, _, geom, p = case
    w, h, nw, nh = (int(v) for v in geom)
    return engine.EvalParams(w / nw, h / nh, p["imgsz"] / nw, p["imgsz"] / nh, w, h, p["imgsz"], p["size_threshold"], p["iou_threshold"])


def update(torch, engine, ev, case, what=None, stream=None):
    _, dets, labels, _, p = case
    buf = det_buffer(torch, dets, int(p.get("count", len(dets))))
    ev.update(buf, labels.copy(), eval_params(engine, case), p["what"] if what is None else what, stream)


def expected(names, whats=None):
    """The host reference of one update per name: counters summed, lists concatenated; a name counts into an output only where
    its `what` has the flag."""
    whats = [ec.ALL] * len(names) if whats is None else whats
    refs = [ec.reference(n) for n in names]
    pick = lambda flag, key, empty: [r[key] for r, w in zip(refs, whats) if w & flag] or [empty]     # noqa: E731
    from unina_yolo_dla_amd import metrics
    return {"counts": np.sum(pick(ec.SMALL, "counts", (0, 0, 0)), axis=0).tolist(),
            "scores": np.concatenate(pick(ec.CONFORMAL, "scores", np.zeros(0))),
            "rows": np.concatenate(pick(ec.AP, "rows", np.zeros(0, dtype=metrics.AP_ROW_DTYPE))),
            "label_counts": np.sum(pick(ec.AP, "label_counts", np.zeros(256, dtype=np.int64)), axis=0).tolist()}


def compare(got, want, name, overflow=0, max_scores=CAP, max_rows=CAP):
    """Byte equality of everything read back with the host reference; the lists as far as the capacity goes, the counts true."""
    res, scores, rows = got
    assert [res.tp, res.fp, res.fn] == want["counts"], (name, [res.tp, res.fp, res.fn], want["counts"])
    assert res.n_scores == len(want["scores"]), (name, res.n_scores, len(want["scores"]))
    assert scores.dtype == np.float64 and scores.tobytes() == want["scores"][:max_scores].tobytes(), (name, scores, want["scores"])
    assert res.n_rows == len(want["rows"]), (name, res.n_rows, len(want["rows"]))
    assert_records_equal(rows, want["rows"][:max_rows], name, "AP")
    assert list(res.label_counts) == want["label_counts"], (name, list(res.label_counts), want["label_counts"])
    assert res.overflow == overflow and res.guard_intact == 1, (name, res.overflow, res.guard_intact)


def run(torch, engine, names, whats=None, max_scores=CAP, max_rows=CAP):
    """One handle, one update per name -> (EvalResult, scores, rows). num_classes is the first case's."""
    ev = engine.DeviceEval(ec.case(names[0])[4].get("num_classes", 4), max_scores, max_rows)
    try:
        ev.reset()
        for i, n in enumerate(names):
            update(torch, engine, ev, ec.case(n), None if whats is None else whats[i])
        return ev.read()
    finally:
        ev.close()


def check(torch, engine, name):
    got = run(torch, engine, [name])
    compare(got, expected([name]), name)
    return got


# ---- 1. ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,j", ec.TIE_PAIRS)
def test_equal_iou_takes_the_lowest_label_index(pkg, torch_cuda, engine, i, j):
    for low in "LR":
        _, _, rows = check(torch_cuda, engine, f"tie_{i}_{j}_{low}")
        assert rows["tp_mask"].tolist() == ec.TIE_MASKS[low], (i, j, low)
        res, _, _ = check(torch_cuda, engine, f"smalltie_{i}_{j}_{low}")
        assert (res.tp, res.fp, res.fn) == ec.SMALL_TIE_COUNTS[low], (i, j, low)


@pytest.mark.parametrize("layout", list(ec.FOUR_LAYOUTS))
def test_four_way_ties_are_consumed_in_index_order(pkg, torch_cuda, engine, layout):
    for perm in ec.FOUR_PERMS:
        check(torch_cuda, engine, f"four_{layout}_{''.join(map(str, perm))}")


# ---- 2. seams --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.names("seam_"))
def test_scores_carry_the_fp32_seams_of_every_edge_combination(pkg, torch_cuda, engine, name):
    check(torch_cuda, engine, name)


@pytest.mark.parametrize("name", ec.names("equal_"))
def test_an_edge_equal_to_the_records_is_the_records(pkg, torch_cuda, engine, name):
    check(torch_cuda, engine, name)


@pytest.mark.parametrize("name", ec.names("scaled_"))
def test_seams_through_the_fp32_scale_of_other_geometries(pkg, torch_cuda, engine, name):
    check(torch_cuda, engine, name)


def test_iou_on_a_threshold_and_one_ulp_below(pkg, torch_cuda, engine):
    _, scores, rows = check(torch_cuda, engine, "iou_thresholds")
    assert rows["tp_mask"].tolist() == ec.THRESHOLD_MASKS and scores.tolist()[:2] == [0.5, 0.25]


@pytest.mark.parametrize("name", ec.names("small_threshold_") + ec.names("size_threshold_"))
def test_small_object_thresholds_are_exact(pkg, torch_cuda, engine, name):
    res, _, _ = check(torch_cuda, engine, name)
    assert (res.tp, res.fp, res.fn) == (1, 1, 1)


# ---- 3. order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ec.RECORD_COUNTS)
def test_record_counts_beside_the_loop_strides(pkg, torch_cuda, engine, n):
    check(torch_cuda, engine, f"count_{n}")


@pytest.mark.parametrize("name", ec.names("conf_"))
def test_confidences_that_are_equal_or_not_numbers(pkg, torch_cuda, engine, name):
    check(torch_cuda, engine, name)


def test_count_word_is_clamped(pkg, torch_cuda, engine):
    res, _, _ = check(torch_cuda, engine, "count_word_5000")
    assert res.n_rows == 1024
    res, scores, rows = check(torch_cuda, engine, "count_word_-3")
    assert (res.tp, res.fp) == (0, 0) and res.fn > 5 and res.n_rows == 0 and res.n_scores == 0


# ---- 4. flags --------------------------------------------------------------------------------------------------------
def test_each_flag_writes_its_own_outputs_only(pkg, torch_cuda, engine):
    names = ["flags_A", "flags_B"]
    full = run(torch_cuda, engine, names)
    compare(full, expected(names), "what=7")
    for what in range(1, 8):
        got = run(torch_cuda, engine, names, [what] * 2)
        compare(got, expected(names, [what] * 2), f"what={what}")
        res, scores, rows = got
        if what & ec.SMALL:
            assert (res.tp, res.fp, res.fn) == (full[0].tp, full[0].fp, full[0].fn)
        else:
            assert (res.tp, res.fp, res.fn) == (0, 0, 0)
        if what & ec.CONFORMAL:
            assert res.n_scores == full[0].n_scores and scores.tobytes() == full[1].tobytes()
        else:
            assert res.n_scores == 0 and len(scores) == 0
        if what & ec.AP:
            assert res.n_rows == full[0].n_rows and rows.tobytes() == full[2].tobytes() and list(res.label_counts) == list(full[0].label_counts)
        else:
            assert res.n_rows == 0 and len(rows) == 0 and not any(res.label_counts)


def test_evaluates_interleaving_on_one_handle(pkg, torch_cuda, engine):
    """Image A with SMALL, then CONFORMAL | AP, then image B likewise: one `what = 7` update per image."""
    names, whats = ["flags_A", "flags_A", "flags_B", "flags_B"], [1, 6, 1, 6]
    got = run(torch_cuda, engine, names, whats)
    compare(got, expected(["flags_A", "flags_B"]), "interleaved")
    compare(got, expected(names, whats), "interleaved, per update")


# ---- 5. classes and degenerate input ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.names("classes_") + ["degenerate"])
def test_classes_outside_the_range_and_boxes_that_are_none(pkg, torch_cuda, engine, name):
    res, _, rows = check(torch_cuda, engine, name)
    if name == "degenerate":
        assert (rows["tp_mask"][rows["confidence"] == np.float32(ec.DEGENERATE_CONF)] == 0).all() and res.tp == 3


# ---- 6. capacity and handles -----------------------------------------------------------------------------------------
def test_lists_exactly_full_and_one_short(pkg, torch_cuda, engine):
    names = ["flags_A", "flags_B"]
    want = expected(names)
    ns, nr, na, sa = len(want["scores"]), len(want["rows"]), len(ec.reference("flags_A")["rows"]), len(ec.reference("flags_A")["scores"])
    assert 0 < sa < ns and 0 < na < nr
    # (max_scores, max_rows, flags): full | one short | the boundary between the updates | inside the first | inside the second
    for ms, mr, flags in ((ns, nr, 0), (ns - 1, nr, 1), (ns, nr - 1, 2), (ns - 1, nr - 1, 3), (sa, na, 3), (sa - 7, na - 30, 3), (sa + 7, na + 30, 3),
                          (sa, nr, 1), (ns, na, 2)):
        got = run(torch_cuda, engine, names, max_scores=ms, max_rows=mr)
        assert len(got[1]) == min(ms, ns) and len(got[2]) == min(mr, nr)
        compare(got, want, f"max_scores={ms} max_rows={mr}", overflow=flags, max_scores=ms, max_rows=mr)


def test_reset_clears_an_overflow_and_the_next_run_is_exact(pkg, torch_cuda, engine):
    ev = engine.DeviceEval(4, 10, 10)
    try:
        ev.reset()
        update(torch_cuda, engine, ev, ec.case("flags_A"))
        compare(ev.read(), expected(["flags_A"]), "overflowing", overflow=3, max_scores=10, max_rows=10)
        ev.reset()
        res, scores, rows = ev.read()
        assert bytes(res)[:48 - 4] == bytes(44) and res.guard_intact == 1 and not any(res.label_counts) and len(scores) == 0 and len(rows) == 0
        update(torch_cuda, engine, ev, ec.case("iou_thresholds"))
        compare(ev.read(), expected(["iou_thresholds"]), "after reset", max_scores=10, max_rows=10)
    finally:
        ev.close()


def uploaded(torch, engine, name):
    """(det buffer, labels on the device, params) of a case, for updates that must not upload on another stream."""
    _, dets, labels, _, p = ec.case(name)
    return det_buffer(torch, dets, len(dets)), torch.from_numpy(labels.copy()).cuda(), eval_params(engine, ec.case(name))


def test_two_handles_updated_alternately_each_on_its_own_stream(pkg, torch_cuda, engine):
    torch = torch_cuda
    a, b = uploaded(torch, engine, "flags_A"), uploaded(torch, engine, "flags_B")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    e1, e2 = engine.DeviceEval(4, CAP, CAP), engine.DeviceEval(4, CAP, CAP)
    try:
        e1.reset(s1)
        e2.reset(s2)
        for first, second in ((a, b), (b, a), (a, a)):
            e1.update(*first, ec.ALL, s1)
            e2.update(*second, ec.ALL, s2)
        compare(e1.read(s1), expected(["flags_A", "flags_B", "flags_A"]), "handle 1")
        compare(e2.read(s2), expected(["flags_B", "flags_A", "flags_A"]), "handle 2")
    finally:
        e1.close()
        e2.close()


def test_one_run_on_a_side_stream(pkg, torch_cuda, engine):
    torch = torch_cuda
    a = uploaded(torch, engine, "flags_A")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ev = engine.DeviceEval(4, CAP, CAP)
    try:
        ev.reset(s)
        ev.update(*a, ec.ALL, s)
        compare(ev.read(s), expected(["flags_A"]), "side stream")
    finally:
        ev.close()


# ---- 7. dense --------------------------------------------------------------------------------------------------------
def test_dense_worst_case(pkg, torch_cuda, engine):
    res, scores, rows = check(torch_cuda, engine, "dense")
    per = [int(((rows["tp_mask"] >> j) & 1).sum()) for j in range(10)]
    assert per[0] >= 200 and per[9] < per[0] and res.tp >= 200
    print(f"dense: labels matched per threshold {per}, tp / fp / fn {res.tp} / {res.fp} / {res.fn}")
