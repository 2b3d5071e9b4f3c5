"""Keeps tests/eval_cases.py honest, on the CPU: every constructed evaluation case is run through the host metrics and must hold
what it says -- tied IoUs bit-equal and the tie's direction visible in the rows, a transcription of the kernel's box_iou_xyxy
bit-equal to metrics._box_iou_xyxy on every seam pair while each wrong variant differs where its branch is taken, thresholds met
exactly and missed by one ulp, matches at the ends of the record loops, NaN confidences last in index order with rows that any
other order changes, classes counted as int() truncates, degenerate boxes matching nothing beside ordinary matches, the dense
case consuming every label. A comparison in tests/test_gpu_eval_edges.py can therefore not pass on an empty or indifferent case."""
import warnings

import numpy as np
import pytest

import eval_cases as ec


@pytest.fixture(scope="module")
def metrics(pkg):
    from unina_yolo_dla_amd import metrics
    return metrics


def pairs_of(case):
    """[(record as four np.float32 in imgsz pixels, label as four np.float64, k)] of the same-class pairs of a case."""
    _, dets, labels, geom, p = case
    c = ec.scaled_records(dets, geom, p["imgsz"])
    g = ec.label_pixels(labels, p["imgsz"])
    return [((c["x1"][i], c["y1"][i], c["x2"][i], c["y2"][i]), tuple(g[k]), (i, k)) for i in range(len(dets)) for k in range(len(labels))
            if int(labels[k, 0]) == int(dets["class_id"][i])]


def test_the_registry_is_complete_and_the_references_are_not_empty(pkg):
    assert len(ec.BUILDERS) == 132 and all(any(n.startswith(f) for f in ec.FAMILIES) for n in ec.BUILDERS)
    for f in ec.FAMILIES:
        assert ec.names(f), f
    for name in ec.BUILDERS:
        _, dets, labels, geom, p = ec.case(name)
        assert dets.dtype == ec.det_dtype() and labels.dtype == np.float64 and labels.shape[1] == 5 and len(labels) <= ec.MAX_LABELS
        assert len(dets) <= ec.MAXD and set(p) >= {"imgsz", "size_threshold", "iou_threshold", "what"} and len(geom) == 4
        ref = ec.reference(name)
        assert len(ref["rows"]) == len(ec.used_records(ec.case(name)))
        if name != "count_word_-3":
            assert len(ref["scores"]) > 0 or sum(ref["counts"][:2]) > 0, name          # something is matched or counted


# ---- 1. ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,j", ec.TIE_PAIRS)
def test_tie_pairs_are_bit_equal_and_the_rows_show_the_direction(metrics, i, j):
    for low in "LR":
        name, dets, labels, geom, p = ec.case(f"tie_{i}_{j}_{low}")
        g = ec.label_pixels(labels, 512)
        d0 = (dets["x1"][0], dets["y1"][0], dets["x2"][0], dets["y2"][0])
        a, b = metrics._box_iou_xyxy(d0, g[i]), metrics._box_iou_xyxy(d0, g[j])
        assert a.tobytes() == b.tobytes() and abs(a - 2 / 3) < 1e-15
        assert [int(labels[k, 0]) for k in (i, j)] == [1, 1] and (labels[:, 0] == 1).sum() == 2 and len(labels) == 256
        assert ec.reference(name)["rows"]["tp_mask"].tolist() == ec.TIE_MASKS[low]
        # wave 0
        name, dets, labels, geom, p = ec.case(f"smalltie_{i}_{j}_{low}")
        row = metrics.coco_to_metric_rows(metrics.detections_to_coco(dets[:1], "x"), 512, 512)[0]
        a, b = metrics.SmallObjectMetric._iou(row[:4], labels[i, 1:]), metrics.SmallObjectMetric._iou(row[:4], labels[j, 1:])
        assert a == b == 0.6 or (a == b and abs(a - 0.6) < 1e-15)
        assert ec.reference(name)["counts"] == ec.SMALL_TIE_COUNTS[low]
    assert ec.TIE_MASKS["L"] != ec.TIE_MASKS["R"] and ec.SMALL_TIE_COUNTS["L"] != ec.SMALL_TIE_COUNTS["R"]


def test_tie_pairs_cover_lanes_slots_and_the_contradicting_order():
    lane = lambda g: g % ec.WAVE                                          # noqa: E731
    assert lane(5) == lane(69) and 5 // ec.WAVE != 69 // ec.WAVE         # one lane, two slots
    assert lane(63) > lane(64) and lane(191) > lane(192)                  # lane order against index order
    assert lane(0) == 0 and lane(255) == 63 and lane(31) ^ lane(32) == 63     # met in the LAST step of the xor reduction
    assert len({lane(g) for g in ec.FOUR_LAYOUTS["lane"]}) == 1 and sorted(g // ec.WAVE for g in ec.FOUR_LAYOUTS["lane"]) == [0, 1, 2, 3]
    assert [lane(g) for g in ec.FOUR_LAYOUTS["lanes"]] == [60, 1, 2, 3]    # four lanes, the lowest index in the highest lane


@pytest.mark.parametrize("layout", list(ec.FOUR_LAYOUTS))
def test_four_way_ties_are_bit_equal_and_every_order_reads_differently(metrics, layout):
    seen = {}
    for perm in ec.FOUR_PERMS:
        name, dets, labels, geom, p = ec.case(f"four_{layout}_{''.join(map(str, perm))}")
        g = ec.label_pixels(labels, 512)
        d0 = (dets["x1"][0], dets["y1"][0], dets["x2"][0], dets["y2"][0])
        ious = [metrics._box_iou_xyxy(d0, g[k]) for group in range(3) for k in ec.four_indices(layout, group)]
        assert len({v.tobytes() for v in ious}) == 1 and abs(ious[0] - 2 / 3) < 1e-15, ious
        assert [(labels[:, 0] == c).sum() for c in (1, 2, 3)] == [4, 4, 4]
        ref = ec.reference(name)
        seen[perm] = tuple(ref["rows"]["tp_mask"].tolist())
        # the probes spell the permutation: in group c the directions at the c + 1 lowest indices are consumed
        by = {(int(r["class_id"]), float(r["confidence"])): int(r["tp_mask"]) for r in ref["rows"]}
        for group in range(3):
            consumed = {d for d in range(4) if by[group + 1, float(ec.F(0.5 - 0.01 * d))] == 0x3f0}
            assert consumed == set(perm[:group + 1]), (perm, group, consumed)
    assert len(set(seen.values())) == 24                                  # the rows name the permutation: no other tie order gives them


# ---- 2. seams --------------------------------------------------------------------------------------------------------
def differing(pairs, **variant):
    return sum(1 for a, b, _ in pairs if (1.0 - ec.kernel_iou(a, b)).tobytes() != (1.0 - ec.kernel_iou(a, b, **variant)).tobytes())


@pytest.mark.parametrize("ci", range(16))
def test_seam_pairs_sit_in_their_combination_and_tell_the_wrong_variants_apart(metrics, ci):
    combo = ec.COMBOS[ci]
    case = ec.case(ec.names("seam_")[ci])
    pairs = pairs_of(case)
    assert len(pairs) == ec.SEAM_PAIRS
    for a, b, _ in pairs:
        assert ec.edge_flags(a, b) == combo
        assert 1 <= a[0] < 8 and 1 <= a[1] < 8 and 300 <= a[2] < 600 and 300 <= a[3] < 600
        assert all(0.4 < abs(np.float64(x) - y) < 3.1 for x, y in zip(a, b))
        want = metrics._box_iou_xyxy(a, b)
        assert ec.kernel_iou(a, b).tobytes() == np.float64(want).tobytes() and 0.95 < want < 1
    ref = ec.reference(case[0])
    assert len(ref["scores"]) == ec.SEAM_PAIRS and (ref["rows"]["tp_mask"] == 0x3ff).all()      # every pair yields a score
    fw, fh = combo[0] and combo[2], combo[1] and combo[3]
    assert (differing(pairs, width64=True) > 0) == (fw and not fh)
    assert (differing(pairs, height64=True) > 0) == (fh and not fw)
    assert (differing(pairs, product64=True) > 0) == (fw and fh)
    print(f"{case[0]}: of {len(pairs)} pairs width64 changes {differing(pairs, width64=True)}, height64 {differing(pairs, height64=True)}, "
          f"product64 {differing(pairs, product64=True)}")


@pytest.mark.parametrize("which", ec.EQUAL_EDGES)
def test_equal_edges_are_bit_equal_and_a_strict_comparison_changes_the_score(metrics, which):
    case = ec.case(f"equal_{which}")
    pairs = pairs_of(case)
    assert len(pairs) == ec.EQUAL_PAIRS
    edges = range(4) if which == "all" else [ec.EQUAL_EDGES.index(which)]
    for a, b, _ in pairs:
        for e in range(4):
            assert (np.float64(a[e]) == b[e]) == (e in edges), (which, e, a, b)
        flags = ec.edge_flags(a, b)
        assert flags == ((True,) * 4 if which == "all" else tuple(e % 2 == edges[0] % 2 for e in range(4)))
        assert ec.kernel_iou(a, b).tobytes() == np.float64(metrics._box_iou_xyxy(a, b)).tobytes()
    assert differing(pairs, strict=True) >= 1
    assert len(ec.reference(case[0])["scores"]) == ec.EQUAL_PAIRS


@pytest.mark.parametrize("name", ec.names("scaled_"))
def test_scaled_cases_leave_every_grid_and_the_scale_changes_the_scores(metrics, name):
    case = ec.case(name)
    _, dets, labels, geom, p = case
    w, h, nw, nh = (int(v) for v in geom)
    imgsz = p["imgsz"]
    assert imgsz / nw != 1 or imgsz / nh != 1
    inexact = [float(ec.F(v)) != v for v in (w / nw, h / nh, imgsz / nw, imgsz / nh)]            # sx, sy, cx, cy round in fp32
    assert sum(inexact) >= 1 and (all(inexact[:2]) or w == 1920)            # 333 x 250: sx and sy both; 1920 x 1080: 1920 / 416
    c = ec.scaled_records(dets, geom, imgsz)
    for f in ("x1", "y1", "x2", "y2"):
        assert (c[f] * 8 != np.round(c[f] * 8)).sum() >= 30                            # off the 1/8-pixel grid
    pairs = [pr for pr in pairs_of(case) if pr[2][0] < 32]
    assert len(pairs) == 32
    for a, b, (i, k) in pairs:
        assert i == k and ec.edge_flags(a, b) == ec.COMBOS[i % 16]
        assert ec.kernel_iou(a, b).tobytes() == np.float64(metrics._box_iou_xyxy(a, b)).tobytes()
    for variant, live in (("width64", lambda f: f[0] and f[2] and not (f[1] and f[3])), ("height64", lambda f: f[1] and f[3] and not (f[0] and f[2])),
                          ("product64", all)):
        assert differing([pr for pr in pairs if live(ec.COMBOS[pr[2][0] % 16])], **{variant: True}) >= 1, variant
    ref = ec.reference(name)
    assert len(ref["scores"]) == 32 + ec.SCALED_SMALL and ref["counts"][0] >= 1       # wave 0 matches through sx, sy
    flat = ec.reference_of((name, dets, labels, ec.square(imgsz), p))                    # the same case at scale 1
    assert flat["scores"].tobytes() != ref["scores"].tobytes() and flat["counts"] != ref["counts"]


def test_iou_thresholds_are_met_exactly_and_missed_by_one_ulp(metrics):
    case = ec.case("iou_thresholds")
    ious = [metrics._box_iou_xyxy(a, b) for a, b, _ in pairs_of(case)]
    assert ious[0] == 0.5 and ious[1] == np.nextafter(0.5, 0) and ious[2] == 0.75 and ious[3] == np.nextafter(0.75, 0)
    ref = ec.reference("iou_thresholds")
    assert ref["rows"]["tp_mask"].tolist() == ec.THRESHOLD_MASKS == [0x001, 0x000, 0x03f, 0x01f]
    assert ref["scores"].tolist() == [0.5, 0.25, 1.0 - np.nextafter(0.75, 0)]


@pytest.mark.parametrize("thr", (0.3, 0.75))
def test_small_object_threshold_met_exactly_and_missed_by_one_ulp(metrics, thr):
    name, dets, labels, geom, p = ec.case(f"small_threshold_{thr}")
    assert p["iou_threshold"] == thr
    ious = [ec.centre_iou((dets["x1"][k], dets["y1"][k], dets["x2"][k], dets["y2"][k]), labels[k]) for k in range(2)]
    assert ious[0] == thr and ious[1] == np.nextafter(thr, 0)
    assert ec.reference(name)["counts"] == (1, 1, 1)
    other = dict(p, iou_threshold=0.5 if thr == 0.3 else 0.8)
    assert ec.reference_of((name, dets, labels, geom, other))["counts"] == ((0, 2, 2) if thr == 0.3 else (0, 2, 2))


@pytest.mark.parametrize("t", (15, 8))
def test_a_side_of_exactly_the_size_threshold_is_not_small(metrics, t):
    name, dets, labels, geom, p = ec.case(f"size_threshold_{t}")
    m = metrics.SmallObjectMetric(size_threshold=t, image_size=512)
    assert [m._is_small(l[3], l[4]) for l in labels] == [False, True, True] and labels[0, 3] * 512 == t
    rows = metrics.coco_to_metric_rows(metrics.detections_to_coco(dets, "x"), 512, 512)
    assert [m._is_small(r[2], r[3]) for r in rows] == [False, True, False, True] and rows[2, 2] * 512 == t
    assert ec.reference(name)["counts"] == (1, 1, 1)
    # one notch up, both exact-t boxes would count: the label as a TP, the prediction as an FP
    assert ec.reference_of((name, dets, labels, geom, dict(p, size_threshold=t + 0.125)))["counts"] == (2, 2, 1)


# ---- 3. order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ec.RECORD_COUNTS)
def test_record_counts_match_at_the_end_of_both_loops(metrics, n):
    name, dets, labels, geom, p = ec.case(f"count_{n}")
    assert len(dets) == n and len(labels) == ec.COUNT_LABELS
    ref = ec.reference(name)
    order = ec.matching_order(dets["confidence"])
    assert order[0] == n - 1 and order[-1] == n // 2
    masks = np.zeros(n, dtype=np.uint32)
    masks[order] = ref["rows"]["tp_mask"]
    assert ref["rows"]["tp_mask"][-64:].any() and ref["rows"]["tp_mask"][-1] != 0      # the last 64 ranks (match bits k & 63, k / 64)
    assert masks[-64:].any() and masks[-1] == 0x3ff                                   # the last 64 indices (the ranking loop)
    if n > 64:
        assert len(np.unique(ref["rows"]["tp_mask"])) >= 5 and ref["counts"][0] > 0 and ref["counts"][1] > 0


@pytest.mark.parametrize("name", ec.names("conf_"))
def test_confidence_order_is_visible_in_the_rows(metrics, name):
    _, dets, labels, geom, p = ec.case(name)
    conf = dets["confidence"]
    order = ec.matching_order(conf)
    nan = np.isnan(conf)
    n = len(conf)
    if name == "conf_nan":
        assert nan[[0, n // 2, n - 1]].all() and 20 < nan.sum() < n // 2
        assert (conf == 0.5).sum() > 20 and (conf == 0.25).sum() > 10
    if name == "conf_inf":
        assert (conf == np.inf).sum() > 10 and (conf == -np.inf).sum() > 10 and nan.sum() > 5
        fin = order[:n - nan.sum()]
        assert np.isposinf(conf[fin[:5]]).all() and np.isneginf(conf[fin[-5:]]).all()
    if name == "conf_zero_sign":
        z = conf == 0
        assert (np.signbit(conf) & z).sum() > 50 and (~np.signbit(conf) & z).sum() > 50
        zi = order[z[order]]
        assert (np.diff(zi) > 0).all()                                                  # -0.0 and +0.0 are one key: index order
    if name == "conf_equal_1024":
        assert n == 1024 and len(np.unique(conf)) == 1 and (order == np.arange(n)).all()
    if nan.any():
        tail = order[n - nan.sum():]
        assert nan[tail].all() and (np.diff(tail) > 0).all()                            # NaN last, in index order
    ref = ec.reference(name)
    right = np.zeros(n, dtype=np.uint32)
    right[order] = ref["rows"]["tp_mask"]
    assert np.array_equal(ec.masks_in_order(dets, labels, p["imgsz"], order), right)      # the surrogate reproduces the order
    others = ec.other_orders(conf)
    assert len(others) >= (1 if name == "conf_equal_1024" else 2)
    for what, alt in others.items():
        if np.array_equal(alt, order):
            assert name == "conf_equal_1024" and what == "index"
            continue
        assert sorted(alt.tolist()) == list(range(n))
        assert not np.array_equal(ec.masks_in_order(dets, labels, p["imgsz"], alt), right), (name, what)


def test_count_words_outside_the_buffer(metrics):
    c = ec.case("count_word_5000")
    assert len(c[1]) == ec.MAXD and len(ec.used_records(c)) == ec.MAXD
    ref = ec.reference("count_word_5000")
    assert len(ref["rows"]) == ec.MAXD and ref["rows"]["tp_mask"][0] == 0x3ff and ref["counts"][0] > 0
    c = ec.case("count_word_-3")
    assert len(c[1]) == 30 and len(ec.used_records(c)) == 0
    ref = ec.reference("count_word_-3")
    small = sum(1 for l in c[2] if l[3] * 640 < 15 and l[4] * 640 < 15)
    assert ref["counts"] == (0, 0, small) and small > 5 and len(ref["rows"]) == 0 and len(ref["scores"]) == 0
    assert ref["label_counts"].sum() == len(c[2])                                       # the labels are still counted
    assert ec.reference_of(("x", c[1], c[2], c[3], dict(c[4], count=30)))["counts"][0] > 0       # the records there are would match


# ---- 4. / 6. the image set of the flag and capacity tests ------------------------------------------------------------
def test_flag_images_fill_every_output(metrics):
    refs = [ec.reference(f"flags_{w}") for w in "AB"]
    for r in refs:
        assert min(r["counts"]) >= 5 and len(r["scores"]) >= 30 and len(np.unique(r["rows"]["tp_mask"])) >= 6
        assert (r["label_counts"][:4] > 0).all()
    assert refs[0]["counts"] != refs[1]["counts"] and len(refs[0]["scores"]) != len(refs[1]["scores"])
    assert len(refs[0]["rows"]) != len(refs[1]["rows"])


# ---- 5. classes and degenerate input ---------------------------------------------------------------------------------
def test_classes_truncate_and_only_those_inside_are_counted(metrics):
    want = {"nc1": {0: 4}, "nc256": {0: 2, 255: 4, 1: 2, 254: 2}, "nc4": {3: 2, 1: 2, 0: 2}}
    for which, counted in want.items():
        name, dets, labels, geom, p = ec.case(f"classes_{which}")
        ref = ec.reference(name)
        lc = {int(k): int(v) for k, v in enumerate(ref["label_counts"]) if v}
        assert lc == counted, (which, lc)
        assert (ref["rows"]["tp_mask"] == 0x1ff).all() and len(ref["scores"]) == len(dets)      # also classes 256, 7 and -3 match
        assert ref["counts"] == (0, 0, len(dets))
        outside = [int(c) for c in labels[:, 0] if not 0 <= int(c) < p["num_classes"]]
        assert len(outside) >= 4 and set(dets["class_id"].tolist()) >= set(outside)
    assert {-3, 256} <= set(ec.case("classes_nc256")[1]["class_id"].tolist()) and {-3, 7} <= set(ec.case("classes_nc4")[1]["class_id"].tolist())
    assert 1.9 in ec.case("classes_nc256")[2][:, 0] and 1 in ec.case("classes_nc256")[1]["class_id"]


def test_degenerate_boxes_match_nothing_beside_ordinary_matches(metrics):
    name, dets, labels, geom, p = ec.case("degenerate")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ref = ec.reference_of(ec.case(name))                               # the host metrics do not raise
    rows = ref["rows"]
    bad = rows["confidence"] == ec.F(ec.DEGENERATE_CONF)
    assert bad.sum() == 13 and (rows["tp_mask"][bad] == 0).all()
    good = rows["confidence"] > 0.6
    assert good.sum() == 6 and (rows["tp_mask"][good] != 0).all() and ref["counts"][0] == 3
    assert (rows["tp_mask"][rows["confidence"] < 0.5] == 0).all()          # ordinary records on degenerate labels: nothing
    d = np.stack([dets[f] for f in ("x1", "y1", "x2", "y2")], axis=1)
    assert np.isnan(d).any(axis=1).sum() == 2 and np.isinf(d).any(axis=1).sum() == 4
    fin = np.isfinite(d).all(axis=1)
    assert (fin & ((d[:, 2] < d[:, 0]) | (d[:, 3] < d[:, 1]))).sum() == 4 and (fin & ((d[:, 2] == d[:, 0]) | (d[:, 3] == d[:, 1]))).sum() == 3
    assert np.isnan(labels).any(axis=1).sum() == 3 and np.isinf(labels).any(axis=1).sum() == 1
    assert ((labels[:, 3] == 0) | (labels[:, 4] == 0)).sum() == 2 and ((labels[:, 3] < 0) | (labels[:, 4] < 0)).sum() == 2
    m = metrics.SmallObjectMetric(size_threshold=15, image_size=512)
    small = [bool(m._is_small(l[3], l[4])) for l in labels]
    # zero-width, negative and NaN-centred small labels: false negatives
    assert sum(small) == 6 and sum(small[6:]) == 3 and ref["counts"][2] == 3


# ---- 7. dense --------------------------------------------------------------------------------------------------------
def test_dense_case_consumes_the_labels(metrics):
    name, dets, labels, geom, p = ec.case("dense")
    assert len(dets) == 1024 and len(labels) == 256 and (labels[:, 0] == 0).all() and (dets["class_id"] == 0).all()
    ref = ec.reference("dense")
    per = [int(((ref["rows"]["tp_mask"] >> j) & 1).sum()) for j in range(10)]
    print("dense: labels matched per threshold", per, "counts", ref["counts"])
    assert per[0] >= 200 and per[9] < per[0] and all(a >= b for a, b in zip(per, per[1:])) and per[9] > 0
    assert ref["counts"][0] >= 200 and len(ref["scores"]) == per[0]
