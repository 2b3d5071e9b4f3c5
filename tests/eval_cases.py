"""Constructed inputs of the evaluation stage (plain numpy, no GPU, no torch): records and labels at the places where
csrc/evalmatch.hip decides -- equal IoU (wave_best), the fp32 / fp64 seams of box_iou_xyxy, the confidence order (sorts_before),
the strides of the ranking, row and match-bit loops, the flags, classes, degenerate boxes and the dense worst case -- and the
host reference of each, built from metrics.* alone. tests/test_eval_cases_cpu.py proves on the host metrics that every case holds
what it says; tests/test_gpu_eval_edges.py runs them, byte for byte.

A case is (name, dets, labels, geom, params): dets a DET_DTYPE array, labels [M, 5] float64 rows cls, xc, yc, w, h, geom
(width, height, net_width, net_height) as evaluate() knows them, params a dict with imgsz, size_threshold, iou_threshold and
what, plus num_classes (default 4) and count (the count word, default len(dets)) where a case needs them.

Coordinates. At imgsz 512 a label on the 1/8-pixel grid normalises exactly and the kernel's (xc -+ w / 2) * imgsz gives the
pixels back exactly, so IoUs there are exact rationals and equal ones are bit-equal. The seam cases want the opposite: records
with full fp32 mantissas, left / top in [1, 8) and right / bottom in [300, 600), so that a2 - a0 rounds in fp32."""
import functools
import itertools
import warnings

import numpy as np

SMALL, CONFORMAL, AP, ALL = 1, 2, 4, 7          # UNINA_EVAL_*
MAXD, MAX_LABELS, WAVE, EVAL_BLOCK = 1024, 256, 64, 704   # MAX_DETECTIONS, UNINA_EVAL_MAX_LABELS, kWave, kEvalBlock
F = np.float32


def det_dtype():
    from unina_yolo_dla_amd.engine import DET_DTYPE
    return DET_DTYPE


# ---- the host reference ----------------------------------------------------------------------------------------------
def host_image(metrics, dets, labels, geom, imgsz=640, size_threshold=15, iou_threshold=0.5):
    """The host path of evaluate() for one image: (tp, fp, fn), conformal scores in order, AP rows."""
    w, h, nw, nh = (int(v) for v in geom)
    s = dets.copy()
    s["x1"], s["x2"], s["y1"], s["y2"] = dets["x1"] * (w / nw), dets["x2"] * (w / nw), dets["y1"] * (h / nh), dets["y2"] * (h / nh)
    m = metrics.SmallObjectMetric(size_threshold=size_threshold, iou_threshold=iou_threshold, image_size=imgsz)
    m.update([metrics.coco_to_metric_rows(metrics.detections_to_coco(s, "x"), w, h)], [labels])
    c = dets.copy()
    c["x1"], c["x2"] = dets["x1"] * (imgsz / nw), dets["x2"] * (imgsz / nw)
    c["y1"], c["y2"] = dets["y1"] * (imgsz / nh), dets["y2"] * (imgsz / nh)
    rows = metrics.ap_rows_numpy(c, labels, imgsz)
    scores = conformal_scores(metrics, c, labels, imgsz)
    assert len(scores) == int((rows["tp_mask"] & 1).sum())
    return (m.true_positives, m.false_positives, m.false_negatives), scores, rows


def conformal_scores(metrics, dets, labels, imgsz):
    """metrics.conformal_quantile's own score list for one image (it only returns statistics): np.quantile is intercepted
    to see the array it is handed."""
    seen = []
    real = np.quantile
    try:
        np.quantile = lambda s, q: (seen.append(np.array(s, dtype=np.float64)), real(s, q))[1]
        try:
            metrics.conformal_quantile([dets], [labels], 0.1, imgsz)
        except ValueError:                               # no matched prediction
            return np.zeros(0)
    finally:
        np.quantile = real
    return seen[0]


def scaled_records(dets, geom, imgsz):
    """The records as conformal_quantile sees them: evaluate()'s fp32 scale to imgsz pixels."""
    nw, nh = int(geom[2]), int(geom[3])
    c = dets.copy()
    c["x1"], c["x2"] = dets["x1"] * (imgsz / nw), dets["x2"] * (imgsz / nw)
    c["y1"], c["y2"] = dets["y1"] * (imgsz / nh), dets["y2"] * (imgsz / nh)
    return c


def label_pixels(labels, imgsz):
    """conformal_quantile's gts: [M, 4] float64 x1, y1, x2, y2."""
    l = np.asarray(labels, dtype=np.float64).reshape(-1, 5)
    return np.stack([(l[:, 1] - l[:, 3] / 2) * imgsz, (l[:, 2] - l[:, 4] / 2) * imgsz, (l[:, 1] + l[:, 3] / 2) * imgsz,
                     (l[:, 2] + l[:, 4] / 2) * imgsz], axis=1)


def used_records(case):
    """The records the count word lets through: min(max(count, 0), MAX_DETECTIONS) of them."""
    _, dets, _, _, p = case
    return dets[:min(max(int(p.get("count", len(dets))), 0), MAXD)]


def label_counts(labels, num_classes):
    """int() truncates; only classes inside [0, num_classes) are counted. int64 [256]."""
    out = np.zeros(256, dtype=np.int64)
    for c in np.asarray(labels, dtype=np.float64).reshape(-1, 5)[:, 0]:
        if 0 <= int(c) < num_classes:
            out[int(c)] += 1
    return out


def reference_of(case):
    """{"counts": (tp, fp, fn), "scores": float64 [n], "rows": AP_ROW_DTYPE [m], "label_counts": int64 [256]} from metrics.*."""
    from unina_yolo_dla_amd import metrics
    _, _, labels, geom, p = case
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)          # inf - inf in the degenerate cases
        counts, scores, rows = host_image(metrics, used_records(case), labels, geom, p["imgsz"], p["size_threshold"], p["iou_threshold"])
    return {"counts": tuple(int(v) for v in counts), "scores": scores, "rows": rows,
            "label_counts": label_counts(labels, p.get("num_classes", 4))}


@functools.lru_cache(maxsize=None)
def reference(name):
    """reference_of(case(name)), computed once per process; callers leave it unchanged."""
    return reference_of(case(name))


# ---- building blocks -------------------------------------------------------------------------------------------------
def params(imgsz=512, size_threshold=15.0, iou_threshold=0.5, what=ALL, **more):
    return dict(imgsz=imgsz, size_threshold=size_threshold, iou_threshold=iou_threshold, what=what, **more)


def square(size):
    return np.array([size, size, size, size])


def records(rows):
    """[(x1, y1, x2, y2, confidence, class_id)] -> DET_DTYPE, valid = 1."""
    out = np.zeros(len(rows), dtype=det_dtype())
    for i, r in enumerate(rows):
        out[i] = (*r[:5], int(r[5]), 1, 0)
    return out


def label_px(cls, x1, y1, x2, y2, imgsz):
    """A label row from pixel corners (exact at imgsz 512 on the 1/8-pixel grid)."""
    return [cls, (x1 + x2) / 2 / imgsz, (y1 + y2) / 2 / imgsz, (x2 - x1) / imgsz, (y2 - y1) / imgsz]


def filler(n, cls=0, imgsz=512):
    """n small labels of class `cls`, 4 x 4 pixels on an 8-pixel grid from (300, 300): far from every constructed box."""
    return np.array([label_px(cls, 300 + 8 * (g % 16), 300 + 8 * (g // 16), 304 + 8 * (g % 16), 304 + 8 * (g // 16), imgsz)
                     for g in range(n)], dtype=np.float64).reshape(-1, 5)


def random_image(seed, n, m, classes=4, imgsz=640):
    """n records and m labels OFF any grid: labels 4..24 pixels, records jittered copies of labels (70 %) or strays, every
    coordinate a full-mantissa float32, distinct confidences k / 2^20."""
    rng = np.random.RandomState(seed)
    w, h = rng.uniform(4, 24, m), rng.uniform(4, 24, m)
    x1, y1 = rng.uniform(0, imgsz - 24, m), rng.uniform(0, imgsz - 24, m)
    cls = rng.randint(0, classes, m)
    labels = np.stack([cls, (x1 + w / 2) / imgsz, (y1 + h / 2) / imgsz, w / imgsz, h / imgsz], axis=1).astype(np.float64).reshape(-1, 5)
    dets = np.zeros(n, dtype=det_dtype())
    conf = rng.permutation(np.arange(1, (1 << 20)))[:n] / float(1 << 20)
    for i in range(n):
        if m and rng.rand() < 0.7:
            g = rng.randint(m)
            j = rng.uniform(-2, 2, 4)
            box, c = (x1[g] + j[0], y1[g] + j[1], x1[g] + w[g] + j[2], y1[g] + h[g] + j[3]), cls[g]
        else:
            bw, bh = rng.uniform(2, 30, 2)
            bx, by = rng.uniform(0, imgsz - 40, 2)
            box, c = (bx, by, bx + bw, by + bh), rng.randint(0, classes)
        dets[i] = (*box, conf[i], int(c), 1, 0)
    return dets, labels


def exact_copy(labels, g, imgsz, conf):
    """A record on label g's own pixels (as fp32 rounds them): IoU 1 up to rounding, a match at every threshold."""
    b = label_pixels(labels[g:g + 1], imgsz)[0]
    return (*b, conf, int(labels[g, 0]), 1, 0)


# ---- 1. ties: the lowest label index wins ----------------------------------------------------------------------------
TIE_PAIRS = ((0, 1), (31, 32), (5, 69), (63, 64), (191, 192), (0, 255))
TIE_MASKS = {"L": [0x00f, 0x3f0], "R": [0x00f, 0x3ff]}        # rows of D0, D1 with L / R at the lower index
SMALL_TIE_COUNTS = {"L": (1, 1, 255), "R": (2, 0, 254)}


def tie_case(i, j, low):
    """D0 = (100, 100, 120, 120) ties between L (4 px left) and R (4 px right) at IoU 2/3; D1 is L's box. With L at the lower
    index D0 takes L up to 0.65 and D1 finds only R (IoU 3/7); with R there, D1 finds L at every threshold."""
    labels = filler(MAX_LABELS)
    L, R = label_px(1, 96, 100, 116, 120, 512), label_px(1, 104, 100, 124, 120, 512)
    labels[i], labels[j] = (L, R) if low == "L" else (R, L)
    dets = records([(100, 100, 120, 120, 0.9, 1), (96, 100, 116, 120, 0.8, 1)])
    return f"tie_{i}_{j}_{low}", dets, labels, square(512), params()


def small_tie_case(i, j, low):
    """The same for wave 0: 8 x 8 boxes, L and R 2 px aside (IoU 0.6 both); every label is small, D1 (L's box) is small."""
    labels = filler(MAX_LABELS, cls=1)
    L, R = label_px(1, 98, 100, 106, 108, 512), label_px(1, 102, 100, 110, 108, 512)
    labels[i], labels[j] = (L, R) if low == "L" else (R, L)
    dets = records([(100, 100, 108, 108, 0.9, 1), (98, 100, 106, 108, 0.8, 1)])
    return f"smalltie_{i}_{j}_{low}", dets, labels, square(512), params()


FOUR_LAYOUTS = {"lane": (7, 71, 135, 199), "lanes": (60, 65, 130, 195)}     # one lane's four slots | lanes 60, 1, 2, 3
FOUR_SHIFTS = ((-4, 0), (4, 0), (0, -4), (0, 4))                            # left, right, up, down
FOUR_PERMS = tuple(itertools.permutations(range(4)))


def four_indices(layout, group):
    """The four label indices of group 0, 1, 2: the layout's, one lane further per group."""
    return tuple(g + group for g in FOUR_LAYOUTS[layout])


def four_way_case(layout, perm):
    """A 20 x 20 record ties between four labels shifted 4 px left, right, up, down (IoU 2/3 each); direction perm[k] sits at
    the layout's k-th index. Three groups of such labels (classes 1, 2, 3, the same boxes, neighbouring lanes): group c gets
    the tying record c times, then four probes, one on each direction's own box. A probe matches at every threshold if its
    label is still free and only from 0.70 on if a tying record has consumed it: the probes of the three groups name the first,
    the first two and the first three labels consumed, that is the whole order."""
    labels = filler(MAX_LABELS)
    box = lambda d: (200 + FOUR_SHIFTS[d][0], 200 + FOUR_SHIFTS[d][1], 220 + FOUR_SHIFTS[d][0], 220 + FOUR_SHIFTS[d][1])   # noqa: E731
    rows = []
    for group in range(3):
        cls = group + 1
        for k, g in enumerate(four_indices(layout, group)):
            labels[g] = label_px(cls, *box(perm[k]), 512)
        rows += [(200, 200, 220, 220, 0.9 - 0.01 * t, cls) for t in range(group + 1)]
        rows += [(*box(d), 0.5 - 0.01 * d, cls) for d in range(4)]
    return f"four_{layout}_{''.join(map(str, perm))}", records(rows), labels, square(512), params()


# ---- 2. the precision seams of box_iou_xyxy --------------------------------------------------------------------------
def kernel_iou(a, b, width64=False, height64=False, product64=False, strict=False):
    """csrc/evalmatch.hip box_iou_xyxy, line for line: a = four np.float32 (the record), b = four np.float64 (the label).
    The switches are the wrong variants the seam cases must tell apart: an x side always the double difference, a y side
    likewise, the intersection always the double product, an equal edge taken from the label."""
    a = [F(v) for v in a]
    b = [np.float64(v) for v in b]
    d = np.float64
    if strict:
        fx1, fy1, fx2, fy2 = b[0] < d(a[0]), b[1] < d(a[1]), b[2] > d(a[2]), b[3] > d(a[3])
    else:
        fx1, fy1, fx2, fy2 = not b[0] > d(a[0]), not b[1] > d(a[1]), not b[2] < d(a[2]), not b[3] < d(a[3])
    x1, y1, x2, y2 = d(a[0]) if fx1 else b[0], d(a[1]) if fy1 else b[1], d(a[2]) if fx2 else b[2], d(a[3]) if fy2 else b[3]
    if x2 <= x1 or y2 <= y1:
        return np.float64(0.0)
    fw, fh = fx1 and fx2, fy1 and fy2
    wf, hf = a[2] - a[0], a[3] - a[1]                                   # fp32
    w = d(wf) if fw and not width64 else x2 - x1
    h = d(hf) if fh and not height64 else y2 - y1
    inter = d(wf * hf) if fw and fh and not product64 else w * h
    area_a = (a[2] - a[0]) * (a[3] - a[1])                              # fp32
    union = d(area_a) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / union if union > 0 else np.float64(0.0)


def edge_flags(a, b):
    """(left, top, right, bottom) taken from the record."""
    return (not b[0] > a[0], not b[1] > a[1], not b[2] < a[2], not b[3] < a[3])


COMBOS = tuple(itertools.product((True, False), repeat=4))       # (left, top, right, bottom) from the record
SEAM_PAIRS = 8


def seam_boxes(rng, combo, scale=1.0):
    """One record (float64 targets, to be rounded to fp32 by the caller) and one label in the same pixels: the label's edge
    0.5 .. 3 px outside the record's where the combination takes the record's edge, inside where it takes the label's."""
    a = np.concatenate([rng.uniform(1, 8, 2), rng.uniform(300, 600, 2)]) * scale
    off = rng.uniform(0.5, 3.0, 4) * scale
    sign = np.array([-1, -1, 1, 1]) * np.where(combo, 1, -1)
    return a, a + sign * off


def seam_case(ci):
    """SEAM_PAIRS record / label pairs of combination COMBOS[ci], one class each, at imgsz 640 and scale 1."""
    rng = np.random.RandomState(4000 + ci)
    rows, labels = [], []
    conf = rng.permutation(SEAM_PAIRS)
    for k in range(SEAM_PAIRS):
        a, b = seam_boxes(rng, COMBOS[ci])
        rows.append((*a, (conf[k] + 1) / 16.0, k))
        labels.append(label_px(k, *b, 640))
    name = "seam_" + "".join("r" if f else "l" for f in COMBOS[ci])
    return name, records(rows), np.array(labels, dtype=np.float64), square(640), params(imgsz=640, num_classes=SEAM_PAIRS)


EQUAL_EDGES = ("left", "top", "right", "bottom", "all")
EQUAL_PAIRS = 6


def equal_edge_case(which):
    """Label edges bit-equal to the record's fp32 edges (imgsz 512: the label normalises and comes back exactly). One edge:
    the opposite edge of that axis lies outside the record (taken from the record, so the equal edge decides whether the side
    is the fp32 difference), the other axis inside (taken from the label). All four: the fp32 product."""
    rng = np.random.RandomState(4100 + EQUAL_EDGES.index(which))
    rows, labels = [], []
    for k in range(EQUAL_PAIRS):
        a = np.concatenate([rng.uniform(1, 8, 2), rng.uniform(300, 500, 2)]).astype(F)
        off = rng.randint(4, 25, 4) / 8.0
        a64 = a.astype(np.float64)
        if which == "all":
            b = a64.copy()
        else:
            e = EQUAL_EDGES.index(which)
            x_axis = e in (0, 2)
            outside = a64 + np.array([-1, -1, 1, 1]) * off
            inside = a64 - np.array([-1, -1, 1, 1]) * off
            b = np.where([x_axis, not x_axis, x_axis, not x_axis], outside, inside)
            b[e] = a64[e]
        rows.append((*a, (k + 1) / 8.0, k))
        labels.append(label_px(k, *b, 512))
    return f"equal_{which}", records(rows), np.array(labels, dtype=np.float64), square(512), params(num_classes=EQUAL_PAIRS)


SCALED_NETS = ((640, 384), (416, 360))
SCALED_IMGSZ = (640, 512, 1280)
SCALED_CAMERAS = ((1920, 1080), (333, 250))
SCALED_SMALL = 6


def scaled_case(net, imgsz, cam):
    """Two pairs of every combination through cx, cy != 1 (and sx, sy inexact in fp32): the records are given in network
    pixels, the labels sit around what evaluate()'s fp32 scale makes of them. Classes 0..31, one per pair. Six small
    label / record pairs (classes 40..45) drive wave 0 through sx, sy."""
    nw, nh = net
    rng = np.random.RandomState(4200 + nw + imgsz + cam[0])
    dets = np.zeros(32 + SCALED_SMALL, dtype=det_dtype())
    labels = np.zeros((32 + SCALED_SMALL, 5))
    conf = rng.permutation(32 + SCALED_SMALL)
    for k in range(32):
        a, _ = seam_boxes(rng, COMBOS[k % 16], imgsz / 640)
        dets[k] = (a[0] / (imgsz / nw), a[1] / (imgsz / nh), a[2] / (imgsz / nw), a[3] / (imgsz / nh), (conf[k] + 1) / 64.0, k, 1, 0)
    for k in range(32, 32 + SCALED_SMALL):
        w, h = rng.uniform(6, 13, 2) / imgsz
        xc, yc = rng.uniform(0.1, 0.9, 2)
        labels[k] = (8 + k, xc, yc, w, h)
        j = rng.uniform(-0.03, 0.03, 4) * np.array([w, h, w, h])
        box = ((xc - w / 2 + j[0]) * nw, (yc - h / 2 + j[1]) * nh, (xc + w / 2 + j[2]) * nw, (yc + h / 2 + j[3]) * nh)
        dets[k] = (*box, (conf[k] + 1) / 64.0, 8 + k, 1, 0)
    geom = np.array([cam[0], cam[1], nw, nh])
    c = scaled_records(dets, geom, imgsz)                   # what the kernel's fp32 scale gives: the labels go around THAT
    rng2 = np.random.RandomState(4300 + nw + imgsz + cam[0])
    for k in range(32):
        a = np.array([c["x1"][k], c["y1"][k], c["x2"][k], c["y2"][k]], dtype=np.float64)
        off = rng2.uniform(0.5, 3.0, 4) * imgsz / 640
        b = a + np.array([-1, -1, 1, 1]) * np.where(COMBOS[k % 16], 1, -1) * off
        labels[k] = label_px(k, *b, imgsz)
    name = f"scaled_{nw}x{nh}_{imgsz}_{cam[0]}x{cam[1]}"
    return name, dets, labels, geom, params(imgsz=imgsz, num_classes=64)


def below(fn, target, tries):
    """The first of `tries` whose fn() value is np.nextafter(target, 0) exactly."""
    want = np.nextafter(np.float64(target), 0.0)
    for t in tries:
        if fn(t) == want:
            return t
    raise AssertionError(f"no companion one ulp below {target}")


def threshold_case():
    """IoU exactly 0.5 (8 x 16 in 16 x 16) and exactly 0.75 (12 x 16 in 16 x 16), and for each a companion ONE ulp below: the
    same record at the origin, its label 2^-49 px higher (0.5: the bottom edge and the height come from the label) or 2^-48 px
    wider (0.75: all four edges from the record, the label's area a hair over 256). Near pixel 0 a label edge resolves such
    steps. Masks 0x001, 0x000, 0x03f, 0x01f in class order."""
    rows = [(64, 128, 72, 144, 0.9, 0), (0, 0, 8, 16, 0.8, 1), (64, 256, 76, 272, 0.7, 2), (0, 0, 12, 16, 0.6, 3)]
    labels = [label_px(0, 60, 128, 76, 144, 512), [1, 16 / 1024, 8 / 512 - 2.0 ** -58, 16 / 512, 16 / 512],
              label_px(2, 62, 256, 78, 272, 512), [3, 16 / 1024 - 2.0 ** -58, 8 / 512, 16 / 512 + 2.0 ** -57, 16 / 512]]
    return "iou_thresholds", records(rows), np.array(labels, dtype=np.float64), square(512), params()


THRESHOLD_MASKS = [0x001, 0x000, 0x03f, 0x01f]


def centre_iou(rec, label, width=512, height=512):
    """SmallObjectMetric._iou of one record against one label row, through detections_to_coco and coco_to_metric_rows."""
    from unina_yolo_dla_amd import metrics
    row = metrics.coco_to_metric_rows(metrics.detections_to_coco(records([(*rec, 0.5, 0)]), "x"), width, height)[0]
    return metrics.SmallObjectMetric._iou(row[:4], np.asarray(label, dtype=np.float64)[1:5])


def small_threshold_case(thr):
    """Wave 0 at iou_threshold 0.3 (3 x 8 in 10 x 8) or 0.75 (6 x 8 in 8 x 8): class 0 meets the threshold exactly (TP),
    class 1 misses it by the last bits (a small prediction: FP, and its label FN). (tp, fp, fn) = (1, 1, 1)."""
    rw, lw = {0.3: (3, 10), 0.75: (6, 8)}[thr]
    rec1 = (64, 0, 64 + rw, 8)
    lab1 = below(lambda lab: centre_iou(rec1, lab), thr,
                 [[1, (64 + 64 + lw) / 2 / 512, 8 / 1024 - m * 2.0 ** -e, lw / 512, 8 / 512 + m * 2.0 ** -(e - 1)]
                  for e in (60, 59, 58, 61) for m in range(1, 9)])
    rows = [(64, 128, 64 + rw, 136, 0.9, 0), (*rec1, 0.8, 1)]
    labels = [label_px(0, 64, 128, 64 + lw, 136, 512), lab1]
    return f"small_threshold_{thr}", records(rows), np.array(labels, dtype=np.float64), square(512), params(iou_threshold=thr)


def size_threshold_case(t):
    """size_threshold t (15 or 8) at imgsz 512. Labels: t x 5 (a side of exactly t pixels: NOT small) and (t - 1/8) x 5
    (small), each with a record on its box, and a small label nobody predicts. Predictions of class 3, which has no label:
    t x 5 (not small: no FP) and (t - 1/8) x 5 (FP). (tp, fp, fn) = (1, 1, 1)."""
    e = t - 0.125
    labels = [label_px(0, 64, 64, 64 + t, 69, 512), label_px(1, 64, 128, 64 + e, 133, 512), label_px(2, 64, 192, 68, 196, 512)]
    rows = [(64, 64, 64 + t, 69, 0.9, 0), (64, 128, 64 + e, 133, 0.8, 1), (64, 256, 64 + t, 261, 0.7, 3), (64, 320, 64 + e, 325, 0.6, 3)]
    return f"size_threshold_{t}", records(rows), np.array(labels, dtype=np.float64), square(512), params(size_threshold=float(t))


# ---- 3. the order of the records -------------------------------------------------------------------------------------
RECORD_COUNTS = (1, 63, 64, 65, 703, 704, 705, 1023, 1024)
COUNT_LABELS = 40


def count_case(n):
    """n off-grid records against 40 labels. The record at the LAST index sits on label 0 with the highest confidence, the
    one at index n // 2 on label 1 with the lowest: a match in the last 64 indices and one in the last 64 ranks."""
    dets, labels = random_image(5000 + n, n, COUNT_LABELS)
    dets[n // 2] = exact_copy(labels, 1, 640, 2.0 ** -21)
    dets[n - 1] = exact_copy(labels, 0, 640, 1.0)
    return f"count_{n}", dets, labels, square(640), params(imgsz=640)


def equal_confidence_case():
    """All 1024 confidences equal: the order is the index order."""
    dets, labels = random_image(5100, MAXD, COUNT_LABELS)
    dets["confidence"] = F(0.5)
    return "conf_equal_1024", dets, labels, square(640), params(imgsz=640)


def _order_image(seed, n=192, m=24):
    return random_image(seed, n, m, classes=2)


def plant_order_witness(dets, labels, first, second, cls):
    """A 20 x 20 label of its own class `cls` and two records on it: `first` 5 px aside (IoU 0.6), `second` 1 px aside (IoU
    0.905); their confidences stay. Matched in this order, `first` takes the label up to 0.60 and `second` from 0.65 to 0.90;
    the other way round `second` takes it up to 0.90 and `first` finds nothing. Returns the labels with the new row."""
    x, y = 20.3 + 40 * (cls % 8), 600.7
    dets[first] = (x + 5, y, x + 25, y + 20, dets["confidence"][first], cls, 1, 0)
    dets[second] = (x + 1, y, x + 21, y + 20, dets["confidence"][second], cls, 1, 0)
    return np.concatenate([labels, [label_px(cls, x, y, x + 20, y + 20, 640)]])


def nan_confidence_case():
    """NaN confidences at the first, a middle and the last index and at every 7th, ties (0.5, 0.25) at every 3rd / 5th.
    Witness pairs: two NaNs (indices 0, 191), two tied at 0.5 (3, 6), the lowest finite one against a NaN (1, 96)."""
    dets, labels = _order_image(5200)
    n = len(dets)
    dets["confidence"][::3] = F(0.5)
    dets["confidence"][::5] = F(0.25)
    dets["confidence"][::7] = np.nan
    dets["confidence"][[0, n // 2, n - 1]] = np.nan
    dets["confidence"][1] = F(2.0 ** -22)
    for k, (first, second) in enumerate(((0, n - 1), (3, 6), (1, n // 2))):
        labels = plant_order_witness(dets, labels, first, second, 10 + k)
    return "conf_nan", dets, labels, square(640), params(imgsz=640, num_classes=16)


def inf_confidence_case():
    """+inf and -inf confidences (several of each: ties), NaN behind them, finite ones between. Witness pairs: two NaNs
    (2, 11), two +inf (0, 4), two -inf (1, 7), -inf against NaN (13, 29)."""
    dets, labels = _order_image(5300)
    dets["confidence"][::4] = np.inf
    dets["confidence"][1::6] = -np.inf
    dets["confidence"][2::9] = np.nan
    for k, (first, second) in enumerate(((2, 11), (0, 4), (1, 7), (13, 29))):
        labels = plant_order_witness(dets, labels, first, second, 10 + k)
    return "conf_inf", dets, labels, square(640), params(imgsz=640, num_classes=16)


def zero_sign_case():
    """-0.0 against +0.0: equal keys, kept by index. Even indices -0.0, odd ones +0.0, some at +-2^-149 around them. Witness
    pairs: (2, 3) -0.0 in front of +0.0, (7, 8) +0.0 in front of -0.0."""
    dets, labels = _order_image(5400)
    n = len(dets)
    dets["confidence"] = np.where(np.arange(n) % 2 == 0, F(-0.0), F(0.0))
    dets["confidence"][::11] = F(2.0 ** -149)
    dets["confidence"][5::11] = F(-2.0 ** -149)
    for k, (first, second) in enumerate(((2, 3), (7, 8))):
        labels = plant_order_witness(dets, labels, first, second, 10 + k)
    return "conf_zero_sign", dets, labels, square(640), params(imgsz=640, num_classes=16)


def matching_order(conf):
    """np.argsort(-confidence, kind="stable"), as every host metric orders the records."""
    return np.argsort(-np.asarray(conf), kind="stable")


def masks_in_order(dets, labels, imgsz, order):
    """tp_mask per ORIGINAL record index when the records are matched in `order`: the host rows of the records re-ranked by
    distinct surrogate confidences."""
    from unina_yolo_dla_amd import metrics
    d = dets[order].copy()
    d["confidence"] = np.linspace(1.0, 0.5, len(d)).astype(F)
    assert len(np.unique(d["confidence"])) == len(d)
    out = np.zeros(len(dets), dtype=np.uint32)
    out[order] = metrics.ap_rows_numpy(d, labels, imgsz)["tp_mask"]
    return out


def other_orders(conf):
    """Plausible wrong orders of the same records: plain index order, ties in descending index order, one zero sign in front
    of the other, NaN first, NaN in descending index order."""
    conf = np.asarray(conf)
    n = len(conf)
    right = matching_order(conf)
    nan = np.isnan(conf)
    out = {"index": np.arange(n), "ties_reversed": np.lexsort((-np.arange(n), np.where(nan, np.inf, -conf)))}
    zero = conf == 0
    if (np.signbit(conf) & zero).any() and (~np.signbit(conf) & zero).any():
        out["plus_zero_first"] = np.lexsort((np.arange(n), np.signbit(conf) & zero, -conf))
        out["minus_zero_first"] = np.lexsort((np.arange(n), ~np.signbit(conf) & zero, -conf))
    if nan.any():
        out["nan_first"] = np.concatenate([right[nan[right]], right[~nan[right]]])
        out["nan_reversed"] = np.concatenate([right[~nan[right]], right[nan[right]][::-1]])
    return out


def count_word_case(word):
    """A count word outside [0, 1024]: 5000 reads the 1024 records there are, -3 reads none."""
    n = MAXD if word > 0 else 30
    dets, labels = random_image(5500 + n, n, COUNT_LABELS)
    dets[n - 1] = exact_copy(labels, 0, 640, 1.0)
    return f"count_word_{word}", dets, labels, square(640), params(imgsz=640, count=word)


# ---- 4. flags / 6. capacity: one image set -------------------------------------------------------------------------
def flag_image(which):
    seed, n, m = {"A": (6000, 130, 50), "B": (6001, 90, 70)}[which]
    dets, labels = random_image(seed, n, m)
    return f"flags_{which}", dets, labels, square(640), params(imgsz=640)


# ---- 5. classes and degenerate input ---------------------------------------------------------------------------------
def _pairs(classes, imgsz=512):
    """One 20 x 20 label per entry of `classes` (the label's class as given, maybe fractional) and a record 1 px aside of
    class int(c): IoU 19 / 21."""
    labels = [label_px(c, 40 * k + 8, 40, 40 * k + 28, 60, imgsz) for k, c in enumerate(classes)]
    rows = [(40 * k + 9, 40, 40 * k + 29, 60, 0.9 - 0.01 * k, int(c)) for k, c in enumerate(classes)]
    return rows, labels


def class_case(which):
    """num_classes 1 / 256 / 4 with label classes on, beside and outside [0, num_classes): 1.9 truncates to 1, 256, 7 and -3
    match records of their own id and are not counted."""
    nc, classes = {"nc1": (1, (0, 0, 1.9, 7, -3)), "nc256": (256, (0, 255, 255, 256, -3, 1.9, 254.5)),
                   "nc4": (4, (3, 7, -3, 1.9, 4, 0.5))}[which]
    rows, labels = _pairs(classes)
    labels += [label_px(c, 40 * k + 8, 100, 40 * k + 12, 104, 512) for k, c in enumerate(classes)]      # small, nobody's
    return f"classes_{which}", records(rows), np.array(labels, dtype=np.float64), square(512), params(num_classes=nc)


DEGENERATE_CONF = 0.5          # confidence of every degenerate record; ordinary ones lie above


def degenerate_case():
    """Ordinary pairs (class 0, some small) among records and labels that are no boxes: NaN / +inf in one coordinate, -inf..inf
    in both axes, inverted and zero-width records; zero-width, negative-width and NaN-centred labels, each with an ordinary
    record on the place where it would be. All class 0, so everything meets everything."""
    nan, inf = np.nan, np.inf
    rows, labels = _pairs((0, 0, 0))
    labels += [label_px(0, 40 * k + 8, 100, 40 * k + 18, 110, 512) for k in range(3)]                # small
    rows += [(40 * k + 9, 100, 40 * k + 19, 110, 0.8 - 0.01 * k, 0) for k in range(3)]
    bad = [(nan, 40, 28, 60), (8, 40, 28, nan), (8, 40, inf, 60), (8, inf, 28, 60), (-inf, -inf, inf, inf), (-inf, 40, inf, 60),
           (28, 40, 8, 60), (8, 60, 28, 40), (28, 60, 8, 40), (18, 100, 8, 110), (8, 40, 8, 60), (8, 100, 18, 100), (48, 50, 48, 50)]
    rows += [(*b, DEGENERATE_CONF, 0) for b in bad]
    labels += [[0, 0.5, 0.5, 0.0, 20 / 512], [0, 0.5, 0.6, 10 / 512, 0.0], [0, 0.6, 0.5, -20 / 512, 20 / 512],
               [0, 0.6, 0.6, -10 / 512, -10 / 512], [0, nan, 0.7, 10 / 512, 10 / 512], [0, 0.7, nan, 20 / 512, 20 / 512],
               [0, 0.7, 0.7, nan, 10 / 512], [0, 0.8, 0.8, inf, 10 / 512]]
    rows += [(246, 246, 266, 266, 0.45, 0), (297, 246, 317, 266, 0.44, 0), (302, 302, 312, 312, 0.43, 0), (353, 353, 363, 363, 0.42, 0)]
    return "degenerate", records(rows), np.array(labels, dtype=np.float64), square(512), params()


# ---- 7. the dense worst case -----------------------------------------------------------------------------------------
def dense_case():
    """1024 records against 256 labels of one class on a 16 x 16 grid of 40-pixel cells, labels 9..14 px (all small), four
    jittered records per label: every lane slot holds a candidate and is consumed."""
    rng = np.random.RandomState(7000)
    gx, gy = np.meshgrid(np.arange(16), np.arange(16))
    w, h = rng.uniform(9, 14, MAX_LABELS), rng.uniform(9, 14, MAX_LABELS)
    x1, y1 = gx.reshape(-1) * 40 + rng.uniform(4, 20, MAX_LABELS), gy.reshape(-1) * 40 + rng.uniform(4, 20, MAX_LABELS)
    labels = np.stack([np.zeros(MAX_LABELS), (x1 + w / 2) / 640, (y1 + h / 2) / 640, w / 640, h / 640], axis=1)
    dets = np.zeros(MAXD, dtype=det_dtype())
    conf = rng.permutation(np.arange(1, 1 << 20))[:MAXD] / float(1 << 20)
    owner = rng.permutation(np.repeat(np.arange(MAX_LABELS), MAXD // MAX_LABELS))
    for i, g in enumerate(owner):
        j = rng.uniform(-1.2, 1.2, 4)
        dets[i] = (x1[g] + j[0], y1[g] + j[1], x1[g] + w[g] + j[2], y1[g] + h[g] + j[3], conf[i], 0, 1, 0)
    return "dense", dets, labels, square(640), params(imgsz=640)


# ---- the registry ----------------------------------------------------------------------------------------------------
def _builders():
    b = {}
    for i, j in TIE_PAIRS:
        for low in "LR":
            b[f"tie_{i}_{j}_{low}"] = functools.partial(tie_case, i, j, low)
            b[f"smalltie_{i}_{j}_{low}"] = functools.partial(small_tie_case, i, j, low)
    for layout in FOUR_LAYOUTS:
        for perm in FOUR_PERMS:
            b[f"four_{layout}_{''.join(map(str, perm))}"] = functools.partial(four_way_case, layout, perm)
    for ci in range(16):
        b["seam_" + "".join("r" if f else "l" for f in COMBOS[ci])] = functools.partial(seam_case, ci)
    for which in EQUAL_EDGES:
        b[f"equal_{which}"] = functools.partial(equal_edge_case, which)
    for net in SCALED_NETS:
        for imgsz in SCALED_IMGSZ:
            for cam in SCALED_CAMERAS:
                b[f"scaled_{net[0]}x{net[1]}_{imgsz}_{cam[0]}x{cam[1]}"] = functools.partial(scaled_case, net, imgsz, cam)
    b["iou_thresholds"] = threshold_case
    for thr in (0.3, 0.75):
        b[f"small_threshold_{thr}"] = functools.partial(small_threshold_case, thr)
    for t in (15, 8):
        b[f"size_threshold_{t}"] = functools.partial(size_threshold_case, t)
    for n in RECORD_COUNTS:
        b[f"count_{n}"] = functools.partial(count_case, n)
    b["conf_equal_1024"], b["conf_nan"] = equal_confidence_case, nan_confidence_case
    b["conf_inf"], b["conf_zero_sign"] = inf_confidence_case, zero_sign_case
    for word in (5000, -3):
        b[f"count_word_{word}"] = functools.partial(count_word_case, word)
    for which in "AB":
        b[f"flags_{which}"] = functools.partial(flag_image, which)
    for which in ("nc1", "nc256", "nc4"):
        b[f"classes_{which}"] = functools.partial(class_case, which)
    b["degenerate"] = degenerate_case
    b["dense"] = dense_case
    return b


BUILDERS = _builders()
FAMILIES = ("tie_", "smalltie_", "four_", "seam_", "equal_", "scaled_", "iou_thresholds", "small_threshold_", "size_threshold_", "count_",
            "conf_", "flags_", "classes_", "degenerate", "dense")


def names(prefix=""):
    return [n for n in BUILDERS if n.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(name, dets, labels, geom, params), built once per process; callers leave the arrays unchanged."""
    c = BUILDERS[name]()
    assert c[0] == name, (c[0], name)
    c[1].setflags(write=False)
    c[2].setflags(write=False)
    return c
