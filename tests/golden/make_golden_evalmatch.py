#!/usr/bin/env python3
"""Generates tests/golden/evalmatch_seed1234.npz by running the REFERENCE's SmallObjectMetric in the dev container.

    python tests/golden/make_golden_evalmatch.py        (needs /root/reference; never runs on the GPU box)

What is pinned, and by what (all data, no code): per image, engine-shaped detection records (fp32 xyxy in network pixels on a
1/8-pixel grid, distinct confidences -- the reference sorts with an unstable argsort), YOLO label rows, the image geometry
(w, h, net_w, net_h), the [N,6] metric rows evaluate() builds from the records (metrics.detections_to_coco /
coco_to_metric_rows after the fp32 rescale), and the tp / fp / fn that data_loader.SmallObjectMetric (size_threshold 15,
image_size 640) adds for that image when fed those rows and labels as float64 tensors.

Images: six hand-built edge cases (below), then seeded random ones with 0..40 detections and 0..70 labels over four classes:
most labels small, a fifth of them near-copies of an earlier label (so detections compete and fall back to second choices),
detections jittered copies of labels (sometimes of another class) or free boxes. A few images have a camera geometry other
than the network's, one of them with scales that are not exact in fp32.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference/unina_yolo_dla")
sys.modules.setdefault("cv2", types.ModuleType("cv2"))   # data_loader.py imports it for image loading only

import numpy as np  # noqa: E402
import torch  # noqa: E402

import data_loader as ref_dl  # noqa: E402  (the reference)
from unina_yolo_dla_amd import metrics  # noqa: E402
from unina_yolo_dla_amd.engine import DET_DTYPE  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NET = 640
N_RANDOM = 36
GEOMS = {7: (1280, 720), 15: (480, 360), 23: (333, 250), 31: (1920, 1080)}   # image index -> camera (w, h); others 640 x 640


def records(boxes):
    """[(x1, y1, x2, y2, conf, cls)] -> engine records."""
    d = np.zeros(len(boxes), dtype=DET_DTYPE)
    for i, b in enumerate(boxes):
        d[i] = (b[0], b[1], b[2], b[3], b[4], int(b[5]), 1, 0)
    return d


def label_rows(boxes):
    """[(cls, x1, y1, x2, y2)] network pixels -> YOLO rows (a stretch keeps normalised coordinates)."""
    return np.array([[c, (x1 + x2) / 2 / NET, (y1 + y2) / 2 / NET, (x2 - x1) / NET, (y2 - y1) / NET] for c, x1, y1, x2, y2 in boxes],
                    dtype=np.float64).reshape(-1, 5)


def edge_cases():
    cases = []
    # 0: no small label (nothing may be counted, not even the small unmatched detection)
    cases.append(("no_small_label", [(10, 10, 18, 19, 0.9, 0), (100, 100, 140, 150, 0.8, 1)], [(1, 100, 100, 140, 150), (0, 300, 300, 315, 330)]))
    # 1: no detection: every small label is a false negative, the large one is not
    cases.append(("no_detection", [], [(0, 10, 10, 20, 20), (1, 50, 50, 58, 62), (2, 90, 90, 99, 97), (3, 200, 200, 214.875, 212), (0, 400, 400, 460, 470)]))
    # 2: two detections compete for one label: the more confident one takes it although the other overlaps better
    cases.append(("two_for_one", [(100, 100, 110, 108, 0.9, 2), (100, 100, 110, 109.75, 0.8, 2)], [(2, 100, 100, 110, 110)]))
    # 3: the second detection's best label is taken, its second choice still clears 0.5
    cases.append(("best_taken", [(100, 100, 112, 112, 0.9, 1), (100.5, 100, 112.5, 112, 0.8, 1)],
                  [(1, 100, 100, 112, 112), (1, 102, 100, 114, 112)]))
    # 4: a side of exactly 15 px is NOT small (strict <), 14.875 is
    cases.append(("side_15", [(300, 300, 315, 310, 0.7, 0), (340, 300, 354.875, 310, 0.6, 0)], [(0, 300, 300, 315, 310), (0, 340, 300, 354.875, 310)]))
    # 5: IoU exactly 0.5 (a 2 x 1 box against a 1 x 1 box, in units of 5 px so that every normalised value is a dyadic
    #    fraction): >= makes it a true positive
    cases.append(("iou_half", [(160, 320, 170, 325, 0.9, 3)], [(3, 160, 320, 165, 325)]))
    return cases


def random_image(rng):
    m, n = int(rng.randint(0, 71)), int(rng.randint(0, 41))
    q = lambda v: np.round(v * 8) / 8                                     # noqa: E731  the 1/8-pixel grid
    labels = []
    for _ in range(m):
        if labels and rng.rand() < 0.2:                                   # near-copy of an earlier label
            c, x1, y1, x2, y2 = labels[rng.randint(len(labels))]
            dx, dy = q(rng.uniform(-3, 3)), q(rng.uniform(-3, 3))
            labels.append((c, x1 + dx, y1 + dy, x2 + dx, y2 + dy))
            continue
        w, h = (q(rng.uniform(3, 15.5)), q(rng.uniform(3, 15.5))) if rng.rand() < 0.7 else (q(rng.uniform(10, 80)), q(rng.uniform(10, 80)))
        x1, y1 = q(rng.uniform(0, NET - w)), q(rng.uniform(0, NET - h))
        labels.append((int(rng.randint(4)), x1, y1, x1 + w, y1 + h))
    confs = rng.permutation(4096)[:n] / 4096.0 * 0.999 + 0.001           # distinct
    dets = []
    for i in range(n):
        if labels and rng.rand() < 0.65:
            c, x1, y1, x2, y2 = labels[rng.randint(len(labels))]
            j = q(rng.uniform(-2.5, 2.5, 4))
            x1, y1, x2, y2 = x1 + j[0], y1 + j[1], max(x2 + j[2], x1 + j[0] + 0.125), max(y2 + j[3], y1 + j[1] + 0.125)
            if rng.rand() < 0.1:
                c = (c + 1) % 4
        else:
            w, h = q(rng.uniform(2, 40)), q(rng.uniform(2, 40))
            x1, y1 = q(rng.uniform(0, NET - w)), q(rng.uniform(0, NET - h))
            c, x2, y2 = int(rng.randint(4)), x1 + w, y1 + h
        dets.append((x1, y1, x2, y2, confs[i], c))
    return dets, labels


def metric_rows(dets, w, h, nw, nh):
    """evaluate()'s chain: fp32 rescale to the image's pixels, predictions.json records, normalised rows."""
    sx, sy = w / nw, h / nh
    scaled = dets.copy()
    scaled["x1"], scaled["x2"] = dets["x1"] * sx, dets["x2"] * sx
    scaled["y1"], scaled["y2"] = dets["y1"] * sy, dets["y2"] * sy
    return metrics.coco_to_metric_rows(metrics.detections_to_coco(scaled, "x"), w, h)


def main():
    rng = np.random.RandomState(1234)
    images = [(name, records(d), label_rows(l)) for name, d, l in edge_cases()]
    for i in range(N_RANDOM):
        d, l = random_image(rng)
        images.append((f"random{i}", records(d), label_rows(l)))
    ref = ref_dl.SmallObjectMetric(size_threshold=15, iou_threshold=0.5, image_size=NET)
    blob, counts, geoms, names = {}, [], [], []
    prev = np.zeros(3, dtype=np.int64)
    for i, (name, dets, labels) in enumerate(images):
        w, h = GEOMS.get(i, (NET, NET))
        rows = metric_rows(dets, w, h, NET, NET)
        ref.update([torch.from_numpy(rows)], [torch.from_numpy(labels)])
        now = np.array([ref.true_positives, ref.false_positives, ref.false_negatives], dtype=np.int64)
        counts.append(now - prev)
        prev = now
        geoms.append((w, h, NET, NET))
        names.append(name)
        blob[f"dets/{i:02d}"], blob[f"labels/{i:02d}"], blob[f"rows/{i:02d}"] = dets, labels, rows
        assert len(np.unique(dets["confidence"])) == len(dets)
    counts = np.stack(counts)
    by = dict(zip(names, counts.tolist()))
    # the edge cases do what they were built for
    assert by["no_small_label"] == [0, 0, 0] and by["no_detection"] == [0, 0, 4] and by["two_for_one"] == [1, 1, 0], by
    assert by["best_taken"] == [2, 0, 0] and by["side_15"] == [1, 0, 0] and by["iou_half"] == [1, 0, 0], by
    assert counts.sum(axis=0).min() >= 20, counts.sum(axis=0)
    blob["counts"], blob["geom"] = counts, np.array(geoms, dtype=np.int64)
    blob["names"] = np.array(names)
    path = os.path.join(GOLD, "evalmatch_seed1234.npz")
    np.savez_compressed(path, **blob)
    print(f"{len(images)} images, tp/fp/fn {counts.sum(axis=0)}, labels up to {max(len(l) for _, _, l in images)}, "
          f"detections up to {max(len(d) for _, d, _ in images)}; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
