#!/usr/bin/env python3
"""Generates tests/golden/tiled_slices.npz by running the REFERENCE's slicing code in the dev container.

    python tests/golden/make_golden_tiled.py        (needs /root/reference; never runs on the GPU box)

What is pinned, and by what (all data, no code):
  * slices ......... SAHI_Wrapper.get_slices on a zero image of every frame size below: the (x, y) offsets it yields and the
                     shape of every slice, in its order, REPEATS INCLUDED (1920x1080 yields the last row twice). Frame sizes:
                     1920x1200, 1920x1080, 1280x720, 640x640, 500x400 (smaller than a slice), 1936x480 (smaller in one
                     dimension), 641x640, 2448x2048, 4096x2160, 1152x1152, and a non-default slice size
                     (512x384, overlap 0.25 / 0.1), overlap 0 and overlap 0.5.
  * map ............ map_boxes_to_global on a few boxes and offsets (float64, as the reference returns them).
  * union .......... a synthetic multi-tile union: per tile of the 1920x1200 default slicing, seeded records (fp32 boxes in
                     tile pixels, distinct confidences, 4 classes) -- planted so that neighbouring tiles see the same objects
                     in their overlap. Mapped with map_boxes_to_global (in fp32 the offset add is exact here: asserted), then
                     the reference's per-class `nms` loop (:261-271) at 0.45; the kept indices INTO THE UNION are recorded.
                     Asserted: all confidences distinct, every same-class pair's float64 IoU at least 1e-4 away from the
                     threshold, so the reference's float64 IoU without the epsilon and the engine's fp32 IoU with it decide alike.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference/unina_yolo_dla")
sys.modules.setdefault("cv2", types.ModuleType("cv2"))   # auto_labeler.py needs it for the GroundingDINO / SAM wrappers only
try:
    import tqdm  # noqa: F401
except ImportError:
    _t = types.ModuleType("tqdm")
    _t.tqdm = lambda it, *a, **k: it
    sys.modules["tqdm"] = _t

import numpy as np  # noqa: E402

import auto_labeler as ref  # noqa: E402  (the reference)

GOLD = os.path.join(ROOT, "tests", "golden")
DET_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("confidence", "<f4"),
                      ("class_id", "<i4"), ("valid", "<i4"), ("_pad", "<i4")])
MERGE_IOU = 0.45

# (frame h, frame w, slice h, slice w, overlap h, overlap w)
CASES = [
    (1200, 1920, 640, 640, 0.2, 0.2),
    (1080, 1920, 640, 640, 0.2, 0.2),
    (720, 1280, 640, 640, 0.2, 0.2),
    (640, 640, 640, 640, 0.2, 0.2),
    (400, 500, 640, 640, 0.2, 0.2),
    (480, 1936, 640, 640, 0.2, 0.2),
    (640, 641, 640, 640, 0.2, 0.2),
    (2048, 2448, 640, 640, 0.2, 0.2),
    (2160, 4096, 640, 640, 0.2, 0.2),
    (1152, 1152, 640, 640, 0.2, 0.2),
    (1200, 1920, 384, 512, 0.25, 0.1),
    (1200, 1920, 640, 640, 0.0, 0.0),
    (1080, 1920, 640, 640, 0.5, 0.5),
]


def ref_slices(h, w, sh, sw, oh, ow):
    wrap = ref.SAHI_Wrapper(slice_height=sh, slice_width=sw, overlap_height_ratio=oh, overlap_width_ratio=ow)
    img = np.zeros((h, w, 3), dtype=np.uint8)
    rows = [(x, y, s.shape[1], s.shape[0]) for s, (x, y) in wrap.get_slices(img)]
    return np.array(rows, dtype=np.int64).reshape(-1, 4)


def union_case():
    """Objects planted in frame coordinates; every tile that contains one whole reports it with its own jitter and confidence."""
    rng = np.random.RandomState(20260)
    tiles = [tuple(int(v) for v in r) for r in dict.fromkeys(map(tuple, ref_slices(1200, 1920, 640, 640, 0.2, 0.2)))]
    n_obj = 160
    cx, cy = rng.uniform(20, 1900, n_obj), rng.uniform(20, 1180, n_obj)
    bw, bh = rng.uniform(10, 60, n_obj), rng.uniform(12, 70, n_obj)
    cls = rng.randint(0, 4, n_obj)
    confs = rng.permutation(np.linspace(0.31, 0.98, 4096).astype(np.float32))   # distinct fp32 values, handed out in turn
    slots = np.zeros((len(tiles), 1024), dtype=DET_DTYPE)
    counts = np.zeros(len(tiles), dtype=np.int32)
    k = 0
    for t, (x0, y0, tw, th) in enumerate(tiles):
        for o in range(n_obj):
            x1, y1, x2, y2 = cx[o] - bw[o] / 2, cy[o] - bh[o] / 2, cx[o] + bw[o] / 2, cy[o] + bh[o] / 2
            if x1 < x0 or y1 < y0 or x2 > x0 + tw or y2 > y0 + th:
                continue
            j = rng.uniform(-1.5, 1.5, 4)
            # quarter-pixel grid: tile coordinate + integer offset is exact in fp32, the two mappings agree bit for bit
            box = np.round((np.array([x1 - x0, y1 - y0, x2 - x0, y2 - y0]) + j) * 4) / 4
            r = slots[t][counts[t]]
            r["x1"], r["y1"], r["x2"], r["y2"] = box
            r["confidence"], r["class_id"], r["valid"] = confs[k], cls[o], 1
            k += 1
            counts[t] += 1
    # the reference's pipeline on it (auto_label_frame :243-271)
    all_boxes, all_scores, all_cls = [], [], []
    for t, (x0, y0, _tw, _th) in enumerate(tiles):
        r = slots[t][:counts[t]]
        boxes = np.stack([r["x1"], r["y1"], r["x2"], r["y2"]], axis=1)
        g = ref.map_boxes_to_global(boxes, x0, y0)
        assert np.array_equal(g.astype(np.float32).astype(np.float64), g), "the offset add must be exact in fp32"
        all_boxes.append(g)
        all_scores.append(r["confidence"])
        all_cls.append(r["class_id"])
    all_boxes, all_scores, all_cls = np.vstack(all_boxes), np.concatenate(all_scores), np.concatenate(all_cls)
    assert len(np.unique(all_scores)) == len(all_scores), "confidences must be distinct"
    kept = []
    for c in np.unique(all_cls):
        idx = np.where(all_cls == c)[0]
        keep = ref.nms(all_boxes[idx], all_scores[idx], iou_threshold=MERGE_IOU)
        kept.extend(int(idx[i]) for i in keep)
        # decision margin of every same-class pair (float64, no epsilon: the reference's expression)
        b = all_boxes[idx]
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        iw = np.maximum(0.0, np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]))
        ih = np.maximum(0.0, np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]))
        inter = iw * ih
        iou = inter / (area[:, None] + area[None, :] - inter)
        np.fill_diagonal(iou, 0.0)
        assert np.abs(iou - MERGE_IOU).min() >= 1e-4, "a pair sits on the threshold: choose another seed"
    kept = np.array(sorted(kept, key=lambda i: -all_scores[i]), dtype=np.int64)
    assert 0 < len(kept) < len(all_scores)
    print(f"union: {len(tiles)} tiles, counts {counts.tolist()}, {len(all_scores)} records, {len(kept)} kept")
    return np.array(tiles, dtype=np.int64), slots[:, :int(counts.max())].copy(), counts, kept


def main():
    blob = {"cases": np.array(CASES, dtype=np.float64)}
    for i, c in enumerate(CASES):
        h, w, sh, sw, oh, ow = c
        rows = ref_slices(int(h), int(w), int(sh), int(sw), oh, ow)
        blob[f"slices/{i}"] = rows
        uniq = len(dict.fromkeys(map(tuple, rows)))
        print(f"{int(w)}x{int(h)} slice {int(sw)}x{int(sh)} overlap {ow}/{oh}: {len(rows)} slices, {uniq} distinct")
    boxes = np.array([[0.0, 0.0, 10.0, 12.0], [3.25, 7.5, 100.125, 220.0], [639.0, 1.0, 640.0, 2.0]], dtype=np.float32)
    offs = np.array([[0, 0], [512, 0], [1280, 560], [7, 13]], dtype=np.int64)
    blob["map/boxes"], blob["map/offsets"] = boxes, offs
    blob["map/global"] = np.stack([ref.map_boxes_to_global(boxes, int(x), int(y)) for x, y in offs])
    assert blob["map/global"].dtype == np.float64
    empty = np.zeros((0, 4), dtype=np.float32)
    assert ref.map_boxes_to_global(empty, 3, 4) is empty
    tiles, slots, counts, kept = union_case()
    blob["union/tiles"], blob["union/slots"], blob["union/counts"], blob["union/kept"] = tiles, slots.view(np.uint8), counts, kept
    blob["union/merge_iou"] = np.array(MERGE_IOU)
    path = os.path.join(GOLD, "tiled_slices.npz")
    np.savez_compressed(path, **blob)
    print("done", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
