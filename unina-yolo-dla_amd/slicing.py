"""Sliced inference on the host side: the reference's slicing helpers (auto_labeler.py) and a numpy twin of the GPU merge.

Same names as the reference where it has one:

  get_slices ............. SAHI_Wrapper.get_slices          auto_labeler.py:132-154   (tiles instead of image views)
  map_boxes_to_global .... map_boxes_to_global              auto_labeler.py:158-165
  merge_numpy ............ the global per-class NMS         auto_labeler.py:167-199, 255-271, with the ENGINE's semantics

``get_slices`` returns what ``unina_slice_tiles`` (include/unina_mi355.h) returns: the reference's sequence with exact repeats
dropped. The reference yields the last row / column of slices twice where the stride does not divide the frame (h = 1080,
slice 640, stride 512: y = 0, 440, 440); the engine's NMS never lets equal confidences suppress each other (SURVEY.md
App. D), so a repeated tile would double every one of its detections.

``merge_numpy`` is the fp32 twin of ``unina_merge_tiles_async`` (csrc/postprocess.hip: tile_gather_kernel + post_nms_kernel): map,
stable sort by confidence (ties: tile-major enumeration order), keep the 1024 best, sequential greedy class-aware NMS at
IoU > merge_iou with the +1e-6f denominator, only a strictly lower confidence is suppressed. It runs without a GPU; the CPU
tests pin it to the reference's recorded results and, byte for byte, to the oracle's uo_sort_nms.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

MAX_DETECTIONS = 1024
MAX_TILES = 64
DET_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("confidence", "<f4"),
                      ("class_id", "<i4"), ("valid", "<i4"), ("_pad", "<i4")])

Tile = Tuple[int, int, int, int]   # x, y, w, h: a region of the camera frame, pixels


def get_slices(h: int, w: int, slice_h: int = 640, slice_w: int = 640, overlap_h: float = 0.2, overlap_w: float = 0.2,
               raw: bool = False) -> List[Tile]:
    """The tiles (x, y, w, h) of an h x w frame, in the reference's order. ``raw=True``: the reference's own sequence,
    repeats included; otherwise exact repeats are dropped (first occurrence kept), as unina_slice_tiles does."""
    if min(h, w, slice_h, slice_w) <= 0:
        raise ValueError("frame and slice sizes must be positive")
    if h <= slice_h and w <= slice_w:                       # "Handle small images" (:139-141): the whole frame
        return [(0, 0, w, h)]
    stride_h = int(slice_h * (1 - overlap_h))
    stride_w = int(slice_w * (1 - overlap_w))
    if stride_h < 1 or stride_w < 1:
        raise ValueError("overlap leaves no stride")
    seq = []
    for y in range(0, h, stride_h):
        for x in range(0, w, stride_w):
            y_end = min(y + slice_h, h)
            x_end = min(x + slice_w, w)
            y_start = max(0, y_end - slice_h)
            x_start = max(0, x_end - slice_w)
            seq.append((x_start, y_start, x_end - x_start, y_end - y_start))
    return seq if raw else list(dict.fromkeys(seq))


def map_boxes_to_global(boxes: np.ndarray, x_offset: int, y_offset: int) -> np.ndarray:
    """Boxes [N, 4] (xyxy) from slice coordinates to frame coordinates (float64, like the reference)."""
    if len(boxes) == 0:
        return boxes
    out = np.array(boxes, dtype=float)
    out[:, [0, 2]] += x_offset
    out[:, [1, 3]] += y_offset
    return out


def map_records(slots: np.ndarray, counts: Sequence[int], tiles: Sequence[Tile], net_w: int = 640, net_h: int = 640) -> np.ndarray:
    """The union of the tiles' records in frame pixels, in enumeration order (tile-major), as the gather kernel maps them:
    X = x * (w / net_w) + x0 in fp32, the product and the sum rounded separately."""
    slots = np.asarray(slots)
    assert slots.dtype == DET_DTYPE and len(slots) >= len(tiles) and len(counts) >= len(tiles)
    parts = []
    for t, (x0, y0, tw, th) in enumerate(tiles):
        n = min(max(int(counts[t]), 0), MAX_DETECTIONS)
        r = np.array(slots[t][:n], dtype=DET_DTYPE)
        sx, sy = np.float32(tw) / np.float32(net_w), np.float32(th) / np.float32(net_h)
        for k, s, o in (("x1", sx, x0), ("y1", sy, y0), ("x2", sx, x0), ("y2", sy, y0)):
            r[k] = (r[k] * s).astype(np.float32) + np.float32(o)
        parts.append(r)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=DET_DTYPE)


def sort_nms_numpy(dets: np.ndarray, iou_thr: float, max_det: int = MAX_DETECTIONS) -> np.ndarray:
    """The engine's sort + cap + greedy NMS (oracle/postprocess_oracle.c uo_sort_nms with uo_semantics_engine) on records in
    enumeration order; fp32 throughout."""
    dets = np.asarray(dets)
    order = np.argsort(-dets["confidence"].astype(np.float64), kind="stable")[:max_det]   # (exact: float64 holds every fp32)
    d = dets[order]
    n = len(d)
    x1, y1, x2, y2 = d["x1"], d["y1"], d["x2"], d["y2"]
    area = (x2 - x1) * (y2 - y1)
    conf, cls = d["confidence"], d["class_id"]
    thr, eps = np.float32(iou_thr), np.float32(1e-6)
    sup = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if sup[i]:
            continue
        keep.append(i)
        j = slice(i + 1, n)
        ix1, iy1 = np.maximum(x1[i], x1[j]), np.maximum(y1[i], y1[j])
        ix2, iy2 = np.minimum(x2[i], x2[j]), np.minimum(y2[i], y2[j])
        hit = ~((ix1 >= ix2) | (iy1 >= iy2))
        inter = (ix2 - ix1) * (iy2 - iy1)
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = inter / (area[i] + area[j] - inter + eps)
        sup[j] |= hit & (cls[j] == cls[i]) & (conf[i] > conf[j]) & (iou > thr)
    out = d[keep].copy()
    out["valid"] = 1
    out["_pad"] = 0
    return out


def merge_numpy(slots: np.ndarray, counts: Sequence[int], tiles: Sequence[Tile], merge_iou: float = 0.45,
                net_w: int = 640, net_h: int = 640) -> np.ndarray:
    """unina_merge_tiles_async on the host: slots [T, MAX_DETECTIONS] (DET_DTYPE), counts [T], tiles [(x, y, w, h)] ->
    the merged records in frame pixels (DET_DTYPE, sorted by confidence, valid = 1, _pad = 0)."""
    return sort_nms_numpy(map_records(slots, counts, tiles, net_w, net_h), merge_iou)
