"""Evaluation entry point over the engine: the counterpart of the reference's ``eval.py::evaluate_model``
(eval.py:18-138) and of ``train.py::calibrate_conformal_prediction`` (train.py:299-520) -- SURVEY.md section 8f rows 2-3.

The reference runs ``ultralytics.YOLO(weights).val(save_json=True)``, re-reads ``predictions.json`` (records
``{'image_id': stem, 'category_id': int, 'bbox': [x_min, y_min, w, h] px, 'score': float}``, eval.py:58-61), walks the
validation images of a YOLO-layout dataset (``<root>/images/<stem>.*`` beside ``<root>/labels/<stem>.txt``, rows
``cls xc yc w h`` normalised, eval.py:110-121), converts each prediction with the image's own width / height
(eval.py:96-108) and feeds ``SmallObjectMetric`` (data_loader.py:249-414). Here the detector is an engine file run
through the C ABI (``unina_infer`` / ``unina_infer_bgra``); everything after the detector is the same sequence.

    python -m unina_yolo_dla_amd.evaluate --engine model.une --data <root> [--out-dir runs/eval] [--conformal]

Frames: ``.npy`` holding the network tensor itself (fp32 ``[3,H,W]``, H x W = the engine's input size) or a camera
frame (uint8 ``[h,w,4]`` BGRA / ``[h,w,3]`` RGB, any size: resized + normalised on the GPU by the stem kernel, i.e.
``unina_infer_bgra``), and ``.png`` / ``.jpg`` when Pillow is importable. Detections come back in network pixels; the
records written to predictions.json are scaled to the image's own pixels, as Ultralytics writes them.

By default a camera frame is STRETCHED to the network input (``unina_infer_bgra``). ``--letterbox`` keeps its aspect ratio, as
``YOLO.val`` does: ``unina_infer_letterbox_bgra`` with pad 114 and ``map_boxes=1``, so the records come back in the image's own
pixels from the GPU and the host rescale is skipped for them.

``--device-metrics`` scores the detections against the labels on the GPU (csrc/evalmatch.hip through ``unina_eval_*``): the
records stay on the device (``unina_infer_async`` and its kin), one small launch per image follows the frame on its stream,
and counters, conformal scores and AP rows come back once, after the last image. Same numbers as the host loops of
``metrics.py``, which remain the definition. ``--map`` adds ``map50`` / ``map50_95`` (``metrics.mean_average_precision``: this
project's own COCO-style definition, parity with the reference's ``model.val`` unpinned) from the low-confidence pass.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import metrics

IMAGE_EXT = (".npy", ".png", ".jpg", ".jpeg")


def list_frames(root: str) -> List[str]:
    """Validation images of a YOLO-layout dataset: <root>/images/* (or <root>/* when there is no images/ dir)."""
    d = os.path.join(root, "images") if os.path.isdir(os.path.join(root, "images")) else root
    files = [f for f in sorted(glob.glob(os.path.join(d, "*"))) if f.lower().endswith(IMAGE_EXT)]
    return files


def label_path(frame_path: str) -> str:
    """eval.py:110-112: labels live in the sibling 'labels' directory, <stem>.txt."""
    stem = os.path.splitext(os.path.basename(frame_path))[0]
    return os.path.join(os.path.dirname(os.path.dirname(frame_path)), "labels", stem + ".txt")


def read_labels(path: str) -> np.ndarray:
    """YOLO txt rows 'cls xc yc w h' (normalised) -> [M,5] (eval.py:113-121); a missing file is an empty image."""
    rows = []
    if os.path.exists(path):
        with open(path) as f:
            for line in f:
                p = line.split()
                if len(p) >= 5:
                    rows.append([float(p[0])] + [float(v) for v in p[1:5]])
    return np.asarray(rows, dtype=np.float64).reshape(-1, 5)


def load_frame(path: str) -> np.ndarray:
    if path.lower().endswith(".npy"):
        return np.load(path, allow_pickle=False)
    try:
        from PIL import Image
    except ImportError as e:                                         # pragma: no cover
        raise RuntimeError(f"{path}: reading image files needs Pillow; store frames as .npy instead") from e
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)


def frame_size(frame: np.ndarray) -> Tuple[int, int]:
    """(width, height) of the image the labels are normalised to."""
    if frame.dtype == np.uint8:
        return frame.shape[1], frame.shape[0]
    return frame.shape[-1], frame.shape[-2]


class EngineDetector:
    """frame -> detections through the C ABI. fp32 [3,H,W] frames go to unina_infer; uint8 camera frames are packed to
    BGRA and go to unina_infer_bgra (pre-process inside the stem kernel, perception_node.cpp:601-656 as one call)."""

    def __init__(self, engine_path: str, device: int = 0, autotune: bool = True, letterbox: bool = False):
        from .engine import Engine
        self.eng = Engine(engine_path, device)
        if autotune:
            self.eng.autotune()
        self.width, self.height = self.eng.width, self.eng.height
        self.num_classes, self.device = self.eng.num_classes, self.eng.device
        self.letterbox = letterbox          # uint8 frames: letterboxed in the stem, boxes returned in the frame's own pixels

    @staticmethod
    def _bgra(frame: np.ndarray) -> np.ndarray:
        h, w = frame.shape[:2]
        if frame.shape[2] == 3:                                      # RGB -> BGRA
            bgra = np.empty((h, w, 4), dtype=np.uint8)
            bgra[..., 0], bgra[..., 1], bgra[..., 2], bgra[..., 3] = frame[..., 2], frame[..., 1], frame[..., 0], 255
        else:
            bgra = np.ascontiguousarray(frame)
        return bgra.reshape(h, w * 4)

    def device_records(self, frame: np.ndarray, conf: float, iou: float, q: float):
        """__call__ with the records left on the device: the int32 CUDA tensor of Engine.infer_async (word 0 = count, records
        from word 8), enqueued on the current stream, nothing synchronised. The tensor is the engine's own and is rewritten
        by the next call; work enqueued on the same stream in between reads it in order. Stretched camera frames take the
        two-step form of unina_infer_bgra (preprocess_bgra[_resize], then unina_infer_async: identical results)."""
        import torch
        dev = torch.device("cuda", self.eng.device)
        if frame.dtype == np.uint8:
            h, w = frame.shape[:2]
            self._cam = cam = torch.from_numpy(self._bgra(frame)).to(dev)
            if self.letterbox:
                return self.eng.infer_letterbox_bgra(cam, w, h, w * 4, None, conf, iou, q, 114.0, True, out=self.eng._det_buf)
            L = self.eng.L
            if getattr(self, "_tensor", None) is None:
                self._tensor = torch.empty((1, 3, self.height, self.width), dtype=torch.float32, device=dev)
            norm, stream = L.create_norm_params_imagenet(), torch.cuda.current_stream().cuda_stream
            if (w, h) == (self.width, self.height):
                rc = L.preprocess_bgra(cam.data_ptr(), self._tensor.data_ptr(), w, h, w * 4, norm, stream)
            else:
                rc = L.preprocess_bgra_resize(cam.data_ptr(), self._tensor.data_ptr(), w, h, w * 4, self.width, self.height, norm, stream)
            if rc:
                raise RuntimeError(f"pre-process of a {w} x {h} camera frame failed (hipError {rc})")
            return self.eng.infer_async(self._tensor, conf, iou, q)
        x = np.ascontiguousarray(frame, dtype=np.float32).reshape(1, 3, self.height, self.width)
        self._frame = torch.from_numpy(x).to(dev)
        return self.eng.infer_async(self._frame, conf, iou, q)

    def __call__(self, frame: np.ndarray, conf: float, iou: float, q: float) -> np.ndarray:
        import torch
        dev = torch.device("cuda", self.eng.device)
        if frame.dtype == np.uint8:
            h, w = frame.shape[:2]
            cam = torch.from_numpy(self._bgra(frame)).to(dev)
            if self.letterbox:
                return self.eng.infer_letterbox_bgra(cam, w, h, w * 4, None, conf, iou, q, 114.0, True)
            return self.eng.infer_bgra(cam, w, h, w * 4, None, conf, iou, q)
        x = np.ascontiguousarray(frame, dtype=np.float32).reshape(1, 3, self.height, self.width)
        return self.eng.infer(torch.from_numpy(x).to(dev), conf, iou, q)

    def close(self):
        self.eng.close()


def evaluate(detect: Callable[[np.ndarray, float, float, float], np.ndarray], root: str, imgsz: int = 640,
             conf: float = 0.5, iou: float = 0.45, conformal_q: float = 0.1, out_dir: Optional[str] = None,
             net_size: Optional[Tuple[int, int]] = None, conformal_alpha: Optional[float] = None,
             conformal_conf: float = 0.001, camera_pixels: bool = False, device_metrics: bool = False,
             map_metrics: bool = False) -> Dict[str, object]:
    """eval.py:18-138 over `detect` (frame, conf, iou, q) -> GpuDetection records in network pixels.

    Writes <out_dir>/predictions.json (eval.py:58-61 schema, boxes in the image's own pixels), computes
    SmallObjectMetric(size_threshold=15, image_size=imgsz) exactly as eval.py:74,96-131 does, and -- with
    `conformal_alpha` -- the conformal quantile of train.py:299-520 from a second pass at a very low confidence
    threshold (train.py:403) without dilation. Returns {'small_object': {...}, 'conformal': {...} | None,
    'predictions': [...], 'images': n}. camera_pixels: `detect` returns the records of uint8 camera frames in the frame's own
    pixels already (a letterboxing detector with the box map on): no host rescale for them.

    map_metrics: also 'map50' / 'map50_95' (metrics.mean_average_precision) from the low-confidence pass, which then runs
    whether or not `conformal_alpha` is given. device_metrics: the matching runs on the GPU (unina_eval_*): `detect` must be an
    EngineDetector (device_records, num_classes, device); the records of the main pass are still copied out for
    predictions.json, the low-confidence pass copies nothing, and every number equals the host path's. An image may then carry
    at most engine.EVAL_MAX_LABELS labels."""
    files = list_frames(root)
    if not files:
        raise FileNotFoundError(f"no frames (*.npy / *.png / *.jpg) under {root}")
    records: List[dict] = []
    so = metrics.SmallObjectMetric(size_threshold=15, image_size=imgsz)           # eval.py:74
    conf_dets, conf_labels = [], []
    low_pass = conformal_alpha is not None or map_metrics
    dev_eval = None
    if device_metrics:
        from . import engine
        dev_eval = engine.DeviceEval(detect.num_classes, len(files) * engine.EVAL_MAX_LABELS if conformal_alpha is not None else 0,
                                     len(files) * engine.MAX_DETECTIONS if map_metrics else 0, detect.device)
        dev_eval.reset()
    for path in files:
        stem = os.path.splitext(os.path.basename(path))[0]
        frame = load_frame(path)
        w, h = frame_size(frame)
        if frame.dtype == np.uint8 and camera_pixels:                 # camera frame, boxes mapped back on the GPU
            nw, nh = w, h
        elif frame.dtype == np.uint8:                                 # camera frame: detections come back in network pixels
            if net_size is None:
                raise ValueError("uint8 camera frames need net_size=(width, height) of the engine input")
            nw, nh = net_size
        else:                                                         # the network tensor itself
            nw, nh = w, h
        sx, sy = w / nw, h / nh
        labels = read_labels(label_path(path))
        if dev_eval is not None:
            params = engine.EvalParams(sx, sy, imgsz / nw, imgsz / nh, w, h, imgsz, so.size_threshold, so.iou_threshold)
            buf = detect.device_records(frame, conf, iou, conformal_q)
            dev_eval.update(buf, labels, params, engine.EVAL_SMALL)
            dets = engine.Engine.unpack(buf)
        else:
            dets = detect(frame, conf, iou, conformal_q)
        scaled = dets.copy()
        scaled["x1"], scaled["x2"] = dets["x1"] * sx, dets["x2"] * sx
        scaled["y1"], scaled["y2"] = dets["y1"] * sy, dets["y2"] * sy
        recs = metrics.detections_to_coco(scaled, stem)
        records += recs
        if dev_eval is not None:
            if low_pass:
                what = (engine.EVAL_CONFORMAL if conformal_alpha is not None else 0) | (engine.EVAL_AP if map_metrics else 0)
                dev_eval.update(detect.device_records(frame, conformal_conf, iou, 0.0), labels, params, what)
            continue
        so.update([metrics.coco_to_metric_rows(recs, w, h)], [labels])           # eval.py:96-108, 124
        if low_pass:
            d0 = detect(frame, conformal_conf, iou, 0.0)
            # conformal_quantile converts labels with ONE size (train.py:346-352): hand it boxes in imgsz pixels
            c = d0.copy()
            c["x1"], c["x2"] = d0["x1"] * (imgsz / nw), d0["x2"] * (imgsz / nw)
            c["y1"], c["y2"] = d0["y1"] * (imgsz / nh), d0["y2"] * (imgsz / nh)
            conf_dets.append(c)
            conf_labels.append(labels)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "predictions.json"), "w") as f:
            json.dump(records, f)
    if dev_eval is not None:
        try:
            res, scores, rows = dev_eval.read()
        finally:
            dev_eval.close()
        if res.overflow:
            raise RuntimeError(f"device metric lists overflowed (flags {res.overflow}): {res.n_scores} scores, {res.n_rows} rows")
        so.true_positives, so.false_positives, so.false_negatives = int(res.tp), int(res.fp), int(res.fn)
        label_counts = list(res.label_counts[:detect.num_classes])
    elif map_metrics:
        rows = np.concatenate([metrics.ap_rows_numpy(d, l, imgsz) for d, l in zip(conf_dets, conf_labels)])
        label_counts = {}
        for l in conf_labels:
            for c in l[:, 0]:
                if c >= 0:
                    label_counts[int(c)] = label_counts.get(int(c), 0) + 1
    result: Dict[str, object] = {"images": len(files), "predictions": records, "small_object": so.compute(), "conformal": None}
    if map_metrics:
        result.update(metrics.mean_average_precision(rows, label_counts))
    if conformal_alpha is not None:
        result["conformal"] = (metrics.conformal_from_scores(scores, conformal_alpha) if dev_eval is not None
                               else metrics.conformal_quantile(conf_dets, conf_labels, conformal_alpha, imgsz))
        if out_dir:
            with open(os.path.join(out_dir, "conformal_params.json"), "w") as f:     # train.py:506-520 writes the same keys
                json.dump(result["conformal"], f, indent=2)
    return result


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(description="small-object P/R/F1 (+ conformal quantile) of an engine file over a YOLO-layout dataset")
    ap.add_argument("--engine", required=True, help=".une engine file (export.export_engine)")
    ap.add_argument("--data", required=True, help="dataset root: images/ + labels/")
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--conf", type=float, default=0.5)
    ap.add_argument("--iou", type=float, default=0.45)
    ap.add_argument("--conformal-q", type=float, default=0.1)
    ap.add_argument("--conformal", action="store_true", help="also calibrate q_hat (train.py:299-520)")
    ap.add_argument("--alpha", type=float, default=0.10)
    ap.add_argument("--out-dir", default="runs/eval")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--letterbox", action="store_true",
                    help="uint8 camera frames keep their aspect ratio (pad 114) instead of being stretched; boxes mapped back on the GPU")
    ap.add_argument("--device-metrics", action="store_true",
                    help="match detections against labels on the GPU (unina_eval_*); same numbers, no per-image host loops")
    ap.add_argument("--map", action="store_true", help="also report map50 / map50_95 from the low-confidence pass (this project's definition)")
    a = ap.parse_args(argv)
    det = EngineDetector(a.engine, a.device, letterbox=a.letterbox)
    try:
        res = evaluate(det, a.data, a.imgsz, a.conf, a.iou, a.conformal_q, a.out_dir, (det.width, det.height),
                       a.alpha if a.conformal else None, camera_pixels=a.letterbox, device_metrics=a.device_metrics,
                       map_metrics=a.map)
    finally:
        det.close()
    print(f"{res['images']} images, {len(res['predictions'])} predictions -> {os.path.join(a.out_dir, 'predictions.json')}")
    for k, v in res["small_object"].items():                                      # eval.py:128-131
        print(f"    {k}: {v}")
    if a.map:
        print(f"    map50: {res['map50']:.6f}  map50_95: {res['map50_95']:.6f}  (own COCO-style definition, unpinned against model.val)")
    if res["conformal"]:
        print(f"    q_hat: {res['conformal']['q_hat']:.6f}  ({res['conformal']['num_calibration_samples']} matched boxes)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
