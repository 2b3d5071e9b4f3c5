#!/usr/bin/env python3
"""Cost of scoring one image's detections against its labels, host loops against the device kernel; prints ONE JSON line and
writes it to profiles/r04/eval_bench.json.

The image is what the conformal pass of evaluate() sees: the 640 x 640 engine (seed-7 synthetic weights) run at conf = 0.001,
about MAX_DETECTIONS records, and `--labels` labels (default 32) derived from its own detections. Per image:
  * host_small_ms / host_conformal_ms: metrics.SmallObjectMetric.update on the rows evaluate() builds, and
    metrics.conformal_quantile (its matching loop; the quantile at the end is negligible), median of `--host-reps` runs;
  * kernel_ms: one unina_eval_update_async launch doing all three parts, HIP events around `--reps` back-to-back launches;
  * frame_ms / frame_plus_eval_ms: wall clock per frame of `--reps` unina_infer_async calls enqueued back to back and
    synchronised once, without and with the update enqueued behind each frame on the same stream; added_ms is the
    difference: what the kernel lengthens the frame loop by.
Asserts that the device counters and scores equal the host's.

    python tools/bench_eval.py [--labels 32] [--reps 200] [--host-reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import median_ms, wall_ms, window_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", type=int, default=32)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "eval_bench.json"))
    args = ap.parse_args()
    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd import engine, metrics
    size = 640
    g = u.graph.Graph()
    eng = engine.Engine.from_state_dict(u.synth.make_state_dict(7, g), g)
    x = torch.from_numpy(u.rng.frame(1234, size, size)).cuda()
    conf, iou = 0.001, 0.45
    dets = eng.infer(x, conf, iou, 0.0)
    top = dets[np.argsort(-dets["confidence"], kind="stable")][:args.labels]
    labels = np.array([[d["class_id"], (d["x1"] + d["x2"]) / 2 / size + 0.0004 * (i % 4), (d["y1"] + d["y2"]) / 2 / size,
                        (d["x2"] - d["x1"]) / size * (0.85 if i % 3 == 0 else 1.0), (d["y2"] - d["y1"]) / size]
                       for i, d in enumerate(top)], dtype=np.float64).reshape(-1, 5)

    def host_small():
        m = metrics.SmallObjectMetric(size_threshold=15, image_size=size)
        m.update([metrics.coco_to_metric_rows(metrics.detections_to_coco(dets, "x"), size, size)], [labels])
        return m
    so, host_small_ms = median_ms(host_small, args.host_reps)
    cq, host_conf_ms = median_ms(lambda: metrics.conformal_quantile([dets], [labels], 0.1, size), args.host_reps)

    params = engine.EvalParams(1.0, 1.0, 1.0, 1.0, size, size, size, 15.0, 0.5)
    what = engine.EVAL_SMALL | engine.EVAL_CONFORMAL | engine.EVAL_AP
    ev = engine.DeviceEval(eng.num_classes, (4 * args.reps + 1) * engine.EVAL_MAX_LABELS, (4 * args.reps + 1) * engine.MAX_DETECTIONS)
    lab = torch.from_numpy(labels).cuda()
    buf = eng.infer_async(x, conf, iou, 0.0)
    ev.reset()
    ev.update(buf, lab, params, what)
    res, scores, _ = ev.read()
    assert (res.tp, res.fp, res.fn) == (so.true_positives, so.false_positives, so.false_negatives), "device counters differ from the host's"
    assert res.n_scores == cq["num_calibration_samples"] and metrics.conformal_from_scores(scores, 0.1) == cq, "device scores differ"

    kernel_ms = window_ms(torch, lambda: ev.update(buf, lab, params, what), args.reps)

    def frame(with_eval):
        b = eng.infer_async(None, conf, iou, 0.0)
        if with_eval:
            ev.update(b, lab, params, what)
    wall_ms(torch, lambda: frame(False), args.reps)
    frame_ms = min(wall_ms(torch, lambda: frame(False), args.reps) for _ in range(3))
    both_ms = min(wall_ms(torch, lambda: frame(True), args.reps) for _ in range(3))
    res, _, _ = ev.read()
    out = {"records": int(len(dets)), "labels": int(len(labels)), "reps": args.reps,
           "host_small_ms": host_small_ms, "host_conformal_ms": host_conf_ms, "host_ms": host_small_ms + host_conf_ms,
           "kernel_ms": kernel_ms, "frame_ms": frame_ms, "frame_plus_eval_ms": both_ms, "added_ms": both_ms - frame_ms,
           "overflow": int(res.overflow),
           "note": "kernel_ms: HIP events around back-to-back launches (dispatch included); frame_*: wall clock per frame, "
                   "best of 3 loops of `reps` frames enqueued back to back, one synchronisation per loop"}
    ev.close()
    eng.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
