#!/usr/bin/env python3
"""Cost of one colour stage (unina_colour_async, csrc/colour.hip: a 32-byte memset and one launch), device against the host route
and against the tracker's launch on the same record count; prints ONE JSON line and writes it to profiles/r04/colour_latency.txt.

Three scenes on a 1280 x 720 image of painted blocks with noise:
  * lidar_only : 80 records, 60 of the camera's (boxes, classes 0..2) and 20 LiDAR-only ones (point boxes, class 9, cones 5..25 m
                 away: SIZE windows of 5 x 7 up to 12 x 17 pixels at the default small-cone geometry), only_class = 9, 3 channels;
  * full_64x64 : 1024 records whose boxes are 64 x 64 pixels, every record selected, taper = 256: 4096 samples each, 4 channels;
  * one_pixel  : 1024 one-pixel windows, 4 channels.
Per scene:
  * host_d2h_ms / host_numpy_ms: the host route a node would otherwise take -- the records, the cones and the image copied to the
    host and colour.colour_numpy on them -- median of `--host-reps` runs;
  * kernel_ms: HIP events around the memset and the launch (dispatch included), median over `--reps` repetitions (the call is
    stateless: it is simply repeated);
  * idle_kernel_ms: the same with an only_class no record carries: every workgroup copies its record and leaves;
  * track_kernel_ms: the same around one unina_track_update_async on the same records, whose table a set-up update filled from
    them: the launch that follows the stage.
Asserts that every output equals colour_numpy's, byte for byte, before printing.

    python tools/bench_colour.py [--reps 50] [--host-reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import median_ms  # noqa: E402

CAM = (900.0, 900.0, 640.0, 360.0)
WIDTH, HEIGHT = 1280, 720
PAINT = ((230, 210, 40), (30, 80, 200), (240, 110, 30), (235, 235, 235), (25, 25, 25), (100, 100, 100), (60, 140, 50))   # R, G, B


def image(channels, order):
    rng = np.random.default_rng(4)
    base = np.array(PAINT, dtype=np.int64)[rng.integers(0, len(PAINT), (HEIGHT // 12, WIDTH // 16))]
    img = np.repeat(np.repeat(base, 12, axis=0), 16, axis=1)
    img = np.clip(img + rng.integers(-12, 13, img.shape), 0, 255).astype(np.uint8)
    img = img if order == 1 else img[..., ::-1]
    if channels == 4:
        img = np.concatenate([img, np.full((HEIGHT, WIDTH, 1), 255, dtype=np.uint8)], axis=2)
    return np.ascontiguousarray(img)


def records(boxes, cls, u, v, z):
    from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DET_DTYPE
    dets, cones = np.zeros(1024, dtype=DET_DTYPE), np.zeros(1024, dtype=CONE3D_DTYPE)
    m = len(boxes)
    dets["x1"][:m], dets["y1"][:m], dets["x2"][:m], dets["y2"][:m] = np.asarray(boxes, dtype=np.float32).T
    dets["confidence"][:m], dets["class_id"][:m], dets["valid"][:m] = 0.6, cls, 1
    cones["u"][:m], cones["v"][:m], cones["z"][:m] = u, v, z
    cones["x"][:m], cones["y"][:m] = (cones["u"][:m] - CAM[2]) * cones["z"][:m] / CAM[0], (cones["v"][:m] - CAM[3]) * cones["z"][:m] / CAM[1]
    cones["n_valid"][:m], cones["n_samples"][:m], cones["valid"][:m] = 12, 12, 1
    return dets, cones, m


def scenes():
    rng = np.random.default_rng(3)
    u, v, z = rng.uniform(40, 1240, 80), rng.uniform(300, 680, 80), rng.uniform(5, 25, 80)
    half = 900.0 * 0.12 / z
    boxes = np.stack([u - half, v - 1.5 * half, u + half, v + 1.3 * half], axis=1)
    boxes[60:] = np.stack([u[60:], v[60:], u[60:], v[60:]], axis=1)                   # the fuser's point boxes
    cls = np.concatenate([rng.integers(0, 3, 60), np.full(20, 9)])
    i = np.arange(1024)
    gu, gv = (i % 32) * 38.0 + 2.0, (i // 32) * 20.0 + 2.0
    far = np.linspace(4.0, 30.0, 1024)
    big = np.stack([gu + 0.25, gv + 0.25, gu + 63.75, gv + 63.75], axis=1)
    dot = np.stack([gu + 0.25, gv + 0.25, gu + 0.75, gv + 0.75], axis=1)
    return [("lidar_only", records(boxes, cls, u, v, z), 3, 0, dict(only_class=9)),
            ("full_64x64", records(big, 9, gu + 32, gv + 32, far), 4, 0, dict(only_class=-1, taper=256)),
            ("one_pixel", records(dot, 9, gu, gv, far), 4, 0, dict(only_class=-1, taper=256, min_pixels=1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "colour_latency.txt"))
    args = ap.parse_args()
    import torch
    from unina_yolo_dla_amd import colour, tracking
    from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DET_DTYPE
    clf, trk = colour.DeviceColourClassifier(), tracking.DeviceTracker()
    tpar = tracking.make_params(gate=0.5, alpha=0.5, birth_confidence=0.3, class_aware=1, confirm_hits=2, max_missed=2)
    names = ("header", "dets", "colours")
    out = {"reps": args.reps, "image": [WIDTH, HEIGHT], "scenes": {}}
    for name, (dets, cones, m), channels, order, extra in scenes():
        par = colour.make_colour_params(order=order, **extra)
        img = image(channels, order)
        det_buf = torch.from_numpy(np.concatenate([np.array([m] + [0] * 7, dtype=np.int32), dets.view(np.int32)])).cuda()
        d_cones, d_img = torch.from_numpy(cones.view(np.int32)).cuda(), torch.from_numpy(img).cuda()
        want = colour.colour_numpy(dets, m, cones, img, CAM, par)

        times, track_times = [], []
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            clf.classify_async(det_buf[8:], det_buf[:1], d_cones, d_img, CAM, par, clf.det_buf[8:])
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop))
        clf.det_buf[:8].copy_(det_buf[:8])
        got = dict(zip(names, clf.read()))
        for what in names:
            assert got[what].tobytes() == want[what].tobytes(), f"{name}: {what} differs"
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            trk.reset()
            trk.update_from_buffer(clf.det_buf, d_cones, tpar)
            start.record()
            trk.update_from_buffer(clf.det_buf, d_cones, tpar)
            stop.record()
            torch.cuda.synchronize()
            track_times.append(start.elapsed_time(stop))
        track_header, _ = trk.read()
        idle = colour.make_colour_params(order=order, **dict(extra, only_class=1 << 20))      # no record carries this id
        idle_times = []
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            clf.classify_async(det_buf[8:], det_buf[:1], d_cones, d_img, CAM, idle, clf.det_buf[8:])
            stop.record()
            torch.cuda.synchronize()
            idle_times.append(start.elapsed_time(stop))

        def d2h():
            torch.cuda.synchronize()
            return det_buf.cpu().numpy(), d_cones.cpu().numpy(), d_img.cpu().numpy()
        (hd, hc, hi), d2h_ms = median_ms(d2h, args.host_reps)
        _, numpy_ms = median_ms(lambda: colour.colour_numpy(hd[8:].view(DET_DTYPE), int(hd[0]), hc.view(CONE3D_DTYPE), hi, CAM, par), args.host_reps)
        h = want["header"][0]
        out["scenes"][name] = {"channels": channels, "n_records": int(h["n_records"]), "n_selected": int(h["n_selected"]), "n_window": int(h["n_window"]),
                               "n_decided": int(h["n_decided"]), "n_class": h["n_class"].tolist(), "samples": int(want["colours"]["n_mask"].sum()),
                               "kernel_ms": float(np.median(times)), "kernel_ms_min": float(np.min(times)),
                               "idle_kernel_ms": float(np.median(idle_times)), "track_kernel_ms": float(np.median(track_times)), "track_n_matched": int(track_header["n_matched"][0]),
                               "host_d2h_ms": d2h_ms, "host_numpy_ms": numpy_ms, "host_ms": d2h_ms + numpy_ms}
    trk.close()
    out["note"] = ("kernel_ms: HIP events around the header's memset and the single launch (dispatch included), median of `reps` repetitions; "
                   "idle_kernel_ms: the same call with no record selected; track_kernel_ms: the same around one tracker update on the same records behind a set-up update with them; host_*: D2H of the "
                   "records, the cones and the image + colour.colour_numpy, median of the host reps; samples: the pixels inside the silhouettes")
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
