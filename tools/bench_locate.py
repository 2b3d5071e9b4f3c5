#!/usr/bin/env python3
"""Cost of lifting one frame's detections to 3-D points from a depth map, device launch against the host path; prints ONE JSON
line and writes it to profiles/r04/locate_latency.txt.

The frame is the 640 x 640 engine (seed-7 synthetic weights) on its synthetic frame, the confidence threshold set so that about
`--records` records (default 500) are kept; the depth map is a 640 x 640 float32 plane (metres, 30 % holes). Per frame:
  * host_d2h_ms / host_numpy_ms: the host path a node would otherwise take -- the depth plane copied to the host (1.6 MB) and
    localize.locate_numpy on the records -- median of `--host-reps` runs;
  * kernel_ms: one unina_locate_async launch, HIP events around `--reps` back-to-back launches (dispatch included);
  * frame_ms / frame_plus_locate_ms: wall clock per frame of `--reps` unina_infer_async calls enqueued back to back and
    synchronised once, without and with the launch enqueued behind each frame on the same stream; added_ms is the difference.
Asserts that the device records equal locate_numpy's, byte for byte, before printing.

    python tools/bench_locate.py [--records 500] [--reps 200] [--host-reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import median_ms, wall_ms, window_ms  # noqa: E402


def synthetic_depth(seed, h, w, holes=0.3):
    rng = np.random.RandomState(seed)
    d = rng.uniform(0.5, 30.0, (h, w)).astype(np.float32)
    marks = np.array([np.nan, np.inf, -np.inf, 0.0], dtype=np.float32)
    return np.where(rng.rand(h, w) < holes, marks[rng.randint(0, 4, (h, w))], d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=500)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "locate_latency.txt"))
    args = ap.parse_args()
    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd import engine, localize
    size = 640
    g = u.graph.Graph()
    eng = engine.Engine.from_state_dict(u.synth.make_state_dict(7, g), g)
    x = torch.from_numpy(u.rng.frame(1234, size, size)).cuda()
    iou = 0.45
    every = eng.infer(x, 0.001, iou, 0.0)
    ranked = np.sort(every["confidence"])[::-1]
    conf = float(ranked[min(args.records, len(ranked)) - 1])            # the threshold that keeps about `records` of them
    depth = synthetic_depth(4321, size, size)
    d_depth = torch.from_numpy(depth).cuda()
    cam = (700.0, 700.0, 319.5, 319.5)
    par = localize.as_params(dict(sx=1.0, sy=1.0, shrink=0.5, min_depth=0.3, max_depth=40.0, max_side=64, min_valid=1))
    loc = localize.DeviceLocator()

    buf = eng.infer_async(x, conf, iou, 0.0)
    loc.update_from_buffer(buf, d_depth, 1.0, cam, par)
    got = loc.read()
    dets = engine.Engine.unpack(buf)

    def d2h():
        torch.cuda.synchronize()
        return d_depth.cpu().numpy()
    host_depth, d2h_ms = median_ms(d2h, args.host_reps)
    want, numpy_ms = median_ms(lambda: localize.locate_numpy(dets, len(dets), host_depth, engine.DEPTH_F32, 1.0, cam, par), args.host_reps)
    assert got.tobytes() == want.tobytes(), "device records differ from locate_numpy's"

    kernel_ms = window_ms(torch, lambda: loc.update_from_buffer(buf, d_depth, 1.0, cam, par), args.reps)

    def frame(with_locate):
        b = eng.infer_async(None, conf, iou, 0.0)
        if with_locate:
            loc.update_from_buffer(b, d_depth, 1.0, cam, par)
    wall_ms(torch, lambda: frame(False), args.reps)
    frame_ms = min(wall_ms(torch, lambda: frame(False), args.reps) for _ in range(3))
    both_ms = min(wall_ms(torch, lambda: frame(True), args.reps) for _ in range(3))
    assert loc.read().tobytes() == want.tobytes(), "device records differ after the timed loops"
    n = len(dets)
    out = {"records": int(n), "located": int((got["valid"] == 1).sum()), "max_samples": int(got["n_samples"].max()),
           "median_samples": int(np.median(got["n_samples"][:n])) if n else 0, "conf_threshold": conf, "reps": args.reps,
           "depth_bytes": int(depth.nbytes), "host_d2h_ms": d2h_ms, "host_numpy_ms": numpy_ms, "host_ms": d2h_ms + numpy_ms,
           "kernel_ms": kernel_ms, "frame_ms": frame_ms, "frame_plus_locate_ms": both_ms, "added_ms": both_ms - frame_ms,
           "note": "kernel_ms: HIP events around back-to-back launches (dispatch included); frame_*: wall clock per frame, "
                   "best of 3 loops of `reps` frames enqueued back to back, one synchronisation per loop"}
    eng.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
