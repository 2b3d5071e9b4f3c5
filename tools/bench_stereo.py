#!/usr/bin/env python3
"""Cost of lifting one frame's detections to 3-D points from a rectified stereo pair, device launch against the host route; prints
ONE JSON line per record count and writes them to profiles/r04/stereo_latency.txt.

The frame is the 640 x 640 engine (seed-7 synthetic weights) on its synthetic frame, the confidence threshold set so that about
`--records` records (default 60 and 500) are kept; the pair is 1280 x 720 (sx = 2, sy = 1.125): a smoothed-noise left plane and
a right plane built from it in eight horizontal bands of disparity 12 .. 300. fx = 700, baseline = 0.12 m, depths 0.25 .. 40 m:
disparities 3 .. 336 are searched. Per frame:
  * host_d2h_ms / host_numpy_ms: the host route a node would otherwise take -- both planes copied to the host (1.8 MB) and
    localize.locate_stereo_numpy on the records -- median of `--host-reps` runs;
  * kernel_ms: one unina_locate_stereo_async launch, HIP events around `--reps` back-to-back launches (dispatch included);
  * frame_ms / frame_plus_stereo_ms: wall clock per frame of `--reps` unina_infer_async calls enqueued back to back and
    synchronised once, without and with the launch enqueued behind each frame on the same stream; added_ms is the difference.
Asserts that the device records (cones and matches) equal locate_stereo_numpy's, byte for byte, before printing.

    python tools/bench_stereo.py [--records 60 500] [--reps 200] [--host-reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import median_ms, wall_ms, window_ms  # noqa: E402

W, H = 1280, 720
BANDS = (12, 24, 40, 64, 96, 140, 200, 300)


def synthetic_pair(seed):
    """left: noise smoothed by two passes of a 5-point average, stretched to 0 .. 255; right: band b of H / 8 rows is left shifted
    by BANDS[b] columns (right[v, u - d] = left[v, u]), other noise where nothing maps."""
    rng = np.random.RandomState(seed)
    a = rng.uniform(0.0, 256.0, (H, W))
    for _ in range(2):
        p = np.pad(a, 1, mode="edge")
        a = (p[1:-1, 1:-1] + p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:]) / 5.0
    left = np.clip(np.rint((a - a.min()) * (255.0 / (a.max() - a.min()))), 0, 255).astype(np.uint8)
    right = rng.randint(0, 256, (H, W)).astype(np.uint8)
    rows = H // len(BANDS)
    for b, d in enumerate(BANDS):
        right[b * rows:(b + 1) * rows, :W - d] = left[b * rows:(b + 1) * rows, d:]
    return left, right


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, nargs="+", default=[60, 500])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "stereo_latency.txt"))
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
    left, right = synthetic_pair(4321)
    d_left, d_right = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    cam, baseline = (700.0, 700.0, 639.5, 359.5), 0.12
    par = localize.make_stereo_params(sx=W / size, sy=H / size, shrink=0.5, min_depth=0.25, max_depth=40.0, max_side=64, max_mean_sad=20,
                                      uniqueness=10)
    loc = localize.DeviceStereoLocator()

    lines = []
    for records in args.records:
        conf = float(ranked[min(records, len(ranked)) - 1])            # the threshold that keeps about `records` of them
        buf = eng.infer_async(x, conf, iou, 0.0)
        loc.update_from_buffer(buf, d_left, d_right, cam, baseline, par)
        got = loc.read()
        dets = engine.Engine.unpack(buf)

        def d2h():
            torch.cuda.synchronize()
            return d_left.cpu().numpy(), d_right.cpu().numpy()
        (host_left, host_right), d2h_ms = median_ms(d2h, args.host_reps)
        want, numpy_ms = median_ms(lambda: localize.locate_stereo_numpy(dets, len(dets), host_left, host_right, cam, baseline, par),
                                   args.host_reps)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), "device records differ from locate_stereo_numpy's"

        kernel_ms = window_ms(torch, lambda: loc.update_from_buffer(buf, d_left, d_right, cam, baseline, par), args.reps)

        def frame(with_stereo):
            b = eng.infer_async(None, conf, iou, 0.0)
            if with_stereo:
                loc.update_from_buffer(b, d_left, d_right, cam, baseline, par)
        wall_ms(torch, lambda: frame(False), args.reps)
        frame_ms = min(wall_ms(torch, lambda: frame(False), args.reps) for _ in range(3))
        both_ms = min(wall_ms(torch, lambda: frame(True), args.reps) for _ in range(3))
        after = loc.read()
        assert after[0].tobytes() == want[0].tobytes() and after[1].tobytes() == want[1].tobytes(), "device records differ after the timed loops"
        n = len(dets)
        cones = got[0][:n]
        work = cones["n_samples"].astype(np.int64) * cones["n_valid"]
        out = {"records": int(n), "located": int((cones["valid"] == 1).sum()), "max_samples": int(cones["n_samples"].max()) if n else 0,
               "median_samples": int(np.median(cones["n_samples"])) if n else 0, "median_disparities": int(np.median(cones["n_valid"])) if n else 0,
               "max_disparities": int(cones["n_valid"].max()) if n else 0, "abs_differences": int(work.sum()), "conf_threshold": conf,
               "reps": args.reps, "plane_bytes": int(left.nbytes + right.nbytes), "host_d2h_ms": d2h_ms, "host_numpy_ms": numpy_ms,
               "host_ms": d2h_ms + numpy_ms, "kernel_ms": kernel_ms, "frame_ms": frame_ms, "frame_plus_stereo_ms": both_ms,
               "added_ms": both_ms - frame_ms,
               "note": "kernel_ms: HIP events around back-to-back launches (dispatch included); frame_*: wall clock per frame, "
                       "best of 3 loops of `reps` frames enqueued back to back, one synchronisation per loop"}
        lines.append(json.dumps(out))
        print(lines[-1])
    eng.close()
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
