#!/usr/bin/env python3
"""Cost of lifting one frame's detections to 3-D points from a LiDAR sweep, device call against the host route; prints ONE JSON
line and writes it to profiles/r04/lidar_latency.txt.

The sweep is synthetic (tools/benchlib.py): 128 rings x 1024 azimuth steps = 131 072 points of 16 bytes (x, y, z, intensity) in firing order (all rings
of one azimuth step, then the next step), over 360 degrees, hitting a flat ground 0.6 m below the LiDAR or nothing (60 m). The
camera is 1920 x 1080 with fx = fy = 1000 (88 degrees across), so about a quarter of the sweep projects into the image. The 200
records are cone-sized boxes (a 0.23 x 0.33 m cone at 3 .. 40 m) standing on the ground. Per call:
  * host_d2h_ms / host_numpy_ms / host_h2d_ms: the host route a node would otherwise take -- the records and the cloud copied to
    the host, localize.locate_lidar_numpy (vectorised numpy), the cones copied back for the tracker -- median of `--host-reps` runs;
  * call_ms: one unina_locate_lidar_async call (memset + four kernels), HIP events around `--reps` calls enqueued back to back
    (dispatch included), after `--warmup` calls; three such windows, all printed, the median reported.
Asserts that the device records and pixels equal the twin's, byte for byte, before and after the timed windows.

    python tools/bench_lidar.py [--points 131072] [--records 200] [--reps 200] [--warmup 20] [--host-reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import CAM, H, LIDAR_TO_CAM, W, cone_boxes, det_words, median_ms, synthetic_sweep, windows_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--records", type=int, default=200)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "lidar_latency.txt"))
    args = ap.parse_args()
    import torch
    from unina_yolo_dla_amd import engine, localize
    if not torch.cuda.is_available():
        raise SystemExit("bench_lidar.py measures on the GPU: no device is visible")
    sweep = synthetic_sweep(args.points, 4321)
    dets = cone_boxes(args.records, 99)
    par = localize.make_lidar_params(shrink=0.5, min_depth=0.5, max_depth=45.0, min_valid=2)
    buf, cloud = torch.from_numpy(det_words(dets)).cuda(), torch.from_numpy(sweep).cuda()
    loc = localize.DeviceLidarLocator(max_points=args.points, max_width=W, max_height=H)

    def call():
        loc.update_from_buffer(buf, cloud, LIDAR_TO_CAM, CAM, W, H, par)

    def d2h():
        torch.cuda.synchronize()
        return buf.cpu().numpy(), cloud.cpu().numpy()
    (host_words, host_sweep), d2h_ms = median_ms(d2h, args.host_reps)
    host_dets = host_words[8:].view(engine.DET_DTYPE)

    def on_host():
        pixels = localize.project_lidar_numpy(host_sweep, LIDAR_TO_CAM, CAM, W, H, par.min_depth, par.max_depth)
        return localize.locate_lidar_numpy(host_dets, int(host_words[0]), host_sweep, LIDAR_TO_CAM, CAM, W, H, par, pixels=pixels), pixels
    (want, want_pixels), numpy_ms = median_ms(on_host, args.host_reps)

    def h2d():
        t = torch.from_numpy(want.view(np.uint8)).cuda()
        torch.cuda.synchronize()
        return t
    _, h2d_ms = median_ms(h2d, args.host_reps)

    call()
    got, got_pixels = loc.read(), loc.read_pixels()
    assert got.tobytes() == want.tobytes() and got_pixels.tobytes() == want_pixels.tobytes(), "device records differ from locate_lidar_numpy's"

    windows = windows_ms(torch, call, args.reps, args.warmup)
    after = loc.read()
    assert after.tobytes() == want.tobytes(), "device records differ after the timed windows"
    loc.close()

    cones = got[:len(dets)]
    out = {"points": int(args.points), "stride": 16, "projectable": int((want_pixels["projectable"] == 1).sum()), "image": [W, H],
           "records": int(len(dets)), "located": int((cones["valid"] == 1).sum()), "median_members": int(np.median(cones["n_samples"])),
           "max_members": int(cones["n_samples"].max()), "reps": args.reps, "warmup": args.warmup, "cloud_bytes": int(sweep.nbytes),
           "host_d2h_ms": d2h_ms, "host_numpy_ms": numpy_ms, "host_h2d_ms": h2d_ms, "host_ms": d2h_ms + numpy_ms + h2d_ms,
           "call_ms": float(np.median(windows)), "call_ms_windows": windows,
           "note": "call_ms: HIP events around `reps` unina_locate_lidar_async calls (memset + 4 kernels each) enqueued back to back, dispatch "
                   "included; median of three windows. host_*: median wall clock of `host-reps` runs, each ending in a synchronise"}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
