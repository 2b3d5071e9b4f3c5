#!/usr/bin/env python3
"""Cost of lifting one frame's detections to 3-D points from a LiDAR sweep, device call against the host route; prints ONE JSON
line and writes it to profiles/r04/lidar_latency.txt.

The sweep is synthetic: 128 rings x 1024 azimuth steps = 131 072 points of 16 bytes (x, y, z, intensity) in firing order (all rings
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
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
CAM = (1000.0, 1000.0, 959.5, 539.5)
# LiDAR x forward, y left, z up -> camera x right, y down, z forward; the LiDAR 0.3 m above and 0.1 m behind the camera
LIDAR_TO_CAM = (0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.3, 1.0, 0.0, 0.0, -0.1)
GROUND = -0.6          # LiDAR frame, metres


def synthetic_sweep(n_points, seed):
    """[n, 4] float32 (x, y, z, intensity) in firing order."""
    rings = 128
    steps = n_points // rings
    rng = np.random.RandomState(seed)
    az = np.repeat(np.arange(steps) * (2 * np.pi / steps), rings)
    el = np.tile(np.deg2rad(np.linspace(-25.0, 15.0, rings)), steps)
    reach = np.where(el < 0, np.minimum(GROUND / np.sin(np.minimum(el, -1e-6)), 60.0), 60.0) + rng.normal(0.0, 0.01, az.size)
    xyz = np.stack([reach * np.cos(el) * np.cos(az), reach * np.cos(el) * np.sin(az), reach * np.sin(el)], axis=1)
    out = np.concatenate([xyz, rng.uniform(0, 255, (az.size, 1))], axis=1).astype(np.float32)
    return np.concatenate([out, np.zeros((n_points - len(out), 4), dtype=np.float32)])


def cone_boxes(n, seed):
    """DET_DTYPE records: cones of 0.23 x 0.33 m on the ground, 3 .. 40 m ahead, across the image."""
    from unina_yolo_dla_amd.engine import DET_DTYPE
    rng = np.random.RandomState(seed)
    z = rng.uniform(3.0, 40.0, n)
    x = rng.uniform(-0.9, 0.9, n) * z * (CAM[2] / CAM[0])
    foot = 0.3 - GROUND                                        # the ground in the camera frame: y down
    u, v_foot = CAM[0] * x / z + CAM[2], CAM[1] * foot / z + CAM[3]
    half_w, height = 0.5 * CAM[0] * 0.23 / z, CAM[1] * 0.33 / z
    d = np.zeros(n, dtype=DET_DTYPE)
    d["x1"], d["x2"], d["y1"], d["y2"] = u - half_w, u + half_w, v_foot - height, v_foot
    d["confidence"] = np.sort(rng.uniform(0.3, 0.99, n))[::-1]
    d["class_id"] = rng.randint(0, 4, n)
    d["valid"] = 1
    return d


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
    words = np.zeros(8 + 8 * engine.MAX_DETECTIONS, dtype=np.int32)
    words[0] = len(dets)
    words[8:8 + 8 * len(dets)] = dets.view(np.int32).reshape(-1)
    buf, cloud = torch.from_numpy(words).cuda(), torch.from_numpy(sweep).cuda()
    loc = localize.DeviceLidarLocator(max_points=args.points, max_width=W, max_height=H)

    def call():
        loc.update_from_buffer(buf, cloud, LIDAR_TO_CAM, CAM, W, H, par)

    def median_ms(fn, reps):
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            times.append(time.perf_counter() - t0)
        return out, float(np.median(times) * 1e3)

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

    for _ in range(args.warmup):
        call()
    windows = []
    for _ in range(3):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.reps):
            call()
        stop.record()
        torch.cuda.synchronize()
        windows.append(start.elapsed_time(stop) / args.reps)
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
