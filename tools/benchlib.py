"""What the latency tools of the stages behind the frame share: the median wall clock of a host step, the HIP-event windows
around a device call, the detection word buffer, and the synthetic LiDAR sweep with its cone-sized records
(tools/bench_lidar.py, tools/bench_ground.py)."""
import time

import numpy as np


def median_ms(fn, reps):
    """(fn's last result, the median wall clock of `reps` runs in ms)."""
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, float(np.median(times) * 1e3)


def window_ms(torch, fn, reps):
    """ms per call of one window: `reps` calls enqueued back to back between two HIP events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def windows_ms(torch, fn, reps, warmup):
    """Three such windows after `warmup` calls."""
    for _ in range(warmup):
        fn()
    return [window_ms(torch, fn, reps) for _ in range(3)]


def wall_ms(torch, fn, reps):
    """ms per call by the wall clock around `reps` calls, the device idle at both ends."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def det_words(dets):
    """Engine.infer_async's int32 buffer on the host: word 0 = count, records from word 8, zeros behind them."""
    from unina_yolo_dla_amd.engine import MAX_DETECTIONS
    words = np.zeros(8 + 8 * MAX_DETECTIONS, dtype=np.int32)
    words[0] = len(dets)
    words[8:8 + 8 * len(dets)] = dets.view(np.int32).reshape(-1)
    return words


# ---------------------------------------------------------------- the synthetic sweep
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
