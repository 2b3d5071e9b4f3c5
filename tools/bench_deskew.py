#!/usr/bin/env python3
"""Cost of de-skewing one LiDAR sweep, device call against the host twin, against the ground filter's call on the same cloud and
against the HBM floor counted from the shapes; prints ONE JSON line per cloud size and writes them to
profiles/r04/deskew_latency.txt.

The sweep is tools/bench_lidar.py's (tools/benchlib.py): 128 rings over 360 degrees in firing order, 16-byte points (x, y, z,
intensity); the time of a point is its place in the firing order over 0.1 s, a float32 plane of its own; the intensity is carried.
The vehicle corners at 15 m/s and 1.5 rad/s; 11 keys of that motion, t_ref = the end of the sweep. Per size (30 000, 120 000 and
260 000 points):
  * host_numpy_ms: deskew.table_numpy + deskew.deskew_numpy on the host copy (vectorised numpy; the interpreter's cost, not a tuned
    implementation's), median of `--host-reps` runs;
  * call_ms: one unina_deskew_async call (the float64 table on the host, one memset, one kernel), HIP events around `--reps` calls
    enqueued back to back (dispatch included), after `--warmup` calls; three such windows, all printed, the median reported;
  * ground_call_ms: unina_ground_filter_async on the same cloud in the same process, timed the same way;
  * chain_call_ms: the de-skew and the ground filter on its output, back to back;
  * hbm_floor_ms: stride + 4 + 16 bytes per point (the point, its time, the entry written) and the header, over 6.3 TB/s (the
    achievable HBM rate; every buffer of a call fits the 256 MiB Infinity Cache, so this is a floor for data that came from HBM,
    not a prediction).
Asserts that the device bytes equal the twin's before and after the timed windows.

    python tools/bench_deskew.py [--points 30000 120000 260000] [--reps 2000] [--warmup 50] [--host-reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import GROUND, median_ms, synthetic_sweep, windows_ms  # noqa: E402

LIDAR_TO_LEVEL = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, -GROUND)     # the ground is z = 0
GRID = dict(x_min=-64.0, y_min=-64.0, cell=0.5, nx=256, ny=256, z_lo=-0.3, z_hi=0.3, rise=0.05, band=0.05, max_height=0.6, reach=2,
            keep_unknown=0)
HBM_BYTES_PER_S = 6.3e12
SWEEP_S, SPEED, YAW_RATE, KEYS = 0.1, 15.0, 1.5, 11


def arc_poses(n_keys):
    """n_keys equally spaced keys (t, qw, qx, qy, qz, px, py, pz) of a constant-twist arc in the plane over the sweep."""
    t = np.linspace(0.0, SWEEP_S, n_keys)
    th = YAW_RATE * t
    zero = np.zeros_like(t)
    return np.stack([t, np.cos(th / 2), zero, zero, np.sin(th / 2), SPEED / YAW_RATE * np.sin(th), SPEED / YAW_RATE * (1.0 - np.cos(th)), zero], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[30000, 120000, 260000])
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "deskew_latency.txt"))
    args = ap.parse_args()
    import torch
    from unina_yolo_dla_amd import deskew, ground
    if not torch.cuda.is_available():
        raise SystemExit("bench_deskew.py measures on the GPU: no device is visible")
    poses = arc_poses(KEYS)
    lines = []
    for n in args.points:
        sweep = synthetic_sweep(n, 4321)
        stamps = (np.arange(n, dtype=np.float64) * (SWEEP_S / n)).astype(np.float32)
        cloud, times = torch.from_numpy(sweep).cuda(), torch.from_numpy(stamps).cuda()
        carry = np.ascontiguousarray(sweep[:, 3]).view(np.uint32)
        dsk = deskew.DeviceDeskewer(max_points=n)
        filt = ground.DeviceGroundFilter(max_points=n)

        want, numpy_ms = median_ms(lambda: deskew.deskew_numpy(sweep, stamps, deskew.TIME_F32_S, carry, deskew.table_numpy(poses, 0.0, SWEEP_S)),
                                   args.host_reps)

        def same_as_twin():
            header, out = dsk.read()
            return out.tobytes() == want["out"].tobytes() and header.tobytes() == want["header"].tobytes()

        def call():
            return dsk.deskew_async(cloud, times, poses, 0.0, SWEEP_S, carry_offset=12)

        def ground_call():
            filt.filter_async(cloud, LIDAR_TO_LEVEL, GRID)

        def chain_call():
            filt.filter_async(call(), LIDAR_TO_LEVEL, GRID)

        call()
        assert same_as_twin(), "device bytes differ from deskew_numpy's"
        call_w = windows_ms(torch, call, args.reps, args.warmup)
        assert same_as_twin(), "device bytes differ after the timed windows"
        ground_w = windows_ms(torch, ground_call, args.reps, args.warmup)
        chain_w = windows_ms(torch, chain_call, args.reps, args.warmup)
        g_header, g_out = filt.read()
        g_want = ground.ground_numpy(want["out"], LIDAR_TO_LEVEL, GRID)
        assert g_out.tobytes() == g_want["out"].tobytes() and g_header.tobytes() == g_want["header"].tobytes(), "the chained filter differs from ground_numpy's on the twin's output"
        filt.close()

        hdr = want["header"][0]
        total = n * (16 + 4 + 16) + 2 * 32                    # the point, its time, the entry written; the header's memset and atomics
        call_ms = float(np.median(call_w))
        out = {"points": int(n), "stride": 16, "keys": KEYS, "times": "float32 plane", "carry_offset": 12, "n_moved": int(hdr["n_moved"]),
               "max_shift_m": float(np.sqrt(np.array([hdr["max_shift2_bits"]], dtype=np.uint32).view(np.float32)[0])), "reps": args.reps,
               "warmup": args.warmup, "host_numpy_ms": numpy_ms, "call_ms": call_ms, "call_ms_windows": call_w,
               "ground_call_ms": float(np.median(ground_w)), "ground_call_ms_windows": ground_w, "chain_call_ms": float(np.median(chain_w)),
               "chain_call_ms_windows": chain_w, "counted_bytes_total": total, "hbm_floor_ms": total / HBM_BYTES_PER_S * 1e3,
               "floor_over_call": total / HBM_BYTES_PER_S * 1e3 / call_ms, "counted_bytes_per_s": total / (call_ms * 1e-3),
               "note": "call_ms: HIP events around `reps` unina_deskew_async calls (the float64 table on the host, 1 memset + 1 kernel each) "
                       "enqueued back to back, dispatch included; median of three windows. ground_call_ms, chain_call_ms: the same for "
                       "unina_ground_filter_async on the raw cloud and for de-skew + filter. hbm_floor_ms: (stride + 4 + 16) bytes per point "
                       "over 6.3 TB/s. host_numpy_ms: median wall clock"}
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
