#!/usr/bin/env python3
"""Cost of stripping the ground from one LiDAR sweep, device call against the host twin, against the locator's call on the same
cloud and against the HBM floor counted from the shapes; prints ONE JSON line per cloud size and writes them to
profiles/r04/ground_latency.txt.

The sweep is tools/bench_lidar.py's (tools/benchlib.py): 128 rings over 360 degrees in firing order, 16-byte points (x, y, z, intensity), a flat
ground 0.6 m below the LiDAR with 1 cm of noise or nothing (60 m); one point in 40 is lifted by 0.05 .. 0.5 m so that there is
something to keep. The grid is 256 x 256 cells of 0.5 m around the LiDAR. Per size (30 000, 120 000 and 260 000 points):
  * host_numpy_ms: ground.ground_numpy on the host copy (vectorised numpy; the interpreter's cost, not a tuned implementation's),
    median of `--host-reps` runs;
  * call_ms: one unina_ground_filter_async call (two memsets + five kernels), HIP events around `--reps` calls enqueued back to
    back (dispatch included), after `--warmup` calls; three such windows, all printed, the median reported;
  * lidar_call_ms: unina_locate_lidar_async on the same cloud in the same process, timed the same way (200 cone-sized records);
  * chain_call_ms: the filter and the locator on its output, back to back;
  * hbm_floor_ms: the bytes the memsets and the five kernels read and write, counted from the shapes below, over 6.3 TB/s (the
    achievable HBM rate; every buffer of a call fits the 256 MiB Infinity Cache, so this is a floor for data that came from HBM,
    not a prediction).
Asserts that the device bytes equal the twin's before and after the timed windows.

    python tools/bench_ground.py [--points 30000 120000 260000] [--reps 200] [--warmup 20] [--host-reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import CAM, GROUND, H, LIDAR_TO_CAM, W, cone_boxes, det_words, median_ms, synthetic_sweep, windows_ms  # noqa: E402

LIDAR_TO_LEVEL = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, -GROUND)     # the ground is z = 0
GRID = dict(x_min=-64.0, y_min=-64.0, cell=0.5, nx=256, ny=256, z_lo=-0.3, z_hi=0.3, rise=0.05, band=0.05, max_height=0.6, reach=2,
            keep_unknown=0)
HBM_BYTES_PER_S = 6.3e12


def sweep_with_objects(n_points, seed):
    sweep = synthetic_sweep(n_points, seed)
    rng = np.random.RandomState(seed + 1)
    lifted = rng.rand(n_points) < 0.025
    sweep[lifted, 2] += rng.uniform(0.05, 0.5, int(lifted.sum())).astype(np.float32)
    return sweep


def counted_bytes(n, stride, n_kept, nx, ny):
    """What one call moves, from the shapes: csrc/ground.hip's kernels in their order."""
    cells, blocks = nx * ny, (n + 1023) // 1024
    return {"memset": 4 * cells + 32,
            "seed": n * min(stride, 16) + 8 * n,                 # the point (16 bytes, or 12 where the loads are dwords), (cell, zl)
            "envelope": 4 * cells + 4 * cells,
            "classify": 8 * n + 4 * n + n + 4 * n + 4 * blocks,      # (cell, zl), g of the cell; label, h, the workgroup's count
            "scan": 8 * blocks + 8,
            "scatter": n + 4 * blocks + 16 * n_kept + 4 * n_kept + 16 * n}   # label, offset; a kept point's words and h; one entry each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[30000, 120000, 260000])
    ap.add_argument("--records", type=int, default=200)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "ground_latency.txt"))
    args = ap.parse_args()
    import torch
    from unina_yolo_dla_amd import ground, localize
    if not torch.cuda.is_available():
        raise SystemExit("bench_ground.py measures on the GPU: no device is visible")
    dets = cone_boxes(args.records, 99)
    buf = torch.from_numpy(det_words(dets)).cuda()
    lpar = localize.make_lidar_params(shrink=0.5, min_depth=0.5, max_depth=45.0, min_valid=2)
    lines = []
    for n in args.points:
        sweep = sweep_with_objects(n, 4321)
        cloud = torch.from_numpy(sweep).cuda()
        filt = ground.DeviceGroundFilter(max_points=n)
        loc = localize.DeviceLidarLocator(max_points=n, max_width=W, max_height=H)

        want, numpy_ms = median_ms(lambda: ground.ground_numpy(sweep, LIDAR_TO_LEVEL, GRID), args.host_reps)

        def same_as_twin():
            header, out = filt.read()
            cellmin, g = filt.read_grids()
            return (out.tobytes() == want["out"].tobytes() and header.tobytes() == want["header"].tobytes()
                    and filt.read_labels().tobytes() == want["labels"].tobytes() and cellmin.tobytes() == want["cellmin"].tobytes()
                    and g.tobytes() == want["ground"].tobytes())

        def call():
            return filt.filter_async(cloud, LIDAR_TO_LEVEL, GRID)

        def lidar_call():
            loc.update_from_buffer(buf, cloud, LIDAR_TO_CAM, CAM, W, H, lpar)

        def chain_call():
            loc.update_from_buffer(buf, call(), LIDAR_TO_CAM, CAM, W, H, lpar)

        call()
        assert same_as_twin(), "device bytes differ from ground_numpy's"
        call_w = windows_ms(torch, call, args.reps, args.warmup)
        assert same_as_twin(), "device bytes differ after the timed windows"
        lidar_w = windows_ms(torch, lidar_call, args.reps, args.warmup)
        chain_w = windows_ms(torch, chain_call, args.reps, args.warmup)
        cones = loc.read()
        want_cones = localize.locate_lidar_numpy(dets, len(dets), want["out"], LIDAR_TO_CAM, CAM, W, H, lpar)
        assert cones.tobytes() == want_cones.tobytes(), "the chained cones differ from locate_lidar_numpy's on the twin's output"
        filt.close()
        loc.close()

        hdr = want["header"][0]
        moved = counted_bytes(n, 16, int(hdr["n_kept"]), GRID["nx"], GRID["ny"])
        total = int(sum(moved.values()))
        call_ms = float(np.median(call_w))
        out = {"points": int(n), "stride": 16, "grid": [GRID["nx"], GRID["ny"]], "reach": GRID["reach"], "n_kept": int(hdr["n_kept"]),
               "n_label": [int(v) for v in hdr["n_label"]], "n_cells_seeded": int(hdr["n_cells_seeded"]), "reps": args.reps,
               "warmup": args.warmup, "host_numpy_ms": numpy_ms, "call_ms": call_ms, "call_ms_windows": call_w,
               "lidar_call_ms": float(np.median(lidar_w)), "lidar_call_ms_windows": lidar_w, "chain_call_ms": float(np.median(chain_w)),
               "chain_call_ms_windows": chain_w, "counted_bytes": moved, "counted_bytes_total": total,
               "hbm_floor_ms": total / HBM_BYTES_PER_S * 1e3, "floor_over_call": total / HBM_BYTES_PER_S * 1e3 / call_ms,
               "note": "call_ms: HIP events around `reps` unina_ground_filter_async calls (2 memsets + 5 kernels each) enqueued back to back, "
                       "dispatch included; median of three windows. lidar_call_ms, chain_call_ms: the same for unina_locate_lidar_async on "
                       "the raw cloud and for filter + locator. hbm_floor_ms: counted bytes over 6.3 TB/s. host_numpy_ms: median wall clock"}
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
