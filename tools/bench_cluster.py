#!/usr/bin/env python3
"""Cost of clustering one LiDAR sweep into cone candidates, device call against the host twin, against the ground stage's call on
the same cloud and against the HBM floor counted from the shapes; prints ONE JSON line per cloud size and writes them to
profiles/r04/cluster_latency.txt.

The sweep is tools/bench_ground.py's (128 rings over 360 degrees in firing order, 16-byte points, a flat ground with 1 cm of noise,
one point in 40 lifted by 0.05 .. 0.5 m). The grid is 512 x 512 cells of 0.1 m around the LiDAR. Per size (30 000, 120 000 and
260 000 points):
  * host_numpy_ms: cluster.cluster_numpy on the host copy of the RAW sweep (vectorised numpy), median of `--host-reps` runs;
  * call_ms: one unina_cluster_async call on the raw sweep -- the heavy case: every ring of the road is a component -- (two
    memsets + eleven kernels), HIP events around `--reps` calls enqueued back to back (dispatch included), after `--warmup` calls;
    three such windows, all printed, the median reported;
  * ground_call_ms: unina_ground_filter_async on the same cloud in the same process (its own 256 x 256 grid of 0.5 m), timed the same way;
  * chain_call_ms: the ground filter and the clusterer on its output, back to back: the use the stage is made for;
  * hbm_floor_ms: the bytes the memsets and the kernels read and write on the raw sweep, counted from the shapes below, over
    6.3 TB/s (every buffer of a call fits the 256 MiB Infinity Cache, so this is a floor for data that came from HBM, not a
    prediction).
Asserts that the device bytes equal the twin's before and after the timed windows, on the raw sweep and on the chain.

    python tools/bench_cluster.py [--points 30000 120000 260000] [--reps 200] [--warmup 20] [--host-reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_ground import GRID as GROUND_GRID, HBM_BYTES_PER_S, LIDAR_TO_LEVEL, sweep_with_objects  # noqa: E402
from benchlib import median_ms, windows_ms  # noqa: E402

GRID = dict(x_min=-25.6, y_min=-25.6, cell=0.1, nx=512, ny=512, min_points=5, max_points=300, min_height=0.1, max_height=0.45, max_width=0.4,
            confidence=0.9, class_id=0)


def counted_bytes(n, stride, hdr, nx, ny):
    """What one call moves, from the shapes: csrc/cluster.hip's kernels in their order."""
    cells, in_grid, occupied, comps = nx * ny, int(hdr["n_in_grid"]), int(hdr["n_cells"]), int(hdr["n_components"])
    cell_blocks, comp_blocks = (cells + 1023) // 1024, (min(n, cells) + 1023) // 1024
    point = n * min(stride, 16)                                 # 16 bytes, or 12 where the loads are dwords
    return {"memset": 4 * cells + 32,
            "mark": point + 4 * in_grid,
            "label": 4 * cells + 4 * cells,
            "merge": 4 * cells,                                     # at most: only the cells on a tile border are read
            "flatten": 4 * cells + 4 * occupied + 4 * cell_blocks,
            "scan": 8 * cell_blocks + 8 * comp_blocks + 32,
            "rank": 4 * cells + 4 * cell_blocks + (4 + 48 + 4) * comps,
            "cells": 4 * cells + 4 * occupied,
            "sums": point + 8 * in_grid + 4 * n,
            "finish": (48 + 48) * comps + 4 * comp_blocks,
            "emit": 4 * comps + 4 * comp_blocks + 2 * 32 * 1024}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[30000, 120000, 260000])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--commit", default="", help="what the run was made on; stored in every line")
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "cluster_latency.txt"))
    args = ap.parse_args()
    import torch
    from unina_yolo_dla_amd import cluster, ground
    if not torch.cuda.is_available():
        raise SystemExit("bench_cluster.py measures on the GPU: no device is visible")
    lines = []
    for n in args.points:
        sweep = sweep_with_objects(n, 4321)
        cloud = torch.from_numpy(sweep).cuda()
        filt = ground.DeviceGroundFilter(max_points=n)
        clus = cluster.DeviceClusterer(max_points=n)

        want, numpy_ms = median_ms(lambda: cluster.cluster_numpy(sweep, LIDAR_TO_LEVEL, GRID), args.host_reps)
        kept = ground.ground_numpy(sweep, LIDAR_TO_LEVEL, GROUND_GRID)["out"]
        want_chain, chain_numpy_ms = median_ms(lambda: cluster.cluster_numpy(kept, LIDAR_TO_LEVEL, GRID), args.host_reps)

        def same_as(twin):
            header, dets, cones, count = clus.read()
            return (header.tobytes() == twin["header"].tobytes() and dets.tobytes() == twin["dets"].tobytes()
                    and cones.tobytes() == twin["cones"].tobytes() and count.tobytes() == twin["count"].tobytes()
                    and clus.read_components().tobytes() == twin["components"].tobytes()
                    and clus.read_point_components().tobytes() == twin["point_component"].tobytes())

        def call():
            clus.cluster_async(cloud, LIDAR_TO_LEVEL, GRID)

        def ground_call():
            return filt.filter_async(cloud, LIDAR_TO_LEVEL, GROUND_GRID)

        def chain_call():
            clus.cluster_async(ground_call(), LIDAR_TO_LEVEL, GRID)

        call()
        assert same_as(want), "device bytes differ from cluster_numpy's"
        call_w = windows_ms(torch, call, args.reps, args.warmup)
        assert same_as(want), "device bytes differ after the timed windows"
        ground_w = windows_ms(torch, ground_call, args.reps, args.warmup)
        chain_w = windows_ms(torch, chain_call, args.reps, args.warmup)
        assert same_as(want_chain), "the chained result differs from cluster_numpy's on ground_numpy's output"
        filt.close()
        clus.close()

        hdr, chain_hdr = want["header"][0], want_chain["header"][0]
        moved = counted_bytes(n, 16, hdr, GRID["nx"], GRID["ny"])
        total = int(sum(moved.values()))
        call_ms = float(np.median(call_w))
        out = {"commit": args.commit, "points": int(n), "stride": 16, "grid": [GRID["nx"], GRID["ny"]], "header": [int(v) for v in hdr.tolist()],
               "chain_header": [int(v) for v in chain_hdr.tolist()], "reps": args.reps, "warmup": args.warmup, "host_numpy_ms": numpy_ms,
               "host_numpy_chain_ms": chain_numpy_ms, "call_ms": call_ms, "call_ms_windows": call_w,
               "ground_call_ms": float(np.median(ground_w)), "ground_call_ms_windows": ground_w, "chain_call_ms": float(np.median(chain_w)),
               "chain_call_ms_windows": chain_w, "counted_bytes": moved, "counted_bytes_total": total,
               "hbm_floor_ms": total / HBM_BYTES_PER_S * 1e3, "floor_over_call": total / HBM_BYTES_PER_S * 1e3 / call_ms,
               "note": "call_ms: HIP events around `reps` unina_cluster_async calls on the RAW sweep (2 memsets + 11 kernels each) enqueued back "
                       "to back, dispatch included; median of three windows. ground_call_ms, chain_call_ms: the same for "
                       "unina_ground_filter_async on the raw cloud and for filter + clusterer. header: n_points, n_in_grid, n_cells, "
                       "n_components, n_cones, n_written, n_dropped, 0 of the raw sweep, chain_header of the filtered one. hbm_floor_ms: "
                       "counted bytes over 6.3 TB/s. host_numpy_ms: median wall clock of cluster_numpy on the raw sweep, "
                       "host_numpy_chain_ms on the filtered one"}
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
