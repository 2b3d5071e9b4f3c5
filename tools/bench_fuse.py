#!/usr/bin/env python3
"""Cost of one fusion launch (unina_fuse_async, csrc/fuse.hip), device launch against the host route and against the tracker's
launch on the same records; prints ONE JSON line and writes it to profiles/r04/fuse_latency.txt.

Three scenes, each one pair of record lists:
  * typical : 60 camera records and 80 LiDAR cones, 50 of them under a box;
  * full    : 1024 boxes of 40 pixels on a 16-pixel grid and 1024 cones jittered by up to 6 pixels around the grid, so every box gates
              several cones;
  * chain64 : 64 boxes and 64 cones alternating on a row with shrinking gaps: one pair per round, 64 rounds.
Per scene:
  * host_d2h_ms / host_numpy_ms: the host route a node would otherwise take -- both branches' record arrays (four arrays of 32 KB
    and two counts) copied to the host and fusion.fuse_numpy on them -- median of `--host-reps` runs;
  * kernel_ms: HIP events around the ONE launch (dispatch included), median over `--reps` repetitions (the call is stateless: the
    same launch is simply repeated);
  * track_kernel_ms: the same around one unina_track_update_async on the fused records, whose table a set-up update filled from
    the same records (every record gated to its own track): the launch the fusion kernel is shaped after.
Asserts that every output equals fuse_numpy's, byte for byte, before printing.

    python tools/bench_fuse.py [--reps 50] [--host-reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import median_ms  # noqa: E402

CAM = (256.0, 256.0, 256.0, 192.0)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def camera(u, v, half):
    from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DET_DTYPE
    dets, cones = np.zeros(1024, dtype=DET_DTYPE), np.zeros(1024, dtype=CONE3D_DTYPE)
    m = len(u)
    dets["x1"][:m], dets["y1"][:m], dets["x2"][:m], dets["y2"][:m] = u - half, v - half, u + half, v + half
    dets["confidence"][:m], dets["class_id"][:m], dets["valid"][:m] = 0.9, 1, 1
    return dets, cones, m


def lidar(u, v, z=4.0):
    from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DET_DTYPE
    dets, cones = np.zeros(1024, dtype=DET_DTYPE), np.zeros(1024, dtype=CONE3D_DTYPE)
    m = len(u)
    cones["x"][:m], cones["y"][:m], cones["z"][:m] = (u - CAM[2]) * z / CAM[0], (v - CAM[3]) * z / CAM[1], z
    cones["n_valid"][:m], cones["n_samples"][:m], cones["valid"][:m] = 12, 12, 1
    dets["confidence"][:m], dets["class_id"][:m], dets["valid"][:m] = 0.5, 9, 1
    return dets, cones, m


def scenes():
    rng = np.random.RandomState(3)
    cu, cv = rng.uniform(20, 1000, 60), rng.uniform(20, 700, 60)
    lu = np.concatenate([cu[:50] + rng.normal(0, 1.5, 50), rng.uniform(20, 1000, 30)])
    lv = np.concatenate([cv[:50] + rng.normal(0, 1.5, 50), rng.uniform(800, 900, 30)])
    i = np.arange(1024)
    gu, gv = (i % 32) * 16.0 + 8.0, (i // 32) * 16.0 + 8.0
    gaps = 8.0 - 0.03125 * np.arange(127)
    pos = 100.0 + np.concatenate([[0.0], np.cumsum(gaps)])
    row = np.full(64, 192.0)
    return [("typical", camera(cu, cv, 8.0), lidar(lu, lv)),
            ("full", camera(gu, gv, 20.0), lidar(gu + rng.uniform(-6, 6, 1024), gv + rng.uniform(-6, 6, 1024))),
            ("chain64", camera(pos[0::2], row, 8.5), lidar(pos[1::2], row))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "fuse_latency.txt"))
    args = ap.parse_args()
    import torch
    from unina_yolo_dla_amd import fusion, tracking
    from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DET_DTYPE
    fuser, trk = fusion.DeviceFuser(), tracking.DeviceTracker()
    par = fusion.make_fuse_params(IDENTITY, CAM, lift=0.0, min_depth=0.5, max_depth=50.0, grow=1.0, pad=0.0, range_abs=0.5, range_rel=0.1)
    tpar = tracking.make_params(gate=0.5, alpha=0.5, birth_confidence=0.3, class_aware=0, confirm_hits=2, max_missed=2)
    names = ("header", "dets", "cones", "count", "links", "lidar_slot")
    out = {"reps": args.reps, "scenes": {}}
    for name, cam_side, lidar_side in scenes():
        def device(side):
            dets, cones, m = side
            return (torch.from_numpy(dets.view(np.int32)).cuda(), torch.tensor([m], dtype=torch.int32, device="cuda"),
                    torch.from_numpy(cones.view(np.int32)).cuda())
        d_cam, d_lidar = device(cam_side), device(lidar_side)
        want = fusion.fuse_numpy(cam_side[0], cam_side[2], cam_side[1], lidar_side[0], lidar_side[2], lidar_side[1], par)

        times, track_times = [], []
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fuser.fuse_async(*d_cam, *d_lidar, par)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop))
        got = dict(zip(names, fuser.read()))
        for what in names:
            assert got[what].tobytes() == want[what].tobytes(), f"{name}: {what} differs"
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            trk.reset()
            trk.update_from_buffer(fuser.det_buf, fuser.cones, tpar)
            start.record()
            trk.update_from_buffer(fuser.det_buf, fuser.cones, tpar)
            stop.record()
            torch.cuda.synchronize()
            track_times.append(start.elapsed_time(stop))
        track_header, _ = trk.read()

        def d2h():
            torch.cuda.synchronize()
            return [(d[0].cpu().numpy(), int(d[1].cpu()[0]), d[2].cpu().numpy()) for d in (d_cam, d_lidar)]
        ((cd, cn, cc), (ld, ln, lc)), d2h_ms = median_ms(d2h, args.host_reps)
        _, numpy_ms = median_ms(lambda: fusion.fuse_numpy(cd.view(DET_DTYPE), cn, cc.view(CONE3D_DTYPE), ld.view(DET_DTYPE), ln,
                                                          lc.view(CONE3D_DTYPE), par), args.host_reps)
        h = want["header"][0]
        out["scenes"][name] = {**{n: int(h[n]) for n in h.dtype.names}, "kernel_ms": float(np.median(times)), "kernel_ms_min": float(np.min(times)),
                               "track_kernel_ms": float(np.median(track_times)), "track_n_matched": int(track_header["n_matched"][0]),
                               "host_d2h_ms": d2h_ms, "host_numpy_ms": numpy_ms, "host_ms": d2h_ms + numpy_ms}
    trk.close()
    out["note"] = ("kernel_ms: HIP events around the single launch (dispatch included), median of `reps` repetitions; track_kernel_ms: the same "
                   "around one tracker update on the fused records behind a set-up update with the same records; host_*: D2H of both "
                   "branches' record arrays + fusion.fuse_numpy, median of the host reps")
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
