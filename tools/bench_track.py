#!/usr/bin/env python3
"""Cost of one tracker update (unina_track_update_async, csrc/track.hip), device launch against the host route; prints ONE JSON
line and writes it to profiles/r04/track_latency.txt.

Three scenes, each a table built by one set-up update from a reset, then the update that is timed:
  * typical : 150 live tracks, 60 records (50 near a track, 10 new);
  * full    : 1024 live tracks on a 1 m grid, 1024 records jittered by up to 0.5 m at a gate of 1.2 m, so every record is gated to
              several slots;
  * chain64 : 64 tracks and 64 records alternating on a line with shrinking gaps: one pair per round, 64 rounds.
Per scene:
  * host_d2h_ms / host_numpy_ms: the host route a node would otherwise take -- both record arrays (records and cones, 32 KB each)
    copied to the host and tracking.update_numpy on them -- median of `--host-reps` runs;
  * kernel_ms: HIP events around the ONE timed launch (dispatch included), median over `--reps` repetitions of reset, set-up
    update, timed update (an update changes the table, so the same launch cannot simply be repeated).
Asserts that header, table and assign equal update_numpy's, byte for byte, before printing.

    python tools/bench_track.py [--reps 50] [--host-reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import median_ms  # noqa: E402


def records(points, conf=0.9):
    from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DET_DTYPE
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    dets, cones = np.zeros(1024, dtype=DET_DTYPE), np.zeros(1024, dtype=CONE3D_DTYPE)
    m = len(pts)
    dets["confidence"][:m], dets["valid"][:m] = conf, 1
    cones["x"][:m], cones["y"][:m], cones["z"][:m] = pts.T
    cones["valid"][:m] = 1
    return dets, cones, m


def scenes():
    rng = np.random.RandomState(3)
    field = np.concatenate([rng.uniform(-30, 30, (150, 2)), np.zeros((150, 1))], axis=1)
    seen = field[rng.permutation(150)[:50]] + rng.normal(0, 0.02, (50, 3))
    new = np.concatenate([rng.uniform(40, 60, (10, 2)), np.zeros((10, 1))], axis=1)
    i = np.arange(1024)
    grid = np.stack([i % 32, i // 32, np.full(1024, 5)], axis=1).astype(np.float64)
    jitter = rng.uniform(-0.5, 0.5, (1024, 3)) * [1, 1, 0]
    gaps = 0.5 - 0.003 * np.arange(127)
    line = np.zeros((128, 3))
    line[:, 0] = np.concatenate([[0.0], np.cumsum(gaps)])
    return [("typical", 0.5, field, np.concatenate([seen, new])), ("full", 1.2, grid, grid + jitter),
            ("chain64", 0.6, line[0::2], line[1::2])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "track_latency.txt"))
    args = ap.parse_args()
    import torch
    from unina_yolo_dla_amd import tracking
    trk = tracking.DeviceTracker()
    out = {"reps": args.reps, "scenes": {}}
    for name, gate, setup_pts, timed_pts in scenes():
        par = tracking.make_params(gate=gate, alpha=0.5, birth_confidence=0.3, class_aware=1, confirm_hits=2, max_missed=2)
        setup, timed = records(setup_pts), records(timed_pts)

        def device(frame):
            dets, cones, m = frame
            return (torch.from_numpy(dets.view(np.int32)).cuda(), torch.tensor([m], dtype=torch.int32, device="cuda"),
                    torch.from_numpy(cones.view(np.int32)).cuda())
        d_setup, d_timed = device(setup), device(timed)
        state, _ = tracking.update_numpy(tracking.new_state(), setup[0], setup[2], setup[1], par)
        want, want_assign = tracking.update_numpy(state, timed[0], timed[2], timed[1], par)

        times = []
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            trk.reset()
            trk.update_async(*d_setup, par)
            start.record()
            trk.update_async(*d_timed, par)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop))
        header, tracks = trk.read()
        assert header.tobytes() == want["header"].tobytes() and tracks.tobytes() == want["tracks"].tobytes(), f"{name}: table differs"
        assert trk.assign.cpu().numpy().tobytes() == want_assign.tobytes(), f"{name}: assign differs"

        def d2h():
            torch.cuda.synchronize()
            return d_timed[0].cpu().numpy(), int(d_timed[1].cpu()[0]), d_timed[2].cpu().numpy()
        (h_dets, h_count, h_cones), d2h_ms = median_ms(d2h, args.host_reps)
        from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DET_DTYPE
        _, numpy_ms = median_ms(lambda: tracking.update_numpy(state, h_dets.view(DET_DTYPE), h_count, h_cones.view(CONE3D_DTYPE), par),
                                 args.host_reps)
        h = want["header"][0]
        out["scenes"][name] = {"live_before": int(state["header"]["n_live"][0]), "records": timed[2], "gate": gate,
                               "n_matched": int(h["n_matched"]), "n_born": int(h["n_born"]), "n_dropped": int(h["n_dropped"]),
                               "kernel_ms": float(np.median(times)), "kernel_ms_min": float(np.min(times)), "host_d2h_ms": d2h_ms,
                               "host_numpy_ms": numpy_ms, "host_ms": d2h_ms + numpy_ms}
    trk.close()
    out["note"] = ("kernel_ms: HIP events around the single timed launch (dispatch included), median of `reps` repetitions of reset + "
                   "set-up update + timed update; host_*: D2H of both record arrays + tracking.update_numpy, median of the host reps")
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
