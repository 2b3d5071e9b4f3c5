#!/usr/bin/env python3
"""Cost of one pose estimate (unina_pose_async, csrc/pose.hip: a memset of the header and one launch), beside the tracker's launch
on the same records and beside the host route; prints ONE JSON line and writes it to profiles/r04/pose_latency.txt.

Three scenes:
  * typical : frame 20 of the world sequence with the biased odometry (tests/pose_cases.py): the table the chain of twins has
              built by then, the frame's 60 .. 110 records, the earlier result chained, 4 iterations;
  * full    : 1024 landmarks of one class on a 1 m grid, 1024 records jittered by up to 0.3 m behind a prior wrong by 0.01 rad and
              0.2 m, gate 1.2 m, 8 iterations: every record walks 1024 landmarks eight times;
  * empty   : the typical frame's records against an empty table (TOO_FEW in the first iteration).
Per scene:
  * kernel_ms: HIP events around the memset and the launch (dispatch included), median over `--reps` calls (the call is
    stateless: the same call is repeated);
  * track_kernel_ms: the same around one tracker update with the identity pose on the cones the stage wrote, the table put back
    before each repetition by a device copy outside the events;
  * host_d2h_ms / host_numpy_ms: the host route a node would otherwise take -- records, cones and the table copied to the host and
    pose.pose_numpy on them -- median of `--host-reps` runs.
Asserts that header, result and out cones equal pose_numpy's, byte for byte, before printing.

    python tools/bench_pose.py [--reps 50] [--host-reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from benchlib import median_ms  # noqa: E402


def scenes():
    import pose_cases as pc
    seed, k = 5, 20
    frames, _, incs = pc.world_chain_inputs(seed)
    chain = pc.chain_results(seed)
    dets, cones = pc.padded_frame(frames[k])
    track_par = dict(frames[k]["params"], pose=None)
    typical = dict(dets=dets, cones=cones, count=frames[k]["count"], tracks=chain[k - 1][1]["tracks"], prev=chain[k - 1][0]["result"],
                   params=dict(pc.POSE_PAR, inc=incs[k]))
    rng = np.random.RandomState(3)
    i = np.arange(1024)
    grid = np.stack([i % 32 - 16.0, i // 32 - 16.0, np.zeros(1024)], axis=1)
    truth = pc.yaw_pose(0.3, 2.0, -1.0, 0.5)
    seen = pc.seen_from(grid + rng.uniform(-0.3, 0.3, (1024, 3)) * [1, 1, 0], truth)
    full = pc.call("full", seen, pc.table(grid), inc=pc.compose(truth, pc.yaw_pose(0.01, 0.15, -0.13)), gate=1.2, iterations=8)
    empty = dict(typical, tracks=pc.table(grid[:0]), prev=None, params=dict(pc.POSE_PAR, inc=chain[k][3]))
    return [("typical", typical, track_par), ("full", full, dict(track_par, gate=1.2)), ("empty", empty, track_par)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "pose_latency.txt"))
    args = ap.parse_args()
    import torch
    import pose_cases as pc
    from unina_yolo_dla_amd import engine, pose, tracking
    from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DET_DTYPE

    def words(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1).copy()).cuda()

    trk = tracking.DeviceTracker()
    trk.reset()
    torch.cuda.synchronize()
    slots_at, header_at = trk.buffers()
    table = engine.device_view(header_at, 32 + 32 * 1024)
    est = pose.DevicePoseEstimator.from_tracker(trk)
    out = {"reps": args.reps, "scenes": {}}
    for name, c, track_par in scenes():
        want = pose.pose_numpy(c["dets"], c["count"], c["cones"], c["tracks"], c["prev"], c["params"])
        d_dets, d_count, d_cones = words(c["dets"]), torch.tensor([c["count"]], dtype=torch.int32, device="cuda"), words(c["cones"])
        state = tracking.new_state()
        state["tracks"] = c["tracks"]
        state["header"]["n_live"] = int((c["tracks"]["id"] != 0).sum())
        state["header"]["next_id"] = int(c["tracks"]["id"].max()) + 1
        saved = torch.from_numpy(np.concatenate([state["header"].view(np.uint8), np.ascontiguousarray(c["tracks"]).view(np.uint8)])).cuda()
        d_prev = None if c["prev"] is None else words(c["prev"])
        table.copy_(saved)
        times, track_times = [], []
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            est.estimate_async(d_dets, d_count, d_cones, c["params"], prev=d_prev, result=est.result)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop))
        header, result, moved = est.read()
        assert header.tobytes() == want["header"].tobytes(), f"{name}: header differs: {header} {want['header']}"
        assert result.tobytes() == want["result"].tobytes(), f"{name}: result differs"
        assert pc.canon_cones(moved).tobytes() == pc.canon_cones(want["cones"]).tobytes(), f"{name}: out cones differ"
        want_state, want_assign = tracking.update_numpy(state, c["dets"], c["count"], want["cones"], track_par)
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            table.copy_(saved)
            start.record()
            trk.update_async(d_dets, d_count, est.cones, track_par)
            stop.record()
            torch.cuda.synchronize()
            track_times.append(start.elapsed_time(stop))
        t_header, t_tracks = trk.read()
        assert t_header.tobytes() == want_state["header"].tobytes() and t_tracks.tobytes() == want_state["tracks"].tobytes(), f"{name}: table differs"
        assert trk.assign.cpu().numpy().tobytes() == want_assign.tobytes(), f"{name}: assign differs"

        def d2h():
            torch.cuda.synchronize()
            return d_dets.cpu().numpy(), int(d_count.cpu()[0]), d_cones.cpu().numpy(), saved.cpu().numpy()
        (h_dets, h_count, h_cones, h_table), d2h_ms = median_ms(d2h, args.host_reps)
        _, numpy_ms = median_ms(lambda: pose.pose_numpy(h_dets.view(DET_DTYPE), h_count, h_cones.view(CONE3D_DTYPE),
                                                        h_table[32:].view(tracking.TRACK_DTYPE), c["prev"], c["params"]), args.host_reps)
        h = want["header"][0]
        out["scenes"][name] = {"records": int(h["n_records"]), "usable": int(h["n_usable"]), "landmarks": int(h["n_landmarks"]),
                               "pairs": int(h["n_pairs"]), "iterations": int(h["iterations"]), "status": int(h["status"]),
                               "kernel_ms": float(np.median(times)), "kernel_ms_min": float(np.min(times)),
                               "track_kernel_ms": float(np.median(track_times)), "track_kernel_ms_min": float(np.min(track_times)),
                               "track_n_matched": int(want_state["header"]["n_matched"][0]),
                               "host_d2h_ms": d2h_ms, "host_numpy_ms": numpy_ms, "host_ms": d2h_ms + numpy_ms}
    trk.close()
    out["note"] = ("kernel_ms: HIP events around the header's memset and the single launch (dispatch included), median of `reps` repetitions "
                   "of the same stateless call; track_kernel_ms: the same around one tracker update with the identity pose on the cones "
                   "the stage wrote, the table restored before each; host_*: D2H of the records, the cones and the table + "
                   "pose.pose_numpy, median of the host reps")
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
