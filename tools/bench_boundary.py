#!/usr/bin/env python3
"""Cost of one boundary call (unina_boundary_async, csrc/boundary.hip: a memset of the header and one launch), beside the tracker's
launch on the same table and beside the host route; prints ONE JSON line and writes it to profiles/r04/boundary_latency.txt.

Three scenes:
  * typical : the oval of tests/boundary_cases.py -- 36 confirmed cones per side, 20 confirmed tracks of a third class -- plus 58
              tracks of the two classes that are not confirmed yet: 150 live tracks in random slots, both chains 36 links;
  * full    : 960 candidates of the left class along a spiral and 64 of the right class along a second one 3 m inside it, every
              slot of the table live: two full chains of 64 links over 960 / 64 list entries and a 64 x 64 ladder of 127 rungs
              (1024 candidates of ONE class leave no slot for the other side: tests/boundary_cases.py has that table);
  * empty   : an empty table.
Per scene:
  * kernel_ms: HIP events around the memset and the launch (dispatch included), median over `--reps` calls (the call is
    stateless: the same call is repeated);
  * track_kernel_ms: the same around one tracker update with the identity pose whose records are the table's own live points, the
    table put back before each repetition by a device copy outside the events;
  * host_read_ms / host_numpy_ms: the host route a node would otherwise take -- unina_track_read (a synchronisation and the copy
    of the header and the 32 KB of slots) and boundary.boundary_numpy on them -- median of `--host-reps` runs.
Asserts that header and points equal boundary_numpy's, byte for byte, before printing.

    python tools/bench_boundary.py [--reps 50] [--host-reps 5]
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
    import boundary_cases as bc
    import pose_cases as pc
    c, n = bc.oval_case(0, 1 / 3)
    rng = np.random.RandomState(7)
    tab = bc.Table()
    tab.t[:] = c["tracks"]
    tab.next_id = 3001
    free = np.nonzero(tab.t["id"] == 0)[0]
    young = np.stack([rng.uniform(-35, 35, 58), rng.uniform(-20, 20, 58)], axis=1)
    tab.add(young[:29], bc.LEFT, hits=1, slots=free[:29]).add(young[29:], bc.RIGHT, hits=2, slots=free[29:58])
    typical = dict(c, name="typical", tracks=tab.t)
    slots = rng.permutation(bc.MAXD)
    full = bc.call("full", bc.Table().add(bc.spiral(960, r0=8.0), bc.LEFT, slots=slots[:960]).add(bc.spiral(64, r0=5.0), bc.RIGHT, slots=slots[960:]),
                   step_gate=3.0, pose=pc.yaw_pose(0.0, -1.0, -6.5))
    return [typical, full, bc.call("empty", bc.Table())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "boundary_latency.txt"))
    args = ap.parse_args()
    import torch
    import boundary_cases as bc
    import track_cases as tc
    from records import padded_words
    from unina_yolo_dla_amd import boundary, engine, tracking

    def words(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1).copy()).cuda()

    trk = tracking.DeviceTracker()
    trk.reset()
    torch.cuda.synchronize()
    slots_at, header_at = trk.buffers()
    table = engine.device_view(header_at, 32 + 32 * 1024)
    find = boundary.DeviceBoundaryFinder(trk)
    out = {"reps": args.reps, "scenes": {}}
    for c in scenes():
        name = c["name"]
        want = bc.run_twin(c)
        live = c["tracks"][c["tracks"]["id"] != 0]
        state = tracking.new_state()
        state["tracks"] = c["tracks"]
        state["header"]["n_live"] = len(live)
        state["header"]["next_id"] = int(c["tracks"]["id"].max()) + 1
        saved = torch.from_numpy(np.concatenate([state["header"].view(np.uint8), np.ascontiguousarray(c["tracks"]).view(np.uint8)])).cuda()
        f = tc.frame(np.stack([live["x"], live["y"], live["z"]], axis=1), cls=live["class_id"], gate=0.5, class_aware=1, confirm_hits=3, max_missed=3)
        d_dets, d_cones = words(padded_words(f["dets"], 8 * 1024)), words(padded_words(f["cones"], 8 * 1024))
        d_count = torch.tensor([f["count"]], dtype=torch.int32, device="cuda")
        table.copy_(saved)
        times, track_times = [], []
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            find.find_async(c["params"])
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop))
        header, points = find.read()
        assert header.tobytes() == want[0].tobytes(), f"{name}: header differs: {header} {want[0]}"
        assert points.tobytes() == want[1].tobytes(), f"{name}: points differ"
        want_state, _ = tracking.update_numpy(state, f["dets"], f["count"], f["cones"], f["params"])
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            table.copy_(saved)
            start.record()
            trk.update_async(d_dets, d_count, d_cones, f["params"])
            stop.record()
            torch.cuda.synchronize()
            track_times.append(start.elapsed_time(stop))
        t_header, t_tracks = trk.read()
        assert t_header.tobytes() == want_state["header"].tobytes() and t_tracks.tobytes() == want_state["tracks"].tobytes(), f"{name}: table differs"
        table.copy_(saved)
        (_, h_tracks), read_ms = median_ms(trk.read, args.host_reps)
        assert h_tracks.tobytes() == np.ascontiguousarray(c["tracks"]).tobytes()
        _, numpy_ms = median_ms(lambda: boundary.boundary_numpy(h_tracks, None, c["params"]), args.host_reps)
        h = want[0][0]
        out["scenes"][name] = {"live": int(len(live)), "candidates": h["n_candidates"].tolist(), "chain": h["n_chain"].tolist(), "end": h["end"].tolist(),
                               "centre": int(h["n_centre"]), "wide": int(h["n_wide"]),
                               "kernel_ms": float(np.median(times)), "kernel_ms_min": float(np.min(times)),
                               "track_kernel_ms": float(np.median(track_times)), "track_kernel_ms_min": float(np.min(track_times)),
                               "track_n_matched": int(want_state["header"]["n_matched"][0]),
                               "host_read_ms": read_ms, "host_numpy_ms": numpy_ms, "host_ms": read_ms + numpy_ms}
    trk.close()
    out["note"] = ("kernel_ms: HIP events around the header's memset and the single launch (dispatch included), median of `reps` repetitions "
                   "of the same stateless call; track_kernel_ms: the same around one tracker update with the identity pose whose records are "
                   "the table's own live points, the table restored before each; host_*: unina_track_read (synchronisation + copy of the "
                   "table) + boundary.boundary_numpy, median of the host reps")
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
