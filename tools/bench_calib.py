#!/usr/bin/env python3
"""Cost of INT8 calibration per frame, host collection beside device collection, on one GPU; prints ONE JSON line.

  * host path (the yardstick): wall time of engine.calibrate_amax on `--frames` frames at 640 x 640, graph (A) -- per frame a
    forward, then unina_debug_read_buffer + np.histogram for every fp16 activation buffer;
  * device path: wall time of engine.calibrate_amax_device on the same frames, and its four parts measured one by one:
    forward (wall clock around enqueue + synchronise), the value-count launch (HIP events; GB/s over the bytes it reads),
    the D2H copy of the tables, the host fold (HistogramCalibrator.collect_counts of every row).

Both totals hold the same one-off costs (engine build and load, the final range selection), so their difference is the
collection. The two dicts must be equal before anything is printed.

    python tools/bench_calib.py [--frames 8] [--method percentile|entropy|mse|max] [--size 640 640]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--method", default="percentile", choices=("max", "entropy", "mse", "percentile"))
    ap.add_argument("--size", type=int, nargs=2, default=(640, 640))
    args = ap.parse_args()
    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd import engine, export
    h, w = args.size
    g = u.graph.Graph(in_h=h, in_w=w)
    sd = u.synth.make_state_dict(7, g)
    frames = [u.rng.frame(5000 + i, h, w) for i in range(args.frames)]
    method = None if args.method == "max" else args.method

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    engine.calibrate_amax_device(sd, g, frames[:1])          # warm-up: library load, kernel upload
    host, t_host = wall(lambda: engine.calibrate_amax(sd, g, frames, method=method))
    dev, t_dev = wall(lambda: engine.calibrate_amax_device(sd, g, frames, method=method))
    assert dev == host, "device and host calibration disagree"

    # the device path's parts
    eng = engine.Engine.from_state_dict(sd, g)
    eng.set_fusion(False)
    names = eng.calib_buffer_names()
    b = export.EngineBuilder(sd, g)
    nbytes = sum(2 * bh * bw * bc for (_n, bh, bw, bc, dtype, _f, _s) in b.buffers if dtype == export.BUF_F16)
    out_t = torch.empty((len(names), export.CALIB_BINS), dtype=torch.int32, device="cuda")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cals = [export.HistogramCalibrator() for _ in names]
    parts = {"forward": [], "histogram": [], "d2h": [], "fold": []}
    for rep in range(2):                                     # the first pass over the frames is a warm-up
        for x in frames:
            xd = torch.from_numpy(x).cuda()
            eng.bind_images(xd)
            _, t = wall(eng.enqueue)
            ev0.record()
            eng.calib_counts_async(None, out_t)
            ev1.record()
            torch.cuda.synchronize()
            t_hist = ev0.elapsed_time(ev1) * 1e-3
            tables, t_copy = wall(lambda: out_t.cpu().numpy().view(np.uint32))
            t0 = time.perf_counter()
            for c, row in zip(cals, tables):
                c.collect_counts(row)
            t_fold = time.perf_counter() - t0
            if rep:
                for k, v in zip(parts, (t, t_hist, t_copy, t_fold)):
                    parts[k].append(v)
    eng.close()
    med = {k: float(np.median(v)) for k, v in parts.items()}
    out = {"size": [h, w], "frames": args.frames, "method": args.method, "buffers": len(names), "bytes_per_frame": nbytes,
           "host_ms_per_frame": t_host / args.frames * 1e3, "device_ms_per_frame": t_dev / args.frames * 1e3,
           "host_over_device": t_host / t_dev, "results_equal": True,
           "device_forward_ms": med["forward"] * 1e3, "device_histogram_ms": med["histogram"] * 1e3,
           "device_histogram_gbps": nbytes / med["histogram"] * 1e-9, "device_d2h_ms": med["d2h"] * 1e3,
           "device_fold_ms": med["fold"] * 1e3}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
