#!/usr/bin/env python3
"""Latency of sliced inference on one GPU, two ways, in one process; writes ONE JSON line to profiles/r04/tiled_bench.json
(and prints it).

For a device-generated 1920x1200 BGRA frame and the default slices (12 tiles of 640x640, 20 % overlap):

  (a) per_crop ... the only form possible without unina_infer_tiled_bgra: one synchronous unina_infer_bgra per crop (a pointer
                   offset into the frame) and the merge on the host with slicing.merge_numpy;
  (b) tiled ...... one unina_infer_tiled_bgra call: the 12 frame graphs and the merge enqueued back to back on one stream.

Both are timed on the host's clock from the call to the merged records in host memory, through the same ctypes binding, in
alternating blocks of 100 calls (A B A B ...) after `--warmup` calls of each; p50 / p99 over `--calls` calls of each. The two
results are compared byte for byte before anything is timed.

The measurement runs in a child process under a time limit (`--timeout` seconds); the parent only waits and writes the file.

    python tools/bench_tiled.py [--calls 2000] [--warmup 200] [--conf 0.3] [--timeout 600]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r04", "tiled_bench.json")


def child(args) -> dict:
    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd import engine, slicing
    W, H = 1920, 1200
    pitch = W * 4
    g = u.graph.Graph()
    eng = engine.Engine.from_state_dict(u.synth.make_state_dict(7, g), g)
    L = eng.L
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    cam = torch.randint(0, 256, (H, pitch), dtype=torch.uint8, device="cuda", generator=gen)
    tiles = eng.default_tiles(W, H)
    arr = engine._tile_array(tiles)
    norm = L.create_norm_params_imagenet()
    stream = torch.cuda.current_stream().cuda_stream
    base = cam.data_ptr()
    T = len(tiles)
    slots = np.zeros((T, engine.MAX_DETECTIONS), dtype=engine.DET_DTYPE)
    counts = np.zeros(T, dtype=np.int32)
    n = C.c_int()
    out = np.zeros(engine.MAX_DETECTIONS, dtype=engine.DET_DTYPE)

    def per_crop():
        for t, (x, y, w, h) in enumerate(tiles):
            rc = L.unina_infer_bgra(eng.h, base + y * pitch + 4 * x, w, h, pitch, C.byref(norm), args.conf, 0.45, 0.1,
                                    slots[t].ctypes.data, C.byref(n), stream)
            assert rc == 0, rc
            counts[t] = n.value
        return slicing.merge_numpy(slots, counts, tiles, 0.45, eng.width, eng.height)

    def tiled():
        rc = L.unina_infer_tiled_bgra(eng.h, base, W, H, pitch, arr, T, C.byref(norm), args.conf, 0.45, 0.1, 0.45,
                                      out.ctypes.data, C.byref(n), stream)
        assert rc == 0, rc
        return out[:n.value]

    a, b = per_crop(), tiled().copy()
    same = a.tobytes() == b.tobytes()
    per_tile = counts.tolist()
    for _ in range(args.warmup):
        per_crop()
        tiled()
    lat = {"per_crop": [], "tiled": []}
    block = 100
    for _ in range((args.calls + block - 1) // block):
        for name, fn in (("per_crop", per_crop), ("tiled", tiled)):
            for _k in range(block):
                t0 = time.perf_counter()
                fn()
                lat[name].append((time.perf_counter() - t0) * 1e3)
    # the host merge's share of (a)
    t0 = time.perf_counter()
    for _ in range(50):
        slicing.merge_numpy(slots, counts, tiles, 0.45, eng.width, eng.height)
    merge_ms = (time.perf_counter() - t0) * 1e3 / 50
    eng.close()
    res = {"frame": [W, H], "tiles": T, "conf": args.conf, "calls": len(lat["tiled"]), "warmup": args.warmup,
           "candidates_per_tile": per_tile, "union": int(sum(per_tile)), "kept": int(len(b)), "results_identical": bool(same),
           "host_merge_numpy_ms": merge_ms}
    for name, v in lat.items():
        res[f"{name}_p50_ms"] = float(np.percentile(v, 50))
        res[f"{name}_p99_ms"] = float(np.percentile(v, 99))
    res["tiled_over_per_crop_p50"] = res["tiled_p50_ms"] / res["per_crop_p50_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--conf", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(args)), flush=True)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print(f"bench_tiled: the measurement did not finish in {args.timeout} s", file=sys.stderr)
        return 124
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode or 1
    line = lines[-1][len("RESULT "):]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
