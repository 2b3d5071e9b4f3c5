#!/usr/bin/env python3
"""Cost of the k-means coreset on one GPU; prints ONE JSON line and writes it to profiles/r04/kmeans_bench.json.

At (n, dim, k) = (100 000, 256, 1 000), synthetic embeddings (the k-center fixture's relu(N(0.16, 0.24^2)) generator):
  * one full iteration (|c|^2, assign, update, inertia), median of `--reps` calls of max_iter = 1 between device syncs.
    The C ABI enqueues an iteration as a whole, so the assignment launch is NOT timed alone here: the iteration time bounds
    it from above (and its FLOP rate from below); a kernel trace of this script (rocprofv3 --kernel-trace --stats) splits it;
  * the selection (unina_nearest_rows, k dependent steps);
  * kmeans_numpy's iteration on the host's cores (float64).
The assignment does 2 n k dim FLOP; its rate is to be judged against the f32-input MFMA peak of the part (157.3 TFLOP/s
spec), not against this code. Asserts that device and host labels agree wherever the float64 margin exceeds the rounding
bound of tests/test_gpu_kmeans.py.

    python tools/bench_kmeans.py [--n 100000] [--dim 256] [--k 1000] [--reps 5] [--skip-numpy]
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
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "kmeans_bench.json"))
    args = ap.parse_args()
    import torch
    from unina_yolo_dla_amd import engine, mining
    n, dim, k = args.n, args.dim, args.k
    rng = np.random.RandomState(17)
    emb = np.maximum(rng.normal(0.16, 0.24, size=(n, dim)), 0).astype(np.float32)
    init = rng.permutation(n)[:k]
    x = torch.from_numpy(emb).cuda()
    start = x[torch.from_numpy(init).cuda()].clone()

    def timed(fn):
        times = []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return out, float(np.median(times[1:]) * 1e3), float(min(times[1:]) * 1e3), float(max(times[1:]) * 1e3)

    (cen, labels, hist, iters, _), it_ms, it_min, it_max = timed(lambda: engine.kmeans(x, k, centroids=start, max_iter=1))
    sel, sel_ms, sel_min, sel_max = timed(lambda: engine.nearest_rows(x, torch.from_numpy(cen).cuda()))
    flop = 2.0 * n * k * dim
    out = {"n": n, "dim": dim, "k": k, "reps": args.reps,
           "iteration_ms": it_ms, "iteration_ms_min": it_min, "iteration_ms_max": it_max,
           "assign_flop": flop, "iteration_tflops_lower_bound_of_assign": flop / (it_ms * 1e-3) / 1e12,
           "f32_mfma_peak_tflops_spec": 157.3,
           "nearest_rows_ms": sel_ms, "nearest_rows_us_per_step": sel_ms * 1e3 / k,
           "note": "iteration_ms is wall clock around engine.kmeans(max_iter=1): 5 + 1 launches, result copies included"}
    if not args.skip_numpy:
        t0 = time.perf_counter()
        wc, wl, wh, _, _ = mining.kmeans_numpy(emb, k, None, 1, centroids=emb[init])
        out["numpy_iteration_ms"] = (time.perf_counter() - t0) * 1e3
        # labels must agree wherever the float64 margin exceeds the rounding bound (tests/test_gpu_kmeans.py)
        u = 2.0 ** -24
        g = (dim + 2) * u / (1 - (dim + 2) * u)
        x64, c64 = emb.astype(np.float64), emb[init].astype(np.float64)
        cn, ac = (c64 * c64).sum(axis=1), np.abs(c64)
        differ = unsure = 0
        for r in range(0, n, 4096):
            blk = x64[r:r + 4096]
            s = cn[None, :] - 2.0 * (blk @ c64.T)
            tol = 2.0 * g * (2.0 * (np.abs(blk) @ ac.T) + cn[None, :])
            rows = np.arange(len(blk))
            best = s.argmin(axis=1)
            gap = s - s[rows, best][:, None] - tol - tol[rows, best][:, None]
            gap[rows, best] = np.inf
            sure = (gap > 0).all(axis=1)
            unsure += int((~sure).sum())
            differ += int((labels[r:r + 4096] != best).sum())
            assert (labels[r:r + 4096][sure] == best[sure]).all(), "device label differs from float64 beyond the rounding bound"
        out.update(labels_differ_from_float64=differ, rows_within_rounding_bound=unsure,
                   inertia_rel_diff_vs_numpy=float(abs(hist[0] - wh[0]) / wh[0]))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
