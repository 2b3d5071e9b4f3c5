#!/usr/bin/env python3
"""Cost of the data-mining path on one GPU; prints ONE JSON line.

  * frames/s of a unina_mine_async loop (2 handles in flight, one stream each, scores and embeddings written to rows of
    device matrices, nothing copied back) beside frames/s of a bare unina_enqueue loop in the same process on the same
    frames: what the mining kernels add to the raw-head forward;
  * time of unina_kcenter at N = 65 536, D = 256, k = 256 beside kcenter_numpy on the host's cores.

Blocks of `--frames` frames alternate between the two loops (A B A B ...); the figure is the median block, the spread is
reported. Wall clock around a device synchronisation; the first block of each loop is a warm-up and is dropped.

    python tools/bench_mining.py [--frames 4000] [--blocks 7] [--precision fp16|strict|fp32] [--skip-numpy]
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
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--precision", default="fp16", choices=("fp16", "strict", "fp32"))
    ap.add_argument("--kcenter-n", type=int, default=65536)
    ap.add_argument("--kcenter-k", type=int, default=256)
    ap.add_argument("--skip-numpy", action="store_true")
    args = ap.parse_args()
    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd import engine, export, mining
    prec = {"fp16": export.FP16, "strict": export.STRICT, "fp32": export.FP32}[args.precision]
    g = u.graph.Graph()
    sd = u.synth.make_state_dict(7, g)
    engines = [engine.Engine.from_state_dict(sd, g, precision=prec) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    ring = [torch.from_numpy(u.rng.frame(1234 + i, 640, 640)).cuda() for i in range(8)]
    n = args.frames
    d = engines[0].embedding_dim
    S = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    E = torch.zeros((n, d), dtype=torch.float32, device="cuda")
    sp = [s.cuda_stream for s in streams]
    L = engines[0].L

    def block(mine: bool) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            e = engines[i & 1]
            img = ring[i & 7].data_ptr()
            if mine:
                rc = L.unina_mine_async(e.h, img, S[i].data_ptr(), E[i].data_ptr(), sp[i & 1])
            else:
                rc = L.unina_set_tensor_address(e.h, b"images", img) or L.unina_enqueue(e.h, sp[i & 1])
            assert rc == 0, rc
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    rates = {True: [], False: []}
    for b in range(args.blocks + 1):
        for mine in (False, True):
            r = block(mine)
            if b:
                rates[mine].append(r)
    out = {"precision": args.precision, "frames_per_block": n, "blocks": args.blocks, "handles": 2,
           "mine_fps": float(np.median(rates[True])), "mine_fps_min": min(rates[True]), "mine_fps_max": max(rates[True]),
           "enqueue_fps": float(np.median(rates[False])), "enqueue_fps_min": min(rates[False]), "enqueue_fps_max": max(rates[False])}
    out["mine_added_us_per_frame"] = 1e6 / out["mine_fps"] - 1e6 / out["enqueue_fps"]
    for e in engines:
        e.close()

    kn, kk = args.kcenter_n, args.kcenter_k
    emb = np.maximum(np.random.RandomState(17).normal(0.16, 0.24, size=(kn, d)), 0).astype(np.float32)
    demb = torch.from_numpy(emb).cuda()
    times = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sel = engine.kcenter(demb, kk, 4242)
        times.append(time.perf_counter() - t0)
    out.update(kcenter_n=kn, kcenter_dim=d, kcenter_k=kk, kcenter_gpu_ms=float(np.median(times[1:]) * 1e3),
               kcenter_gpu_us_per_step=float(np.median(times[1:]) * 1e6 / max(kk - 1, 1)))
    if not args.skip_numpy:
        t0 = time.perf_counter()
        ref = mining.kcenter_numpy(emb, kk, 4242)
        out["kcenter_numpy_ms"] = (time.perf_counter() - t0) * 1e3
        out["kcenter_same_selection_as_numpy"] = bool((ref == sel).all())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
