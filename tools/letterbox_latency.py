#!/usr/bin/env python3
"""Camera frame -> detections latency with the letterbox (sibling of tools/nv12_latency.py), four paths in one run:

  (a) unina_preprocess_letterbox_bgra + unina_infer      the two-step form: the fp32 tensor written and read back
  (b) unina_infer_letterbox_bgra, boxes mapped           the letterbox inside the stem kernel, the map at the output write
  (c) unina_infer_bgra                                   the stretch: the unchanged path, the yardstick
  (d) unina_infer_letterbox_nv12, boxes mapped           (b) for an NV12 frame

each at a 1280x720 and a 1920x1080 camera into the 640x640 fp16 engine, in alternating blocks (a b c d a b c d ...) so that
drift of the box hits all four alike; the spread of a path's block medians is the run-to-run margin. Every call is synchronous
(the records are on the host when it returns), timed on the host clock.

  python tools/letterbox_latency.py [--out FILE.json] [--blocks 6] [--calls 200] [--paths a,b,c,d]

--paths c runs on a tree from before the letterbox entry points too (the parent commit, for (c) against (c) on the same box)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import unina_yolo_dla_amd as u
from unina_yolo_dla_amd.engine import Engine

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--blocks", type=int, default=6)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--paths", default="a,b,c,d")
args = ap.parse_args()
paths = args.paths.split(",")

e = Engine.from_state_dict(u.synth.make_state_dict(7))
L = e.L
norm = L.create_norm_params_imagenet()
s = torch.cuda.current_stream().cuda_stream
images = torch.empty((1, 3, 640, 640), dtype=torch.float32, device="cuda")
e.autotune(images.normal_(), iters=5)
RING = 4
PAD = 114.0


def frames(h, w):
    """RING seeded NV12 frames and their BGRA renderings (BT.601, rounded to u8), on the device."""
    out = []
    for k in range(RING):
        rng = np.random.default_rng(400 + k)
        y = rng.integers(0, 256, (h, w), dtype=np.uint8)
        uv = rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
        Y = y.astype(np.float32)
        U = np.repeat(np.repeat(uv[:, 0::2], 2, 0), 2, 1).astype(np.float32) - 128
        V = np.repeat(np.repeat(uv[:, 1::2], 2, 0), 2, 1).astype(np.float32) - 128
        bgra = np.full((h, w, 4), 255, dtype=np.uint8)
        for c, v in enumerate((Y + 1.772 * U, Y - 0.344136 * U - 0.714136 * V, Y + 1.402 * V)):
            bgra[..., c] = np.clip(np.rint(v), 0, 255)
        out.append((torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), torch.from_numpy(bgra.reshape(h, w * 4)).cuda()))
    return out


def make_paths(h, w, ring):
    def a(k):
        L.unina_preprocess_letterbox_bgra(ring[k][2].data_ptr(), images.data_ptr(), w, h, w * 4, 640, 640, PAD, norm, s)
        return e.infer(images, 0.5, 0.45, 0.1)

    def b(k):
        return e.infer_letterbox_bgra(ring[k][2], w, h, w * 4, norm, 0.5, 0.45, 0.1, PAD, True)

    def c(k):
        return e.infer_bgra(ring[k][2], w, h, w * 4, norm, 0.5, 0.45, 0.1)

    def d(k):
        y, uv, _ = ring[k]
        return e.infer_letterbox_nv12(y, uv, w, h, w, w, norm, 0.5, 0.45, 0.1, PAD, True)

    return {"a": a, "b": b, "c": c, "d": d}


NAMES = {"a": "unina_preprocess_letterbox_bgra + unina_infer", "b": "unina_infer_letterbox_bgra", "c": "unina_infer_bgra (stretch)",
         "d": "unina_infer_letterbox_nv12"}
result = {"version": L.unina_version().decode(), "device": torch.cuda.get_device_name(0), "blocks": args.blocks,
          "calls_per_block": args.calls, "unit": "ms", "cameras": {}}
for (h, w) in ((720, 1280), (1080, 1920)):
    ring = frames(h, w)
    fns = make_paths(h, w, ring)
    for p in paths:                       # warm-up: every shape and path of the timed window
        for i in range(30):
            fns[p](i % RING)
    lat = {p: [] for p in paths}
    for _blk in range(args.blocks):
        for p in paths:
            blk = []
            for i in range(args.calls):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fns[p](i % RING)
                blk.append((time.perf_counter() - t) * 1e3)
            lat[p].append(blk)
    cam = {}
    for p in paths:
        allv = np.concatenate(lat[p])
        bp = [round(float(np.percentile(b, 50)), 4) for b in lat[p]]
        cam[p] = {"path": NAMES[p], "p50": round(float(np.percentile(allv, 50)), 4), "p99": round(float(np.percentile(allv, 99)), 4),
                  "block_p50": bp, "block_p50_spread": round(max(bp) - min(bp), 4)}
        print(f"{w}x{h} ({p}) {NAMES[p]:46s} p50 {cam[p]['p50']:.4f} ms  p99 {cam[p]['p99']:.4f} ms  blocks {bp}")
    result["cameras"][f"{w}x{h}"] = cam
e.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({k: {p: v["p50"] for p, v in cam.items()} for k, cam in result["cameras"].items()}))
