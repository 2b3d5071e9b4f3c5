#!/usr/bin/env python3
"""Camera frame -> detections latency of unina_infer_frame per pixel format (sibling of tools/nv12_latency.py): every
unina_pixel_format at a 640x640 (the stem's tap and quad loaders) and a 1280x720 camera (its resize), beside unina_infer_bgra on a
frame of the same size in the same run -- the yardstick: no format reads more bytes per pixel than BGRA. The paths run in
alternating blocks (bgra rgb rgba ... bgra rgb ...) so that drift of the box hits all of them alike. Every call is synchronous
(the records are on the host when it returns), timed on the host clock.

  python tools/format_latency.py [--out profiles/r04/format_latency.json] [--blocks 4] [--calls 150] [--bench-json FILE ...]

--bench-json: result lines of `bench.py --gpus 1` (e.g. of the parent commit and of this tree on the same box) to store beside the
latencies, keyed by file name."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import unina_yolo_dla_amd as u
from unina_yolo_dla_amd import camera as twin
from unina_yolo_dla_amd.engine import Engine, Frame

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r04", "format_latency.json"))
ap.add_argument("--blocks", type=int, default=4)
ap.add_argument("--calls", type=int, default=150)
ap.add_argument("--bench-json", nargs="*", default=[])
args = ap.parse_args()

e = Engine.from_state_dict(u.synth.make_state_dict(7))
L = e.L
norm = L.create_norm_params_imagenet()
images = torch.empty((1, 3, 640, 640), dtype=torch.float32, device="cuda")
e.autotune(images.normal_(), iters=5)
RING = 4
FORMATS = {"bgra": 0, "nv12": 1, "rgb": 2, "rgba": 3, "yuyv": 4, "uyvy": 5, "bayer_rggb": 6, "bayer_bggr": 7, "bayer_grbg": 8, "bayer_gbrg": 9}
BYTES_PER_PIXEL = {"bgra": 4, "nv12": 1.5, "rgb": 3, "rgba": 4, "yuyv": 2, "uyvy": 2, "bayer_rggb": 1, "bayer_bggr": 1, "bayer_grbg": 1,
                   "bayer_gbrg": 1}


def scene(k, h, w):
    """Frame k of the ring as a grey picture uint8 [h, w]: a smooth pattern under mild noise. EVERY format renders this one picture
    (R = G = B = luma, neutral chroma, the mosaic of a grey scene is its luma), so the network sees nearly the same input and the
    post-process nearly the same number of records whatever the format: what differs between the paths is the stem's loader."""
    rng = np.random.default_rng(400 + k)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = 0.5 + 0.3 * np.sin(xx * (6.0 / w) + 0.3 + k) * np.cos(yy * (5.0 / h)) + 0.15 * np.sin((xx + yy) * (40.0 / (w + h)))
    return np.clip(smooth * 255 + rng.integers(-24, 25, (h, w)), 0, 255).astype(np.uint8)


def ring_of(name, h, w):
    """RING frames of one format on the device: (tensors kept alive, Frame)."""
    out = []
    for k in range(RING):
        y = scene(k, h, w)
        uv = np.full(((h + 1) // 2, w), 128, dtype=np.uint8)
        fmt = FORMATS[name]
        if name == "nv12":
            d, d_uv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
            out.append(((d, d_uv), Frame.from_tensors(fmt, w, h, d, w, d_uv, w)))
            continue
        if name in ("yuyv", "uyvy"):
            rows = twin.nv12_to_yuv422(y, uv, name)
        elif name.startswith("bayer"):
            rows = y
        else:
            n = 3 if name == "rgb" else 4
            rows = np.repeat(y[..., None], n, axis=2)
            if n == 4:
                rows[..., 3] = 255
            rows = rows.reshape(h, w * n)
        d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        out.append(((d,), Frame.from_tensors(fmt, w, h, d, rows.shape[1])))
    return out


result = {"version": L.unina_version().decode(), "device": torch.cuda.get_device_name(0), "blocks": args.blocks,
          "calls_per_block": args.calls, "unit": "ms", "cameras": {}, "bench": {}}
for (h, w) in ((640, 640), (720, 1280)):
    rings = {name: ring_of(name, h, w) for name in FORMATS}
    fns = {name: (lambda k, r=rings[name]: e.infer_frame(r[k][1], norm, 0.5, 0.45, 0.1)) for name in FORMATS}
    bgra = rings["bgra"]
    fns = {"unina_infer_bgra": lambda k: e.infer_bgra(bgra[k][0][0], w, h, 4 * w, norm, 0.5, 0.45, 0.1), **fns}
    for p in fns:                          # warm-up: every shape and path of the timed window
        for i in range(30):
            fns[p](i % RING)
    lat = {p: [] for p in fns}
    for _blk in range(args.blocks):
        for p in fns:
            blk = []
            for i in range(args.calls):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fns[p](i % RING)
                blk.append((time.perf_counter() - t) * 1e3)
            lat[p].append(blk)
    cam = {}
    base = float(np.percentile(np.concatenate(lat["unina_infer_bgra"]), 50))
    for p in fns:
        allv = np.concatenate(lat[p])
        cam[p] = {"p50": round(float(np.percentile(allv, 50)), 4), "p99": round(float(np.percentile(allv, 99)), 4),
                  "p50_vs_unina_infer_bgra": round(float(np.percentile(allv, 50)) / base, 4),
                  "block_p50": [round(float(np.percentile(b, 50)), 4) for b in lat[p]]}
        if p in BYTES_PER_PIXEL:
            cam[p]["bytes_per_pixel"] = BYTES_PER_PIXEL[p]
        # (the post-process's share goes with the number of records: it must be about the same for every path)
        cam[p]["detections"] = [int(len(fns[p](k))) for k in range(RING)]
        print(f"{w}x{h} {p:18s} p50 {cam[p]['p50']:.4f} ms ({cam[p]['p50_vs_unina_infer_bgra']:.3f} x bgra)  p99 {cam[p]['p99']:.4f} ms  "
              f"blocks {cam[p]['block_p50']}  detections {cam[p]['detections']}")
    result["cameras"][f"{w}x{h}"] = cam
e.close()
for path in args.bench_json:
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
    result["bench"][os.path.basename(path)] = json.loads(lines[-1]) if lines else None
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({k: {p: v["p50"] for p, v in cam.items()} for k, cam in result["cameras"].items()}))
