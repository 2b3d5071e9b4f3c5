#!/usr/bin/env python3
"""Cost of rectifying one frame's raw images on the device against the host route; prints ONE JSON line and writes it to
profiles/r04/rectify_latency.txt.

The frame is what a stereo head with a colour stream delivers: a 1920 x 1080 luma pair and one 1920 x 1080 BGRA frame, rectified
to the same sizes in ONE unina_rectify_async call. Calibration: fx = fy = 1400, a mild barrel (k1 = -0.08, k2 = 0.01, p1 = 5e-4,
p2 = -3e-4), a 2-degree rotation about a skew axis (mirrored for the right camera), the rectified pinhole at fx = 1330.
  * kernel_ms: HIP events around `reps` back-to-back calls (dispatch included) after `--warmup` calls; reps is chosen from a
    short trial so that the timed window is at least `--window` seconds;
  * bytes: computed from the shapes, raw bytes (every raw image read once) plus rectified bytes; bytes_per_s = bytes / kernel_ms;
  * hbm_floor_ms: the same bytes at the MI355X's HBM3E peak of 8.0 TB/s (the data sheet's figure; a float4 copy reaches 6.29 TB/s);
    share_of_hbm_floor = hbm_floor_ms / kernel_ms. The working set (24.9 MB) fits the 256 MB Infinity Cache, so back-to-back
    calls need not reach HBM at all: the share says how far the launch is from a pure streaming bound, not what HBM delivered;
  * host_d2h_ms / host_numpy_ms / host_h2d_ms: the route a node would otherwise take -- the three raw images copied to the host,
    rectify.rectify_numpy on each, the three results copied back -- median of `--host-reps` runs.
Asserts that the device images equal rectify_numpy's, byte for byte, before printing.

    python tools/bench_rectify.py [--window 0.5] [--warmup 20] [--host-reps 3]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import median_ms, window_ms  # noqa: E402

W, H = 1920, 1080
HBM_PEAK = 8.0e12          # bytes / s, HBM3E peak of the MI355X
HBM_COPY = 6.29e12         # bytes / s, what a float4 copy reaches


def raw_image(seed, channels):
    """Smoothed noise, 0 .. 255."""
    rng = np.random.RandomState(seed)
    a = rng.uniform(0.0, 256.0, (H, W, channels))
    p = np.pad(a, ((1, 1), (1, 1), (0, 0)), mode="edge")
    a = (p[1:-1, 1:-1] + p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:]) / 5.0
    img = np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return img[:, :, 0] if channels == 1 else img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "r04", "rectify_latency.txt"))
    args = ap.parse_args()
    import torch
    from unina_yolo_dla_amd import rectify
    src = (1400.0, 1400.0, 959.5, 539.5)
    dist = (-0.08, 0.01, 5e-4, -3e-4, 0.0)
    dst = (1330.0, 1330.0, 959.5, 539.5)
    axis = (0.3, -0.8, 0.52)
    cam_l = rectify.make_rectify_cam(src, dist, rectify.rotation(axis, 2.0), dst)
    cam_r = rectify.make_rectify_cam(src, dist, rectify.rotation(axis, -2.0), dst)
    raws = [raw_image(1, 1), raw_image(2, 1), raw_image(3, 4)]
    specs = [(cam_l, (H, W), 1, 0), (cam_r, (H, W), 1, 0), (cam_l, (H, W), 4, 114)]
    d_raws = [torch.from_numpy(r).cuda() for r in raws]
    rect = rectify.DeviceRectifier(specs)

    def d2h():
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in d_raws]
    hosts, d2h_ms = median_ms(d2h, args.host_reps)
    want, numpy_ms = median_ms(lambda: [rectify.rectify_numpy(h, s[0], s[1], s[3]) for h, s in zip(hosts, specs)], args.host_reps)

    def h2d():
        out = [torch.from_numpy(w).cuda() for w in want]
        torch.cuda.synchronize()
        return out
    _, h2d_ms = median_ms(h2d, args.host_reps)

    rect.update(d_raws)
    got = rect.read()
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "device image differs from rectify_numpy's"

    def timed(reps):
        return window_ms(torch, lambda: rect.update(d_raws), reps)
    timed(args.warmup)
    trial_ms = timed(50)
    reps = max(50, int(math.ceil(args.window * 1.2e3 / trial_ms)))
    kernel_ms = timed(reps)
    window_s = kernel_ms * reps / 1e3
    assert window_s >= args.window, (window_s, args.window)
    after = rect.read()
    for g, w in zip(after, want):
        assert g.tobytes() == w.tobytes(), "device image differs after the timed loop"

    n_bytes = int(sum(r.nbytes for r in raws) + sum(w.nbytes for w in want))
    floor_ms = n_bytes / HBM_PEAK * 1e3
    inside = [float(rectify.rectify_source_numpy(s[0], s[1], (H, W))[2].mean()) for s in specs[:2]]
    out = {"images": [f"{W}x{H}x{r.shape[2] if r.ndim == 3 else 1}" for r in raws], "bytes": n_bytes, "reps": reps, "window_s": window_s,
           "kernel_ms": kernel_ms, "bytes_per_s": n_bytes / (kernel_ms * 1e-3), "hbm_peak_bytes_per_s": HBM_PEAK, "hbm_floor_ms": floor_ms,
           "share_of_hbm_floor": floor_ms / kernel_ms, "share_of_float4_copy_rate": n_bytes / HBM_COPY * 1e3 / kernel_ms,
           "inside_fraction": inside, "host_d2h_ms": d2h_ms, "host_numpy_ms": numpy_ms, "host_h2d_ms": h2d_ms,
           "host_ms": d2h_ms + numpy_ms + h2d_ms,
           "note": "kernel_ms: HIP events around back-to-back calls of three images each (dispatch included), one run, no repeat to give "
                   "a spread; bytes: raw + rectified image bytes from the shapes; the 24.9 MB working set fits the Infinity Cache"}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
