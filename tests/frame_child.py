"""Shared by tests/test_gpu_frame_formats.py and its child process: seeded camera frames of every unina_pixel_format, and -- run
as a script -- the frame-descriptor path in a fresh process, because UNINA_STEM_V1 (the one-thread-per-pixel stem) is read once
per process.

  python tests/frame_child.py <out.npz>     runs CHILD_CASES through Engine.infer_frame on the seed-7 engine and stores, per case
                                            k, the detection records (det<k>) and the stem buffer (stem<k>)
"""
import os
import sys

import numpy as np

from nv12_child import CONF, IOU, Q, ROOT, nv12_planes, upload

BGRA, NV12, RGB, RGBA, YUYV, UYVY, RGGB, BGGR, GRBG, GBRG = range(10)      # include/unina_mi355.h: unina_pixel_format
NEW_FORMATS = (RGB, RGBA, YUYV, UYVY, RGGB, BGGR, GRBG, GBRG)
NAMES = {BGRA: "bgra", NV12: "nv12", RGB: "rgb", RGBA: "rgba", YUYV: "yuyv", UYVY: "uyvy", RGGB: "rggb", BGGR: "bggr", GRBG: "grbg",
         GBRG: "gbrg"}

# (seed, height, width, misaligned): the cameras of tests/nv12_child.py. misaligned: an odd pitch and the plane one byte off an
# aligned address (RGBA, which must stay 4-byte aligned: pitch + 4)
CAMERAS = {
    "640_wide": (51, 640, 640, False),         # the network's size, aligned: the quad loaders' wide loads
    "640_bytes": (52, 640, 640, True),         # the network's size, misaligned: their byte loads
    "720p_down": (53, 720, 1280, False),
    "45x77_up": (54, 45, 77, False),           # odd both ways: the last 4:2:2 pair of a row is read whole
}
CHILD_CASES = ((UYVY, "45x77_up"), (YUYV, "640_bytes"), (BGGR, "640_wide"), (GRBG, "720p_down"))


def frame_rows(twin, fmt, seed, h, w, lo=0, hi=256):
    """(rows uint8 [h, bytes of a row], what the numpy twin takes as `planes`) of a w x h frame: the smooth pattern under noise of
    nv12_child.nv12_planes as the luma, so that some cells pass the confidence threshold at any camera size."""
    y, uv = nv12_planes(seed, h, w, lo=lo, hi=hi)
    rng = np.random.default_rng(seed + 1000)
    if fmt in (YUYV, UYVY):
        rows = twin.nv12_to_yuv422(y, uv, NAMES[fmt])
        return rows, rows
    if fmt in (RGGB, BGGR, GRBG, GBRG):
        return y, y                                                    # (a grey scene under a colour filter array: the mosaic is the luma)
    rgb = np.clip(y[..., None].astype(np.int32) + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
    if fmt == RGB:
        return rgb.reshape(h, 3 * w), rgb
    rgba = np.concatenate([rgb, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=-1)
    if fmt == BGRA:
        rgba = np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])
    return rgba.reshape(h, 4 * w), rgba


def make_frame(torch, engine, twin, fmt, seed, h, w, misaligned=False, lo=0, hi=256):
    """A frame on the device and on the host: dict(fmt, w, h, pitch, planes (the twin's), d (the device bytes), frame (engine.Frame))."""
    if fmt == NV12:
        yp, uvp, off = (w + 1, 2 * ((w + 1) // 2) + 1, 1) if misaligned else (w, 2 * ((w + 1) // 2), 0)
        y, uv = nv12_planes(seed, h, w, yp, uvp, lo=lo, hi=hi)
        d_y, d_uv = upload(torch, y, off), upload(torch, uv, off)
        return dict(fmt=fmt, w=w, h=h, pitch=yp, uv_pitch=uvp, planes=(y[:, :w], uv[:, :2 * ((w + 1) // 2)]), d=d_y, d_uv=d_uv,
                    frame=engine.Frame.from_tensors(fmt, w, h, d_y, yp, d_uv, uvp))
    rows, planes = frame_rows(twin, fmt, seed, h, w, lo, hi)
    n = rows.shape[1]
    four = fmt in (BGRA, RGBA)
    pitch, off = n, 0
    if misaligned:
        pitch, off = (n + 4, 0) if four else (n + 1 + (n & 1), 1)      # an odd pitch
    buf = np.random.default_rng(seed + 2000).integers(0, 256, (h, pitch), dtype=np.uint8)
    buf[:, :n] = rows
    d = upload(torch, buf, off)
    return dict(fmt=fmt, w=w, h=h, pitch=pitch, planes=planes, d=d, frame=engine.Frame.from_tensors(fmt, w, h, d, pitch))


def camera(torch, engine, twin, fmt, name):
    seed, h, w, misaligned = CAMERAS[name]
    return make_frame(torch, engine, twin, fmt, seed, h, w, misaligned)


def main():
    sys.path.insert(0, ROOT)
    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd import camera as twin, engine
    e = engine.Engine.from_state_dict(u.synth.make_state_dict(7, u.graph.Graph()))
    out = {"kernel": np.array([o["kernel"] for o in e.op_infos() if o["kernel"].startswith("stem_")][0])}
    for k, (fmt, name) in enumerate(CHILD_CASES):
        c = camera(torch, engine, twin, fmt, name)
        out[f"det{k}"] = e.infer_frame(c["frame"], None, CONF, IOU, Q)
        out[f"stem{k}"] = e.read_buffer("backbone.stem")
    e.close()
    np.savez(sys.argv[1], **out)
    print("FRAME_CHILD_OK")


if __name__ == "__main__":
    main()
