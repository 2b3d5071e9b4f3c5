"""Shared by tests/test_letterbox_cpu.py, tests/test_gpu_letterbox.py and the latter's child process: the seeded cameras of the
letterbox tests, and -- run as a script -- the letterboxed camera path in a fresh process, because UNINA_STEM_V1 (the
one-thread-per-pixel stem) is read once per process.

  python tests/letterbox_child.py <out.npz>   runs every camera, BGRA and NV12, through Engine.infer_letterbox_* (network pixels)
                                              on the 64 x 64 seed-7 engine and stores, per camera k and format f, the detection
                                              records (det_<f><k>) and the stem buffer (stem_<f><k>)
"""
import os
import sys

import numpy as np

from nv12_child import nv12_planes, upload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = 64                      # the engine's input is NET x NET
PAD = 114.0
# The confidence threshold comes from the CPU oracle, not from the engine: oracle.forward + oracle.postprocess on the twins'
# letterboxed tensors of every camera below (both formats) keep between 21 and 54 records at 0.15, and the strongest record of
# the weakest camera (5x128, BGRA) has confidence 0.447: three times the threshold, against an fp16 engine whose scores differ
# from the oracle's by ~3e-3. So no list is empty at 0.15.
CONF, IOU, Q = 0.15, 0.45, 0.1

# name: (seed, width, height, BGRA pitch, y_pitch, uv_pitch, byte offset of the NV12 planes' base address)
CAMERAS = {
    "128x72_down": (81, 128, 72, 128 * 4 + 64, 136, 132, 0),    # down-scale; every row padded
    "40x30_up": (82, 40, 30, 160, 40, 40, 0),                   # up-scale
    "64x37_r1": (83, 64, 37, 64 * 4 + 16, 65, 67, 1),           # r == 1: the no-resize path at (0, 13), odd remainder (top 13,
                                                                # bottom 14); odd pitches, planes one byte off: byte loads
    "5x128_even": (84, 5, 128, 20, 5, 6, 0),                    # r = 0.5: round(2.5) = 2, a 2-pixel-wide inner rectangle
    "200x23_wide": (85, 200, 23, 800, 200, 200, 0),             # very wide: 64 x 7 at (0, 28)
    "64x64_identity": (86, 64, 64, 256, 64, 64, 0),             # the network's size: no letterbox at all
}


def host_camera(name):
    """The camera's frame in both formats, host side, with the padding bytes: bgra [h, pitch] (B, G, R from the NV12 luma pattern
    plus per-channel noise, random alpha), y [h, y_pitch], uv [(h + 1) // 2, uv_pitch]."""
    seed, w, h, pitch, yp, uvp, off = CAMERAS[name]
    y, uv = nv12_planes(seed, h, w, yp, uvp)
    rng = np.random.default_rng(seed + 1000)
    bgra = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    px = bgra[:, :4 * w].reshape(h, w, 4)
    px[..., :3] = np.clip(y[:, :w, None].astype(np.int32) + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
    return dict(name=name, w=w, h=h, pitch=pitch, y_pitch=yp, uv_pitch=uvp, off=off, bgra=bgra, y=y, uv=uv)


def visible(c):
    """What the twins take: bgra [h, w, 4], y [h, w], uv [(h + 1) // 2, 2 * ((w + 1) // 2)]."""
    w, h = c["w"], c["h"]
    return (np.ascontiguousarray(c["bgra"][:, :4 * w]).reshape(h, w, 4), c["y"][:, :w], c["uv"][:, :2 * ((w + 1) // 2)])


def device_camera(torch, name):
    c = host_camera(name)
    c["d_bgra"] = upload(torch, c["bgra"])
    c["d_y"] = upload(torch, c["y"], c["off"])
    c["d_uv"] = upload(torch, c["uv"], c["off"])
    return c


def run_letterbox(e, c, fmt, map_boxes=False, out=None, conf=CONF):
    if fmt == "bgra":
        return e.infer_letterbox_bgra(c["d_bgra"], c["w"], c["h"], c["pitch"], None, conf, IOU, Q, PAD, map_boxes, out=out)
    return e.infer_letterbox_nv12(c["d_y"], c["d_uv"], c["w"], c["h"], c["y_pitch"], c["uv_pitch"], None, conf, IOU, Q, PAD, map_boxes,
                                  out=out)


def main():
    sys.path.insert(0, ROOT)
    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd.engine import Engine
    g = u.graph.Graph(in_h=NET, in_w=NET)
    e = Engine.from_state_dict(u.synth.make_state_dict(7, g), g)
    out = {"kernel": np.array([o["kernel"] for o in e.op_infos() if o["kernel"].startswith("stem_")][0])}
    for k, name in enumerate(CAMERAS):
        c = device_camera(torch, name)
        for fmt in ("bgra", "nv12"):
            out[f"det_{fmt}{k}"] = run_letterbox(e, c, fmt)
            out[f"stem_{fmt}{k}"] = e.read_buffer("backbone.stem")
    e.close()
    np.savez(sys.argv[1], **out)
    print("LETTERBOX_CHILD_OK")


if __name__ == "__main__":
    main()
