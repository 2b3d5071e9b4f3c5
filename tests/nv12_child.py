"""Shared by tests/test_gpu_nv12.py and its child process: seeded NV12 camera frames, and -- run as a script -- the NV12 camera
path in a fresh process, because UNINA_STEM_V1 (the one-thread-per-pixel stem) is read once per process.

  python tests/nv12_child.py <out.npz>     runs CHILD_CAMERAS through Engine.infer_nv12 on the seed-7 engine and stores, per
                                           camera k, the detection records (det<k>) and the stem buffer (stem<k>)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF, IOU, Q = 0.3, 0.45, 0.1

# (seed, height, width, y_pitch, uv_pitch, byte offset of both planes' base address)
CAMERAS = {
    "640_wide": (51, 640, 640, 640, 640, 0),        # the network's size, everything 4-byte aligned: dword loads
    "640_bytes": (52, 640, 640, 641, 641, 1),       # odd pitches, planes one byte off an aligned address: byte loads
    "720p_down": (53, 720, 1280, 1280, 1280, 0),
    "45x77_up": (54, 45, 77, 77, 78, 0),            # odd both ways: 23 chroma rows, the last pair of a row read whole
}
CHILD_CAMERAS = ("45x77_up", "640_wide")


def nv12_planes(seed, h, w, y_pitch=None, uv_pitch=None, lo=0, hi=256):
    """Host planes with their padding, y [h, y_pitch] and uv [(h + 1) // 2, uv_pitch]: a smooth pattern under noise in the luma
    (so that some cells pass the confidence threshold at any camera size), random chroma, random padding bytes."""
    rng = np.random.default_rng(seed)
    y_pitch = w if y_pitch is None else y_pitch
    uv_pitch = 2 * ((w + 1) // 2) if uv_pitch is None else uv_pitch
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = 0.5 + 0.3 * np.sin(xx * (6.0 / w) + 0.3) * np.cos(yy * (5.0 / h)) + 0.15 * np.sin((xx + yy) * (40.0 / (w + h)))
    noise = rng.integers(-24, 25, (h, w))
    y = rng.integers(0, 256, (h, y_pitch), dtype=np.uint8)
    y[:, :w] = np.clip(lo + smooth * (hi - lo) + noise, 0, 255).astype(np.uint8)
    uv = rng.integers(64, 192, ((h + 1) // 2, uv_pitch), dtype=np.uint8)
    return y, uv


def upload(torch, plane, offset=0):
    """The plane on the device, its first byte `offset` bytes behind an allocation's (256-byte aligned) start."""
    flat = torch.empty(plane.size + offset, dtype=torch.uint8, device="cuda")
    flat[offset:] = torch.from_numpy(np.ascontiguousarray(plane).reshape(-1)).cuda()
    view = flat[offset:]
    assert view.data_ptr() % 256 == offset
    return view


def camera(torch, name):
    seed, h, w, yp, uvp, off = CAMERAS[name]
    y, uv = nv12_planes(seed, h, w, yp, uvp)
    return dict(h=h, w=w, y_pitch=yp, uv_pitch=uvp, y=y, uv=uv, d_y=upload(torch, y, off), d_uv=upload(torch, uv, off))


def main():
    sys.path.insert(0, ROOT)
    import torch
    import unina_yolo_dla_amd as u
    from unina_yolo_dla_amd.engine import Engine
    e = Engine.from_state_dict(u.synth.make_state_dict(7, u.graph.Graph()))
    out = {"kernel": np.array([o["kernel"] for o in e.op_infos() if o["kernel"].startswith("stem_")][0])}
    for k, name in enumerate(CHILD_CAMERAS):
        c = camera(torch, name)
        out[f"det{k}"] = e.infer_nv12(c["d_y"], c["d_uv"], c["w"], c["h"], c["y_pitch"], c["uv_pitch"], None, CONF, IOU, Q)
        out[f"stem{k}"] = e.read_buffer("backbone.stem")
    e.close()
    np.savez(sys.argv[1], **out)
    print("NV12_CHILD_OK")


if __name__ == "__main__":
    main()
