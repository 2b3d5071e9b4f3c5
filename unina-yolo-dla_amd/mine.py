"""Active-learning data mining from the command line, in the shape of the reference's mine_data.py:164-255.

    python -m unina_yolo_dla_amd.mine --engine m.une --data <dir> --output difficulty_map.json [--limit N]
                                      [--mode entropy|loc_var] [--coreset K --coreset-output coreset.json]
                                      [--coreset-method kcenter|kmeans]

Writes ``{path: score}`` (``indent=2``, the reference's schema) and prints the five most uncertain images; with
``--coreset K`` it also pools the embeddings and writes the K paths the k-center greedy selection picks (the list itself, as
before), or with ``--coreset-method kmeans`` ``{"method": "kmeans", "paths": [...]}``: the K paths nearest to k-means centroids.

Images are read with PIL: letterbox to the engine's input size with grey 114, RGB, ``/255`` -- what mine_data.py:77-81
describes. PARITY OF THE IMAGE LOADING IS UNPINNED: the reference uses Ultralytics' ``LetterBox`` and ``cv2.resize``,
neither of which is available to this build's tests, so resampled pixels may differ from the reference's in the last bits.
``.npy`` files holding a ready ``[3,H,W]`` fp32 frame are taken as they are (and are the pinned path).

``--device-letterbox`` moves the letterbox to the GPU: an image file is uploaded as BGRA ``uint8`` (4 B/px instead of a 12 B/px
fp32 tensor) and letterboxed there by ``unina_preprocess_letterbox_bgra`` with mean 0 / std 1, i.e. the same ``/255`` frame, by
this project's own resize definition (include/unina_mi355.h at unina_letterbox_geometry) instead of PIL's.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import List, Tuple

import numpy as np

IMAGE_EXTS = (".jpg", ".jpeg", ".png", ".bmp", ".npy")


def letterbox_geometry(src_w: int, src_h: int, dst_w: int, dst_h: int) -> Tuple[int, int, int, int]:
    """(new_w, new_h, left, top): the aspect-preserving resize and the centred paste position of a letterbox
    (LetterBox(auto=False, center=True): ratio = min(dst/src), unpadded size rounded, padding split with -0.1 / +0.1 rounding)."""
    r = min(dst_h / src_h, dst_w / src_w)
    new_w, new_h = max(1, int(round(src_w * r))), max(1, int(round(src_h * r)))   # (a strip thinner than half a pixel keeps one)
    dw, dh = (dst_w - new_w) / 2, (dst_h - new_h) / 2
    return new_w, new_h, int(round(dw - 0.1)), int(round(dh - 0.1))


def load_frame(path: str, width: int, height: int) -> np.ndarray:
    """[3,H,W] fp32 in [0,1], RGB."""
    if path.lower().endswith(".npy"):
        x = np.load(path).astype(np.float32)
        if x.shape != (3, height, width):
            raise ValueError(f"{path}: frame of shape {x.shape}, the engine takes {(3, height, width)}")
        return x
    from PIL import Image
    img = Image.open(path).convert("RGB")
    new_w, new_h, left, top = letterbox_geometry(img.width, img.height, width, height)
    if (new_w, new_h) != (img.width, img.height):
        img = img.resize((new_w, new_h), Image.BILINEAR)
    canvas = np.full((height, width, 3), 114, dtype=np.uint8)
    canvas[top:top + new_h, left:left + new_w] = np.asarray(img)
    return np.ascontiguousarray(canvas.transpose(2, 0, 1)).astype(np.float32) / 255.0


def load_bgra(path: str) -> np.ndarray:
    """The image file as uint8 [h, w, 4] BGRA (alpha 255), nothing resized: what --device-letterbox uploads."""
    from PIL import Image
    rgb = np.asarray(Image.open(path).convert("RGB"))
    out = np.full(rgb.shape[:2] + (4,), 255, dtype=np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = rgb[..., 2], rgb[..., 1], rgb[..., 0]
    return out


class DeviceLetterbox:
    """load_frame's letterbox on the GPU: BGRA uint8 up, unina_preprocess_letterbox_bgra (pad 114, mean 0 / std 1) into a CUDA
    fp32 [1,3,H,W] tensor that the mining calls take as it is (mining._device_frame passes a CUDA tensor through), on the
    same stream. .npy frames are the network tensor already and go the usual way."""

    def __init__(self, engine):
        self.eng = engine
        self.norm = engine.L.create_norm_params(0.0, 0.0, 0.0, 1.0, 1.0, 1.0)

    def __call__(self, path: str):
        import torch
        e = self.eng
        if path.lower().endswith(".npy"):
            return load_frame(path, e.width, e.height)
        bgra = load_bgra(path)
        h, w = bgra.shape[:2]
        dev = torch.device("cuda", e.device)
        cam = torch.from_numpy(bgra.reshape(h, w * 4)).to(dev)
        out = torch.empty((1, 3, e.height, e.width), dtype=torch.float32, device=dev)
        rc = e.L.unina_preprocess_letterbox_bgra(cam.data_ptr(), out.data_ptr(), w, h, w * 4, e.width, e.height, 114.0, self.norm,
                                                 torch.cuda.current_stream(dev).cuda_stream)
        if rc:
            raise RuntimeError(f"{path}: unina_preprocess_letterbox_bgra failed ({rc}) for a {w} x {h} image")
        return out


def list_files(root: str) -> List[str]:
    out = []
    for d, _dirs, files in os.walk(root):
        out += [os.path.join(d, f) for f in files if f.lower().endswith(IMAGE_EXTS)]
    return sorted(out)


def run(engine, args) -> dict:
    """The body of the command with the engine object given (tests pass a stub)."""
    from . import mining
    files = list_files(args.data)
    print(f"    Found {len(files)} images.")
    if not files:
        print("Exiting.")
        return {}
    if args.limit > 0 and args.limit < len(files):
        files = files[:args.limit]
        print(f"    Limited to {args.limit} images.")
    if getattr(args, "device_letterbox", False):
        on_device = DeviceLetterbox(engine)
        frames = (on_device(p) for p in files)
    else:
        frames = (load_frame(p, engine.width, engine.height) for p in files)
    k = 6 + mining.MODES.index(args.mode)
    if args.coreset > 0:
        sc, emb, paths = mining.mine_frames(engine, frames, files)
        scores = {p: float(s[k]) for p, s in zip(paths, sc)}
    else:
        scores = mining.compute_difficulty_scores(engine, frames, files, args.mode)
    print(f">>> Mining complete. Computed scores for {len(scores)} images.")
    with open(args.output, "w") as f:
        json.dump(scores, f, indent=2)
    print("\nTop 5 Most Uncertain Images:")
    for path, score in sorted(scores.items(), key=lambda kv: kv[1], reverse=True)[:5]:
        print(f"  {os.path.basename(path)}: {score:.4f}")
    if args.coreset > 0:
        method = getattr(args, "coreset_method", "kcenter")
        chosen = mining.coreset_selection(emb, paths, args.coreset, method=method, seed=args.seed, device=getattr(args, "device_kcenter", None))
        with open(args.coreset_output, "w") as f:
            # k-center writes the bare list it has always written; another method names itself beside its paths
            json.dump(chosen if method == "kcenter" else {"method": method, "paths": chosen}, f, indent=2)
        print(f">>> Coreset ({method}): {len(chosen)} paths -> {args.coreset_output}")
    return scores


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Active Learning Data Mining (MI355X engine)")
    ap.add_argument("--engine", required=True, help="engine file written by export.py (.une)")
    ap.add_argument("--data", required=True, help="folder of unlabeled images (or .npy frames)")
    ap.add_argument("--output", default="difficulty_map.json", help="output JSON path")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--limit", type=int, default=0, help="limit the number of images (0 = all)")
    ap.add_argument("--mode", default="entropy", choices=("entropy", "loc_var"))
    ap.add_argument("--coreset", type=int, default=0, help="also select this many diverse samples (k-center greedy)")
    ap.add_argument("--coreset-output", default="coreset.json")
    ap.add_argument("--coreset-method", default="kcenter", choices=("kcenter", "kmeans"),
                    help="kcenter: k-center greedy; kmeans: the samples nearest to k-means centroids (for large sets)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the k-center start point / of the k-means++ starts")
    ap.add_argument("--device-letterbox", action="store_true",
                    help="letterbox image files on the GPU (BGRA uint8 upload + unina_preprocess_letterbox_bgra) instead of with PIL")
    return ap


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    import torch  # noqa: F401  (first: the engine library then shares the HIP runtime that torch has loaded)
    from .engine import Engine
    print(f">>> Loading engine {args.engine}...")
    eng = Engine(args.engine, args.device)
    try:
        run(eng, args)
    finally:
        eng.close()
    print(">>> Done!")
    return 0


if __name__ == "__main__":
    sys.exit(main())
