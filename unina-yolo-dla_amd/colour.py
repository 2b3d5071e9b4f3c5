"""Class from pixels for records without one -- the LiDAR cones the detector missed -- behind the fuser or any locator and in front
of the tracker (include/unina_mi355.h "class from pixels").

``colour_numpy`` is the DEFINITION: the window in fp32 scalars, one rounding per operation in the order the header states, and
everything behind it in integers; csrc/colour.hip (through ``DeviceColourClassifier``) returns its bytes. It is also the twin of
csrc/colour_math.h, which tests/colour_math_host.cpp runs on the host.
NOT covered: cones cut by the image border (the silhouette is centred on the clipped grid), a camera that is not level, white
balance or exposure correction, NV12 or planar colour, raising a record's confidence, learning the thresholds from data.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import re

import numpy as np

from .engine import (COLOUR_BGR, COLOUR_DECIDED, COLOUR_DTYPE, COLOUR_HEADER_DTYPE, COLOUR_LARGE, COLOUR_LARGE_ORANGE, COLOUR_MAX_SIDE,
                     COLOUR_ORANGE, COLOUR_RGB, COLOUR_SELECTED, COLOUR_SIZE_WINDOW, COLOUR_WINDOW, COLOUR_YELLOW, DET_DTYPE, MAX_DETECTIONS,
                     ColourParams, Image, _addr, _raise_on, _stream_ptr, _torch, clamp_count, det_buffer_ptrs, load_library, read_records)
from .localize import as_pinhole, window_numpy

F = np.float32
WHITE, BLACK, OTHER = 3, 4, -1            # the bins of a pixel behind the three colours
MAX_DIM = 16384


def make_colour_params(sx=1.0, sy=1.0, shrink=1.0, half_width=0.114, above=0.175, below=0.15, max_side=COLOUR_MAX_SIDE, order=COLOUR_BGR,
                       only_class=-1, class_of=(0, 1, 2, 3), black_max=50, sat_min=96, val_min=60, white_min=150, hue_lo=(171, 850, 20),
                       hue_hi=(300, 1110, 170), taper=64, min_pixels=12, min_share=96, max_rival=128, require_stripe=0) -> ColourParams:
    """unina_colour_params. The defaults: the geometry of a small cone (228 mm base, 325 mm tall, represented 0.15 m above its
    base), class_of = fsd_data.yaml's ids (yellow 0, blue 1, orange 2, large orange 3), hue ranges yellow 171..300, blue 850..1110,
    orange 20..170 of 1536. The floats are rounded to fp32 once, here."""
    return ColourParams(float(sx), float(sy), float(shrink), float(half_width), float(above), float(below), int(max_side), int(order),
                        int(only_class), (C.c_int * 4)(*[int(v) for v in class_of]), int(black_max), int(sat_min), int(val_min), int(white_min),
                        (C.c_int * 3)(*[int(v) for v in hue_lo]), (C.c_int * 3)(*[int(v) for v in hue_hi]), int(taper), int(min_pixels),
                        int(min_share), int(max_rival), int(require_stripe))


def as_colour_params(params) -> ColourParams:
    """A ColourParams, or a dict of make_colour_params' arguments."""
    return params if isinstance(params, ColourParams) else make_colour_params(**params)


def check_params(p: ColourParams) -> None:
    """The refusals of unina_colour_async that concern the parameters."""
    ok = all(np.isfinite(v) and v > 0 for v in (p.sx, p.sy, p.shrink)) and p.shrink <= 1
    ok = ok and all(np.isfinite(v) and v >= 0 for v in (p.half_width, p.above, p.below))
    ok = ok and 1 <= p.max_side <= COLOUR_MAX_SIDE and p.order in (COLOUR_BGR, COLOUR_RGB)
    ok = ok and all(0 <= v <= 255 for v in (p.black_max, p.val_min, p.white_min)) and 1 <= p.sat_min <= 256
    ok = ok and all(0 <= v <= 1535 for v in (*p.hue_lo, *p.hue_hi))
    ok = ok and all(0 <= v <= 256 for v in (p.taper, p.min_share, p.max_rival)) and p.min_pixels >= 1
    if not ok:
        raise ValueError("colour parameters outside what unina_colour_async accepts")


def window_of(p: ColourParams, det, cone, fx, fy, width: int, height: int):
    """csrc/colour_math.h colour_window: (window dict of localize.window_numpy or None, 1 for a SIZE window). det: one DET_DTYPE
    record; cone: one CONE3D_DTYPE record or None."""
    with np.errstate(all="ignore"):
        x1, y1, x2, y2 = (F(det[n]) for n in ("x1", "y1", "x2", "y2"))
        sx, sy = F(p.sx), F(p.sy)
        X1, X2, Y1, Y2 = x1 * sx, x2 * sx, y1 * sy, y2 * sy
        if all(np.isfinite(v) for v in (X1, X2, Y1, Y2)) and X2 > X1 and Y2 > Y1:
            return window_numpy((x1, y1, x2, y2), sx, sy, p.shrink, width, height, p.max_side), 0
        if cone is None or cone["valid"] == 0:
            return None, 0
        u, v, z = F(cone["u"]), F(cone["v"]), F(cone["z"])
        if not (np.isfinite(u) and np.isfinite(v) and np.isfinite(z) and z > 0):
            return None, 0
        hw, up, down = (F(fx) * F(p.half_width)) / z, (F(fy) * F(p.above)) / z, (F(fy) * F(p.below)) / z
        w = window_numpy((u - hw, v - up, u + hw, v + down), 1.0, 1.0, p.shrink, width, height, p.max_side)
        return w, 0 if w is None else 1


def inside_numpy(cols: int, rows: int, taper: int) -> np.ndarray:
    """csrc/colour_math.h colour_inside over the grid: bool [rows, cols]."""
    c, k = np.arange(cols, dtype=np.int64)[None, :], np.arange(rows, dtype=np.int64)[:, None]
    return np.abs(2 * c - (cols - 1)) * 256 * rows <= cols * (taper * rows + (256 - taper) * (k + 1))


def hue_numpy(R, G, B):
    """csrc/colour_math.h colour_hue for integer arrays: 0..1535 where max > min, 0 elsewhere."""
    R, G, B = (np.asarray(a, dtype=np.int64) for a in (R, G, B))
    mx, mn = np.maximum(np.maximum(R, G), B), np.minimum(np.minimum(R, G), B)
    d = np.maximum(mx - mn, 1)
    hr = np.where(G >= B, 256 * (G - B) // d, (1536 - 256 * (B - G) // d) % 1536)
    hg = np.where(B >= R, 512 + 256 * (B - R) // d, 512 - 256 * (R - B) // d)
    hb = np.where(R >= G, 1024 + 256 * (R - G) // d, 1024 - 256 * (G - R) // d)
    return np.where(mx == mn, 0, np.where(mx == R, hr, np.where(mx == G, hg, hb)))


def pixel_numpy(p: ColourParams, px) -> np.ndarray:
    """csrc/colour_math.h colour_pixel: px = uint8 [..., 3 or 4] in the image's byte order -> the bins, int64 [...]: 0..2 a colour,
    WHITE, BLACK or OTHER."""
    px = np.asarray(px).astype(np.int64)
    G = px[..., 1]
    R, B = (px[..., 2], px[..., 0]) if p.order == COLOUR_BGR else (px[..., 0], px[..., 2])
    mx, mn = np.maximum(np.maximum(R, G), B), np.minimum(np.minimum(R, G), B)
    d = mx - mn
    h = hue_numpy(R, G, B)
    vote = np.full(h.shape, OTHER, dtype=np.int64)
    for c in (2, 1, 0):                                                          # the first range in the order 0, 1, 2 wins
        lo, hi = p.hue_lo[c], p.hue_hi[c]
        vote = np.where((h >= lo) & (h <= hi) if lo <= hi else (h >= lo) | (h <= hi), c, vote)
    coloured = (d * 256 >= p.sat_min * mx) & (mx >= p.val_min)
    return np.where(mx <= p.black_max, BLACK, np.where(coloured, vote, np.where(mx >= p.white_min, WHITE, OTHER)))


def rank_numpy(votes):
    """(best, second): the colour with the most votes and the one with the most of the other two; ties go to the earlier."""
    best = max(range(3), key=lambda c: (votes[c], -c))
    second = max((c for c in range(3) if c != best), key=lambda c: (votes[c], -c))
    return best, second


def letters_numpy(counts, best: int) -> str:
    """The row string: counts = int [rows, 6] (votes_k[3], white_k, black_k, mask_k) -> "B", "S" per remaining row."""
    out = []
    for v in np.asarray(counts).tolist():
        mask, stripe = v[5], v[BLACK if best == COLOUR_YELLOW else WHITE]
        if mask > 0 and 2 * v[best] >= mask:
            out.append("B")
        elif mask > 0 and 2 * stripe >= mask:
            out.append("S")
    return "".join(out)


def stripes_numpy(letters: str) -> int:
    """The maximal runs of S with a B somewhere before and a B somewhere after them."""
    first, last = letters.find("B"), letters.rfind("B")
    return 0 if first < 0 else len(re.findall("S+", letters[first:last + 1]))


def decide_numpy(p: ColourParams, votes, best: int, second: int, n_mask: int, n_stripes: int):
    """csrc/colour_math.h colour_decide: (decided, large, colour index, class_id)."""
    large = best == COLOUR_ORANGE and n_stripes >= 2 and p.class_of[COLOUR_LARGE_ORANGE] >= 0
    index = COLOUR_LARGE_ORANGE if large else best
    cls = p.class_of[index]
    decided = (n_mask >= p.min_pixels and votes[best] * 256 >= p.min_share * n_mask and votes[second] * 256 <= p.max_rival * votes[best]
               and votes[best] > 0 and (p.require_stripe == 0 or n_stripes >= 1) and cls >= 0)
    return bool(decided), bool(large and decided), index, cls


def check_image(image) -> np.ndarray:
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] not in (3, 4) or not (1 <= image.shape[0] <= MAX_DIM and 1 <= image.shape[1] <= MAX_DIM):
        raise ValueError("image: uint8 [H, W, 3 or 4] with H, W in 1..16384")
    return image


def colour_numpy(dets, count: int, cones, image, cam, params) -> dict:
    """dets / count: DET_DTYPE records and the count as the device word; cones: CONE3D_DTYPE records index-aligned with them, or
    None; image: uint8 [H, W, 3 or 4] in the byte order params.order names; cam: (fx, fy, cx, cy) or a Pinhole. Returns header (one
    COLOUR_HEADER_DTYPE record), dets and colours (MAX_DETECTIONS records each, zero behind the count)."""
    p = as_colour_params(params)
    check_params(p)
    cam = as_pinhole(cam)
    if not (all(np.isfinite(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy)) and cam.fx > 0 and cam.fy > 0):
        raise ValueError("pinhole outside what unina_colour_async accepts")
    image = check_image(image)
    height, width = image.shape[:2]
    n = clamp_count(count, dets) if cones is None else clamp_count(count, dets, cones)
    out, colours = np.zeros(MAX_DETECTIONS, dtype=DET_DTYPE), np.zeros(MAX_DETECTIONS, dtype=COLOUR_DTYPE)
    header = np.zeros(1, dtype=COLOUR_HEADER_DTYPE)
    h = header[0]
    out[:n] = np.asarray(dets)[:n]
    h["n_records"] = n
    for i in range(n):
        if p.only_class >= 0 and out["class_id"][i] != p.only_class:
            continue
        h["n_selected"] += 1
        colours["status"][i] = COLOUR_SELECTED
        w, size = window_of(p, out[i], None if cones is None else cones[i], cam.fx, cam.fy, width, height)
        if w is None:
            continue
        h["n_window"] += 1
        rows, cols = w["rows"], w["cols"]
        px = image[w["v0"]:w["v0"] + (rows - 1) * w["stride_y"] + 1:w["stride_y"], w["u0"]:w["u0"] + (cols - 1) * w["stride_x"] + 1:w["stride_x"]]
        inside = inside_numpy(cols, rows, p.taper)
        bins = pixel_numpy(p, px)
        counts = np.stack([((bins == b) & inside).sum(axis=1) for b in range(5)] + [inside.sum(axis=1)], axis=1)
        tot = counts.sum(axis=0).tolist()
        best, second = rank_numpy(tot[:3])
        n_stripes = stripes_numpy(letters_numpy(counts, best))
        decided, large, index, cls = decide_numpy(p, tot[:3], best, second, tot[5], n_stripes)
        status = COLOUR_WINDOW | COLOUR_SELECTED | (COLOUR_DECIDED if decided else 0) | (COLOUR_LARGE if large else 0) | \
            (COLOUR_SIZE_WINDOW if size else 0) | (best << 8)
        colours[i] = (tot[:3], tot[3], tot[4], tot[5], n_stripes, status)
        if decided:
            out["class_id"][i] = cls
            h["n_decided"] += 1
            h["n_class"][index] += 1
    return {"header": header, "dets": out, "colours": colours}


class DeviceColourClassifier:
    """unina_colour_async (csrc/colour.hip): a memset and one launch per frame behind DeviceFuser.fuse_from_buffers (or a locator),
    in front of DeviceTracker.update_from_buffer. The call itself is stateless; this class holds the buffers it writes: `det_buf`
    (Engine.infer_async's layout: word 0 = count, records from word 8; unused where the call is in place), `colours` and `header`."""

    def __init__(self, device: int = 0):
        torch = _torch()
        self.L = load_library()
        self.device = device
        dev = f"cuda:{device}"
        self.det_buf = torch.zeros(8 + 8 * MAX_DETECTIONS, dtype=torch.int32, device=dev)
        self.colours = torch.zeros(MAX_DETECTIONS * COLOUR_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.header = torch.zeros(COLOUR_HEADER_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.out = self.det_buf

    def classify_async(self, d_dets, d_count, d_cones, image, cam, params, d_out_dets, stream=None):
        """Enqueues the memset and the launch; nothing is synchronised. d_dets / d_count / d_cones / d_out_dets: device addresses
        (or tensors), d_cones may be None; image: a uint8 CUDA tensor [H, W, 3 or 4] (rectify.describe's rules) or an Image."""
        from .rectify import describe
        img = image if isinstance(image, Image) else describe(image)
        p, cam = as_colour_params(params), as_pinhole(cam)
        _raise_on(self.L.unina_colour_async(_addr(d_dets), _addr(d_count), _addr(d_cones), C.byref(img), C.byref(cam), C.byref(p),
                                            _addr(d_out_dets), self.colours.data_ptr(), self.header.data_ptr(), _stream_ptr(stream)),
                  "unina_colour_async")

    def classify_from_buffers(self, det_buf, cones, image, cam, params, stream=None, in_place=False):
        """The same behind Engine.infer_async's int32 buffer (DeviceFuser's det_buf) and a locator's or the fuser's cones (or None).
        in_place: the records of det_buf itself are rewritten; else the classifier's own det_buf receives them and a copy of the
        count word, on the same stream. Returns the det_buf DeviceTracker.update_from_buffer takes."""
        records, count = det_buffer_ptrs(det_buf)
        self.out = det_buf if in_place else self.det_buf
        if not in_place:
            torch = _torch()
            s = torch.cuda.ExternalStream(stream) if isinstance(stream, int) and stream else stream
            with contextlib.nullcontext() if s is None or isinstance(s, int) else torch.cuda.stream(s):
                self.det_buf[:8].copy_(det_buf[:8], non_blocking=True)
        self.classify_async(records, count, cones, image, cam, params, det_buffer_ptrs(self.out)[0], stream)
        return self.out

    def read(self, stream=None):
        """Synchronises `stream`; returns (header, dets, colours): the COLOUR_HEADER_DTYPE record and all MAX_DETECTIONS records of
        the last call's two arrays (zero behind the count)."""
        u8 = _torch().uint8
        return read_records(stream, (self.header, COLOUR_HEADER_DTYPE), (self.out[8:].view(u8), DET_DTYPE), (self.colours, COLOUR_DTYPE))


__all__ = ["colour_numpy", "window_of", "inside_numpy", "hue_numpy", "pixel_numpy", "rank_numpy", "letters_numpy", "stripes_numpy", "decide_numpy",
           "make_colour_params", "as_colour_params", "check_params", "DeviceColourClassifier", "ColourParams", "COLOUR_DTYPE", "COLOUR_HEADER_DTYPE",
           "COLOUR_BGR", "COLOUR_RGB", "COLOUR_WINDOW", "COLOUR_SELECTED", "COLOUR_DECIDED", "COLOUR_LARGE", "COLOUR_SIZE_WINDOW"]
