"""Raw camera images rectified -- lens undistortion and the stereo rotation in one remap (include/unina_mi355.h "Rectification").

``rectify_numpy`` is the DEFINITION and ``rectify_source_numpy`` its coordinate half, the twin of csrc/rectify_map.h: fp32
arrays, one rounding per operation in the order the header states, then integers. csrc/rectify.hip (through ``rectify_async``
and ``DeviceRectifier``) returns its bytes. Coordinates index pixel centres, as OpenCV's initUndistortRectifyMap does: K, D, R1 /
R2 and P1 / P2 of stereoRectify (or of a ROS camera_info) apply unchanged.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import (RECTIFY_MAX_DIM, RECTIFY_MAX_IMAGES, Image, Pinhole, RectifyCam, RectifyJob, _raise_on, _stream_ptr, _torch,
                     load_library)

F = np.float32
CHANNELS = (1, 3, 4)


def _pinhole(cam) -> Pinhole:
    return Pinhole(cam.fx, cam.fy, cam.cx, cam.cy) if isinstance(cam, Pinhole) else Pinhole(*[float(v) for v in cam])


def make_rectify_cam(src, dist=(0.0, 0.0, 0.0, 0.0, 0.0), r=None, dst=None) -> RectifyCam:
    """unina_rectify_cam. src: (fx, fy, cx, cy) of the raw camera matrix K; dist: (k1, k2, p1, p2, k3), OpenCV's order; r: 9
    values or a [3, 3] array, row-major, p_rect = R * p_raw (None: the identity); dst: (fx, fy, cx, cy) of P[:, :3] (None: src).
    Every field is rounded to fp32 once, here."""
    k = [float(v) for v in dist]
    if len(k) != 5:
        raise ValueError("five distortion coefficients: k1, k2, p1, p2, k3")
    rot = np.eye(3) if r is None else np.asarray(r, dtype=np.float64)
    if rot.size != 9:
        raise ValueError("r is a 3 x 3 matrix")
    return RectifyCam(_pinhole(src), *k, (C.c_float * 9)(*rot.reshape(-1).tolist()), _pinhole(src if dst is None else dst))


def rotation(axis, degrees) -> np.ndarray:
    """The float64 [3, 3] rotation by `degrees` about `axis` (Rodrigues): a stand-in for R1 / R2 where no calibration is at hand."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)


def _check_dims(what, hw):
    h, w = int(hw[0]), int(hw[1])
    if not (1 <= w <= RECTIFY_MAX_DIM and 1 <= h <= RECTIFY_MAX_DIM):
        raise ValueError(f"{what} width and height must lie in 1..{RECTIFY_MAX_DIM}")
    return h, w


def rectify_source_numpy(cam: RectifyCam, dst_hw, src_hw):
    """csrc/rectify_map.h rectify_source, rectify_inside and rectify_split for every pixel of a dst_hw = (height, width) image
    taken from a src_hw raw image. Returns (us, vs, inside, qx, qy): us, vs float32 raw-image positions of the pixel centres;
    inside bool; qx, qy int32 = floor(us * 32 + 0.5), floor(vs * 32 + 0.5) where inside, 0 elsewhere."""
    (dh, dw), (sh, sw) = _check_dims("destination", dst_hw), _check_dims("source", src_hw)
    s, d, r = cam.src, cam.dst, [F(v) for v in cam.r]
    k1, k2, p1, p2, k3 = F(cam.k1), F(cam.k2), F(cam.p1), F(cam.p2), F(cam.k3)
    one, two = F(1), F(2)
    with np.errstate(all="ignore"):
        x = ((np.arange(dw, dtype=np.float32) - F(d.cx)) / F(d.fx))[None, :]
        y = ((np.arange(dh, dtype=np.float32) - F(d.cy)) / F(d.fy))[:, None]
        X = (r[0] * x + r[3] * y) + r[6]
        Y = (r[1] * x + r[4] * y) + r[7]
        W = (r[2] * x + r[5] * y) + r[8]
        xn, yn = X / W, Y / W
        r2 = xn * xn + yn * yn
        rad = ((k3 * r2 + k2) * r2 + k1) * r2 + one
        xy2 = (two * xn) * yn
        xd = (xn * rad + p1 * xy2) + p2 * (r2 + two * (xn * xn))
        yd = (yn * rad + p1 * (r2 + two * (yn * yn))) + p2 * xy2
        us = F(s.fx) * xd + F(s.cx)
        vs = F(s.fy) * yd + F(s.cy)
        tx = us * F(32) + F(0.5)
        ty = vs * F(32) + F(0.5)
        inside = (W > F(0)) & (F(-32) <= tx) & (tx < F(32 * sw)) & (F(-32) <= ty) & (ty < F(32 * sh))      # a NaN fails
        qx = np.floor(np.where(inside, tx, F(0))).astype(np.int32)
        qy = np.floor(np.where(inside, ty, F(0))).astype(np.int32)
    assert us.dtype == np.float32 and us.shape == (dh, dw) and inside.shape == (dh, dw)
    return us, vs, inside, qx, qy


def rectify_numpy(img: np.ndarray, cam: RectifyCam, dst_hw, border: int = 0) -> np.ndarray:
    """img: [H, W] or [H, W, C] uint8, C in {1, 3, 4}. Returns the rectified image of dst_hw = (height, width) with img's channel
    layout: four taps at 1/32-pixel weights in integers, `border` for a tap or a pixel outside the raw image."""
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in CHANNELS):
        raise ValueError("img must be a [H, W] or [H, W, C] uint8 array with C in {1, 3, 4}")
    if not 0 <= int(border) <= 255:
        raise ValueError("border outside 0..255")
    sh, sw = img.shape[:2]
    _, _, inside, qx, qy = rectify_source_numpy(cam, dst_hw, (sh, sw))
    px = img.reshape(sh, sw, -1).astype(np.int32)
    padded = np.full((sh + 2, sw + 2, px.shape[2]), int(border), dtype=np.int32)        # a ring of border taps: index = tap + 1
    padded[1:-1, 1:-1] = px
    x0, y0 = (qx >> 5) + 1, (qy >> 5) + 1                                                # arithmetic shifts: tap -1 is index 0
    ax, ay = (qx & 31)[..., None], (qy & 31)[..., None]
    t00, t10, t01, t11 = padded[y0, x0], padded[y0, x0 + 1], padded[y0 + 1, x0], padded[y0 + 1, x0 + 1]
    out = ((32 - ax) * (32 - ay) * t00 + ax * (32 - ay) * t10 + (32 - ax) * ay * t01 + ax * ay * t11 + 512) >> 10
    out[~inside] = int(border)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8).reshape(tuple(int(v) for v in dst_hw) + img.shape[2:])


# ---------------------------------------------------------------- on the device
def describe(t) -> Image:
    """A uint8 CUDA tensor or view -> unina_image: [H, W] is one channel, [H, W, C] is C interleaved channels (C in {1, 3, 4}); the
    row stride is the pitch, the storage offset is arbitrary."""
    torch = _torch()
    assert t.is_cuda and t.dtype == torch.uint8 and t.dim() in (2, 3), "a uint8 CUDA tensor [H, W] or [H, W, C]"
    ch = 1 if t.dim() == 2 else int(t.shape[2])
    assert ch in CHANNELS, "1, 3 or 4 interleaved channels"
    if t.dim() == 3:
        assert (ch == 1 or t.stride(2) == 1) and (t.shape[1] == 1 or t.stride(1) == ch), "pixels are interleaved and packed along a row"
    else:
        assert t.shape[1] == 1 or t.stride(1) == 1, "pixels are packed along a row"
    h, w = int(t.shape[0]), int(t.shape[1])
    pitch = int(t.stride(0)) if h > 1 else max(int(t.stride(0)), w * ch)
    return Image(w, h, pitch, ch, t.data_ptr())


def rectify_async(jobs, stream=None) -> None:
    """unina_rectify_async: jobs = 1..4 of (cam, src, dst, border) with src and dst tensors `describe` takes (or Image structs).
    Enqueues ONE launch; nothing is synchronised. The caller keeps the tensors alive until the stream has passed the launch."""
    jobs = list(jobs)
    arr = (RectifyJob * max(1, len(jobs)))()
    for a, (cam, src, dst, border) in zip(arr, jobs):
        a.cam = cam
        a.src = src if isinstance(src, Image) else describe(src)
        a.dst = dst if isinstance(dst, Image) else describe(dst)
        a.border = int(border)
    _raise_on(load_library().unina_rectify_async(arr, len(jobs), _stream_ptr(stream)), "unina_rectify_async")


class RectifySpec:
    """One image of a DeviceRectifier: its calibration (`cam.dst` is the pinhole the locators take), the size and channel count of
    the rectified image and the border value."""

    def __init__(self, cam: RectifyCam, dst_hw, channels: int = 1, border: int = 0):
        self.cam, self.channels, self.border = cam, int(channels), int(border)
        self.dst_hw = _check_dims("destination", dst_hw)
        if self.channels not in CHANNELS or not 0 <= self.border <= 255:
            raise ValueError("channels must be 1, 3 or 4 and border in 0..255")


class DeviceRectifier:
    """unina_rectify_async (csrc/rectify.hip) for a fixed set of 1..4 cameras: holds the rectified tensors on the device ([H, W]
    uint8 for one channel, [H, W, C] otherwise; contiguous, so two planes of one size share a pitch, as DeviceStereoLocator
    wants). jobs_spec: RectifySpec objects, dicts of their arguments, or tuples (cam, dst_hw[, channels[, border]])."""

    def __init__(self, jobs_spec, device: int = 0):
        torch = _torch()
        self.L = load_library()
        self.jobs = [s if isinstance(s, RectifySpec) else RectifySpec(**s) if isinstance(s, dict) else RectifySpec(*s) for s in jobs_spec]
        if not 1 <= len(self.jobs) <= RECTIFY_MAX_IMAGES:
            raise ValueError(f"1..{RECTIFY_MAX_IMAGES} images per call")
        self.outputs = [torch.zeros(j.dst_hw if j.channels == 1 else (*j.dst_hw, j.channels), dtype=torch.uint8, device=f"cuda:{device}")
                        for j in self.jobs]
        self._keep = None      # the sources of the launch in flight

    def update(self, srcs, stream=None):
        """srcs: one uint8 CUDA tensor or view per job ([H, W] or [H, W, C]; the row stride is the pitch). Enqueues the launch;
        nothing is synchronised. Returns `outputs`."""
        srcs = list(srcs)
        assert len(srcs) == len(self.jobs), "one source per job"
        self._keep = srcs
        rectify_async([(j.cam, s, o, j.border) for j, s, o in zip(self.jobs, srcs, self.outputs)], stream)
        return self.outputs

    def read(self, stream=None):
        """Synchronises `stream`; returns the rectified images as host arrays."""
        torch = _torch()
        s = torch.cuda.current_stream() if stream is None else stream
        with torch.cuda.stream(s):
            hosts = [o.cpu() for o in self.outputs]
        self._keep = None
        return [h.numpy() for h in hosts]


__all__ = ["make_rectify_cam", "rotation", "rectify_source_numpy", "rectify_numpy", "describe", "rectify_async", "RectifySpec", "DeviceRectifier"]
