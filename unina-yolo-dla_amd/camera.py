"""Camera frames on the host side: numpy float32 twins of the pre-process the stem kernel computes (NV12, the letterbox with its
box map, and every unina_pixel_format of the frame descriptor: ``frame_to_tensor`` / ``letterbox_frame_to_tensor`` below).

``nv12_to_tensor`` is to ``unina_infer_nv12`` / ``unina_infer_tiled_nv12`` / ``unina_preprocess_nv12_resize`` what
``slicing.merge_numpy`` is to the GPU merge: the same arithmetic without a GPU, operation for operation on ``np.float32``
in the written order, so the results agree bit for bit. The definition (include/unina_mi355.h at unina_infer_nv12):

  tap at camera pixel (X, Y)      cuda_preprocess.cu:224-241
      Yv = y[Y, X];  U = uv[Y // 2, (X // 2) * 2] - 128;  V = uv[Y // 2, (X // 2) * 2 + 1] - 128
      r = Yv + 1.402 V;  g = Yv - 0.344136 U - 0.714136 V;  b = Yv + 1.772 U;  each clamped to [0, 255], kept as float
  region of the output's size     the tap, then ((v / 255) - mean) / std               (preprocess_nv12)
  any other size                  the reference has no NV12 resize; ours takes the coordinates, clamps and weights of
                                  preprocess_bgra_resize (cuda_preprocess.cu:155-178), the four float taps blended
                                  w00 t00 + w01 t01 + w10 t10 + w11 t11 left to right, then normalised
  tile (x0, y0, w, h)             source coordinates tile-local (a frame of w x h), the tap read at (x0 + xs, y0 + ys):
                                  the origin enters the chroma index, so it may be odd

``letterbox_bgra_to_tensor`` / ``letterbox_nv12_to_tensor`` / ``unmap_boxes`` are the twins of ``unina_preprocess_letterbox_*`` /
``unina_infer_letterbox_*`` (include/unina_mi355.h at unina_letterbox_geometry): the frame resized -- or, where the inner
rectangle has the frame's size, tapped -- into ``mine.letterbox_geometry``'s rectangle by the forms above evaluated for a
destination of new_w x new_h, ``pad_value`` around it, one normalise for both; kept boxes back to camera pixels as
``(x - left) * (src_w / new_w)``, each step rounded to float32, nothing clamped.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

IMAGENET = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)   # mean r, g, b, std r, g, b (cuda_preprocess.cu:73-75)

_F = np.float32


def _norm6(norm) -> Tuple[np.float32, ...]:
    if hasattr(norm, "mean_r"):                           # engine.NormParams
        norm = (norm.mean_r, norm.mean_g, norm.mean_b, norm.std_r, norm.std_g, norm.std_b)
    assert len(norm) == 6
    return tuple(_F(v) for v in norm)


def _tap(y: np.ndarray, uv: np.ndarray, X: np.ndarray, Y: np.ndarray):
    """Clamped float r, g, b at camera pixels (X, Y) (integer index arrays, broadcast against each other)."""
    Yv = y[Y, X].astype(_F)
    cx = (X // 2) * 2
    U = uv[Y // 2, cx].astype(_F) - _F(128.0)
    V = uv[Y // 2, cx + 1].astype(_F) - _F(128.0)
    r = Yv + _F(1.402) * V
    g = Yv - _F(0.344136) * U - _F(0.714136) * V
    b = Yv + _F(1.772) * U
    clamp = lambda v: np.maximum(_F(0.0), np.minimum(_F(255.0), v))
    return clamp(r), clamp(g), clamp(b)


def _axis(dst: int, src: int):
    """Source coordinates of one axis of the resize: (lower tap, upper tap, fraction), cuda_preprocess.cu:155-170."""
    scale = _F(src) / _F(dst)
    s = (np.arange(dst).astype(_F) + _F(0.5)) * scale - _F(0.5)
    s = np.maximum(_F(0.0), np.minimum(s, _F(src) - _F(1.0)))
    i0 = s.astype(np.int32)                               # (int)sx: truncation
    i1 = np.minimum(i0 + 1, src - 1)
    return i0, i1, s - i0.astype(_F)


def nv12_to_tensor(y: np.ndarray, uv: np.ndarray, dst_hw: Optional[Tuple[int, int]] = None, norm: Sequence[float] = IMAGENET,
                   origin: Tuple[int, int] = (0, 0), region: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """NV12 frame -> float32 [3, H, W] network input, RGB planar, normalised.

    y: uint8 [h, >= w] luma plane; uv: uint8 [(h + 1) // 2, >= 2 * ((w + 1) // 2)] interleaved U, V (columns beyond the frame,
    a pitch, are ignored). origin = (x0, y0) and region = (w, h): the part of the frame to read, default the whole frame
    right and below the origin. dst_hw = (H, W): the output size, default the region's (no resize)."""
    y = np.asarray(y)
    uv = np.asarray(uv)
    assert y.dtype == np.uint8 and uv.dtype == np.uint8 and y.ndim == 2 and uv.ndim == 2
    x0, y0 = int(origin[0]), int(origin[1])
    sw, sh = (y.shape[1] - x0, y.shape[0] - y0) if region is None else (int(region[0]), int(region[1]))
    if x0 < 0 or y0 < 0 or sw <= 0 or sh <= 0 or x0 + sw > y.shape[1] or y0 + sh > y.shape[0]:
        raise ValueError(f"region {sw} x {sh} at ({x0}, {y0}) is empty or not inside the {y.shape[1]} x {y.shape[0]} frame")
    if uv.shape[0] < (y0 + sh + 1) // 2 or uv.shape[1] < 2 * ((x0 + sw + 1) // 2):
        raise ValueError("chroma plane too small for the region")
    dh, dw = (sh, sw) if dst_hw is None else (int(dst_hw[0]), int(dst_hw[1]))
    if dh <= 0 or dw <= 0:
        raise ValueError("output size must be positive")
    return _normalise(_nv12_rgb(y, uv, x0, y0, sw, sh, dh, dw), norm)


def _nv12_rgb(y, uv, x0: int, y0: int, sw: int, sh: int, dh: int, dw: int):
    """Float r, g, b [dh, dw] of the region before the normalisation: the tap, or the resize's blend of four taps."""
    if (dh, dw) == (sh, sw):
        r, g, b = _tap(y, uv, x0 + np.arange(sw)[None, :], y0 + np.arange(sh)[:, None])
    else:
        xa, xb, fx = _axis(dw, sw)
        ya, yb, fy = _axis(dh, sh)
        fx, fy = fx[None, :], fy[:, None]
        one = _F(1.0)
        w00, w01, w10, w11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
        t00 = _tap(y, uv, x0 + xa[None, :], y0 + ya[:, None])
        t01 = _tap(y, uv, x0 + xb[None, :], y0 + ya[:, None])
        t10 = _tap(y, uv, x0 + xa[None, :], y0 + yb[:, None])
        t11 = _tap(y, uv, x0 + xb[None, :], y0 + yb[:, None])
        r, g, b = (w00 * t00[c] + w01 * t01[c] + w10 * t10[c] + w11 * t11[c] for c in range(3))
    return r, g, b


def _normalise(rgb, norm) -> np.ndarray:
    """((v / 255) - mean) / std per channel: float32 [3, H, W]."""
    n = _norm6(norm)
    out = np.empty((3,) + rgb[0].shape, dtype=_F)
    for c, v in enumerate(rgb):
        assert v.dtype == _F
        out[c] = ((v / _F(255.0)) - n[c]) / n[3 + c]
    return out


def _bgra_rgb(img: np.ndarray, dh: int, dw: int):
    """Float r, g, b [dh, dw] of a BGRA frame [h, w, 4] before the normalisation: the u8 channels (preprocess_bgra), or
    preprocess_bgra_resize's blend w00 p00 + w01 p01 + w10 p10 + w11 p11 left to right (cuda_preprocess.cu:155-198)."""
    sh, sw = img.shape[:2]
    if (dh, dw) == (sh, sw):
        return tuple(img[..., c].astype(_F) for c in (2, 1, 0))
    xa, xb, fx = _axis(dw, sw)
    ya, yb, fy = _axis(dh, sh)
    fx, fy = fx[None, :], fy[:, None]
    one = _F(1.0)
    w00, w01, w10, w11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    p00, p01 = img[ya[:, None], xa[None, :]], img[ya[:, None], xb[None, :]]
    p10, p11 = img[yb[:, None], xa[None, :]], img[yb[:, None], xb[None, :]]
    return tuple(w00 * p00[..., c].astype(_F) + w01 * p01[..., c].astype(_F) + w10 * p10[..., c].astype(_F) + w11 * p11[..., c].astype(_F)
                 for c in (2, 1, 0))


def _letterbox(inner_rgb, src_w: int, src_h: int, dst_hw, pad_value: float, norm) -> np.ndarray:
    from .mine import letterbox_geometry
    dh, dw = int(dst_hw[0]), int(dst_hw[1])
    if src_w <= 0 or src_h <= 0 or dh <= 0 or dw <= 0:
        raise ValueError("frame and output sizes must be positive")
    new_w, new_h, left, top = letterbox_geometry(src_w, src_h, dw, dh)
    canvas = [np.full((dh, dw), _F(pad_value), dtype=_F) for _ in range(3)]
    for plane, v in zip(canvas, inner_rgb(new_h, new_w)):
        plane[top:top + new_h, left:left + new_w] = v
    return _normalise(canvas, norm)


def letterbox_bgra_to_tensor(img: np.ndarray, dst_hw: Tuple[int, int], pad_value: float = 114.0,
                             norm: Sequence[float] = IMAGENET) -> np.ndarray:
    """BGRA frame uint8 [h, w, 4] -> float32 [3, H, W]: unina_preprocess_letterbox_bgra / the stem of
    unina_infer_letterbox_bgra, bit for bit."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 4
    return _letterbox(lambda nh, nw: _bgra_rgb(img, nh, nw), img.shape[1], img.shape[0], dst_hw, pad_value, norm)


def letterbox_nv12_to_tensor(y: np.ndarray, uv: np.ndarray, dst_hw: Tuple[int, int], pad_value: float = 114.0,
                             norm: Sequence[float] = IMAGENET) -> np.ndarray:
    """NV12 frame (planes as nv12_to_tensor takes them, the whole frame) -> float32 [3, H, W]: unina_preprocess_letterbox_nv12 /
    the stem of unina_infer_letterbox_nv12, bit for bit."""
    y = np.asarray(y)
    uv = np.asarray(uv)
    assert y.dtype == np.uint8 and uv.dtype == np.uint8 and y.ndim == 2 and uv.ndim == 2
    sh, sw = y.shape
    if uv.shape[0] < (sh + 1) // 2 or uv.shape[1] < 2 * ((sw + 1) // 2):
        raise ValueError("chroma plane too small for the frame")
    return _letterbox(lambda nh, nw: _nv12_rgb(y, uv, 0, 0, sw, sh, nh, nw), sw, sh, dst_hw, pad_value, norm)


def unmap_boxes(dets: np.ndarray, src_w: int, src_h: int, dst_w: int, dst_h: int) -> np.ndarray:
    """Records in network pixels -> a copy in camera pixels: what map_boxes = 1 does where the post-process writes the kept
    records. X = (x - float32(left)) * (float32(src_w) / float32(new_w)), each step rounded to float32; no clamp."""
    from .mine import letterbox_geometry
    new_w, new_h, left, top = letterbox_geometry(src_w, src_h, dst_w, dst_h)
    sx, sy = _F(src_w) / _F(new_w), _F(src_h) / _F(new_h)
    out = np.array(dets, copy=True)
    for k, off, sc in (("x1", left, sx), ("y1", top, sy), ("x2", left, sx), ("y2", top, sy)):
        v = (out[k].astype(_F) - _F(off)) * sc
        assert v.dtype == _F
        out[k] = v
    return out


# ---------------------------------------------------------------------------------------------- the frame descriptor's formats
# unina_pixel_format (include/unina_mi355.h); 0..3 are the transport message's codes
FMT_BGRA, FMT_NV12, FMT_RGB, FMT_RGBA, FMT_YUYV, FMT_UYVY, FMT_BAYER_RGGB, FMT_BAYER_BGGR, FMT_BAYER_GRBG, FMT_BAYER_GBRG = range(10)
BAYER_PATTERNS = {"rggb": FMT_BAYER_RGGB, "bggr": FMT_BAYER_BGGR, "grbg": FMT_BAYER_GRBG, "gbrg": FMT_BAYER_GBRG}
# where the pattern has its red site: (X & 1, Y & 1) == (rx, ry); blue lies diagonal to it
_RED_SITE = {FMT_BAYER_RGGB: (0, 0), FMT_BAYER_BGGR: (1, 1), FMT_BAYER_GRBG: (1, 0), FMT_BAYER_GBRG: (0, 1)}


def _bayer_format(pattern) -> int:
    fmt = BAYER_PATTERNS[pattern.lower()] if isinstance(pattern, str) else int(pattern)
    if fmt not in _RED_SITE:
        raise ValueError(f"not a Bayer pattern: {pattern!r}")
    return fmt


def bgra_to_rgb(img: np.ndarray) -> np.ndarray:
    """BGRA uint8 [h, w, 4] -> the same picture as packed RGB [h, w, 3]."""
    return np.ascontiguousarray(np.asarray(img)[..., [2, 1, 0]])


def bgra_to_rgba(img: np.ndarray) -> np.ndarray:
    """BGRA uint8 [h, w, 4] -> the same picture as RGBA [h, w, 4]."""
    return np.ascontiguousarray(np.asarray(img)[..., [2, 1, 0, 3]])


def nv12_to_yuv422(y: np.ndarray, uv: np.ndarray, order: str = "yuyv") -> np.ndarray:
    """NV12 planes (y [h, w], uv [(h + 1) // 2, >= 2 * ((w + 1) // 2)]) -> packed 4:2:2 uint8 [h, 4 * ((w + 1) // 2)] whose every pixel
    converts as the NV12 pixel does: row Y takes chroma row Y // 2. order: "yuyv" (Y0 U Y1 V) or "uyvy" (U Y0 V Y1). The second
    luma of the last pair of an odd-width row is 0 (it is no pixel)."""
    y, uv = np.asarray(y), np.asarray(uv)
    assert y.dtype == np.uint8 and uv.dtype == np.uint8 and y.ndim == 2 and uv.ndim == 2
    h, w = y.shape
    pairs = (w + 1) // 2
    yo = {"yuyv": 0, "uyvy": 1}[order.lower()]
    out = np.zeros((h, pairs, 4), dtype=np.uint8)
    ypad = np.zeros((h, 2 * pairs), dtype=np.uint8)
    ypad[:, :w] = y
    c = uv[np.arange(h) // 2, :2 * pairs].reshape(h, pairs, 2)
    out[..., yo], out[..., yo + 2] = ypad[:, 0::2], ypad[:, 1::2]
    out[..., 1 - yo], out[..., 3 - yo] = c[..., 0], c[..., 1]
    return out.reshape(h, 4 * pairs)


def mosaic(rgb_u8: np.ndarray, pattern) -> np.ndarray:
    """RGB uint8 [h, w, 3] -> the 8-bit Bayer mosaic [h, w] a sensor of that pattern would deliver: at each site the one channel
    the pattern has there. pattern: "rggb" / "bggr" / "grbg" / "gbrg" or the format code."""
    rgb = np.asarray(rgb_u8)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    rx, ry = _RED_SITE[_bayer_format(pattern)]
    h, w = rgb.shape[:2]
    red_col, red_row = (np.arange(w)[None, :] & 1) == rx, (np.arange(h)[:, None] & 1) == ry
    return np.where(red_col & red_row, rgb[..., 0], np.where(~red_col & ~red_row, rgb[..., 2], rgb[..., 1])).astype(np.uint8)


def bayer_to_rgb(raw: np.ndarray, pattern):
    """The bilinear demosaic of a WHOLE Bayer frame uint8 [h >= 2, w >= 2]: float32 r, g, b [h, w], the definition at
    unina_pixel_format in include/unina_mi355.h. Neighbours beyond the frame are reflected (-1 -> 1, w -> w - 2), which keeps the
    colour phase; every value is an exact multiple of 0.25."""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint8 and raw.ndim == 2 and raw.shape[0] >= 2 and raw.shape[1] >= 2
    rx, ry = _RED_SITE[_bayer_format(pattern)]
    h, w = raw.shape
    p = np.pad(raw, 1, mode="reflect").astype(_F)                 # (numpy's "reflect" is reflect-101)
    n = lambda dy, dx: p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    own = n(0, 0)
    cross = (n(-1, 0) + n(0, -1) + n(0, 1) + n(1, 0)) * _F(0.25)
    diag = (n(-1, -1) + n(-1, 1) + n(1, -1) + n(1, 1)) * _F(0.25)
    horz = (n(0, -1) + n(0, 1)) * _F(0.5)
    vert = (n(-1, 0) + n(1, 0)) * _F(0.5)
    red_col, red_row = (np.arange(w)[None, :] & 1) == rx, (np.arange(h)[:, None] & 1) == ry
    site = red_col == red_row                                      # an R or a B site
    r = np.where(site, np.where(red_row, own, diag), np.where(red_row, horz, vert))
    g = np.where(site, cross, own)
    b = np.where(site, np.where(red_row, diag, own), np.where(red_row, vert, horz))
    return r.astype(_F), g.astype(_F), b.astype(_F)


def _frame_tap(fmt: int, planes):
    """(tap(X, Y) -> float r, g, b at frame pixels, frame width, frame height) for a frame of format `fmt`."""
    fmt = int(fmt)
    if fmt == FMT_NV12:
        y, uv = (np.asarray(a) for a in planes)
        assert y.dtype == np.uint8 and uv.dtype == np.uint8 and y.ndim == 2 and uv.ndim == 2
        return (lambda X, Y: _tap(y, uv, X, Y)), y.shape[1], y.shape[0]
    a = np.asarray(planes)
    assert a.dtype == np.uint8
    if fmt in (FMT_BGRA, FMT_RGB, FMT_RGBA):
        order = (2, 1, 0) if fmt == FMT_BGRA else (0, 1, 2)
        assert a.ndim == 3 and a.shape[2] == (3 if fmt == FMT_RGB else 4)
        return (lambda X, Y: tuple(a[Y, X, c].astype(_F) for c in order)), a.shape[1], a.shape[0]
    if fmt in (FMT_YUYV, FMT_UYVY):
        assert a.ndim == 2 and a.shape[1] >= 4
        yo = 1 if fmt == FMT_UYVY else 0

        def tap(X, Y):
            pair = (X // 2) * 4
            Yv = a[Y, pair + yo + 2 * (X & 1)].astype(_F)
            U = a[Y, pair + 1 - yo].astype(_F) - _F(128.0)
            V = a[Y, pair + 3 - yo].astype(_F) - _F(128.0)
            r = Yv + _F(1.402) * V
            g = Yv - _F(0.344136) * U - _F(0.714136) * V
            b = Yv + _F(1.772) * U
            clamp = lambda v: np.maximum(_F(0.0), np.minimum(_F(255.0), v))
            return clamp(r), clamp(g), clamp(b)
        return tap, 2 * (a.shape[1] // 4), a.shape[0]
    if fmt in _RED_SITE:
        assert a.ndim == 2
        full = bayer_to_rgb(a, fmt)                                # a region's pixels are the full-frame demosaic's pixels
        return (lambda X, Y: tuple(c[Y, X] for c in full)), a.shape[1], a.shape[0]
    raise ValueError(f"unknown pixel format {fmt}")


def _region_rgb(tap, x0: int, y0: int, sw: int, sh: int, dh: int, dw: int):
    """Float r, g, b [dh, dw] of region (x0, y0, sw, sh) before the normalisation: the tap, or the resize's blend of four taps
    (the geometry of _nv12_rgb for any tap function)."""
    if (dh, dw) == (sh, sw):
        return tap(x0 + np.arange(sw)[None, :], y0 + np.arange(sh)[:, None])
    xa, xb, fx = _axis(dw, sw)
    ya, yb, fy = _axis(dh, sh)
    fx, fy = fx[None, :], fy[:, None]
    one = _F(1.0)
    w00, w01, w10, w11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    t00 = tap(x0 + xa[None, :], y0 + ya[:, None])
    t01 = tap(x0 + xb[None, :], y0 + ya[:, None])
    t10 = tap(x0 + xa[None, :], y0 + yb[:, None])
    t11 = tap(x0 + xb[None, :], y0 + yb[:, None])
    return tuple(w00 * t00[c] + w01 * t01[c] + w10 * t10[c] + w11 * t11[c] for c in range(3))


def frame_to_tensor(fmt: int, planes, dst_hw: Optional[Tuple[int, int]] = None, norm: Sequence[float] = IMAGENET,
                    origin: Tuple[int, int] = (0, 0), region: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """A camera frame of any unina_pixel_format -> float32 [3, H, W]: unina_preprocess_frame / the stem of unina_infer_frame and
    unina_infer_tiled_frame, bit for bit.

    planes: BGRA / RGBA uint8 [h, w, 4]; RGB [h, w, 3]; NV12 the pair (y, uv) as nv12_to_tensor takes it; YUYV / UYVY the packed
    rows [h, >= 4 * ((w + 1) // 2)] (the frame is taken as 2 * (columns // 4) wide: give `region` for an odd width); Bayer the
    mosaic [h, w]. origin = (x0, y0), region = (w, h): the part of the frame to read, default everything right and below the
    origin; dst_hw = (H, W): the output size, default the region's (no resize)."""
    tap, fw, fh = _frame_tap(fmt, planes)
    x0, y0 = int(origin[0]), int(origin[1])
    sw, sh = (fw - x0, fh - y0) if region is None else (int(region[0]), int(region[1]))
    if x0 < 0 or y0 < 0 or sw <= 0 or sh <= 0 or x0 + sw > fw or y0 + sh > fh:
        raise ValueError(f"region {sw} x {sh} at ({x0}, {y0}) is empty or not inside the {fw} x {fh} frame")
    dh, dw = (sh, sw) if dst_hw is None else (int(dst_hw[0]), int(dst_hw[1]))
    if dh <= 0 or dw <= 0:
        raise ValueError("output size must be positive")
    return _normalise(_region_rgb(tap, x0, y0, sw, sh, dh, dw), norm)


def letterbox_frame_to_tensor(fmt: int, planes, dst_hw: Tuple[int, int], pad_value: float = 114.0, norm: Sequence[float] = IMAGENET,
                              size: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """The whole frame (planes as frame_to_tensor takes them; size = (w, h) where they do not tell, i.e. a 4:2:2 frame of odd
    width) letterboxed into float32 [3, H, W]: unina_preprocess_letterbox_frame / the stem of unina_infer_letterbox_frame."""
    tap, fw, fh = _frame_tap(fmt, planes)
    sw, sh = (fw, fh) if size is None else (int(size[0]), int(size[1]))
    if sw <= 0 or sh <= 0 or sw > fw or sh > fh:
        raise ValueError(f"frame size {sw} x {sh} does not fit the planes ({fw} x {fh})")
    return _letterbox(lambda nh, nw: _region_rgb(tap, 0, 0, sw, sh, nh, nw), sw, sh, dst_hw, pad_value, norm)
