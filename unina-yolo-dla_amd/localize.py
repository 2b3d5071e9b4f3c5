"""Detections lifted to 3-D cone positions from a depth map (include/unina_mi355.h "3-D localisation") or from a rectified
stereo pair ("3-D localisation from a stereo pair"), or from a LiDAR sweep ("3-D localisation from a LiDAR sweep").

``locate_numpy`` is the DEFINITION: fp32 scalars throughout, one rounding per operation, in the order the header states;
csrc/locate.hip (through ``DeviceLocator``) returns its bytes. ``window_numpy`` is the twin of csrc/locate_window.h.
``locate_stereo_numpy`` is the definition of the stereo route in the same sense: integer costs, fp32 scalars, the twin of
csrc/stereo_match.h; csrc/stereo.hip (through ``DeviceStereoLocator``) returns its bytes.
``locate_lidar_numpy`` is the definition of the LiDAR route, ``project_lidar_numpy`` (the twin of csrc/lidar_project.h) its
per-point half; csrc/lidar.hip (through ``DeviceLidarLocator``) returns their bytes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import (CONE3D_DTYPE, DEPTH_F32, DEPTH_U16, LIDAR_MAX_DIM, LIDAR_PIXEL_DTYPE, MAX_DETECTIONS,
                     STEREO_MATCH_DTYPE, STEREO_MAX_DISPARITIES, STEREO_MAX_SIDE, Cloud, Depth, EngineError, LidarParams, LocateParams,
                     Pinhole, StereoPair, StereoParams, _addr, _raise_on, _stream_ptr, _torch, as_struct, clamp_count, det_buffer_ptrs,
                     device_view, load_library, read_records)

F = np.float32


def as_pinhole(cam) -> Pinhole:
    """(fx, fy, cx, cy) or a Pinhole -> Pinhole (the fields are rounded to fp32 once, here)."""
    return cam if isinstance(cam, Pinhole) else Pinhole(*[float(v) for v in cam])


def as_params(params) -> LocateParams:
    """A LocateParams, a dict of its fields, or (sx, sy, shrink, min_depth, max_depth, max_side, min_valid)."""
    return as_struct(LocateParams, LocateParams, params)


def _axis(c, h, n: int, max_side: int):
    """One axis of csrc/locate_window.h: (lo, hi, stride, count) or None where the window misses the map."""
    flo, fhi = np.floor(c - h), np.floor(c + h)
    if not (np.isfinite(flo) and np.isfinite(fhi)):
        return None
    last = F(n - 1)
    if fhi < F(0) or flo > last:
        return None
    lo = 0 if flo < F(0) else int(flo)
    hi = n - 1 if fhi > last else int(fhi)
    span = hi - lo + 1
    stride = (span + max_side - 1) // max_side
    return lo, hi, stride, (span - 1) // stride + 1


def window_numpy(box, sx, sy, shrink, width: int, height: int, max_side: int):
    """The window and sampling grid of one record: None where it is empty, else a dict u0, u1, v0, v1, stride_x, stride_y,
    cols, rows, n_samples (ints) and uc, vc (np.float32). `box` = (x1, y1, x2, y2)."""
    with np.errstate(all="ignore"):
        x1, y1, x2, y2 = (F(v) for v in box)
        sx, sy, shrink = F(sx), F(sy), F(shrink)
        X1, X2, Y1, Y2 = x1 * sx, x2 * sx, y1 * sy, y2 * sy
        if not (np.isfinite(X1) and np.isfinite(X2) and np.isfinite(Y1) and np.isfinite(Y2)):
            return None
        if X2 < X1 or Y2 < Y1:
            return None
        uc, vc = F(0.5) * (X1 + X2), F(0.5) * (Y1 + Y2)
        hs = F(0.5) * shrink
        hw, hh = hs * (X2 - X1), hs * (Y2 - Y1)
        ax = _axis(uc, hw, width, max_side)
        ay = _axis(vc, hh, height, max_side)
        if ax is None or ay is None:
            return None
        return {"u0": ax[0], "u1": ax[1], "stride_x": ax[2], "cols": ax[3], "v0": ay[0], "v1": ay[1], "stride_y": ay[2],
                "rows": ay[3], "n_samples": ax[3] * ay[3], "uc": uc, "vc": vc}


def point_numpy(uc, vc, Z, fx, fy, cx, cy):
    """csrc/locate_window.h locate_point: (x, y, z), the pixel (uc, vc) back-projected through the pinhole at depth Z; all
    arguments np.float32 scalars or arrays."""
    return ((uc - cx) * Z) / fx, ((vc - cy) * Z) / fy, Z


def locate_numpy(dets, count: int, depth: np.ndarray, fmt: int, unit, cam, params) -> np.ndarray:
    """dets: DET_DTYPE records; count: as the device word (clamped to 0..MAX_DETECTIONS, and to len(dets)); depth: [H, W]
    float32 (DEPTH_F32) or uint16 (DEPTH_U16). Returns MAX_DETECTIONS CONE3D_DTYPE records, zero behind the count."""
    cam, p = as_pinhole(cam), as_params(params)
    want = np.float32 if fmt == DEPTH_F32 else np.uint16
    if fmt not in (DEPTH_F32, DEPTH_U16) or depth.dtype != want or depth.ndim != 2:
        raise ValueError(f"depth map of format {fmt} must be a 2-D {np.dtype(want).name} array")
    height, width = depth.shape
    unit, lo, hi = F(unit), F(p.min_depth), F(p.max_depth)
    fx, fy, cx, cy = F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy)
    out = np.zeros(MAX_DETECTIONS, dtype=CONE3D_DTYPE)
    n = clamp_count(count, dets)
    with np.errstate(all="ignore"):
        for i in range(n):
            d = dets[i]
            w = window_numpy((d["x1"], d["y1"], d["x2"], d["y2"]), p.sx, p.sy, p.shrink, width, height, p.max_side)
            if w is None:
                continue                                                    # an empty window: the all-zero record
            raw = depth[w["v0"]:w["v1"] + 1:w["stride_y"], w["u0"]:w["u1"] + 1:w["stride_x"]].reshape(-1)
            assert raw.size == w["n_samples"]
            z = raw.astype(np.float32) * unit
            ok = (z >= lo) & (z <= hi)
            ok &= np.isfinite(raw) if fmt == DEPTH_F32 else raw != 0
            valid_raw = raw[ok]
            r = out[i]
            r["u"], r["v"], r["n_samples"], r["n_valid"] = w["uc"], w["vc"], raw.size, valid_raw.size
            if valid_raw.size >= max(1, p.min_valid):
                Z = F(np.sort(valid_raw)[(valid_raw.size - 1) // 2]) * unit    # the lower median, an actual sample
                r["x"], r["y"], r["z"] = point_numpy(w["uc"], w["vc"], Z, fx, fy, cx, cy)
                r["valid"] = 1
    return out


class DeviceLocator:
    """unina_locate_async (csrc/locate.hip): one launch per frame behind the call that produced the records. Holds the
    MAX_DETECTIONS-record output buffer on the device; engine.DeviceEval's counterpart."""

    def __init__(self, device: int = 0):
        torch = _torch()
        self.L = load_library()
        self.out = torch.zeros(MAX_DETECTIONS * CONE3D_DTYPE.itemsize, dtype=torch.uint8, device=f"cuda:{device}")
        self._keep = None      # the depth tensor of the launch in flight

    @staticmethod
    def describe(depth_tensor, fmt=None, width=None, unit: float = 1.0) -> Depth:
        """A CUDA tensor -> unina_depth. [H, W] float32: DEPTH_F32; [H, W] int16 / uint16: DEPTH_U16 (the bits are read as
        unsigned); a row stride is carried as the pitch. [H, pitch_bytes] uint8 with `fmt` and `width` given: a pitched plane
        as a camera driver hands it over."""
        torch = _torch()
        assert depth_tensor.is_cuda and depth_tensor.dim() == 2 and depth_tensor.stride(1) == 1
        if depth_tensor.dtype == torch.uint8:
            assert fmt in (DEPTH_F32, DEPTH_U16) and width is not None, "a byte plane needs its format and width"
            return Depth(fmt, int(width), int(depth_tensor.shape[0]), int(depth_tensor.stride(0)), depth_tensor.data_ptr(), unit)
        if depth_tensor.dtype == torch.float32:
            f, elem = DEPTH_F32, 4
        elif depth_tensor.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)):
            f, elem = DEPTH_U16, 2
        else:
            raise EngineError(f"no depth format for a {depth_tensor.dtype} tensor")
        assert fmt in (None, f)
        return Depth(f, int(depth_tensor.shape[1]), int(depth_tensor.shape[0]), int(depth_tensor.stride(0)) * elem,
                     depth_tensor.data_ptr(), unit)

    def update_async(self, d_dets, d_count, depth_tensor, unit, cam, params, fmt=None, width=None, stream=None):
        """Enqueues the launch; nothing is synchronised. d_dets / d_count: device addresses (or tensors) of the records and
        the count, as the _async calls write them. Returns the output tensor (bytes; read() gives the records)."""
        depth = depth_tensor if isinstance(depth_tensor, Depth) else self.describe(depth_tensor, fmt, width, unit)
        cam, p = as_pinhole(cam), as_params(params)
        self._keep = depth_tensor
        _raise_on(self.L.unina_locate_async(_addr(d_dets), _addr(d_count), C.byref(depth), C.byref(cam), C.byref(p), self.out.data_ptr(),
                                            _stream_ptr(stream)), "unina_locate_async")
        return self.out

    def update_from_buffer(self, det_buf, depth_tensor, unit, cam, params, fmt=None, width=None, stream=None):
        """The same behind Engine.infer_async's int32 buffer (word 0 = count, records from word 8)."""
        return self.update_async(*det_buffer_ptrs(det_buf), depth_tensor, unit, cam, params, fmt, width, stream)

    def read(self, stream=None) -> np.ndarray:
        """Synchronises `stream`; returns all MAX_DETECTIONS CONE3D_DTYPE records (zero behind the count)."""
        cones, = read_records(stream, (self.out, CONE3D_DTYPE))
        self._keep = None
        return cones


# ---------------------------------------------------------------- from a stereo pair
STEREO_NONE = 0xFFFFFFFF          # "no such cost" in unina_stereo_match


def make_stereo_params(sx=1.0, sy=1.0, shrink=0.5, min_depth=0.3, max_depth=40.0, max_side=64, max_mean_sad=20,
                       uniqueness=10) -> StereoParams:
    """unina_stereo_params. sx, sy: record -> plane pixels; max_mean_sad: grey levels per sample; uniqueness: per cent by which
    the second-best cost (two or more disparities away) must exceed the best."""
    return StereoParams(float(sx), float(sy), float(shrink), float(min_depth), float(max_depth), int(max_side), int(max_mean_sad),
                        int(uniqueness))


def as_stereo_params(params) -> StereoParams:
    """A StereoParams, a dict of make_stereo_params' arguments, or a tuple in the struct's order."""
    return as_struct(StereoParams, make_stereo_params, params)


def stereo_range_numpy(fx, baseline, min_depth, max_depth, width: int):
    """csrc/stereo_match.h stereo_range: (fxB, d_lo, d_hi_all), fp32, both bounds clipped in float before they become ints.
    ValueError where the entry point answers UNINA_ERR_ARG."""
    with np.errstate(all="ignore"):
        fxB = F(fx) * F(baseline)
        nearest, farthest = fxB / F(min_depth), fxB / F(max_depth)
        if not (np.isfinite(fxB) and np.isfinite(nearest)):
            raise ValueError("fx * baseline or fx * baseline / min_depth is not finite")
        lo, hi = np.ceil(farthest), np.floor(nearest)
        w, last = F(width), F(width - 1)
        lo = F(1) if lo < F(1) else lo
        lo = w if lo > w else lo
        hi = last if hi > last else hi
        d_lo, d_hi_all = int(lo), int(hi)
    if d_hi_all - d_lo + 1 > STEREO_MAX_DISPARITIES:
        raise ValueError(f"{d_hi_all - d_lo + 1} disparities ({d_lo}..{d_hi_all}): more than {STEREO_MAX_DISPARITIES}; raise min_depth")
    return fxB, d_lo, d_hi_all


def stereo_costs_numpy(left: np.ndarray, right: np.ndarray, w: dict, d_lo: int, d_hi: int) -> np.ndarray:
    """cost(d) for d = d_lo .. d_hi (uint32, index d - d_lo): the sum of |L[v, u] - R[v, u - d]| over the window's sampling grid."""
    rows = slice(w["v0"], w["v1"] + 1, w["stride_y"])
    tmpl = left[rows, w["u0"]:w["u1"] + 1:w["stride_x"]].astype(np.int32)
    last = w["u0"] + (w["cols"] - 1) * w["stride_x"]                       # the last sampled column
    strip = right[rows, w["u0"] - d_hi:last - d_lo + 1].astype(np.int32)   # offset o holds column u0 - d_hi + o
    span = last - w["u0"] + 1
    win = np.lib.stride_tricks.sliding_window_view(strip, span, axis=1)[:, :, ::w["stride_x"]]   # [rows, nd, cols], d = d_hi - o
    assert win.shape == (w["rows"], d_hi - d_lo + 1, w["cols"])
    cost = np.abs(win - tmpl[:, None, :]).sum(axis=(0, 2), dtype=np.int64)
    return cost[::-1].astype(np.uint32)


def stereo_select_numpy(cost: np.ndarray):
    """(index of the best cost -- the smaller index wins a tie --, the best cost, the least cost at two or more indices from
    it or STEREO_NONE)."""
    k = int(np.argmin(cost))                                                # the first minimum
    far = np.abs(np.arange(len(cost)) - k) > 1
    return k, int(cost[k]), int(cost[far].min()) if far.any() else STEREO_NONE


def stereo_accept_numpy(nd: int, cost_best: int, cost_second: int, n_samples: int, max_mean_sad: int, uniqueness: int) -> bool:
    """python integers: nothing overflows."""
    if nd < 1 or cost_best > max_mean_sad * n_samples:
        return False
    return cost_second == STEREO_NONE or cost_second * 100 > cost_best * (100 + uniqueness)


def stereo_disparity_numpy(d_best: int, d_lo: int, d_hi: int, cm: int, c0: int, cp: int):
    delta = F(0)
    if d_lo < d_best < d_hi:
        den = cm - 2 * c0 + cp
        if den != 0:
            delta = F(cm - cp) / F(2 * den)
    return F(d_best) + delta


def stereo_point_numpy(fxB, disparity, uc, vc, fx, fy, cx, cy):
    """(x, y, z): the box centre back-projected at Z = fxB / disparity; all arguments np.float32."""
    return point_numpy(uc, vc, fxB / disparity, fx, fy, cx, cy)


def locate_stereo_numpy(dets, count: int, left: np.ndarray, right: np.ndarray, cam, baseline, params):
    """dets: DET_DTYPE records; count: as the device word; left, right: [H, W] uint8 rectified planes. Returns (cones, matches):
    MAX_DETECTIONS CONE3D_DTYPE and MAX_DETECTIONS STEREO_MATCH_DTYPE records, zero behind the count."""
    cam, p = as_pinhole(cam), as_stereo_params(params)
    if left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim != 2 or left.shape != right.shape:
        raise ValueError("left and right must be 2-D uint8 arrays of one shape")
    if not 1 <= p.max_side <= STEREO_MAX_SIDE:
        raise ValueError(f"max_side outside 1..{STEREO_MAX_SIDE}")
    height, width = left.shape
    fx, fy, cx, cy = F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy)
    fxB, d_lo, d_hi_all = stereo_range_numpy(cam.fx, baseline, p.min_depth, p.max_depth, width)
    cones = np.zeros(MAX_DETECTIONS, dtype=CONE3D_DTYPE)
    matches = np.zeros(MAX_DETECTIONS, dtype=STEREO_MATCH_DTYPE)
    n = clamp_count(count, dets)
    with np.errstate(all="ignore"):
        for i in range(n):
            d = dets[i]
            w = window_numpy((d["x1"], d["y1"], d["x2"], d["y2"]), p.sx, p.sy, p.shrink, width, height, p.max_side)
            if w is None:
                continue                                                    # an empty window: all-zero records
            d_hi = min(d_hi_all, w["u0"])
            nd = max(0, d_hi - d_lo + 1)
            r, m = cones[i], matches[i]
            r["u"], r["v"], r["n_samples"], r["n_valid"] = w["uc"], w["vc"], w["n_samples"], nd
            if nd == 0:
                m["cost_best"] = m["cost_second"] = STEREO_NONE
                continue
            cost = stereo_costs_numpy(left, right, w, d_lo, d_hi)
            k, best, second = stereo_select_numpy(cost)
            m["d_best"], m["cost_best"], m["cost_second"] = d_lo + k, best, second
            if not stereo_accept_numpy(nd, best, second, w["n_samples"], p.max_mean_sad, p.uniqueness):
                continue
            inner = 0 < k < nd - 1
            disparity = stereo_disparity_numpy(d_lo + k, d_lo, d_hi, int(cost[k - 1]) if inner else 0, best,
                                               int(cost[k + 1]) if inner else 0)
            r["x"], r["y"], r["z"] = stereo_point_numpy(fxB, disparity, w["uc"], w["vc"], fx, fy, cx, cy)
            r["valid"] = 1
            m["disparity"] = disparity
    return cones, matches


class DeviceStereoLocator:
    """unina_locate_stereo_async (csrc/stereo.hip): one launch per frame behind the call that produced the records. Holds the
    two MAX_DETECTIONS-record output buffers on the device: `out` (unina_cone3d, what DeviceTracker.update_from_buffer takes)
    and `match` (unina_stereo_match)."""

    def __init__(self, device: int = 0):
        torch = _torch()
        self.L = load_library()
        self.out = torch.zeros(MAX_DETECTIONS * CONE3D_DTYPE.itemsize, dtype=torch.uint8, device=f"cuda:{device}")
        self.match = torch.zeros(MAX_DETECTIONS * STEREO_MATCH_DTYPE.itemsize, dtype=torch.uint8, device=f"cuda:{device}")
        self._keep = None      # the planes of the launch in flight

    @staticmethod
    def describe(left, right) -> StereoPair:
        """Two uint8 CUDA tensors or views [H, W] of one shape and row stride -> unina_stereo_pair; the row stride is the
        pitch. The halves of a side-by-side buffer (buf[:, :W] and buf[:, W:]) are such a pair."""
        torch = _torch()
        for t in (left, right):
            assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and t.stride(1) == 1
        assert left.shape == right.shape and left.stride(0) == right.stride(0), "the planes share one size and one pitch"
        return StereoPair(int(left.shape[1]), int(left.shape[0]), int(left.stride(0)), left.data_ptr(), right.data_ptr())

    def update_async(self, d_dets, d_count, pair, cam, baseline, params, stream=None, match=True):
        """Enqueues the launch; nothing is synchronised. d_dets / d_count: device addresses (or tensors) of the records and
        the count; pair: a StereoPair or (left, right) tensors; match=False passes d_match = NULL. Returns the cone tensor."""
        self._keep = pair
        desc = pair if isinstance(pair, StereoPair) else self.describe(*pair)
        cam, p = as_pinhole(cam), as_stereo_params(params)
        _raise_on(self.L.unina_locate_stereo_async(_addr(d_dets), _addr(d_count), C.byref(desc), C.byref(cam), float(baseline), C.byref(p),
                                                   self.out.data_ptr(), self.match.data_ptr() if match else None, _stream_ptr(stream)),
                  "unina_locate_stereo_async")
        return self.out

    def update_from_buffer(self, det_buf, left, right, cam, baseline, params, stream=None, match=True):
        """The same behind Engine.infer_async's int32 buffer (word 0 = count, records from word 8)."""
        return self.update_async(*det_buffer_ptrs(det_buf), (left, right), cam, baseline, params, stream, match)

    def read(self, stream=None):
        """Synchronises `stream`; returns (cones, matches): all MAX_DETECTIONS records of each (zero behind the count)."""
        records = read_records(stream, (self.out, CONE3D_DTYPE), (self.match, STEREO_MATCH_DTYPE))
        self._keep = None
        return records

# ---------------------------------------------------------------- from a LiDAR sweep
def make_lidar_params(sx=1.0, sy=1.0, shrink=0.5, min_depth=0.3, max_depth=40.0, min_valid=1) -> LidarParams:
    """unina_lidar_params. sx, sy: record -> image pixels."""
    return LidarParams(float(sx), float(sy), float(shrink), float(min_depth), float(max_depth), int(min_valid))


def as_lidar_params(params) -> LidarParams:
    """A LidarParams, a dict of make_lidar_params' arguments, or a tuple in the struct's order."""
    return as_struct(LidarParams, make_lidar_params, params)


def as_extrinsic(lidar_to_cam) -> np.ndarray:
    """12 values or a [3, 4] array, row-major [R|t], LiDAR frame -> camera frame -> 12 np.float32 (rounded once, here)."""
    m = np.asarray(lidar_to_cam, dtype=np.float64).reshape(-1).astype(np.float32)
    if m.size != 12:
        raise ValueError("an extrinsic is 12 values: the rows of [R|t]")
    return m


def check_points(points) -> np.ndarray:
    """What every twin of a sweep stage takes: a [n, >= 3] float32 array, x, y, z in the first three columns; ValueError otherwise."""
    pts = np.asarray(points)
    if pts.dtype != np.float32 or pts.ndim != 2 or pts.shape[1] < 3:
        raise ValueError("points must be a [n, >= 3] float32 array")
    return pts


def transform_numpy(m, pts):
    """csrc/cloud_io.h cloud_transform_row for every point and the three rows of the extrinsic m (12 np.float32): the three
    transformed columns, each sum rounded in the order written. The caller holds np.errstate."""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return (((m[0] * x + m[1] * y) + m[2] * z) + m[3],
            ((m[4] * x + m[5] * y) + m[6] * z) + m[7],
            ((m[8] * x + m[9] * y) + m[10] * z) + m[11])


def project_lidar_numpy(points, lidar_to_cam, cam, width: int, height: int, min_depth, max_depth) -> np.ndarray:
    """csrc/lidar_project.h lidar_project for every point. points: [n, >= 3] float32, x, y, z in the first three columns (the
    others are not read). Returns n LIDAR_PIXEL_DTYPE records in point order, all-zero where a point is not projectable."""
    cam, m = as_pinhole(cam), as_extrinsic(lidar_to_cam)
    if not (1 <= width <= LIDAR_MAX_DIM and 1 <= height <= LIDAR_MAX_DIM):
        raise ValueError(f"width and height must lie in 1..{LIDAR_MAX_DIM}")
    pts = check_points(points)
    fx, fy, cx, cy = F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy)
    out = np.zeros(len(pts), dtype=LIDAR_PIXEL_DTYPE)
    with np.errstate(all="ignore"):
        xc, yc, zc = transform_numpy(m, pts)
        u = (fx * xc) / zc + cx
        v = (fy * yc) / zc + cy
        ok = np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc) & (zc > F(0))
        ok &= (u >= F(0)) & (u < F(width)) & (v >= F(0)) & (v < F(height))                # a NaN fails
        in_range = ok & (zc >= F(min_depth)) & (zc <= F(max_depth))
    out["u"] = np.where(ok, u, F(0)).astype(np.int32)                                   # truncation; -0.0 is pixel 0
    out["v"] = np.where(ok, v, F(0)).astype(np.int32)
    out["key"] = np.where(in_range, np.ascontiguousarray(zc, dtype=np.float32).view(np.uint32), np.uint32(0))
    out["projectable"] = ok
    return out


def locate_lidar_numpy(dets, count: int, points, lidar_to_cam, cam, width: int, height: int, params, pixels=None) -> np.ndarray:
    """dets: DET_DTYPE records; count: as the device word; points: [n, >= 3] float32 (n may be 0); lidar_to_cam: 12 values, row-major
    [R|t]; width, height: the image's size. Returns MAX_DETECTIONS CONE3D_DTYPE records, zero behind the count. `pixels`: the
    result of project_lidar_numpy on the same arguments, where the caller has it already."""
    cam, p = as_pinhole(cam), as_lidar_params(params)
    if pixels is None:
        pixels = project_lidar_numpy(points, lidar_to_cam, cam, width, height, p.min_depth, p.max_depth)
    fx, fy, cx, cy = F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy)
    px = pixels[pixels["projectable"] != 0]
    pu, pv, pk = px["u"], px["v"], px["key"]
    out = np.zeros(MAX_DETECTIONS, dtype=CONE3D_DTYPE)
    n = clamp_count(count, dets)
    with np.errstate(all="ignore"):
        for i in range(n):
            d = dets[i]
            w = window_numpy((d["x1"], d["y1"], d["x2"], d["y2"]), p.sx, p.sy, p.shrink, width, height, LIDAR_MAX_DIM)
            if w is None:
                continue                                                    # an empty window: the all-zero record
            assert w["stride_x"] == w["stride_y"] == 1
            member = (pu >= w["u0"]) & (pu <= w["u1"]) & (pv >= w["v0"]) & (pv <= w["v1"])
            keys = pk[member]
            valid_keys = keys[keys != 0]
            r = out[i]
            r["u"], r["v"], r["n_samples"], r["n_valid"] = w["uc"], w["vc"], keys.size, valid_keys.size
            if valid_keys.size >= max(1, p.min_valid):
                k = (valid_keys.size - 1) // 2
                Z = np.sort(valid_keys)[k:k + 1].view(np.float32)[0]        # the lower median, an actual point's zc
                r["x"], r["y"], r["z"] = point_numpy(w["uc"], w["vc"], Z, fx, fy, cx, cy)
                r["valid"] = 1
    return out


def device_words(address: int, n_words: int, device: int = 0):
    """engine.device_view of int32 words, under the name callers of this module know."""
    return device_view(address, n_words, "<i4", device)


class SweepStage:
    """What the handles of the stages that take a LiDAR sweep share (DeviceLidarLocator, ground.DeviceGroundFilter, cluster.DeviceClusterer): the handle
    of a named create / destroy pair of the ABI, the cloud of the call in flight, and a cloud and an extrinsic as the ABI takes them."""

    def _create(self, device: int, create: str, destroy: str, *limits):
        self.L = load_library()
        self.device = device
        self._destroy = destroy
        self.h = C.c_void_p()
        _raise_on(getattr(self.L, create)(device, *[int(v) for v in limits], C.byref(self.h)), create)
        self._keep = None      # the cloud of the call in flight
        self._n_points = 0     # of the last call

    def close(self):
        if self.h:
            getattr(self.L, self._destroy)(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def _marshal(self, points, extrinsic):
        """(unina_cloud, float[12]) of a Cloud or a tensor DeviceLidarLocator.describe() takes, and 12 values; keeps the cloud alive."""
        self._keep = points
        cloud = points if isinstance(points, Cloud) else DeviceLidarLocator.describe(points)
        return cloud, (C.c_float * 12)(*as_extrinsic(extrinsic).tolist())


class DeviceLidarLocator(SweepStage):
    """unina_lidar_* (csrc/lidar.hip): one call per frame behind the call that produced the records. Holds the handle (its device
    workspace is bounded by max_points and the image limits) and the MAX_DETECTIONS-record output buffer `out`, which is what
    DeviceTracker.update_from_buffer takes."""

    def __init__(self, max_points: int = 1 << 18, max_width: int = 4096, max_height: int = 4096, device: int = 0):
        torch = _torch()
        self._create(device, "unina_lidar_create", "unina_lidar_destroy", max_points, max_width, max_height)
        self.out = torch.zeros(MAX_DETECTIONS * CONE3D_DTYPE.itemsize, dtype=torch.uint8, device=f"cuda:{device}")

    @staticmethod
    def describe(points, n_points=None) -> Cloud:
        """A CUDA tensor -> unina_cloud. [n, k] float32 with k >= 3 (x, y, z first; a row stride is carried as the point stride), or
        [n, stride_bytes] uint8 as a driver hands a packed sweep over. n_points: fewer points than the tensor holds."""
        torch = _torch()
        assert points.is_cuda and points.dim() == 2 and (points.shape[1] == 1 or points.stride(1) == 1)
        if points.dtype == torch.float32:
            assert points.shape[1] >= 3
            stride = int(points.stride(0)) * 4
        elif points.dtype == torch.uint8:
            stride = int(points.stride(0))
        else:
            raise EngineError(f"no point layout for a {points.dtype} tensor")
        n = int(points.shape[0]) if n_points is None else int(n_points)
        assert 0 <= n <= points.shape[0]
        return Cloud(n, stride, points.data_ptr() if n else None)

    def update_async(self, d_dets, d_count, points, lidar_to_cam, cam, width: int, height: int, params, stream=None):
        """Enqueues the kernels; nothing is synchronised. d_dets / d_count: device addresses (or tensors) of the records and the
        count; points: a Cloud or a tensor describe() takes. Returns the cone tensor (bytes; read() gives the records)."""
        cloud, m = self._marshal(points, lidar_to_cam)
        cam, p = as_pinhole(cam), as_lidar_params(params)
        _raise_on(self.L.unina_locate_lidar_async(self.h, _addr(d_dets), _addr(d_count), C.byref(cloud), C.byref(m), C.byref(cam), int(width),
                                                  int(height), C.byref(p), self.out.data_ptr(), _stream_ptr(stream)), "unina_locate_lidar_async")
        self._n_points = cloud.n_points
        return self.out

    def update_from_buffer(self, det_buf, points, lidar_to_cam, cam, width: int, height: int, params, stream=None):
        """The same behind Engine.infer_async's int32 buffer (word 0 = count, records from word 8)."""
        return self.update_async(*det_buffer_ptrs(det_buf), points, lidar_to_cam, cam, width, height, params, stream)

    def read(self, stream=None) -> np.ndarray:
        """Synchronises `stream`; returns all MAX_DETECTIONS CONE3D_DTYPE records (zero behind the count)."""
        cones, = read_records(stream, (self.out, CONE3D_DTYPE))
        self._keep = None
        return cones

    def read_pixels(self, stream=None) -> np.ndarray:
        """Synchronises `stream`; returns the LIDAR_PIXEL_DTYPE record of every point of the last call, in point order."""
        if self._n_points == 0:
            return np.zeros(0, dtype=LIDAR_PIXEL_DTYPE)
        address = C.c_void_p()
        _raise_on(self.L.unina_lidar_buffers(self.h, C.byref(address)), "unina_lidar_buffers")
        words = device_view(address.value, 4 * self._n_points, "<i4", self.device)
        pixels, = read_records(stream, (words, LIDAR_PIXEL_DTYPE))
        return pixels


__all__ = ["locate_numpy", "window_numpy", "point_numpy", "DeviceLocator", "as_pinhole", "as_params", "locate_stereo_numpy", "make_stereo_params",
           "as_stereo_params", "stereo_range_numpy", "DeviceStereoLocator", "locate_lidar_numpy", "project_lidar_numpy", "make_lidar_params",
           "as_lidar_params", "as_extrinsic", "check_points", "transform_numpy", "SweepStage", "DeviceLidarLocator"]
