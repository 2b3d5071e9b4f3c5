"""A ground-free LiDAR sweep clustered into cone candidates, behind the ground filter and in front of the tracker
(include/unina_mi355.h "cone candidates from a ground-free LiDAR sweep").

``cluster_numpy`` is the DEFINITION: fp32 arrays throughout, one rounding per operation in the order the header states, integer
keys, counters and sums behind the transform; csrc/cluster.hip (through ``DeviceClusterer``) returns its bytes. It is also the
twin of csrc/cluster_cell.h, which tests/cluster_cell_host.cpp runs on the host. Pure numpy: the components come from a
min-propagation loop, not from scipy. The records carry no colour: fusion.DeviceFuser (unina_fuse_async) associates them with the
camera's records, and a matched cone takes the detector's class.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import (CLUSTER_DTYPE, CLUSTER_HEADER_DTYPE, CONE3D_DTYPE, DET_DTYPE, GROUND_MAX_SIDE, MAX_DETECTIONS, ClusterParams, _raise_on,
                     _stream_ptr, _torch, as_struct, device_view, read_records)
from .ground import key_numpy, unkey_numpy
from .localize import SweepStage, as_extrinsic, check_points, transform_numpy

F = np.float32


def make_cluster_params(x_min=0.0, y_min=-25.6, cell=0.1, nx=512, ny=512, min_points=3, max_points=400, min_height=0.05, max_height=0.6,
                        max_width=0.45, confidence=1.0, class_id=0) -> ClusterParams:
    """unina_cluster_params. The grid covers x_min .. x_min + nx * cell by y_min .. y_min + ny * cell of the level frame (metres);
    a component is a cone candidate with min_points .. max_points points, no wider than max_width along x and along y and
    min_height .. max_height tall; confidence and class_id are what its record carries to the tracker."""
    return ClusterParams(float(x_min), float(y_min), float(cell), int(nx), int(ny), int(min_points), int(max_points), float(min_height),
                         float(max_height), float(max_width), float(confidence), int(class_id))


def as_cluster_params(params) -> ClusterParams:
    """A ClusterParams, a dict of make_cluster_params' arguments, or a tuple in the struct's order."""
    return as_struct(ClusterParams, make_cluster_params, params)


def check_params(p: ClusterParams) -> None:
    """The refusals of unina_cluster_async that concern the parameters."""
    finite = all(np.isfinite(v) for v in (p.x_min, p.y_min, p.cell, p.min_height, p.max_height, p.max_width))
    if not (finite and p.cell > 0 and 1 <= p.nx <= GROUND_MAX_SIDE and 1 <= p.ny <= GROUND_MAX_SIDE and 1 <= p.min_points <= p.max_points
            and 0 <= p.min_height <= p.max_height and p.max_width >= 0 and not np.isnan(p.confidence)):
        raise ValueError("cluster parameters outside what unina_cluster_async accepts")


def components_numpy(occupied) -> np.ndarray:
    """occupied: bool [ny, nx]. Returns int32 [ny, nx]: for an occupied cell the smallest cell index (row * nx + column) of its
    component under 8-connectivity, -1 for an empty cell. Every cell takes the minimum of the 3 x 3 labels around it and of that
    label's label until nothing changes."""
    occupied = np.asarray(occupied, dtype=bool)
    ny, nx = occupied.shape
    none = ny * nx                                                         # above every cell index; its own label
    label = np.where(occupied, np.arange(none, dtype=np.int64).reshape(ny, nx), none)
    while True:
        padded = np.full((ny + 2, nx + 2), none, dtype=np.int64)
        padded[1:-1, 1:-1] = label
        m = label
        for dj in range(3):
            for di in range(3):
                m = np.minimum(m, padded[dj:dj + ny, di:di + nx])
        m = np.where(occupied, m, none).reshape(-1)
        table = np.append(m, none)
        for _ in range(4):
            m = table[m]                                                   # a label's label is at most the label
            table[:-1] = m
        m = m.reshape(ny, nx)
        if np.array_equal(m, label):
            break
        label = m
    return np.where(occupied, label, -1).astype(np.int32)


def point_numpy(points, lidar_to_level, params):
    """csrc/cluster_cell.h cluster_point for every point: (cell int32 [n], -1 where a point is not IN_GRID; kx, ky, kz uint32 keys of
    xl, yl, zl; qx, qy int64 offsets (int)(fx * 256)); the last five are 0 where cell is -1."""
    p, m = as_cluster_params(params), as_extrinsic(lidar_to_level)
    pts = check_points(points)
    nx, ny = p.nx, p.ny
    with np.errstate(all="ignore"):
        xl, yl, zl = transform_numpy(m, pts)
        fx = (xl - F(p.x_min)) / F(p.cell)
        fy = (yl - F(p.y_min)) / F(p.cell)
        in_grid = np.isfinite(xl) & np.isfinite(yl) & np.isfinite(zl) & (fx >= F(0)) & (fx < F(nx)) & (fy >= F(0)) & (fy < F(ny))   # a NaN fails
        fx, fy = np.where(in_grid, fx, F(0)), np.where(in_grid, fy, F(0))
        cell = np.where(in_grid, fy.astype(np.int32) * nx + fx.astype(np.int32), -1).astype(np.int32)   # truncation; -0.0 is column 0
        qx, qy = (fx * F(256)).astype(np.int64), (fy * F(256)).astype(np.int64)   # exact products below 2^18
    zero = np.uint32(0)
    return (cell, np.where(in_grid, key_numpy(xl), zero), np.where(in_grid, key_numpy(yl), zero), np.where(in_grid, key_numpy(zl), zero), qx, qy)


def finish_numpy(p: ClusterParams, k_lo, k_hi, n_points, n_cells, sx, sy, root) -> np.ndarray:
    """csrc/cluster_cell.h cluster_finish for every component: k_lo, k_hi uint32 [3, k] (the minimum and maximum keys of xl, yl,
    zl), int counts, int64 sums and roots -> k CLUSTER_DTYPE records."""
    out = np.zeros(len(root), dtype=CLUSTER_DTYPE)
    n = np.asarray(n_points, dtype=np.int64)
    with np.errstate(all="ignore"):
        mean_x, mean_y = np.asarray(sx, dtype=np.int64) // np.maximum(n, 1), np.asarray(sy, dtype=np.int64) // np.maximum(n, 1)
        out["x"] = F(p.x_min) + (mean_x.astype(np.float32) * F(0.00390625)) * F(p.cell)
        out["y"] = F(p.y_min) + (mean_y.astype(np.float32) * F(0.00390625)) * F(p.cell)
        for axis, name in enumerate("xyz"):
            out[name + "_lo"], out[name + "_hi"] = unkey_numpy(k_lo[axis]), unkey_numpy(k_hi[axis])
        wx, wy, h = out["x_hi"] - out["x_lo"], out["y_hi"] - out["y_lo"], out["z_hi"] - out["z_lo"]      # an overflow to inf fails the gate
        cone = ((n >= p.min_points) & (n <= p.max_points) & (wx <= F(p.max_width)) & (wy <= F(p.max_width)) & (h >= F(p.min_height))
                & (h <= F(p.max_height)))
    out["n_points"], out["n_cells"], out["root"], out["cone"] = n, n_cells, root, cone
    return out


def records_numpy(p: ClusterParams, components):
    """(dets, cones, count): the MAX_DETECTIONS DET_DTYPE and CONE3D_DTYPE records and the count word of a component table."""
    dets, cones = np.zeros(MAX_DETECTIONS, dtype=DET_DTYPE), np.zeros(MAX_DETECTIONS, dtype=CONE3D_DTYPE)
    c = components[components["cone"] != 0][:MAX_DETECTIONS]
    k = len(c)
    d, o = dets[:k], cones[:k]
    d["x1"], d["y1"], d["x2"], d["y2"] = c["x_lo"], c["y_lo"], c["x_hi"], c["y_hi"]
    d["confidence"], d["class_id"], d["valid"] = F(p.confidence), p.class_id, 1
    o["x"], o["y"], o["z"] = c["x"], c["y"], c["z_lo"]
    o["n_valid"], o["n_samples"], o["valid"] = c["n_points"], c["n_points"], 1
    return dets, cones, np.array([k], dtype=np.int32)


def cluster_numpy(points, lidar_to_level, params) -> dict:
    """points: [n, >= 3] float32, x, y, z in the first three columns (n may be 0); lidar_to_level: 12 values, row-major [R|t].
    Returns header (one CLUSTER_HEADER_DTYPE record), components (CLUSTER_DTYPE, ascending root), point_component (int32 [n], -1
    where a point is not IN_GRID), dets and cones (MAX_DETECTIONS DET_DTYPE / CONE3D_DTYPE records, zero behind the count), count
    (int32 [1]), and cell (int32 [n]) and root (int32 [ny, nx], -1 for an empty cell) for the tests."""
    p, m = as_cluster_params(params), as_extrinsic(lidar_to_level)
    check_params(p)
    pts = check_points(points)
    if not np.isfinite(m).all():
        raise ValueError("lidar_to_level must be finite")
    n, nx, ny = len(pts), p.nx, p.ny
    cell, kx, ky, kz, qx, qy = point_numpy(pts, m, p)
    inside = cell >= 0
    occupied = np.zeros(nx * ny, dtype=bool)
    occupied[cell[inside]] = True
    root = components_numpy(occupied.reshape(ny, nx)).reshape(-1)
    roots = np.unique(root[occupied])                                       # ascending: the order of the table
    k = len(roots)
    comp = np.full(n, -1, dtype=np.int32)
    comp[inside] = np.searchsorted(roots, root[cell[inside]])
    ci = comp[inside]
    k_lo, k_hi = np.full((3, k), 0xffffffff, dtype=np.uint32), np.zeros((3, k), dtype=np.uint32)
    for axis, keys in enumerate((kx, ky, kz)):
        np.minimum.at(k_lo[axis], ci, keys[inside])
        np.maximum.at(k_hi[axis], ci, keys[inside])
    sx, sy = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
    np.add.at(sx, ci, qx[inside])
    np.add.at(sy, ci, qy[inside])
    n_points = np.bincount(ci, minlength=k)
    n_cells = np.bincount(np.searchsorted(roots, root[occupied]), minlength=k)
    components = finish_numpy(p, k_lo, k_hi, n_points, n_cells, sx, sy, roots)
    dets, cones, count = records_numpy(p, components)
    header = np.zeros(1, dtype=CLUSTER_HEADER_DTYPE)
    if n:                                                                   # n_points == 0: the all-zero header
        n_cones = int((components["cone"] != 0).sum())
        header["n_points"], header["n_in_grid"], header["n_cells"], header["n_components"] = n, int(inside.sum()), int(occupied.sum()), k
        header["n_cones"], header["n_written"], header["n_dropped"] = n_cones, int(count[0]), n_cones - int(count[0])
    return {"header": header, "components": components, "point_component": comp, "dets": dets, "cones": cones, "count": count,
            "cell": cell, "root": root.reshape(ny, nx)}


class DeviceClusterer(SweepStage):
    """unina_cluster_* (csrc/cluster.hip): one call per sweep behind DeviceGroundFilter.filter_async. Holds the handle (its device
    workspace is bounded by max_points and the largest grid) and the three outputs in the tracker's input format: `dets`
    (MAX_DETECTIONS GpuDetection), `count` (one int) and `cones` (MAX_DETECTIONS unina_cone3d, what
    DeviceTracker.update_from_buffer takes). The coordinates are the level frame's: the tracker's pose is level -> tracking."""

    def __init__(self, max_points: int = 1 << 18, device: int = 0):
        torch = _torch()
        self._create(device, "unina_cluster_create", "unina_cluster_destroy", max_points)
        self.det_buf = torch.zeros(8 + 8 * MAX_DETECTIONS, dtype=torch.int32, device=f"cuda:{device}")   # Engine.infer_async's layout
        self.count, self.dets = self.det_buf[:1], self.det_buf[8:]
        self.cones = torch.zeros(MAX_DETECTIONS * CONE3D_DTYPE.itemsize, dtype=torch.uint8, device=f"cuda:{device}")

    def cluster_async(self, points, lidar_to_level, params, stream=None):
        """Enqueues the kernels; nothing is synchronised. points: a Cloud or a tensor DeviceLidarLocator.describe() takes, normally
        what DeviceGroundFilter.filter_async returned. Returns (det_buf, cones): tracker.update_from_buffer(det_buf, cones, ...)
        goes behind it on the same stream."""
        cloud, m = self._marshal(points, lidar_to_level)
        p = as_cluster_params(params)
        _raise_on(self.L.unina_cluster_async(self.h, C.byref(cloud), C.byref(m), C.byref(p), self.dets.data_ptr(), self.count.data_ptr(),
                                             self.cones.data_ptr(), _stream_ptr(stream)), "unina_cluster_async")
        self._n_points = cloud.n_points
        return self.det_buf, self.cones

    def buffers(self):
        """Device addresses (components, point_component, header) of the workspace; EngineError before the first call."""
        a = [C.c_void_p() for _ in range(3)]
        _raise_on(self.L.unina_cluster_buffers(self.h, *[C.byref(v) for v in a]), "unina_cluster_buffers")
        return tuple(v.value for v in a)

    def read(self, stream=None):
        """Synchronises `stream`; returns (header, dets, cones, count): the CLUSTER_HEADER_DTYPE record, all MAX_DETECTIONS records
        of each array (zero behind the count) and the count word."""
        header_at = self.buffers()[2]
        header, dets, cones, count = read_records(stream, (device_view(header_at, 32, device=self.device), CLUSTER_HEADER_DTYPE),
                                                  (self.dets.view(_torch().uint8), DET_DTYPE), (self.cones, CONE3D_DTYPE),
                                                  (self.count.view(_torch().uint8), np.int32))
        self._keep = None
        return header, dets, cones, count

    def read_components(self, stream=None) -> np.ndarray:
        """Synchronises `stream`; returns the n_components CLUSTER_DTYPE records of the last call, in ascending root."""
        table_at, _, header_at = self.buffers()
        header, = read_records(stream, (device_view(header_at, 32, device=self.device), CLUSTER_HEADER_DTYPE))
        k = int(header["n_components"][0])
        if k == 0:
            return np.zeros(0, dtype=CLUSTER_DTYPE)
        table, = read_records(stream, (device_view(table_at, 48 * k, device=self.device), CLUSTER_DTYPE))
        return table

    def read_point_components(self, stream=None) -> np.ndarray:
        """Synchronises `stream`; returns the component index of every point of the last call, in point order (-1: not IN_GRID)."""
        if self._n_points == 0:
            return np.zeros(0, dtype=np.int32)
        comp, = read_records(stream, (device_view(self.buffers()[1], 4 * self._n_points, device=self.device), np.int32))
        return comp


__all__ = ["cluster_numpy", "components_numpy", "point_numpy", "finish_numpy", "records_numpy", "make_cluster_params", "as_cluster_params",
           "check_params", "DeviceClusterer"]
