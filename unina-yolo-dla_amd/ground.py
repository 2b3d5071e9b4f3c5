"""The ground stripped from a LiDAR sweep, in front of the LiDAR locator (include/unina_mi355.h "ground removal from a LiDAR
sweep").

``ground_numpy`` is the DEFINITION: fp32 arrays throughout, one rounding per operation in the order the header states, integer
keys and counters behind the transform; csrc/ground.hip (through ``DeviceGroundFilter``) returns its bytes. It is also the twin
of csrc/ground_cell.h, which tests/ground_cell_host.cpp runs on the host.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import (GROUND_HEADER_DTYPE, GROUND_MAX_REACH, GROUND_MAX_SIDE, GroundParams, _raise_on, _stream_ptr, _torch, as_struct,
                     device_view, read_records)
from .localize import SweepStage, as_extrinsic, check_points, transform_numpy

F = np.float32
EMPTY = np.uint32(0xffffffff)          # no finite float's key: a cell without a seed, a cell without an envelope
NAN_WORD = np.uint32(0x7fc00000)       # the words of an entry behind the kept points, and h of a kept UNKNOWN point
OUTSIDE, UNKNOWN, GROUND, OBJECT, ABOVE = range(5)


def make_ground_params(x_min=0.0, y_min=-20.0, cell=0.5, nx=128, ny=80, z_lo=-0.5, z_hi=0.5, rise=0.1, band=0.05, max_height=0.6, reach=2,
                       keep_unknown=0) -> GroundParams:
    """unina_ground_params. The grid covers x_min .. x_min + nx * cell by y_min .. y_min + ny * cell of the level frame (metres);
    z_lo .. z_hi: the heights that may found a ground height; rise: metres per ring of cells the envelope may climb; band: a point
    up to this far above the envelope is ground; max_height: a point above this is not an object of interest."""
    return GroundParams(float(x_min), float(y_min), float(cell), int(nx), int(ny), float(z_lo), float(z_hi), float(rise), float(band),
                        float(max_height), int(reach), int(keep_unknown))


def as_ground_params(params) -> GroundParams:
    """A GroundParams, a dict of make_ground_params' arguments, or a tuple in the struct's order."""
    return as_struct(GroundParams, make_ground_params, params)


def key_numpy(values) -> np.ndarray:
    """csrc/ground_cell.h ground_key: float32 -> uint32 whose unsigned order is the order of the finite floats, -0.0 below +0.0."""
    b = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xffffffff), np.uint32(0x80000000))


def unkey_numpy(keys) -> np.ndarray:
    """ground_unkey: the float32 of a key (EMPTY gives a NaN, which no caller compares)."""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    return np.where(k >> np.uint32(31), k ^ np.uint32(0x80000000), ~k).view(np.float32)


def check_params(p: GroundParams) -> None:
    """The refusals of unina_ground_filter_async that concern the parameters."""
    finite = all(np.isfinite(v) for v in (p.x_min, p.y_min, p.cell, p.z_lo, p.z_hi, p.rise, p.band, p.max_height))
    if not (finite and p.cell > 0 and 1 <= p.nx <= GROUND_MAX_SIDE and 1 <= p.ny <= GROUND_MAX_SIDE and p.z_lo <= p.z_hi and p.rise >= 0
            and p.band >= 0 and p.max_height >= p.band and 0 <= p.reach <= GROUND_MAX_REACH):
        raise ValueError("ground parameters outside what unina_ground_filter_async accepts")


def envelope_numpy(cellmin, nx: int, ny: int, reach: int, rise) -> np.ndarray:
    """g of every cell from the nx * ny keys of cellmin: the minimum of key(value(cellmin[n]) + (float)k * rise) over the seeded
    cells n within Chebyshev distance `reach`."""
    padded = np.full((ny + 2 * reach, nx + 2 * reach), EMPTY, dtype=np.uint32)
    padded[reach:reach + ny, reach:reach + nx] = np.asarray(cellmin, dtype=np.uint32).reshape(ny, nx)
    g = np.full((ny, nx), EMPTY, dtype=np.uint32)
    with np.errstate(all="ignore"):
        for dj in range(-reach, reach + 1):
            for di in range(-reach, reach + 1):
                n = padded[reach + dj:reach + dj + ny, reach + di:reach + di + nx]
                lift = F(max(abs(di), abs(dj))) * F(rise)                              # one multiply
                term = np.where(n != EMPTY, key_numpy(unkey_numpy(n) + lift), EMPTY)   # one add
                g = np.minimum(g, term)
    return g.reshape(-1)


def ground_numpy(points, lidar_to_level, params) -> dict:
    """points: [n, >= 3] float32, x, y, z in the first three columns (n may be 0); lidar_to_level: 12 values, row-major [R|t].
    Returns labels (uint8 [n]), cell (int32 [n], -1 where a point is not IN_GRID), cellmin and ground (uint32 [ny, nx] keys),
    header (one GROUND_HEADER_DTYPE record) and out (float32 [n, 4]: the kept points' x, y, z, h first, NaN words behind)."""
    p, m = as_ground_params(params), as_extrinsic(lidar_to_level)
    check_params(p)
    pts = check_points(points)
    if not np.isfinite(m).all():
        raise ValueError("lidar_to_level must be finite")
    n, nx, ny = len(pts), p.nx, p.ny
    with np.errstate(all="ignore"):
        xl, yl, zl = transform_numpy(m, pts)
        fx = (xl - F(p.x_min)) / F(p.cell)
        fy = (yl - F(p.y_min)) / F(p.cell)
        in_grid = np.isfinite(xl) & np.isfinite(yl) & np.isfinite(zl) & (fx >= F(0)) & (fx < F(nx)) & (fy >= F(0)) & (fy < F(ny))   # a NaN fails
        seed = in_grid & (zl >= F(p.z_lo)) & (zl <= F(p.z_hi))
    ix = np.where(in_grid, fx, F(0)).astype(np.int32)                     # truncation; -0.0 is column 0
    iy = np.where(in_grid, fy, F(0)).astype(np.int32)
    cell = np.where(in_grid, iy * nx + ix, -1).astype(np.int32)
    cellmin = np.full(nx * ny, EMPTY, dtype=np.uint32)
    np.minimum.at(cellmin, cell[seed], key_numpy(zl[seed]))
    g = envelope_numpy(cellmin, nx, ny, p.reach, p.rise)
    g_pt = g[np.where(in_grid, cell, 0)]
    known = in_grid & (g_pt != EMPTY)
    with np.errstate(all="ignore"):
        gf = unkey_numpy(g_pt)
        labels = np.full(n, ABOVE, dtype=np.uint8)
        labels[zl <= gf + F(p.max_height)] = OBJECT
        labels[zl <= gf + F(p.band)] = GROUND
        h = np.ascontiguousarray(zl - gf, dtype=np.float32).view(np.uint32)
    labels[~known] = UNKNOWN
    labels[~in_grid] = OUTSIDE
    h = np.where(known, h, NAN_WORD)
    kept = (labels == OBJECT) | ((labels == UNKNOWN) & (p.keep_unknown != 0))
    n_kept = int(kept.sum())
    out = np.full((n, 4), NAN_WORD, dtype=np.uint32)
    out[:n_kept, :3] = np.ascontiguousarray(pts[kept][:, :3]).view(np.uint32)
    out[:n_kept, 3] = h[kept]
    header = np.zeros(1, dtype=GROUND_HEADER_DTYPE)
    header["n_points"], header["n_kept"], header["n_cells_seeded"] = n, n_kept, int((cellmin != EMPTY).sum())
    header["n_label"][0] = np.bincount(labels, minlength=5)
    return {"labels": labels, "cell": cell, "cellmin": cellmin.reshape(ny, nx), "ground": g.reshape(ny, nx), "header": header,
            "out": out.view(np.float32)}


def device_bytes(address: int, n_bytes: int, device: int = 0):
    """engine.device_view of bytes, under the name callers of this module know."""
    return device_view(address, n_bytes, "|u1", device)


class DeviceGroundFilter(SweepStage):
    """unina_ground_* (csrc/ground.hip): one call per sweep in front of DeviceLidarLocator.update_async. Holds the handle (its device
    workspace is bounded by max_points and the largest grid) and the max_points x 16-byte output buffer `out`."""

    def __init__(self, max_points: int = 1 << 18, device: int = 0):
        torch = _torch()
        self._create(device, "unina_ground_create", "unina_ground_destroy", max_points)
        self.out = torch.zeros((int(max_points), 16), dtype=torch.uint8, device=f"cuda:{device}")
        self._grid = (0, 0)      # nx, ny of the last call

    def filter_async(self, points, lidar_to_level, params, stream=None):
        """Enqueues the kernels; nothing is synchronised. points: a Cloud or a tensor DeviceLidarLocator.describe() takes. Returns
        the filtered cloud, a [n_points, 16] uint8 view of `out`: what DeviceLidarLocator.update_async takes as its cloud."""
        cloud, m = self._marshal(points, lidar_to_level)
        p = as_ground_params(params)
        _raise_on(self.L.unina_ground_filter_async(self.h, C.byref(cloud), C.byref(m), C.byref(p), self.out.data_ptr(), _stream_ptr(stream)),
                  "unina_ground_filter_async")
        self._n_points, self._grid = cloud.n_points, (p.nx, p.ny)
        return self.out[:cloud.n_points]

    def buffers(self):
        """Device addresses (labels, cellmin, ground, header) of the workspace; EngineError before the first call."""
        a = [C.c_void_p() for _ in range(4)]
        _raise_on(self.L.unina_ground_buffers(self.h, *[C.byref(v) for v in a]), "unina_ground_buffers")
        return tuple(v.value for v in a)

    def read(self, stream=None):
        """Synchronises `stream`; returns (header, out): the GROUND_HEADER_DTYPE record and the float32 [n_points, 4] entries of
        the last call."""
        header_at = self.buffers()[3]
        header, out = read_records(stream, (device_view(header_at, 32, device=self.device), GROUND_HEADER_DTYPE),
                                   (self.out[:self._n_points].reshape(-1), np.float32))
        self._keep = None
        return header, out.reshape(-1, 4)

    def read_labels(self, stream=None) -> np.ndarray:
        """Synchronises `stream`; returns the label byte of every point of the last call, in point order."""
        if self._n_points == 0:
            return np.zeros(0, dtype=np.uint8)
        labels, = read_records(stream, (device_view(self.buffers()[0], self._n_points, device=self.device), np.uint8))
        return labels

    def read_grids(self, stream=None):
        """Synchronises `stream`; returns (cellmin, ground): the uint32 [ny, nx] keys of the last call."""
        nx, ny = self._grid
        _, cellmin_at, ground_at, _ = self.buffers()
        cellmin, ground = read_records(stream, (device_view(cellmin_at, 4 * nx * ny, device=self.device), np.uint32),
                                       (device_view(ground_at, 4 * nx * ny, device=self.device), np.uint32))
        return cellmin.reshape(ny, nx), ground.reshape(ny, nx)


__all__ = ["ground_numpy", "envelope_numpy", "key_numpy", "unkey_numpy", "make_ground_params", "as_ground_params", "check_params",
           "DeviceGroundFilter", "device_bytes", "device_view", "EMPTY", "NAN_WORD", "OUTSIDE", "UNKNOWN", "GROUND", "OBJECT", "ABOVE"]
