"""A LiDAR sweep de-skewed for the vehicle's motion, in front of the ground filter (include/unina_mi355.h "motion de-skew of a
LiDAR sweep").

``table_numpy`` is the DEFINITION of the host half: float64 scalars, one rounding per operation in the order the header states;
unina_deskew_table returns its bytes. ``deskew_numpy`` is the DEFINITION of the device half: fp32 arrays throughout, one rounding
per operation in the order the header states, integer counters behind them; csrc/deskew.hip (through ``DeviceDeskewer``) returns
its bytes. Both are the twins of csrc/deskew_math.h, which tests/deskew_math_host.cpp runs on the host.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .engine import (DESKEW_HEADER_DTYPE, DESKEW_KEY_DTYPE, DESKEW_MAX_KEYS, DESKEW_POSE_DTYPE, TIME_F32_S, TIME_U32_NS, Cloud, PointTimes,
                     _raise_on, _stream_ptr, _torch, load_library, read_records)
from .localize import DeviceLidarLocator, check_points, transform_numpy

F = np.float32
NAN_WORD = np.uint32(0x7fc00000)       # every word of an INVALID point, the carried word where there is none, a NaN result


def as_poses(poses) -> np.ndarray:
    """DESKEW_POSE_DTYPE records, or K rows of (t, qw, qx, qy, qz, px, py, pz) -> K DESKEW_POSE_DTYPE records."""
    a = np.asarray(poses)
    if a.dtype == DESKEW_POSE_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError("poses are K rows of t, qw, qx, qy, qz, px, py, pz")
    return a.view(DESKEW_POSE_DTYPE).reshape(-1)


def _dot(a, b):
    return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]


def _normalise(q):
    n = math.sqrt(_dot(q, q))
    if not (n > 0.0 and math.isfinite(n)):
        raise ValueError("a quaternion without a norm")
    return [v / n for v in q]


def _mul(a, b):
    """The Hamilton product a (x) b of (w, x, y, z) lists."""
    return [((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3], ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2],
            ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1], ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0]]


def rotation(w, x, y, z, one, two):
    """The nine elements of R(q), row by row, by the header's expressions; scalars or arrays of one float type, `one` and `two` of it."""
    return (one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
            two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
            two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y))


def table_numpy(poses, t_sweep: float, t_ref: float) -> np.ndarray:
    """The K DESKEW_KEY_DTYPE rows unina_deskew_table writes: the keys' poses relative to the pose at t_ref, in the five steps of
    the header. ValueError where the call answers UNINA_ERR_ARG."""
    P = as_poses(poses)
    K = len(P)
    t_sweep, t_ref = float(t_sweep), float(t_ref)
    if not 2 <= K <= DESKEW_MAX_KEYS:
        raise ValueError(f"2 .. {DESKEW_MAX_KEYS} keys")
    t = [float(v) for v in P["t"]]
    if not all(math.isfinite(v) for v in (t_sweep, t_ref, *t, *P["q"].reshape(-1).tolist(), *P["p"].reshape(-1).tolist())):
        raise ValueError("a non-finite field")
    q = [_normalise(row.tolist()) for row in P["q"]]                                               # step 1
    p = [row.tolist() for row in P["p"]]
    with np.errstate(all="ignore"):
        tf = (np.array(t, dtype=np.float64) - np.float64(t_sweep)).astype(np.float32)
    if not (np.isfinite(tf).all() and (tf[1:] > tf[:-1]).all()):
        raise ValueError("the float32 key times must be finite and strictly increasing")
    if not t[0] <= t_ref <= t[-1]:
        raise ValueError("t_ref outside the keys")
    r = min(sum(v <= t_ref for v in t) - 1, K - 2)                                                 # step 2
    s = (t_ref - t[r]) / (t[r + 1] - t[r])
    a, b = q[r], q[r + 1]
    if _dot(a, b) < 0.0:
        b = [-v for v in b]
    q_ref = _normalise([a[i] + s * (b[i] - a[i]) for i in range(4)])
    p_ref = [p[r][i] + s * (p[r + 1][i] - p[r][i]) for i in range(3)]
    c = [q_ref[0], -q_ref[1], -q_ref[2], -q_ref[3]]
    R = rotation(*c, 1.0, 2.0)
    D, d = [], []
    for k in range(K):
        Dk = _normalise(_mul(c, q[k]))                                                             # step 3
        v = [p[k][i] - p_ref[i] for i in range(3)]
        d.append([(R[3 * i] * v[0] + R[3 * i + 1] * v[1]) + R[3 * i + 2] * v[2] for i in range(3)])
        if (Dk[0] < 0.0) if k == 0 else (_dot(Dk, D[k - 1]) < 0.0):                                # step 4
            Dk = [-e for e in Dk]
        if k > 0 and not _dot(Dk, D[k - 1]) >= 0.5:
            raise ValueError("more than 120 degrees between two keys")
        D.append(Dk)
    out = np.zeros(K, dtype=DESKEW_KEY_DTYPE)                                                      # step 5
    with np.errstate(all="ignore"):
        rows = (np.concatenate([np.array(D, dtype=np.float64), np.array(d, dtype=np.float64)], axis=1) + 0.0).astype(np.float32)   # -0.0 + 0.0 = +0.0
    if not np.isfinite(rows).all():
        raise ValueError("a relative translation beyond fp32")
    for i, name in enumerate(("qw", "qx", "qy", "qz", "px", "py", "pz")):
        out[name] = rows[:, i]
    out["t"] = tf
    return out


def tau_numpy(times, fmt: int) -> np.ndarray:
    """tau of every point: float32 seconds as they are, uint32 nanoseconds by one conversion and one multiply."""
    times = np.asarray(times)
    if fmt == TIME_F32_S and times.dtype == np.float32:
        return times
    if fmt == TIME_U32_NS and times.dtype == np.uint32:
        return times.astype(np.float32) * F(1e-9)
    raise ValueError("times are float32 seconds (TIME_F32_S) or uint32 nanoseconds (TIME_U32_NS)")


def words(values) -> np.ndarray:
    """The words results leave as: their bits, every NaN as NAN_WORD."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    return np.where(np.isnan(v), NAN_WORD, v.view(np.uint32))


def deskew_numpy(points, times, fmt: int, carry, table) -> dict:
    """points: [n, >= 3] float32, x, y, z in the first three columns (n may be 0); times: n float32 or uint32 values as `fmt`
    names them; carry: the n uint32 words that travel with the points, or None; table: table_numpy's rows. Returns out (float32
    [n, 4]: x', y', z' and the carried word), header (one DESKEW_HEADER_DTYPE record), and per point invalid, before, after, segment,
    s and shift2 (the word of the squared shift, 0 where the point is INVALID)."""
    pts = check_points(points)
    table = np.asarray(table)
    n, K = len(pts), len(table)
    if table.dtype != DESKEW_KEY_DTYPE or not 2 <= K <= DESKEW_MAX_KEYS:
        raise ValueError(f"the table is 2 .. {DESKEW_MAX_KEYS} DESKEW_KEY_DTYPE rows")
    tau = tau_numpy(times, fmt)
    if tau.shape != (n,) or (carry is not None and (np.asarray(carry).dtype != np.uint32 or np.asarray(carry).shape != (n,))):
        raise ValueError("one time, and one uint32 carried word, per point")
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    t = table["t"]
    with np.errstate(all="ignore"):
        invalid = ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(tau))
        k = np.clip((t[None, :] <= tau[:, None]).sum(axis=1) - 1, 0, K - 2)                         # a NaN counts no key
        s = (tau - t[k]) / (t[k + 1] - t[k])
        s = np.where(s < F(0), F(0), np.where(s > F(1), F(1), s))
        before, after = ~invalid & (tau < t[0]), ~invalid & (tau > t[K - 1])
        qw, qx, qy, qz, px, py, pz = (table[name][k] + s * (table[name][k + 1] - table[name][k]) for name in ("qw", "qx", "qy", "qz", "px", "py", "pz"))
        norm = np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
        qw, qx, qy, qz = qw / norm, qx / norm, qy / norm, qz / norm
        R = rotation(qw, qx, qy, qz, F(1), F(2))
        xo, yo, zo = transform_numpy((R[0], R[1], R[2], px, R[3], R[4], R[5], py, R[6], R[7], R[8], pz), pts)
        dx, dy, dz = xo - x, yo - y, zo - z
        shift2 = words((dx * dx + dy * dy) + dz * dz)
    out = np.full((n, 4), NAN_WORD, dtype=np.uint32)
    for col, v in enumerate((xo, yo, zo)):
        out[:, col] = np.where(invalid, NAN_WORD, words(v))
    if carry is not None:
        out[:, 3] = np.where(invalid, NAN_WORD, np.asarray(carry))
    header = np.zeros(1, dtype=DESKEW_HEADER_DTYPE)
    header["n_points"], header["n_invalid"], header["n_moved"] = n, int(invalid.sum()), int((~invalid).sum())
    header["n_before"], header["n_after"] = int(before.sum()), int(after.sum())
    header["max_shift2_bits"] = int(shift2[~invalid].max()) if (~invalid).any() else 0
    return {"out": out.view(np.float32), "header": header, "invalid": invalid, "before": before, "after": after, "segment": k.astype(np.int32),
            "s": s, "shift2": np.where(invalid, np.uint32(0), shift2)}


def describe_times(times, cloud: Cloud, fmt=None) -> PointTimes:
    """unina_point_times of: a PointTimes; an int, the byte offset of the time inside each point of `cloud` (fmt names the format);
    or a 1-D CUDA tensor, one time per point: float32 seconds, or int32 / uint32 nanoseconds (a column of a wider tensor carries
    its stride)."""
    if isinstance(times, PointTimes):
        return times
    if isinstance(times, int):
        if fmt not in (TIME_F32_S, TIME_U32_NS):
            raise ValueError("a time inside the point needs fmt = TIME_F32_S or TIME_U32_NS")
        return PointTimes((cloud.points or 0) + times if cloud.n_points else None, cloud.stride, fmt)
    torch = _torch()
    assert times.is_cuda and times.dim() == 1 and times.shape[0] >= cloud.n_points
    kinds = {torch.float32: TIME_F32_S, torch.int32: TIME_U32_NS}
    if hasattr(torch, "uint32"):
        kinds[torch.uint32] = TIME_U32_NS
    if times.dtype not in kinds:
        raise ValueError(f"no time format for a {times.dtype} tensor")
    return PointTimes(times.data_ptr() if cloud.n_points else None, 4 * int(times.stride(0)) if times.shape[0] > 1 else 4, kinds[times.dtype])


class DeviceDeskewer:
    """unina_deskew_async (csrc/deskew.hip): one call per sweep in front of DeviceGroundFilter.filter_async, DeviceClusterer.cluster_async
    or DeviceLidarLocator.update_async. The call itself is stateless; this class holds the buffers it writes: the max_points x 16-byte
    cloud `out` and the 32-byte `header`."""

    def __init__(self, max_points: int = 1 << 18, device: int = 0):
        torch = _torch()
        self.L = load_library()
        self.device = device
        self.out = torch.zeros((int(max_points), 16), dtype=torch.uint8, device=f"cuda:{device}")
        self.header = torch.zeros(DESKEW_HEADER_DTYPE.itemsize, dtype=torch.uint8, device=f"cuda:{device}")
        self._keep = None      # the cloud and the times of the call in flight
        self._n_points = 0     # of the last call

    def deskew_async(self, points, times, poses, t_sweep: float, t_ref: float, carry_offset: int = -1, stream=None, fmt=None):
        """Enqueues the memset and the kernel; nothing is synchronised. points: a Cloud or a tensor DeviceLidarLocator.describe()
        takes; times: what describe_times takes; poses: what as_poses takes (host). Returns the de-skewed cloud, a [n_points, 16]
        uint8 view of `out`: what the ground filter, the clusterer and the LiDAR locator take as their cloud."""
        cloud = points if isinstance(points, Cloud) else DeviceLidarLocator.describe(points)
        if cloud.n_points > self.out.shape[0]:
            raise ValueError(f"{cloud.n_points} points, `out` holds {self.out.shape[0]}")
        when = describe_times(times, cloud, fmt)
        keys = as_poses(poses)
        self._keep = (points, times)
        _raise_on(self.L.unina_deskew_async(C.byref(cloud), C.byref(when), int(carry_offset), keys.ctypes.data, len(keys), float(t_sweep),
                                            float(t_ref), self.out.data_ptr(), self.header.data_ptr(), _stream_ptr(stream)), "unina_deskew_async")
        self._n_points = cloud.n_points
        return self.out[:cloud.n_points]

    def read(self, stream=None):
        """Synchronises `stream`; returns (header, out): the DESKEW_HEADER_DTYPE record and the float32 [n_points, 4] entries of the
        last call."""
        header, out = read_records(stream, (self.header, DESKEW_HEADER_DTYPE), (self.out[:self._n_points].reshape(-1), np.float32))
        self._keep = None
        return header, out.reshape(-1, 4)


def table_native(poses, t_sweep: float, t_ref: float) -> np.ndarray:
    """unina_deskew_table through the C ABI (no device is needed): the rows, or ValueError on UNINA_ERR_ARG."""
    keys = as_poses(poses)
    out = np.zeros(len(keys), dtype=DESKEW_KEY_DTYPE)
    if load_library().unina_deskew_table(keys.ctypes.data, len(keys), float(t_sweep), float(t_ref), out.ctypes.data):
        raise ValueError("unina_deskew_table refused the poses")
    return out


__all__ = ["table_numpy", "deskew_numpy", "tau_numpy", "words", "rotation", "as_poses", "describe_times", "table_native", "DeviceDeskewer", "PointTimes",
           "DESKEW_KEY_DTYPE", "DESKEW_HEADER_DTYPE", "DESKEW_POSE_DTYPE", "DESKEW_MAX_KEYS", "TIME_F32_S", "TIME_U32_NS", "NAN_WORD"]
