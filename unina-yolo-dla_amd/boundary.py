"""Track limits and centre line from the tracked cones (include/unina_mi355.h "track limits and centre line"): a stateless stage
behind the tracker. It reads the tracker's table and the camera's pose where they lie on the device and writes the left limit, the
right limit and the line between them as ordered points.

``boundary_numpy`` is the DEFINITION: fp32 scalars and arrays, one rounding per operation in the order the header states;
csrc/boundary.hip (through ``DeviceBoundaryFinder``) returns its bytes. It is also the twin of csrc/boundary_math.h, which
tests/boundary_math_host.cpp runs on the host.
NOT covered: a track seen on one side only (offsetting one chain); orange start / finish cones; closing the loop; smoothing or
splines; curvature and speed; a Delaunay or graph search in place of the greedy chain.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .engine import (BOUNDARY_FULL, BOUNDARY_HEADER_DTYPE, BOUNDARY_MAX_CHAIN, BOUNDARY_NO_FIRST, BOUNDARY_NO_HEADING, BOUNDARY_NO_NEXT,
                     BOUNDARY_POINT_DTYPE, POSE_RESULT_DTYPE, BoundaryParams, _addr, _raise_on, _stream_ptr, _torch, load_library,
                     read_records)
from .tracking import IDENTITY, TRACK_DTYPE, TRACK_MAX

F = np.float32
LIMIT = F(32768.0)                    # |x|, |y| of a candidate
N_POINTS = 4 * BOUNDARY_MAX_CHAIN     # left [0, 64), right [64, 128), centre [128, 256)
NO_KEY = np.uint64(2 ** 64 - 1)


def params(pose=None, forward=(0.0, 0.0, 1.0), first_gate=8.0, step_gate=7.4, cos_turn=math.cos(math.radians(70.0)), width_gate=6.0,
           class_left=1, class_right=0, min_hits=3, max_chain=BOUNDARY_MAX_CHAIN) -> BoundaryParams:
    """pose: 12 values or a [3, 4] array, row-major [R|t], camera -> tracking frame (None is the identity), read only where no
    device pose is given; forward: the vehicle's forward axis in the camera frame. The defaults are fsd_data.yaml's ids (blue 1 on
    the left, yellow 0 on the right) and a track of 3 m width with a cone every 5 m at the most. The floats are rounded to fp32
    once, here."""
    flat = [float(v) for v in np.asarray(IDENTITY if pose is None else pose, dtype=np.float64).reshape(-1)]
    fwd = [float(v) for v in np.asarray(forward, dtype=np.float64).reshape(-1)]
    if len(flat) != 12 or len(fwd) != 3:
        raise ValueError("a pose is 12 values, the rows of [R|t]; forward is 3")
    return BoundaryParams((C.c_float * 12)(*flat), (C.c_float * 3)(*fwd), first_gate, step_gate, cos_turn, width_gate, int(class_left),
                          int(class_right), int(min_hits), int(max_chain))


def as_params(par) -> BoundaryParams:
    """A BoundaryParams, or a dict of params' arguments."""
    return par if isinstance(par, BoundaryParams) else params(**par)


def check_params(p: BoundaryParams, device_pose: bool = False) -> None:
    """What unina_boundary_async refuses in its parameters."""
    with np.errstate(all="ignore"):
        if not device_pose and not all(np.isfinite(F(v)) for v in p.pose):
            raise ValueError("pose must be finite")
        if not all(np.isfinite(F(v)) for v in p.forward):
            raise ValueError("forward must be finite")
        for g in (p.first_gate, p.step_gate, p.width_gate):
            if not (g > 0 and np.isfinite(F(g)) and np.isfinite(F(g) * F(g))):
                raise ValueError("a gate and its square must be finite and positive")
    if not 0.0 <= p.cos_turn < 1.0:
        raise ValueError("cos_turn in [0, 1)")
    if p.min_hits < 1 or not 1 <= p.max_chain <= BOUNDARY_MAX_CHAIN:
        raise ValueError("min_hits >= 1 and max_chain in 1..64")
    if p.class_left < 0 or p.class_right < 0 or p.class_left == p.class_right:
        raise ValueError("class ids >= 0 and different")


def chain_numpy(x, y, ox, oy, hx, hy, first2, step2, cos2, max_chain):
    """One side's chain over its candidates (fp32 arrays in ascending slot order) -> (list indices in chain order, end code)."""
    used = np.zeros(len(x), dtype=bool)
    index = np.arange(len(x), dtype=np.uint64)
    chain = []
    cx, cy, ddx, ddy = ox, oy, hx, hy
    while True:
        m = len(chain)
        if m == max_chain:
            return chain, BOUNDARY_FULL
        dx, dy = x - cx, y - cy
        d2 = dx * dx + dy * dy
        dot = dx * ddx + dy * ddy
        if m == 0:
            ok = (d2 <= first2) & (dot >= 0)
        else:
            ok = (d2 <= step2) & (dot > 0) & (dot * dot >= cos2 * (d2 * (ddx * ddx + ddy * ddy)))             # a NaN fails every test
        ok &= ~used
        if not ok.any():
            return chain, BOUNDARY_NO_FIRST if m == 0 else BOUNDARY_NO_NEXT
        keys = np.where(ok, (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index, NO_KEY)
        e = int(keys.argmin())
        if m >= 1:
            ddx, ddy = x[e] - cx, y[e] - cy
        cx, cy = x[e], y[e]
        used[e] = True
        chain.append(e)


def ladder_numpy(L, R, width2):
    """The ladder walk over two chains of BOUNDARY_POINT_DTYPE records -> (centre points, n_wide)."""
    centre, n_wide = [], 0
    nl, nr = len(L), len(R)
    if nl == 0 or nr == 0:
        return centre, n_wide

    def d2(i, j):
        dx, dy = L["x"][i] - R["x"][j], L["y"][i] - R["y"][j]
        return dx * dx + dy * dy

    i = j = 0
    while True:
        if d2(i, j) <= width2:
            centre.append(((L["x"][i] + R["x"][j]) * F(0.5), (L["y"][i] + R["y"][j]) * F(0.5), (L["z"][i] + R["z"][j]) * F(0.5), i | j << 16))
        else:
            n_wide += 1
        has_i, has_j = i + 1 < nl, j + 1 < nr
        if not has_i and not has_j:
            return centre, n_wide
        if has_i and (not has_j or d2(i + 1, j) <= d2(i, j + 1)):
            i += 1
        else:
            j += 1


def boundary_numpy(tracks, pose12, par):
    """One call. tracks: the tracker's TRACK_MAX TRACK_DTYPE slots; pose12: the 12 values of the pose the call uses (the device
    pose's, or the parameters' -- None takes par.pose); par: a BoundaryParams or a dict of params' arguments. Returns (header,
    points): one BOUNDARY_HEADER_DTYPE record and the 256 BOUNDARY_POINT_DTYPE records."""
    p = as_params(par)
    check_params(p, device_pose=pose12 is not None)
    tracks = np.asarray(tracks)
    P = np.array([F(v) for v in (p.pose if pose12 is None else np.asarray(pose12).reshape(12))], dtype=F)
    f = [F(v) for v in p.forward]
    header, points = np.zeros(1, dtype=BOUNDARY_HEADER_DTYPE), np.zeros(N_POINTS, dtype=BOUNDARY_POINT_DTYPE)
    h = header[0]
    with np.errstate(all="ignore"):
        first2, step2 = F(p.first_gate) * F(p.first_gate), F(p.step_gate) * F(p.step_gate)
        cos2, width2 = F(p.cos_turn) * F(p.cos_turn), F(p.width_gate) * F(p.width_gate)
        ox, oy = P[3], P[7]
        hx = (P[0] * f[0] + P[1] * f[1]) + P[2] * f[2]
        hy = (P[4] * f[0] + P[5] * f[1]) + P[6] * f[2]
        n2 = hx * hx + hy * hy
        if not (np.isfinite(ox) and np.isfinite(oy) and np.isfinite(n2) and n2 > 0):
            h["end"][:] = BOUNDARY_NO_HEADING
            return header, points
        live = (tracks["id"] != 0) & (tracks["hits"] >= p.min_hits) & (np.abs(tracks["x"]) <= LIMIT) & (np.abs(tracks["y"]) <= LIMIT)
        chains = []
        for k, cls in enumerate((p.class_left, p.class_right)):
            slots = np.nonzero(live & (tracks["class_id"] == cls))[0]                                          # ascending slot order
            c = tracks[slots]
            order, end = chain_numpy(c["x"], c["y"], ox, oy, hx, hy, first2, step2, cos2, p.max_chain)
            side = points[k * BOUNDARY_MAX_CHAIN:k * BOUNDARY_MAX_CHAIN + len(order)]
            for name, src in (("x", "x"), ("y", "y"), ("z", "z"), ("ref", "id")):
                side[name] = c[src][order]
            h["n_candidates"][k], h["n_chain"][k], h["end"][k] = len(slots), len(order), end
            chains.append(side)
        centre, n_wide = ladder_numpy(chains[0], chains[1], width2)
        for m, c in enumerate(centre):
            points[2 * BOUNDARY_MAX_CHAIN + m] = c
        h["n_centre"], h["n_wide"] = len(centre), n_wide
    return header, points


class DeviceBoundaryFinder:
    """unina_boundary_async (csrc/boundary.hip): a memset and one launch per frame behind DeviceTracker.update_async, on the same
    stream. The call itself is stateless; this class holds the device address of the tracker's slots, the optional device pose
    (pose.DevicePoseEstimator.result) and the `points` and `header` the call writes."""

    def __init__(self, tracks, pose=None, device: int = 0):
        """tracks: a tracking.DeviceTracker (reset or updated once), or the device address (or a tensor) of UNINA_TRACK_MAX
        unina_track slots; pose: the device address (or a tensor) of a unina_pose_result, or None: the parameters' pose is used."""
        torch = _torch()
        self.L = load_library()
        self.device = device
        dev = f"cuda:{device}"
        self.tracks = tracks.buffers()[0] if hasattr(tracks, "buffers") else tracks
        self.pose = pose
        self.points = torch.zeros(N_POINTS * BOUNDARY_POINT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.header = torch.zeros(BOUNDARY_HEADER_DTYPE.itemsize, dtype=torch.uint8, device=dev)

    def find_async(self, par, stream=None, pose=None):
        """Enqueues the memset and the launch; nothing is synchronised. pose: a device pose in place of the finder's own. Returns
        (points, header), the uint8 device tensors the call writes."""
        p = as_params(par)
        d_pose = self.pose if pose is None else pose
        _raise_on(self.L.unina_boundary_async(_addr(self.tracks), _addr(d_pose), C.byref(p), self.points.data_ptr(), self.header.data_ptr(),
                                              _stream_ptr(stream)), "unina_boundary_async")
        return self.points, self.header

    def read(self, stream=None):
        """Synchronises `stream`; returns (header, points): one BOUNDARY_HEADER_DTYPE record and the 256 BOUNDARY_POINT_DTYPE
        records of the last call."""
        return read_records(stream, (self.header, BOUNDARY_HEADER_DTYPE), (self.points, BOUNDARY_POINT_DTYPE))


def split(header, points):
    """(left, right, centre): the points of a result behind their counts cut off."""
    h, n = header[0], BOUNDARY_MAX_CHAIN
    return points[:h["n_chain"][0]], points[n:n + h["n_chain"][1]], points[2 * n:2 * n + h["n_centre"]]


__all__ = ["boundary_numpy", "chain_numpy", "ladder_numpy", "params", "as_params", "check_params", "split", "DeviceBoundaryFinder",
           "BoundaryParams", "BOUNDARY_POINT_DTYPE", "BOUNDARY_HEADER_DTYPE", "BOUNDARY_MAX_CHAIN", "BOUNDARY_NO_FIRST", "BOUNDARY_NO_NEXT",
           "BOUNDARY_FULL", "BOUNDARY_NO_HEADING", "N_POINTS", "POSE_RESULT_DTYPE", "TRACK_DTYPE", "TRACK_MAX"]
