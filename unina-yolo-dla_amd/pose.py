"""The camera's pose from the tracked cones (include/unina_mi355.h "pose from the tracked cones"): a stateless stage behind any
locator, the fuser or the colour stage and in front of the tracker, which then runs with the identity pose.

``pose_numpy`` is the DEFINITION: fp32 and float64 scalars and arrays, one rounding per operation in the order the header states,
exact 64-bit integer sums; csrc/pose.hip (through ``DevicePoseEstimator``) returns its bytes. It is also the twin of
csrc/pose_math.h, which tests/pose_math_host.cpp runs on the host.
NOT covered: roll, pitch and height correction; re-orthonormalising a long chain of composed poses (re-seed without `prev`);
outlier-robust weights; loop closure; feeding the estimate to unina_deskew_table.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import (CONE3D_DTYPE, DET_DTYPE, MAX_DETECTIONS, POSE_DEGENERATE, POSE_HEADER_DTYPE, POSE_MAX_ITERATIONS, POSE_OK,
                     POSE_RESULT_DTYPE, POSE_TOO_FEW, PoseParams, _addr, _raise_on, _stream_ptr, _torch, clamp_count, det_buffer_ptrs,
                     load_library, read_records)
from .tracking import IDENTITY, TRACK_DTYPE, TRACK_MAX, d2_numpy, point_numpy

F = np.float32
D = np.float64
LIMIT = F(32768.0)                    # |x|, |y| of a point or a landmark that may vote
SCALE = F(1024.0)                     # fixed-point steps per metre
NO_KEY = np.uint64(2 ** 64 - 1)


def make_params(inc=None, gate=1.0, class_aware=1, min_hits=3, iterations=4, min_pairs=3) -> PoseParams:
    """inc: 12 values or a [3, 4] array, row-major [R|t]: the prior camera -> tracking pose, or with `prev` this frame's camera ->
    the last frame's camera; None is the identity. The floats are rounded to fp32 once, here."""
    flat = [float(v) for v in np.asarray(IDENTITY if inc is None else inc, dtype=np.float64).reshape(-1)]
    if len(flat) != 12:
        raise ValueError("a pose is 12 values: the rows of [R|t]")
    return PoseParams((C.c_float * 12)(*flat), gate, int(class_aware), int(min_hits), int(iterations), int(min_pairs))


def as_params(params) -> PoseParams:
    """A PoseParams, or a dict of make_params' arguments."""
    return params if isinstance(params, PoseParams) else make_params(**params)


def check_params(p: PoseParams) -> None:
    """What unina_pose_async refuses in its parameters."""
    with np.errstate(all="ignore"):
        if not all(np.isfinite(F(v)) for v in p.inc):
            raise ValueError("inc must be finite")
        if not (p.gate > 0 and np.isfinite(F(p.gate) * F(p.gate))):
            raise ValueError("gate and gate * gate must be finite and positive")
    if p.min_hits < 1 or not 1 <= p.iterations <= POSE_MAX_ITERATIONS or p.min_pairs < 2:
        raise ValueError("min_hits >= 1, iterations in 1..8 and min_pairs >= 2")


def compose_numpy(a, b) -> np.ndarray:
    """csrc/pose_math.h pose_compose: a o b for two row-major 3 x 4 [R|t] of 12 fp32 values each."""
    a, b = np.asarray(a, dtype=F).reshape(12), np.asarray(b, dtype=F).reshape(12)
    o = np.zeros(12, dtype=F)
    with np.errstate(all="ignore"):
        for r in range(3):
            for k in range(4):
                v = (a[4 * r] * b[k] + a[4 * r + 1] * b[4 + k]) + a[4 * r + 2] * b[8 + k]
                o[4 * r + k] = v + a[4 * r + 3] if k == 3 else v
    return o


def move_numpy(corr, px, py):
    """pose_move: fp32 scalars or arrays under the correction (c, s, tx, ty)."""
    c, s, tx, ty = corr
    return (c * px - s * py) + tx, (s * px + c * py) + ty


def solve_numpy(n, spx, spy, smx, smy, sdot, scross):
    """pose_solve: the seven integer sums of n >= 1 pairs -> ((c, s, tx, ty) as fp32, status)."""
    with np.errstate(all="ignore"):
        n, px, py, mx, my = D(int(n)), D(int(spx)), D(int(spy)), D(int(smx)), D(int(smy))
        a = D(int(sdot)) - (px * mx + py * my) / n
        b = D(int(scross)) - (px * my - py * mx) / n
        af, bf = F(a), F(b)
        h = np.sqrt(af * af + bf * bf)
        if np.isfinite(h) and h > 0:
            c, s, status = af / h, bf / h, POSE_OK
        else:
            c, s, status = F(1.0), F(0.0), POSE_DEGENERATE
        cd, sd = D(c), D(s)
        tx = F(((mx - (cd * px - sd * py)) / n) / D(1024.0))
        ty = F(((my - (sd * px + cd * py)) / n) / D(1024.0))
    return (c, s, tx, ty), status


def corrected_numpy(corr, prior) -> np.ndarray:
    """pose_corrected: rows 0 and 1 of the prior turned and shifted, row 2 kept."""
    c, s, tx, ty = corr
    o = np.array(prior, dtype=F)
    with np.errstate(all="ignore"):
        for k in range(4):
            a, b = c * prior[k] - s * prior[4 + k], s * prior[k] + c * prior[4 + k]
            o[k], o[4 + k] = (a + tx, b + ty) if k == 3 else (a, b)
    return o


def in_field(x, y):
    with np.errstate(invalid="ignore"):
        return (np.abs(x) <= LIMIT) & (np.abs(y) <= LIMIT)                    # a NaN fails


def pose_numpy(dets, count: int, cones, tracks, prev, params) -> dict:
    """One call. dets / count / cones: DET_DTYPE records, the count as the device word and CONE3D_DTYPE records, index-aligned;
    tracks: the tracker's TRACK_MAX TRACK_DTYPE slots; prev: one POSE_RESULT_DTYPE record (an earlier result) or None. Returns
    header (one POSE_HEADER_DTYPE record), result (one POSE_RESULT_DTYPE record) and cones (the records in the tracking frame, as
    many as were given)."""
    p = as_params(params)
    check_params(p)
    inc = np.array([F(v) for v in p.inc], dtype=F)
    prior = inc if prev is None else compose_numpy(np.asarray(prev)["pose"].reshape(12), inc)
    gate2 = F(p.gate) * F(p.gate)
    cones, tracks = np.asarray(cones), np.asarray(tracks)
    n = clamp_count(count, dets, cones)
    out = cones.copy()
    header, result = np.zeros(1, dtype=POSE_HEADER_DTYPE), np.zeros(1, dtype=POSE_RESULT_DTYPE)
    corr = (F(1.0), F(0.0), F(0.0), F(0.0))
    status, n_pairs, updates, max_bits = POSE_OK, 0, 0, 0
    with np.errstate(all="ignore"):
        px, py, pz = point_numpy(prior, cones["x"][:n], cones["y"][:n], cones["z"][:n])
        usable = (cones["valid"][:n] != 0) & np.isfinite(px) & np.isfinite(py) & np.isfinite(pz) & in_field(px, py)
        lm = np.nonzero((tracks["id"] != 0) & (tracks["hits"] >= p.min_hits) & in_field(tracks["x"], tracks["y"]))[0]
        recs = np.nonzero(usable)[0]
        ipx, ipy = np.rint(px[recs] * SCALE).astype(np.int64), np.rint(py[recs] * SCALE).astype(np.int64)
        imx, imy = np.rint(tracks["x"][lm] * SCALE).astype(np.int64), np.rint(tracks["y"][lm] * SCALE).astype(np.int64)
        same = np.ones((len(lm), len(recs)), dtype=bool)
        if p.class_aware:
            same = tracks["class_id"][lm][:, None] == np.asarray(dets)["class_id"][recs][None, :]
        for _ in range(p.iterations):
            qx, qy = move_numpy(corr, px[recs], py[recs])
            d2 = d2_numpy(qx[None, :], qy[None, :], pz[recs][None, :], tracks["x"][lm][:, None], tracks["y"][lm][:, None],
                          tracks["z"][lm][:, None])
            cand = (d2 <= gate2) & same                                        # a NaN d2 fails
            pk, pj = [], []
            if cand.any():
                bits = d2.view(np.uint32).astype(np.uint64) << np.uint64(32)
                by_rec = np.where(cand, bits | np.arange(len(lm), dtype=np.uint64)[:, None], NO_KEY)      # record j: least (d2, k)
                by_lm = np.where(cand, bits | recs.astype(np.uint64)[None, :], NO_KEY)                     # landmark k: least (d2, j)
                k_of = by_rec.argmin(axis=0)
                j_of = by_lm.argmin(axis=1)
                pj = np.nonzero((by_rec.min(axis=0) != NO_KEY) & (j_of[k_of] == np.arange(len(recs))))[0]
                pk = k_of[pj]
            n_pairs = len(pj)
            max_bits = int(d2[pk, pj].view(np.uint32).max()) if n_pairs else 0
            if n_pairs < p.min_pairs:
                status = POSE_TOO_FEW
                break
            sums = (n_pairs, ipx[pj].sum(), ipy[pj].sum(), imx[pk].sum(), imy[pk].sum(), (ipx[pj] * imx[pk] + ipy[pj] * imy[pk]).sum(),
                    (ipx[pj] * imy[pk] - ipy[pj] * imx[pk]).sum())
            corr, status = solve_numpy(*sums)
            updates += 1
        out["x"][:n], out["y"][:n] = move_numpy(corr, px, py)
        out["z"][:n] = pz
        result["pose"][0] = corrected_numpy(corr, prior)
    r, h = result[0], header[0]
    r["c"], r["s"], r["tx"], r["ty"] = corr
    h["n_records"], h["n_usable"], h["n_landmarks"], h["n_pairs"] = n, len(recs), len(lm), n_pairs
    h["iterations"], h["status"], h["max_d2_bits"] = updates, status, max_bits
    return {"header": header, "result": result, "cones": out}


class DevicePoseEstimator:
    """unina_pose_async (csrc/pose.hip): a memset and one launch per frame in front of DeviceTracker.update_from_buffer, which then
    takes the identity pose. The call itself is stateless; this class holds what it reads and writes between the frames: the device
    address of the tracker's slots, `result` (the corrected pose, which a chained call reads as its `prev`), `header` and `cones`
    (unused where the call is in place)."""

    def __init__(self, tracks, device: int = 0):
        """tracks: the device address (or a tensor) of UNINA_TRACK_MAX unina_track slots, e.g. DeviceTracker.buffers()[0]."""
        torch = _torch()
        self.L = load_library()
        self.device = device
        dev = f"cuda:{device}"
        self.tracks = tracks
        self.cones = torch.zeros(MAX_DETECTIONS * CONE3D_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.result = torch.zeros(POSE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.header = torch.zeros(POSE_HEADER_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.out = self.cones

    @classmethod
    def from_tracker(cls, tracker, device: int = 0):
        """Reads the table of a tracking.DeviceTracker (tracker.buffers(): the tracker must have been reset or updated once)."""
        return cls(tracker.buffers()[0], device)

    def estimate_async(self, d_dets, d_count, d_cones, params, chain=False, in_place=False, stream=None, prev=None, result=None):
        """Enqueues the memset and the launch; nothing is synchronised. d_dets / d_count / d_cones: device addresses (or tensors).
        chain: the last call's result is this call's `prev` and params.inc the odometry increment (d_result == d_prev); else
        params.inc is the prior pose itself. prev / result: other device buffers in place of the estimator's own. in_place: d_cones
        itself is rewritten. Returns the cones DeviceTracker.update_async takes."""
        p = as_params(params)
        self.out = d_cones if in_place else self.cones
        res = self.result if result is None else result
        d_prev = prev if prev is not None else (res if chain else None)
        _raise_on(self.L.unina_pose_async(_addr(d_dets), _addr(d_count), _addr(d_cones), _addr(self.tracks), _addr(d_prev), C.byref(p),
                                          _addr(self.out), _addr(res), self.header.data_ptr(), _stream_ptr(stream)), "unina_pose_async")
        return self.out

    def estimate_from_buffer(self, det_buf, cones, params, chain=False, in_place=False, stream=None):
        """The same behind Engine.infer_async's int32 buffer (word 0 = count, records from word 8) and a locator's output."""
        return self.estimate_async(*det_buffer_ptrs(det_buf), cones, params, chain, in_place, stream)

    def read(self, stream=None):
        """Synchronises `stream`; returns (header, result, cones): the POSE_HEADER_DTYPE and POSE_RESULT_DTYPE records and all
        MAX_DETECTIONS records the last call wrote."""
        u8 = _torch().uint8
        out = self.out if not isinstance(self.out, int) else None
        if out is None:
            raise ValueError("the last call wrote to a raw address: read that buffer yourself")
        return read_records(stream, (self.header, POSE_HEADER_DTYPE), (self.result, POSE_RESULT_DTYPE), (out.view(u8), CONE3D_DTYPE))


__all__ = ["pose_numpy", "compose_numpy", "move_numpy", "solve_numpy", "corrected_numpy", "make_params", "as_params", "check_params",
           "DevicePoseEstimator", "PoseParams", "POSE_RESULT_DTYPE", "POSE_HEADER_DTYPE", "POSE_OK", "POSE_TOO_FEW", "POSE_DEGENERATE",
           "TRACK_DTYPE", "TRACK_MAX", "CONE3D_DTYPE", "DET_DTYPE"]
