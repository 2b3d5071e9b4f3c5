"""Located cones tracked across frames (include/unina_mi355.h "tracking").

``update_numpy`` is the DEFINITION: fp32 throughout, one rounding per operation, in the order the header states, and the
association is the plain greedy loop over the sorted candidate pairs; csrc/track.hip (through ``DeviceTracker``) returns its
bytes. Cones are static landmarks: there is no motion model, the caller supplies the camera's pose in a fixed frame.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import (CONE3D_DTYPE, DET_DTYPE, MAX_DETECTIONS, TrackParams, _addr, _raise_on, _stream_ptr, _torch, clamp_count,
                     det_buffer_ptrs, load_library)

F = np.float32
TRACK_MAX = 1024                      # UNINA_TRACK_MAX
MAX_HITS = 1_000_000_000
INT_MAX = 2 ** 31 - 1
TRACK_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("confidence", "<f4"), ("id", "<i4"), ("class_id", "<i4"),
                        ("hits", "<i4"), ("missed", "<i4")])                                  # unina_track
TRACK_HEADER_DTYPE = np.dtype([(n, "<i4") for n in ("frame", "n_live", "n_confirmed", "next_id", "n_matched", "n_born", "n_died",
                                                    "n_dropped")])                            # unina_track_header
assert TRACK_DTYPE.itemsize == 32 and TRACK_HEADER_DTYPE.itemsize == 32
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def make_params(pose=None, gate=0.5, alpha=0.5, birth_confidence=0.0, class_aware=1, confirm_hits=3, max_missed=5) -> TrackParams:
    """pose: 12 values or a [3, 4] array, row-major [R|t], camera frame -> tracking frame; None is the identity. The floats are
    rounded to fp32 once, here."""
    flat = [float(v) for v in np.asarray(IDENTITY if pose is None else pose, dtype=np.float64).reshape(-1)]
    if len(flat) != 12:
        raise ValueError("a pose is 12 values: the rows of [R|t]")
    return TrackParams((C.c_float * 12)(*flat), gate, alpha, birth_confidence, int(class_aware), int(confirm_hits), int(max_missed))


def as_params(params) -> TrackParams:
    """A TrackParams, or a dict of make_params' arguments."""
    return params if isinstance(params, TrackParams) else make_params(**params)


def new_state() -> dict:
    """The table after unina_track_reset_async: no track, frame = 0, next_id = 1."""
    header = np.zeros(1, dtype=TRACK_HEADER_DTYPE)
    header["next_id"] = 1
    return {"header": header, "tracks": np.zeros(TRACK_MAX, dtype=TRACK_DTYPE)}


def point_numpy(pose, x, y, z):
    """csrc/track_math.h track_point: fp32 scalars or arrays -> (px, py, pz); pose: 12 np.float32."""
    return (((pose[0] * x + pose[1] * y) + pose[2] * z) + pose[3], ((pose[4] * x + pose[5] * y) + pose[6] * z) + pose[7],
            ((pose[8] * x + pose[9] * y) + pose[10] * z) + pose[11])


def d2_numpy(px, py, pz, tx, ty, tz):
    """track_d2: the squared distance, rounded operation by operation."""
    dx, dy, dz = px - tx, py - ty, pz - tz
    return (dx * dx + dy * dy) + dz * dz


def step_numpy(t, alpha, p):
    """track_step: one coordinate of a matched slot."""
    return t + alpha * (p - t)


def update_numpy(state: dict, dets, count: int, cones, params):
    """One update. state: new_state() or an earlier result (left unchanged); dets: DET_DTYPE records; count: as the device word
    (clamped to 0..MAX_DETECTIONS, and to the arrays' lengths); cones: CONE3D_DTYPE records, index-aligned with dets. Returns
    (state, assign): the new table and MAX_DETECTIONS int32 ids."""
    p = as_params(params)
    pose = [F(v) for v in p.pose]
    alpha, birth = F(p.alpha), F(p.birth_confidence)
    if not (p.gate > 0 and np.isfinite(F(p.gate) * F(p.gate))):
        raise ValueError("gate and gate * gate must be finite and positive")
    hdr, tr = state["header"].copy(), state["tracks"].copy()
    assign = np.zeros(MAX_DETECTIONS, dtype=np.int32)
    n = clamp_count(count, dets, cones)
    dets, cones = np.asarray(dets)[:n], np.asarray(cones)[:n]
    with np.errstate(all="ignore"):
        x, y, z = cones["x"], cones["y"], cones["z"]
        px, py, pz = point_numpy(pose, x, y, z)
        usable = (cones["valid"] != 0) & np.isfinite(px) & np.isfinite(py) & np.isfinite(pz)
        live, recs = np.nonzero(tr["id"] != 0)[0], np.nonzero(usable)[0]
        # every candidate pair, then the greedy loop in ascending (d2 bits, slot, record)
        d2 = d2_numpy(px[recs][None, :], py[recs][None, :], pz[recs][None, :], tr["x"][live][:, None], tr["y"][live][:, None],
                      tr["z"][live][:, None])
        cand = d2 <= F(p.gate) * F(p.gate)                                   # a NaN d2 fails
        if p.class_aware:
            cand &= tr["class_id"][live][:, None] == dets["class_id"][recs][None, :]
        si, ji = np.nonzero(cand)
        order = np.lexsort((recs[ji], live[si], d2[si, ji].view(np.uint32)))
        slot_of, rec_of = {}, {}                                             # record -> slot, slot -> record
        most = min(len(live), len(recs))
        for s, j in zip(live[si][order].tolist(), recs[ji][order].tolist()):
            if s not in rec_of and j not in slot_of:
                rec_of[s], slot_of[j] = j, s
                if len(rec_of) == most:
                    break
        n_died = 0
        for s in live.tolist():
            t = tr[s]
            if s in rec_of:
                j = rec_of[s]
                t["x"], t["y"], t["z"] = step_numpy(t["x"], alpha, px[j]), step_numpy(t["y"], alpha, py[j]), step_numpy(t["z"], alpha, pz[j])
                t["confidence"], t["class_id"] = dets["confidence"][j], dets["class_id"][j]
                t["hits"], t["missed"] = min(int(t["hits"]) + 1, MAX_HITS), 0
                assign[j] = t["id"]
            else:
                t["missed"] = min(int(t["missed"]) + 1, INT_MAX)
                if t["missed"] > p.max_missed:
                    tr[s] = np.zeros((), dtype=TRACK_DTYPE)
                    n_died += 1
        free = iter(np.nonzero(tr["id"] == 0)[0].tolist())
        next_id, n_born, n_dropped = int(hdr["next_id"][0]), 0, 0
        for j in recs.tolist():
            if j in slot_of or not dets["confidence"][j] >= birth:            # a NaN confidence fails
                continue
            s = next(free, None) if next_id < INT_MAX else None
            if s is None:
                n_dropped += 1
                continue
            tr[s] = (px[j], py[j], pz[j], dets["confidence"][j], next_id, dets["class_id"][j], 1, 0)
            assign[j] = next_id
            next_id += 1
            n_born += 1
    h = hdr[0]
    h["frame"] = (int(h["frame"]) + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31            # wraps like the device's unsigned add
    alive = tr["id"] != 0
    h["n_live"], h["n_confirmed"] = int(alive.sum()), int((alive & (tr["hits"] >= p.confirm_hits)).sum())
    h["next_id"], h["n_matched"], h["n_born"], h["n_died"], h["n_dropped"] = next_id, len(rec_of), n_born, n_died, n_dropped
    return {"header": hdr, "tracks": tr}, assign


class DeviceTracker:
    """unina_track_* (csrc/track.hip): the table of tracks on the device and one launch per frame behind unina_locate_async.
    Holds the MAX_DETECTIONS int32 `assign` tensor the updates write; localize.DeviceLocator's counterpart."""

    def __init__(self, device: int = 0):
        torch = _torch()
        self.L = load_library()
        self.h = C.c_void_p()
        _raise_on(self.L.unina_track_create(device, C.byref(self.h)), "unina_track_create")
        self.assign = torch.zeros(MAX_DETECTIONS, dtype=torch.int32, device=f"cuda:{device}")

    def close(self):
        if self.h:
            self.L.unina_track_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def reset(self, stream=None):
        _raise_on(self.L.unina_track_reset_async(self.h, _stream_ptr(stream)), "unina_track_reset_async")

    def update_async(self, d_dets, d_count, d_cones, params, stream=None, assign=None):
        """Enqueues the launch; nothing is synchronised. d_dets / d_count / d_cones: device addresses (or tensors) of the
        records, the count and the unina_cone3d points. assign: an int32 tensor of MAX_DETECTIONS words (or a device address)
        in place of the tracker's own, or False for none. Returns the assign tensor."""
        p = as_params(params)
        out = self.assign if assign is None else assign
        _raise_on(self.L.unina_track_update_async(self.h, _addr(d_dets), _addr(d_count), _addr(d_cones), C.byref(p),
                                                  None if out is False else _addr(out), _stream_ptr(stream)), "unina_track_update_async")
        return out

    def update_from_buffer(self, det_buf, locator_out, params, stream=None, assign=None):
        """The same behind Engine.infer_async's int32 buffer (word 0 = count, records from word 8) and DeviceLocator's output."""
        return self.update_async(*det_buffer_ptrs(det_buf), locator_out, params, stream, assign)

    def buffers(self):
        """(device address of the slots, device address of the header) for a consumer that stays on the GPU."""
        tracks, header = C.c_void_p(), C.c_void_p()
        _raise_on(self.L.unina_track_buffers(self.h, C.byref(tracks), C.byref(header)), "unina_track_buffers")
        return tracks.value, header.value

    def read(self, stream=None):
        """Synchronises `stream`; returns (header, tracks): one TRACK_HEADER_DTYPE record and all TRACK_MAX TRACK_DTYPE slots."""
        header, tracks = np.zeros(1, dtype=TRACK_HEADER_DTYPE), np.zeros(TRACK_MAX, dtype=TRACK_DTYPE)
        _raise_on(self.L.unina_track_read(self.h, header.ctypes.data, tracks.ctypes.data, TRACK_MAX, _stream_ptr(stream)),
                  "unina_track_read")
        return header, tracks


__all__ = ["update_numpy", "point_numpy", "d2_numpy", "step_numpy", "new_state", "make_params", "as_params", "DeviceTracker", "TRACK_DTYPE", "TRACK_HEADER_DTYPE", "TRACK_MAX",
           "CONE3D_DTYPE", "DET_DTYPE"]
