"""LiDAR cone candidates fused with camera records: one record list in the camera frame and a link per record, behind the
clusterer and a locator and in front of ONE tracker (include/unina_mi355.h "fusion of LiDAR cone candidates with camera records").

``fuse_numpy`` is the DEFINITION: fp32 scalars and arrays throughout, one rounding per operation in the order the header states,
and the association is the plain greedy loop over the sorted candidate pairs; csrc/fuse.hip (through ``DeviceFuser``) returns its
bytes. It is also the twin of csrc/fuse_math.h, which tests/fuse_math_host.cpp runs on the host.
Class from pixels for the LiDAR-only records is the stage behind this one (colour.py).
NOT covered: time alignment of sweep and frame, motion de-skew, a globally optimal (Hungarian) assignment, raising the confidence
of a matched record, lens distortion (the image is rectified).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import (CONE3D_DTYPE, DET_DTYPE, FUSE_BOTH, FUSE_CAMERA, FUSE_HEADER_DTYPE, FUSE_LIDAR, FUSE_LINK_DTYPE, MAX_DETECTIONS, FuseParams,
                     _addr, _raise_on, _stream_ptr, _torch, clamp_count, det_buffer_ptrs, load_library, read_records)
from .localize import as_extrinsic, as_pinhole

F = np.float32


def make_fuse_params(level_to_cam, cam, sx=1.0, sy=1.0, lift=0.15, min_depth=0.3, max_depth=40.0, grow=1.0, pad=4.0, range_abs=0.5,
                     range_rel=0.1) -> FuseParams:
    """unina_fuse_params. level_to_cam: 12 values or a [3, 4] array, row-major [R|t], level frame -> camera optical frame
    (level_to_camera gives it); cam: (fx, fy, cx, cy) or a Pinhole; sx, sy: record -> image pixels. The floats are rounded to fp32
    once, here."""
    return FuseParams((C.c_float * 12)(*as_extrinsic(level_to_cam).tolist()), as_pinhole(cam), float(sx), float(sy), float(lift),
                      float(min_depth), float(max_depth), float(grow), float(pad), float(range_abs), float(range_rel))


def as_fuse_params(params) -> FuseParams:
    """A FuseParams, or a dict of make_fuse_params' arguments."""
    return params if isinstance(params, FuseParams) else make_fuse_params(**params)


def check_params(p: FuseParams) -> None:
    """The refusals of unina_fuse_async that concern the parameters."""
    m, cam = [F(v) for v in p.level_to_cam], (p.cam.fx, p.cam.fy, p.cam.cx, p.cam.cy)
    ok = all(np.isfinite(v) for v in m) and all(np.isfinite(v) for v in cam) and p.cam.fx != 0 and p.cam.fy != 0
    ok = ok and all(np.isfinite(v) and v > 0 for v in (p.sx, p.sy, p.min_depth)) and np.isfinite(p.lift)
    ok = ok and np.isfinite(p.max_depth) and p.max_depth >= p.min_depth
    ok = ok and all(np.isfinite(v) and v >= 0 for v in (p.grow, p.pad, p.range_abs, p.range_rel))
    if not ok:
        raise ValueError("fuse parameters outside what unina_fuse_async accepts")


def level_to_camera(lidar_to_level, lidar_to_cam) -> np.ndarray:
    """The two extrinsics a node has -- LiDAR frame -> level frame (the ground filter's and the clusterer's) and LiDAR frame ->
    camera optical frame (the LiDAR locator's), each 12 values or [3, 4], rigid -> level frame -> camera optical frame as 12
    np.float32: the rigid inverse of the first and the product with the second in float64, rounded to fp32 once."""
    a = np.asarray(lidar_to_level, dtype=np.float64).reshape(3, 4)
    b = np.asarray(lidar_to_cam, dtype=np.float64).reshape(3, 4)
    r = b[:, :3] @ a[:, :3].T                                  # R_cam * R_level^T
    t = b[:, 3] - r @ a[:, 3]
    return np.concatenate([r, t[:, None]], axis=1).reshape(-1).astype(np.float32)


def point_numpy(p: FuseParams, x, y, z, valid):
    """csrc/fuse_math.h fuse_point for fp32 arrays: (xc, yc, zc, u, v, usable, projected); u = v = 0 where not projected. The
    caller holds np.errstate."""
    m = [F(v) for v in p.level_to_cam]
    zl = z + F(p.lift)
    xc = ((m[0] * x + m[1] * y) + m[2] * zl) + m[3]
    yc = ((m[4] * x + m[5] * y) + m[6] * zl) + m[7]
    zc = ((m[8] * x + m[9] * y) + m[10] * zl) + m[11]
    usable = (np.asarray(valid) != 0) & np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc)
    projected = usable & (zc >= F(p.min_depth)) & (zc <= F(p.max_depth))
    u = np.where(projected, (F(p.cam.fx) * xc) / zc + F(p.cam.cx), F(0))
    v = np.where(projected, (F(p.cam.fy) * yc) / zc + F(p.cam.cy), F(0))
    return xc, yc, zc, u.astype(np.float32), v.astype(np.float32), usable, projected


def box_numpy(p: FuseParams, x1, y1, x2, y2):
    """csrc/fuse_math.h fuse_box for fp32 arrays: (uc, vc, hw, hh, boxed); the floats are 0 where not boxed."""
    sx, sy = F(p.sx), F(p.sy)
    X1, X2, Y1, Y2 = x1 * sx, x2 * sx, y1 * sy, y2 * sy
    boxed = np.isfinite(X1) & np.isfinite(X2) & np.isfinite(Y1) & np.isfinite(Y2) & (X2 >= X1) & (Y2 >= Y1)
    uc, vc = F(0.5) * (X1 + X2), F(0.5) * (Y1 + Y2)
    hg = F(0.5) * F(p.grow)
    hw, hh = hg * (X2 - X1) + F(p.pad), hg * (Y2 - Y1) + F(p.pad)
    zero = F(0)
    return (np.where(boxed, uc, zero).astype(np.float32), np.where(boxed, vc, zero).astype(np.float32),
            np.where(boxed, hw, zero).astype(np.float32), np.where(boxed, hh, zero).astype(np.float32), boxed)


def candidate_numpy(p: FuseParams, u, v, zc, uc, vc, hw, hh, has_depth, cz):
    """csrc/fuse_math.h fuse_candidate for fp32 arrays that broadcast: (candidate, d2). A NaN fails every comparison."""
    du, dv = u - uc, v - vc
    d2 = du * du + dv * dv
    cand = (np.abs(du) <= hw) & (np.abs(dv) <= hh)
    depth = np.abs(zc - cz) <= F(p.range_abs) + F(p.range_rel) * zc
    return cand & (~np.asarray(has_depth, dtype=bool) | depth), d2


def fuse_numpy(dets, count: int, cones, ldets, lcount: int, lcones, params) -> dict:
    """dets / count / cones: the camera branch (DET_DTYPE and CONE3D_DTYPE records, the count as the device word); ldets / lcount /
    lcones: the clusterer's. Returns header (one FUSE_HEADER_DTYPE record), dets, cones, links (MAX_DETECTIONS records each, zero
    behind the count), count (int32 [1]) and lidar_slot (MAX_DETECTIONS int32)."""
    p = as_fuse_params(params)
    check_params(p)
    nc, nl = clamp_count(count, dets, cones), clamp_count(lcount, ldets, lcones)
    dets, cones, ldets, lcones = np.asarray(dets)[:nc], np.asarray(cones)[:nc], np.asarray(ldets)[:nl], np.asarray(lcones)[:nl]
    out_dets, out_cones = np.zeros(MAX_DETECTIONS, dtype=DET_DTYPE), np.zeros(MAX_DETECTIONS, dtype=CONE3D_DTYPE)
    links, lidar_slot = np.zeros(MAX_DETECTIONS, dtype=FUSE_LINK_DTYPE), np.full(MAX_DETECTIONS, -1, dtype=np.int32)
    with np.errstate(all="ignore"):
        xc, yc, zc, u, v, usable, projected = point_numpy(p, lcones["x"], lcones["y"], lcones["z"], lcones["valid"])
        uc, vc, hw, hh, boxed = box_numpy(p, dets["x1"], dets["y1"], dets["x2"], dets["y2"])
        ci, lj = np.nonzero(boxed)[0], np.nonzero(projected)[0]
        # every candidate pair, then the greedy loop in ascending (d2 bits, i, j)
        cand, d2 = candidate_numpy(p, u[lj][None, :], v[lj][None, :], zc[lj][None, :], uc[ci][:, None], vc[ci][:, None], hw[ci][:, None],
                                   hh[ci][:, None], (cones["valid"][ci] != 0)[:, None], cones["z"][ci][:, None])
        a, b = np.nonzero(cand)
        pair_d2 = np.ascontiguousarray(d2[a, b], dtype=np.float32)
        order = np.lexsort((lj[b], ci[a], pair_d2.view(np.uint32)))
        lidar_of, camera_of = {}, {}                                        # camera record -> (cone, d2), cone -> camera record
        most = min(len(ci), len(lj))
        for i, j, d in zip(ci[a][order].tolist(), lj[b][order].tolist(), pair_d2[order]):
            if i not in lidar_of and j not in camera_of:
                lidar_of[i], camera_of[j] = (j, d), i
                if len(lidar_of) == most:
                    break
        out_dets[:nc], out_cones[:nc] = dets, cones
        links["camera"][:nc], links["lidar"][:nc], links["kind"][:nc] = np.arange(nc), -1, FUSE_CAMERA
        for i, (j, d) in lidar_of.items():
            out_cones[i] = (xc[j], yc[j], zc[j], u[j], v[j], lcones["n_valid"][j], lcones["n_samples"][j], 1)
            links[i] = (i, j, d, FUSE_BOTH)
            lidar_slot[j] = i
        only = [j for j in np.nonzero(usable)[0].tolist() if j not in camera_of]
        out_words, lwords = out_dets.view(np.uint32).reshape(-1, 8), np.ascontiguousarray(ldets).view(np.uint32).reshape(-1, 8)
        n_written = nc
        for j in only[:MAX_DETECTIONS - nc]:
            s = n_written
            bx, by = (u[j] / F(p.sx), v[j] / F(p.sy)) if projected[j] else (F(0), F(0))
            out_dets[s] = (bx, by, bx, by, 0, 0, 1, 0)
            out_words[s, 4:6] = lwords[j, 4:6]                             # confidence and class_id, bit for bit
            out_cones[s] = (xc[j], yc[j], zc[j], u[j], v[j], lcones["n_valid"][j], lcones["n_samples"][j], 1)
            links[s] = (-1, j, 0, FUSE_LIDAR)
            lidar_slot[j] = s
            n_written += 1
    header = np.zeros(1, dtype=FUSE_HEADER_DTYPE)
    header[0] = (nc, nl, int(projected.sum()), len(lidar_of), nc - len(lidar_of), len(only), n_written, len(only) - (n_written - nc))
    return {"header": header, "dets": out_dets, "cones": out_cones, "links": links, "count": np.array([n_written], dtype=np.int32),
            "lidar_slot": lidar_slot}


class DeviceFuser:
    """unina_fuse_async (csrc/fuse.hip): one launch per frame behind DeviceClusterer.cluster_async and a locator, in front of
    DeviceTracker.update_from_buffer. The call itself is stateless; this class holds the buffers it writes: `det_buf`
    (Engine.infer_async's layout: word 0 = count, records from word 8), `cones`, `links`, `lidar_slot` and `header`."""

    def __init__(self, device: int = 0):
        torch = _torch()
        self.L = load_library()
        self.device = device
        dev = f"cuda:{device}"
        self.det_buf = torch.zeros(8 + 8 * MAX_DETECTIONS, dtype=torch.int32, device=dev)
        self.count, self.dets = self.det_buf[:1], self.det_buf[8:]
        self.cones = torch.zeros(MAX_DETECTIONS * CONE3D_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.links = torch.zeros(MAX_DETECTIONS * FUSE_LINK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.lidar_slot = torch.zeros(MAX_DETECTIONS, dtype=torch.int32, device=dev)
        self.header = torch.zeros(FUSE_HEADER_DTYPE.itemsize, dtype=torch.uint8, device=dev)

    def fuse_async(self, d_dets, d_count, d_cones, d_ldets, d_lcount, d_lcones, params, stream=None, lidar_slot=None):
        """Enqueues the launch; nothing is synchronised. The six inputs are device addresses (or tensors): the camera branch's
        records, count and cones, then the clusterer's. lidar_slot: an int32 tensor of MAX_DETECTIONS words (or a device address)
        in place of the fuser's own, or False for none. Returns (det_buf, cones): tracker.update_from_buffer(det_buf, cones, ...)
        goes behind it on the same stream."""
        p = as_fuse_params(params)
        slot = self.lidar_slot if lidar_slot is None else lidar_slot
        _raise_on(self.L.unina_fuse_async(_addr(d_dets), _addr(d_count), _addr(d_cones), _addr(d_ldets), _addr(d_lcount), _addr(d_lcones),
                                          C.byref(p), self.dets.data_ptr(), self.count.data_ptr(), self.cones.data_ptr(),
                                          self.links.data_ptr(), None if slot is False else _addr(slot), self.header.data_ptr(),
                                          _stream_ptr(stream)), "unina_fuse_async")
        return self.det_buf, self.cones

    def fuse_from_buffers(self, det_buf, cones, ldet_buf, lcones, params, stream=None, lidar_slot=None):
        """The same behind Engine.infer_async's int32 buffer plus a locator's output, and DeviceClusterer.cluster_async's pair."""
        return self.fuse_async(*det_buffer_ptrs(det_buf), cones, *det_buffer_ptrs(ldet_buf), lcones, params, stream, lidar_slot)

    def read(self, stream=None):
        """Synchronises `stream`; returns (header, dets, cones, count, links, lidar_slot): the FUSE_HEADER_DTYPE record, all
        MAX_DETECTIONS records of the three arrays (zero behind the count), the count word and the MAX_DETECTIONS slot words."""
        u8 = _torch().uint8
        return read_records(stream, (self.header, FUSE_HEADER_DTYPE), (self.dets.view(u8), DET_DTYPE), (self.cones, CONE3D_DTYPE),
                            (self.count.view(u8), np.int32), (self.links, FUSE_LINK_DTYPE), (self.lidar_slot.view(u8), np.int32))


__all__ = ["fuse_numpy", "point_numpy", "box_numpy", "candidate_numpy", "level_to_camera", "make_fuse_params", "as_fuse_params", "check_params",
           "DeviceFuser", "FuseParams", "FUSE_LINK_DTYPE", "FUSE_HEADER_DTYPE", "FUSE_BOTH", "FUSE_CAMERA", "FUSE_LIDAR"]
