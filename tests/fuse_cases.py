"""Inputs shared by tests/test_fuse_cpu.py and tests/test_gpu_fuse.py: the named pairs of record lists of unina_fuse_async
(include/unina_mi355.h "fusion of LiDAR cone candidates with camera records") and a seeded scene with known truth. A case is the
camera branch's records, cones and count word, the clusterer's, and the parameters of one call. Pure numpy; nothing here touches
the device.

A PLACED case sees the level frame through the identity with lift = 0 and a pinhole of fx = fy = 256, cx = 256, cy = 192: the LiDAR
cone ((u - 256) * z / 256, (v - 192) * z / 256, z) has zc = z and, for z = 4 and u, v on a fine binary grid, the pixel (u, v)
exactly; at_pixel asserts it. tests/test_fuse_cpu.py asserts on the twin what each case contains."""
import numpy as np

from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DET_DTYPE

MAXD = 1024
F = np.float32
NAN, INF = float("nan"), float("inf")
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
CAM = (256.0, 256.0, 256.0, 192.0)
UNKNOWN = 9                       # the class_id the LiDAR records carry


def params(**kw):
    p = dict(level_to_cam=IDENTITY, cam=CAM, sx=1.0, sy=1.0, lift=0.0, min_depth=0.5, max_depth=50.0, grow=1.0, pad=0.0, range_abs=0.5,
             range_rel=0.0)
    p.update(kw)
    return p


def project(point, cam=CAM):
    """The pixel of a placed point, in fp32 as the definition rounds it."""
    x, y, z = (F(v) for v in point)
    with np.errstate(all="ignore"):
        return (F(cam[0]) * x) / z + F(cam[2]), (F(cam[1]) * y) / z + F(cam[3])


def at_pixel(u, v, z=4.0):
    """The placed point whose pixel is (u, v) exactly."""
    p = np.array([(np.float64(u) - CAM[2]) * z / CAM[0], (np.float64(v) - CAM[3]) * z / CAM[1], z]).astype(np.float32)
    got = project(p)
    assert got[0] == F(u) and got[1] == F(v), (u, v, got)
    return p


def camera(boxes, depth=None, cls=1, conf=0.9):
    """boxes: [m, 4] x1, y1, x2, y2 in record coordinates; depth: None (no cone has a depth) or m values, NaN-free entries give
    valid = 1 cones with that z. cls / conf broadcast."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    m = len(b)
    dets, cones = np.zeros(m, dtype=DET_DTYPE), np.zeros(m, dtype=CONE3D_DTYPE)
    dets["x1"], dets["y1"], dets["x2"], dets["y2"] = b.T
    dets["confidence"], dets["class_id"], dets["valid"] = conf, cls, 1
    if depth is not None:
        cones["z"], cones["valid"] = depth, 1
        cones["u"], cones["v"], cones["n_valid"], cones["n_samples"] = 0.5 * (b[:, 0] + b[:, 2]), 0.5 * (b[:, 1] + b[:, 3]), 5, 9
    return dets, cones


def lidar(points, cls=UNKNOWN, conf=0.5, valid=1, n_points=12):
    """points: [m, 3] positions in the level frame -> the clusterer's records."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    m = len(p)
    dets, cones = np.zeros(m, dtype=DET_DTYPE), np.zeros(m, dtype=CONE3D_DTYPE)
    dets["x1"], dets["y1"], dets["x2"], dets["y2"] = p[:, 0] - F(0.1), p[:, 1] - F(0.1), p[:, 0] + F(0.1), p[:, 1] + F(0.1)
    dets["confidence"], dets["class_id"], dets["valid"] = conf, cls, 1
    cones["x"], cones["y"], cones["z"] = p.T
    cones["n_valid"], cones["n_samples"], cones["valid"] = n_points, n_points, valid
    return dets, cones


def case(name, cam_side, lidar_side, count=None, lcount=None, **par):
    (dets, cones), (ldets, lcones) = cam_side, lidar_side
    return {"name": name, "dets": dets, "cones": cones, "count": len(dets) if count is None else count, "ldets": ldets, "lcones": lcones,
            "lcount": len(ldets) if lcount is None else lcount, "params": params(**par)}


def square(u, v, half=6.0):
    """Boxes of side 2 * half around the pixels (u, v)."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return np.stack([u - half, v - half, u + half, v + half], axis=-1)


def grid_pixels(n, step=16.0, cols=32):
    i = np.arange(n)
    return (i % cols) * step + 8.0, (i // cols) * step + 8.0


def pixels_to_points(u, v, z=4.0):
    return np.stack([at_pixel(a, b, z) for a, b in zip(np.atleast_1d(u), np.atleast_1d(v))])


def chain(n=64):
    """Camera boxes and LiDAR pixels alternating on the row v = 192, every gap 1/32 pixel shorter than the one before, from 8
    pixels; a box reaches 8.5 pixels to either side, so each record's nearest cone and each cone's nearest record is its RIGHT
    neighbour, only the last pair is mutual and the matching takes n rounds. Returns (boxes, LiDAR points)."""
    gaps = 8.0 - 0.03125 * np.arange(2 * n - 1)
    pos = 100.0 + np.concatenate([[0.0], np.cumsum(gaps)])
    return square(pos[0::2], np.full(n, 192.0), 8.5), pixels_to_points(pos[1::2], np.full(n, 192.0))


def edge_cases():
    out = []
    gu, gv = grid_pixels(MAXD)
    boxes, pts = square(gu, gv), pixels_to_points(gu + 2.0, gv + 1.0)
    # counts on each side: the first `count` of 1024 records against 100, boxes on a 16-pixel grid and a cone 2 pixels off each centre
    for c in (0, 1, 63, 64, 65, 1024, 5000, -7):
        out.append(case(f"camera{c}", camera(boxes), lidar(pts[:100]), count=c))
        out.append(case(f"lidar{c}", camera(boxes[:100]), lidar(pts), lcount=c))
    out.append(case("both_empty", camera(boxes[:0]), lidar(pts[:0])))
    away = pixels_to_points(*[a[:100] for a in grid_pixels(MAXD)], z=4.0) + np.array([0, 40.0, 0], dtype=np.float32)   # pixels far below every box
    out.append(case("room_for_24", camera(boxes[:1000]), lidar(away)))
    out.append(case("no_room", camera(boxes), lidar(away[:10])))
    out.append(case("all_lidar_invalid", camera(boxes[:10]), lidar(pts[:10], valid=0)))
    bad = pts[:8].copy()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0] = NAN, INF, -INF, -INF
    out.append(case("non_finite_points", camera(boxes[:8]), lidar(bad)))
    over = pts[:8].copy()
    over[:4, 0] = 3e38
    out.append(case("transform_overflows", camera(boxes[:8]), lidar(over), level_to_cam=[1, 0, 0, 3e38, 0, 1, 0, 0, 0, 0, 1, 0]))
    behind = pts[:4].copy()
    behind[:2, 2] = -4.0
    out.append(case("behind_the_camera", camera(boxes[:4]), lidar(behind)))
    lo, hi = F(0.5), F(50.0)
    zs = [lo, np.nextafter(lo, F(0)), hi, np.nextafter(hi, F(INF))]
    out.append(case("depth_range_bounds", camera(square([256.0] * 4, [192.0] * 4)[:0]), lidar([[0, 0, z] for z in zs])))
    # the pixel 300 is the right (lower) border of a box 280..300; one ulp further it is outside
    up = np.nextafter(F(300.0), F(INF))
    out.append(case("border_u_on", camera([[280, 100, 300, 140]]), lidar([at_pixel(300.0, 120.0)])))
    out.append(case("border_u_outside", camera([[280, 100, 300, 140]]), lidar([at_pixel(up, 120.0)])))
    out.append(case("border_v_on", camera([[100, 280, 140, 300]]), lidar([at_pixel(120.0, 300.0)])))
    out.append(case("border_v_outside", camera([[100, 280, 140, 300]]), lidar([at_pixel(120.0, up)])))
    centre = square([256.0], [192.0], 10.0)
    out.append(case("depth_gate_equal", camera(centre, depth=[4.0]), lidar([[0, 0, 4.5]])))
    out.append(case("depth_gate_one_ulp_over", camera(centre, depth=[4.0]), lidar([[0, 0, np.nextafter(F(4.5), F(INF))]])))
    d, c = camera(centre, depth=[40.0])
    c["valid"] = 0
    out.append(case("no_depth_no_gate", (d, c), lidar([[0, 0, 4.5]])))
    out.append(case("nan_depth_fails_the_gate", camera(centre, depth=[NAN]), lidar([[0, 0, 4.5]])))
    out.append(case("inverted_and_nan_boxes", camera([[140, 100, 100, 140], [100, 140, 140, 100], [NAN, 100, 140, 140], [100, 100, INF, 140],
                                                      [100, 100, 140, 140]]),
                    lidar([at_pixel(120.0, 120.0), at_pixel(121.0, 120.0)])))
    out.append(case("centre_hit_only", camera([[100, 100, 140, 140], [200, 100, 240, 140]]),
                    lidar([at_pixel(120.0, 120.0), at_pixel(220.0, 120.0078125)]), grow=0.0, pad=0.0))
    # 8 x 8 boxes of 16 pixels on a 16-pixel grid and a cone on every corner shared by four of them: every d2 is 128
    q = np.arange(64)
    qu, qv = (q % 8) * 16.0 + 108.0, (q // 8) * 16.0 + 108.0
    out.append(case("grid_ties", camera(square(qu, qv, 8.0)), lidar(pixels_to_points(qu + 8.0, qv + 8.0))))
    two = [[100, 100, 140, 140], [110, 100, 150, 140]]
    out.append(case("one_cone_two_boxes", camera(two), lidar([at_pixel(124.0, 120.0)])))
    out.append(case("one_cone_two_boxes_depth", camera(two, depth=[4.0, 8.0]), lidar([at_pixel(124.0, 120.0, z=8.0)])))
    out.append(case("two_cones_one_box", camera([[100, 100, 140, 140]]), lidar([at_pixel(126.0, 120.0), at_pixel(117.0, 120.0)])))
    cb, cp = chain(64)
    out.append(case("chain64", camera(cb), lidar(cp)))
    fu, fv = grid_pixels(32, step=20.0)
    out.append(case("chain64_across_waves", camera(np.concatenate([square(fu, fv + 400.0), cb])),
                    lidar(np.concatenate([pixels_to_points(fu + 1.0, fv + 400.0), cp]))))
    out.append(case("nan_confidence", camera(boxes[:4], conf=[NAN, 0.9, NAN, 0.9]),
                    lidar(np.concatenate([pts[:2], away[:2]]), conf=[NAN, 0.5, NAN, 0.5])))
    out.append(case("scaled_records", camera(square(gu[:50], gv[:50]) / np.array([2.0, 1.5, 2.0, 1.5])), lidar(pts[:60]), sx=2.0, sy=1.5, pad=1.0,
                    grow=0.5))
    return out


# ---------------------------------------------------------------- the scene
LEVEL_TO_CAM = (0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 1.0, 1.0, 0.0, 0.0, 0.0)     # x forward, y left, z up -> optical; the camera 1 m above the ground
SCENE_CAM = (600.0, 600.0, 640.0, 360.0)
SCENE_SIZE = (1280, 720)


def scene(noise=True, pad=0.0, seed=7):
    """About 150 cones on the two borders of a closed track in the level frame, the car on its centre line at the origin. The
    camera sees those inside its 1280 x 720 image up to 40 m, drops 15 %, adds 10 false boxes and (noise) 2 pixels of projection
    noise; half of its cones carry a depth, (noise) with 3 % range error. The clusterer sees those within 25 m, drops 10 % and adds
    5 false candidates, (noise) with 1 cm of position noise. Both lists are shuffled; case["truth"] / case["ltruth"] name the
    cone of every record, -1 for a false one."""
    rng = np.random.RandomState(seed)
    t = np.linspace(0.0, 2 * np.pi, 75, endpoint=False) + 0.02
    centre = np.stack([30.0 * np.sin(t), 12.0 * (1.0 - np.cos(t))], axis=1)
    tangent = np.stack([30.0 * np.cos(t), 12.0 * np.sin(t)], axis=1)
    normal = np.stack([-tangent[:, 1], tangent[:, 0]], axis=1) / np.linalg.norm(tangent, axis=1, keepdims=True)
    cones = np.concatenate([centre + 1.5 * normal, centre - 1.5 * normal])             # [150, 2], level frame, on the ground
    colour = np.concatenate([np.zeros(75, dtype=int), np.ones(75, dtype=int)])
    fx, fy, cx, cy = SCENE_CAM
    # camera: the cone's mid-height point through the pinhole; a box of 0.23 m x 0.3 m at its depth
    zc, xc, yc = cones[:, 0], -cones[:, 1], np.full(150, 1.0 - 0.15)
    with np.errstate(all="ignore"):
        u, v = fx * xc / zc + cx, fy * yc / zc + cy
        w, h = fx * 0.23 / zc, fy * 0.3 / zc
    seen = np.nonzero((zc > 1.0) & (zc < 40.0) & (u > 0) & (u < SCENE_SIZE[0]) & (v > 0) & (v < SCENE_SIZE[1]) & (rng.rand(150) > 0.15))[0]
    jitter = rng.normal(0.0, 2.0, (len(seen), 2)) * (1.0 if noise else 0.0)
    range_err = 1.0 + rng.normal(0.0, 0.03, len(seen)) * (1.0 if noise else 0.0)
    has_depth = rng.rand(len(seen)) < 0.5
    bu, bv = u[seen] + jitter[:, 0], v[seen] + jitter[:, 1]
    boxes = np.stack([bu - w[seen] / 2, bv - h[seen] / 2, bu + w[seen] / 2, bv + h[seen] / 2], axis=1)
    fu, fv, fs = rng.uniform(50, 1230, 10), rng.uniform(200, 700, 10), rng.uniform(5, 30, 10)
    boxes = np.concatenate([boxes, np.stack([fu - fs / 2, fv - fs / 2, fu + fs / 2, fv + fs / 2], axis=1)])
    truth = np.concatenate([seen, np.full(10, -1)])
    depth = np.concatenate([np.where(has_depth, zc[seen] * range_err, NAN), np.where(rng.rand(10) < 0.5, rng.uniform(3, 30, 10), NAN)])
    cls = np.concatenate([colour[seen], rng.randint(0, 2, 10)])
    conf = np.concatenate([rng.uniform(0.5, 0.95, len(seen)), rng.uniform(0.3, 0.6, 10)])
    order = rng.permutation(len(boxes))
    dets, ccones = camera(boxes[order], depth=depth[order], cls=cls[order], conf=conf[order])
    ccones["valid"] = ~np.isnan(depth[order])
    ccones["z"] = np.where(ccones["valid"] != 0, ccones["z"], 0)
    ccones["x"] = (ccones["u"] - F(cx)) * ccones["z"] / F(fx)
    ccones["y"] = (ccones["v"] - F(cy)) * ccones["z"] / F(fy)
    # clusterer: every cone within 25 m, the car's sides and back included
    near = np.nonzero((np.linalg.norm(cones, axis=1) < 25.0) & (rng.rand(150) > 0.10))[0]
    lp = np.concatenate([cones[near] + rng.normal(0.0, 0.01, (len(near), 2)) * (1.0 if noise else 0.0), rng.uniform(-20, 20, (5, 2))])
    lp = np.concatenate([lp, rng.normal(0.0, 0.005, (len(lp), 1)) * (1.0 if noise else 0.0)], axis=1)
    ltruth = np.concatenate([near, np.full(5, -1)])
    lorder = rng.permutation(len(lp))
    ldets, lcones = lidar(lp[lorder], n_points=rng.randint(5, 40, len(lp)))
    c = case(f"scene_{'noisy' if noise else 'exact'}_pad{pad:g}", (dets, ccones), (ldets, lcones), level_to_cam=LEVEL_TO_CAM, cam=SCENE_CAM, lift=0.15,
             min_depth=0.5, max_depth=40.0, grow=1.0, pad=pad, range_abs=0.5, range_rel=0.1)
    c["truth"], c["ltruth"] = truth[order], ltruth[lorder]
    return c


def scene_cases():
    return [scene(noise=False, pad=0.0), scene(noise=True, pad=0.0), scene(noise=True, pad=4.0)]


def run_twin(c):
    from unina_yolo_dla_amd import fusion
    return fusion.fuse_numpy(c["dets"], c["count"], c["cones"], c["ldets"], c["lcount"], c["lcones"], c["params"])


_cache = {}


def cached(key, build):
    """Cases and their twin results are built once per process and shared, unchanged, by every test."""
    if key not in _cache:
        _cache[key] = [(c, run_twin(c)) for c in build()]
    return _cache[key]
