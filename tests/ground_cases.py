"""Inputs shared by tests/test_ground_cpu.py and tests/test_gpu_ground.py: clouds built so that every point's cell and height
are known, and the named edge cases of unina_ground_filter_async (include/unina_mi355.h "ground removal from a LiDAR sweep").
Pure numpy; nothing here touches the device.

A PLACED cloud is seen through the identity extrinsic by a grid with x_min = y_min = 0 and cell = 1: the point (cx + 0.5, cy + 0.5, z)
has fx = cx + 0.5 and fy = cy + 0.5 exactly, so it lies in column cx of row cy, and its height is z itself.
tests/test_ground_cpu.py asserts on the twin that every placed point landed where it was put."""
import numpy as np

from locate_cases import boxes

IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
# the identity with -0.0 for every zero: ((1 * x + -0.0 * y) + -0.0 * z) + -0.0 is x for every x, y, z >= 0, -0.0 included, where
# IDENTITY gives +0.0 for x = -0.0
NEGATIVE_ZEROS = tuple(v if v else -0.0 for v in IDENTITY)

# the sizes at which csrc/ground.hip changes path
WAVE = 64                           # kWave: the seeds of a wave that share a cell fold into one atomicMin
SEED_BLOCK = 256                    # kSeedBlock
POINT_BLOCK = 1024                  # kPtBlock: the kept points of one classify / scatter workgroup are one word of the scan
SCAN_PER = 4                        # kScanPer: workgroup counts a thread of the scan takes; 2049 points are 3 counts, 4097 are 5
TILE_X, TILE_Y = 32, 8              # kTileX, kTileY: the cells an envelope workgroup owns
MAX_REACH = 4                       # kGroundMaxReach = UNINA_GROUND_MAX_REACH: the halo of the envelope's tile
MAX_SIDE = 1024                     # kGroundMaxSide = UNINA_GROUND_MAX_SIDE

CLOUD_SIZES = (0, 1, WAVE - 1, WAVE, WAVE + 1, POINT_BLOCK - 1, POINT_BLOCK, POINT_BLOCK + 1, 2 * POINT_BLOCK + 1, 70001)
TILE_GRIDS = tuple((nx, ny) for nx in (TILE_X - 1, TILE_X, TILE_X + 1) for ny in (TILE_Y - 1, TILE_Y, TILE_Y + 1))
THIN_GRIDS = ((1, 1), (1, 300), (300, 1))


def params(**kw):
    """Thresholds that are exact in fp32, so a placed height is on or beside them by construction."""
    p = dict(x_min=0.0, y_min=0.0, cell=1.0, nx=16, ny=12, z_lo=-1.0, z_hi=1.0, rise=0.125, band=0.0625, max_height=0.5, reach=1, keep_unknown=0)
    p.update(kw)
    return p


def case(name, points, m=IDENTITY, **kw):
    return {"name": name, "points": np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3), "m": m, "params": params(**kw)}


def place(rows):
    """(cx, cy, z) rows -> [n, 3] float32 points for the identity extrinsic and a unit grid at the origin."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    return np.stack([rows[:, 0] + 0.5, rows[:, 1] + 0.5, rows[:, 2]], axis=1).astype(np.float32)


def random_cloud(seed, n, nx, ny):
    """n points over a unit grid of nx x ny cells and one cell beyond each side: 60 % road (heights of a few centimetres around 0),
    25 % objects, 5 % above any object, 5 % far below the road, 5 % spoiled (a NaN or an infinity in one coordinate)."""
    rng = np.random.RandomState(seed)
    kind = rng.choice(5, n, p=[0.6, 0.25, 0.05, 0.05, 0.05])
    z = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [rng.normal(0.0, 0.02, n), rng.uniform(0.08, 0.45, n), rng.uniform(0.7, 3.0, n),
                                                                  rng.uniform(-9.0, -4.0, n)], 0.0)
    pts = np.stack([rng.uniform(-1.0, nx + 1.0, n), rng.uniform(-1.0, ny + 1.0, n), z], axis=1).astype(np.float32)
    bad = np.nonzero(kind == 4)[0]
    pts[bad, rng.randint(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), len(bad))
    return pts


def random_case(seed, n, nx=16, ny=12, **kw):
    return case(f"random{n}_{nx}x{ny}", random_cloud(seed, n, nx, ny), nx=nx, ny=ny, **kw)


def cloud_size_cases():
    """0, 1, a wave less one, a wave, a wave and one, a classify workgroup less one, exact and plus one, three workgroup counts (a
    thread of the scan with fewer than four), and 69 workgroups."""
    return [random_case(100 + k, n, keep_unknown=k % 2) for k, n in enumerate(CLOUD_SIZES)]


def kept_pattern_cases():
    """What the scan and the scatter see: every point kept, none, every other one, and only points of the last workgroup."""
    n = 3 * POINT_BLOCK + 100
    cells = np.stack([(np.arange(n) // 2) % 16, (np.arange(n) // 32) % 12], axis=1)   # points 2j and 2j + 1 share a cell
    high = place(np.concatenate([cells, np.full((n, 1), 3.0)], axis=1))          # no seed anywhere: every point UNKNOWN
    z = np.where(np.arange(n) % 2 == 0, 0.0, 0.25)
    z_last = np.where(np.arange(n) >= n - 50, 0.25, 0.0)
    return [case("all_kept", high, keep_unknown=1), case("none_kept", high, keep_unknown=0),
            case("alternating", place(np.concatenate([cells, z[:, None]], axis=1)), z_hi=0.125),
            case("last_workgroup", place(np.concatenate([cells, z_last[:, None]], axis=1)), z_hi=0.125)]


def one_cell_case():
    """5000 seeds and 1000 objects in ONE cell of a 3 x 3 grid: one atomic target, one ground word for every point."""
    rng = np.random.RandomState(5)
    z = np.concatenate([rng.uniform(-0.05, 0.05, 5000), rng.uniform(0.2, 0.4, 1000)])[rng.permutation(6000)]
    return case("one_cell", place(np.stack([np.ones(6000), np.ones(6000), z], axis=1)), nx=3, ny=3, z_hi=0.125, band=0.125, reach=0)


def distinct_cells_case():
    """4096 seeds, point i in cell i of a 64 x 64 grid: every lane of every wave in a cell of its own, 64 atomics a wave."""
    i = np.arange(4096)
    z = np.random.RandomState(6).uniform(-0.5, 0.5, 4096)
    return case("distinct_cells", place(np.stack([i % 64, i // 64, z], axis=1)), nx=64, ny=64, reach=0)


def shared_lanes_case():
    """Nine waves of 64 seeds in sweep order: the lanes of a wave in runs of 2, 3 or 64 that share a cell, the run's minimum in its
    first, a middle or its last lane; every run has a cell of its own. Returns the case and, per run, (cell, minimum)."""
    rows, runs = [], []
    rng = np.random.RandomState(7)
    cell = 0
    for share in (2, 3, WAVE):
        for where in ("first", "middle", "last"):
            for start in range(0, WAVE, share):
                length = min(share, WAVE - start)
                z = rng.uniform(0.0, 0.9, length)
                low = {"first": 0, "middle": length // 2, "last": length - 1}[where]
                z[low] = -0.5 - 0.001 * cell
                rows += [(cell % 64, cell // 64, v) for v in z]
                runs.append((cell, np.float32(z[low])))
                cell += 1
    assert len(rows) == 9 * WAVE and cell <= 64 * 64
    return case("shared_lanes", place(rows), nx=64, ny=64, reach=0), runs


def grid_case(nx, ny, reach, seed=8, **kw):
    """A random cloud of 40 points a cell at most, 3000 at least, on a grid of nx x ny."""
    return random_case(seed + nx + 7 * ny, min(max(3000, 4 * nx * ny), 40 * nx * ny), nx, ny, reach=reach, **kw)


def grid_cases():
    """1 x 1, one column, one row; the envelope tile's width and height less one, exact and plus one; reach 0 and 4 on each."""
    out = []
    for k, (nx, ny) in enumerate(THIN_GRIDS + TILE_GRIDS):
        for reach in (0, MAX_REACH):
            out.append(grid_case(nx, ny, reach, keep_unknown=(k + reach // 4) % 2))
    return out


def corners_case(reach=MAX_REACH):
    """1024 x 1024 cells, seeds only in the four corner cells, one object point over each and a point in the middle of the grid
    and of every side (UNKNOWN there: no seed within reach)."""
    last = MAX_SIDE - 1
    rows = []
    for k, (cx, cy) in enumerate(((0, 0), (last, 0), (0, last), (last, last))):
        rows += [(cx, cy, 0.01 * k), (cx, cy, 0.01 * k + 0.25), (abs(cx - 3), abs(cy - 2), 0.4)]
    rows += [(512, 512, 2.0), (512, 0, 2.0), (0, 512, 2.0), (last, 512, 2.0), (512, last, 2.0)]
    return case(f"corners_reach{reach}", place(rows), nx=MAX_SIDE, ny=MAX_SIDE, z_hi=0.125, reach=reach, keep_unknown=1)


def envelope_case(reach, rise, nx=11, ny=9):
    """Seeds in the four corners, the middle of every side and the centre of an 11 x 9 grid, each with a height of its own, and a
    probe (a point too high to be a seed) in EVERY cell, whose h shows the envelope there."""
    seeds = [(cx, cy, 0.03125 * (1 + k) - 0.2) for k, (cx, cy) in enumerate((x, y) for y in (0, ny // 2, ny - 1) for x in (0, nx // 2, nx - 1))]
    probes = [(cx, cy, 4.0) for cy in range(ny) for cx in range(nx)]
    return case(f"envelope_reach{reach}_rise{rise}", place(seeds + probes), nx=nx, ny=ny, reach=reach, rise=rise, max_height=8.0), seeds


# ---------------------------------------------------------------- the scene that justifies the stage
LIDAR_HEIGHT = 0.8                   # metres above a level road
CONE_X, CONE_H, CONE_R = 15.0, 0.325, 0.114   # a small Formula Student cone (228 mm base, 325 mm tall), straight ahead
LIDAR_TO_LEVEL = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, LIDAR_HEIGHT)   # the road is z = 0
# LiDAR x forward, y left, z up -> camera x right, y down, z forward; the camera sits 0.2 m below and 0.1 m ahead of the LiDAR
SCENE_TO_CAM = (0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, -0.2, 1.0, 0.0, 0.0, -0.1)
SCENE_CAM = (1400.0, 1400.0, 959.5, 539.5)
SCENE_W, SCENE_H = 1920, 1080
SCENE_GROUND = dict(x_min=0.0, y_min=-32.0, cell=2.0, nx=32, ny=32, z_lo=-0.3, z_hi=0.3, rise=0.05, band=0.03, max_height=0.6, reach=1,
                    keep_unknown=0)
SCENE_LIDAR = dict(sx=1.0, sy=1.0, shrink=0.9, min_depth=0.5, max_depth=60.0, min_valid=1)


def cone_scene():
    """A ring LiDAR over a level road with one cone 15 m ahead: 48 rings from -11.85 to +2.15 degrees (the lowest ring on the cone meets it 4 cm above the road), 0.1 degree in azimuth over the 60
    degrees ahead, in firing order. A ray returns from the cone, else from the road within 60 m, else not at all. The record is the
    cone's outline in the image, as a detector draws it. Returns points, the masks of the cone's and the road's returns, the
    record and everything the two stages take."""
    el = np.deg2rad(np.linspace(-11.85, 2.15, 48))
    az = np.deg2rad(np.arange(-30.0, 30.0, 0.1))
    a, e = [v.reshape(-1) for v in np.meshgrid(az, el, indexing="ij")]
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=1)
    # the cone: (x - CONE_X)^2 + y^2 = (c * (z - apex))^2 for apex - CONE_H <= z <= apex
    apex, c2 = CONE_H - LIDAR_HEIGHT, (CONE_R / CONE_H) ** 2
    qa = d[:, 0] ** 2 + d[:, 1] ** 2 - c2 * d[:, 2] ** 2
    qb = -2.0 * CONE_X * d[:, 0] + 2.0 * c2 * d[:, 2] * apex
    qc = CONE_X ** 2 - c2 * apex ** 2
    disc = qb ** 2 - 4.0 * qa * qc
    t_cone = np.where(disc >= 0, (-qb - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * qa), np.inf)
    z_hit = t_cone * d[:, 2]
    on_cone = np.isfinite(t_cone) & (t_cone > 0) & (z_hit <= apex) & (z_hit >= apex - CONE_H)
    with np.errstate(divide="ignore"):
        t_road = np.where(d[:, 2] < 0, -LIDAR_HEIGHT / d[:, 2], np.inf)
    on_road = ~on_cone & (t_road < 60.0)
    t = np.where(on_cone, t_cone, t_road)
    keep = on_cone | on_road
    pts = (t[keep, None] * d[keep]).astype(np.float32)
    # the cone's outline through the camera: base corners and apex
    m = np.asarray(SCENE_TO_CAM).reshape(3, 4)
    outline = np.array([[CONE_X, CONE_R, -LIDAR_HEIGHT, 1.0], [CONE_X, -CONE_R, -LIDAR_HEIGHT, 1.0], [CONE_X, 0.0, apex, 1.0]]) @ m.T
    u = SCENE_CAM[0] * outline[:, 0] / outline[:, 2] + SCENE_CAM[2]
    v = SCENE_CAM[1] * outline[:, 1] / outline[:, 2] + SCENE_CAM[3]
    dets = boxes([(u.min(), v.min(), u.max(), v.max())])
    return {"name": "cone_scene", "points": pts, "is_cone": on_cone[keep], "is_road": on_road[keep], "dets": dets, "count": 1,
            "m": LIDAR_TO_LEVEL, "params": dict(SCENE_GROUND), "to_cam": SCENE_TO_CAM, "cam": SCENE_CAM, "width": SCENE_W, "height": SCENE_H,
            "lidar_params": dict(SCENE_LIDAR), "cone_depth": CONE_X - 0.1}


def assert_scene(s, raw, filtered, out):
    """What the scene was built to show, on any pair of results: the raw cloud's depth is a road return more than 1 m behind the
    cone, the filtered cloud's depth is a cone return."""
    from unina_yolo_dla_amd import localize                # numpy only: no device is touched
    p = s["lidar_params"]
    px = localize.project_lidar_numpy(s["points"], s["to_cam"], s["cam"], s["width"], s["height"], p["min_depth"], p["max_depth"])
    depth = px["key"].view(np.float32)
    assert raw["valid"][0] == 1 and filtered["valid"][0] == 1
    assert raw["z"][0] in depth[s["is_road"]] and raw["z"][0] not in depth[s["is_cone"]] and raw["z"][0] > s["cone_depth"] + 1.0
    assert filtered["z"][0] in depth[s["is_cone"]] and abs(filtered["z"][0] - s["cone_depth"]) < 0.15
    assert filtered["n_samples"][0] < raw["n_samples"][0] - filtered["n_samples"][0]          # fewer cone returns than road returns in the box
    assert out[:int(s["is_cone"].sum()), :3].tobytes() == s["points"][s["is_cone"]].tobytes()
