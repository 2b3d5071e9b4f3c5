"""Inputs shared by tests/test_cluster_cpu.py and tests/test_gpu_cluster.py: clouds built so that every point's cell is known,
and the named edge cases of unina_cluster_async (include/unina_mi355.h "cone candidates from a ground-free LiDAR sweep"). Pure
numpy; nothing here touches the device.

A PLACED cloud (tests/ground_cases.py) is seen through the identity extrinsic by a grid with x_min = y_min = 0 and cell = 1: the
point (cx + 0.5, cy + 0.5, z) lies in column cx of row cy, xl, yl and zl are the point's own x, y and z.
tests/test_cluster_cpu.py asserts on the twin what each case contains."""
import numpy as np

import ground_cases as gc
from clouds import ulp

F = np.float32
IDENTITY = gc.IDENTITY

# the sizes at which csrc/cluster.hip changes path
WAVE = 64                           # kWave: the points of a wave that share a component fold into one set of atomics
POINT_BLOCK = 256                   # kPtBlock: the workgroup of mark
SUM_BLOCK = 1024                    # kSumBlock: the workgroup of sums, whose waves meet in SLOTS LDS slots before the table's atomics
SLOTS = 64                          # kSlots: a workgroup of sums or cells with more components than this sends the rest to global memory
TILE = 32                           # kTile: the cells a label workgroup owns are TILE x TILE; merge joins across its borders
ROW_BLOCK = 1024                    # kRowBlock: cells (flatten, rank, cells) or components (finish, emit) that are one word of a scan
MAXD = 1024                         # MAX_DETECTIONS
MAX_SIDE = 1024                     # kGroundMaxSide

CLOUD_SIZES = (0, 1, WAVE - 1, WAVE, WAVE + 1, POINT_BLOCK - 1, POINT_BLOCK, POINT_BLOCK + 1, SUM_BLOCK - 1, SUM_BLOCK, SUM_BLOCK + 1)
TILE_GRIDS = tuple((nx, ny) for nx in (TILE - 1, TILE, TILE + 1) for ny in (TILE - 1, TILE, TILE + 1))
THIN_GRIDS = ((1, 1), (1, 300), (300, 1))


def params(**kw):
    """A gate that is exact in fp32 and lets every small component through unless a case narrows it."""
    p = dict(x_min=0.0, y_min=0.0, cell=1.0, nx=16, ny=12, min_points=1, max_points=1 << 22, min_height=0.0, max_height=4.0, max_width=4.0,
             confidence=0.75, class_id=2)
    p.update(kw)
    return p


def case(name, points, m=IDENTITY, **kw):
    return {"name": name, "points": np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3), "m": m, "params": params(**kw)}


def cells_cloud(occupied, per_cell=1, seed=0):
    """bool [ny, nx] -> per_cell points in every occupied cell, in random order, at random places inside the cell and heights 0 .. 1."""
    rng = np.random.RandomState(seed)
    cy, cx = np.nonzero(occupied)
    cx, cy = np.repeat(cx, per_cell), np.repeat(cy, per_cell)
    n = len(cx)
    pts = np.stack([cx + rng.uniform(0.05, 0.95, n), cy + rng.uniform(0.05, 0.95, n), rng.uniform(0.0, 1.0, n)], axis=1)
    return pts[rng.permutation(n)].astype(np.float32)


def occupancy_case(name, occupied, per_cell=1, seed=0, **kw):
    ny, nx = occupied.shape
    return case(name, cells_cloud(occupied, per_cell, seed), nx=nx, ny=ny, **kw)


def random_case(seed, n, nx=40, ny=30, **kw):
    """gc.random_cloud: points over the grid and one cell beyond each side, 5 % of them with a NaN or an infinity."""
    return case(f"random{n}_{nx}x{ny}", gc.random_cloud(seed, n, nx, ny), nx=nx, ny=ny, **kw)


def cloud_size_cases():
    """0, 1, a wave less one, a wave, a wave and one, and the two point workgroups less one, exact and plus one; the three largest on
    a grid they fill to a third, so that a workgroup of sums holds more components than it has LDS slots."""
    return [random_case(200 + k, n, *((40, 30) if n < SUM_BLOCK - 1 else (80, 60))) for k, n in enumerate(CLOUD_SIZES)]


def wall_case():
    """70 001 points, all in the last cell of a 1024-wide row: one atomic target for every wave, and Sx = 70 001 * ~262 000 > 2^32."""
    rng = np.random.RandomState(11)
    n = 70001
    pts = np.stack([1023.0 + rng.uniform(0.0, 0.999, n), rng.uniform(0.0, 0.999, n), rng.uniform(0.0, 2.0, n)], axis=1)
    return case("wall", pts, nx=MAX_SIDE, ny=1)


def grid_cases():
    """1 x 1, one column, one row; the label tile's edge less one, exact and plus one in each axis: random occupancy of 30 %."""
    out = []
    for k, (nx, ny) in enumerate(THIN_GRIDS + TILE_GRIDS):
        occupied = np.random.RandomState(300 + k).rand(ny, nx) < 0.3
        occupied[ny - 1, nx - 1] = True
        out.append(occupancy_case(f"grid{nx}x{ny}", occupied, per_cell=2, seed=k))
    return out


def corners_case():
    """1024 x 1024 cells, points only in the four corner cells (three in each): four components, 1024 label tiles of which 1020 are empty."""
    last = MAX_SIDE - 1
    rows = [(cx, cy, 0.1 * k + 0.05 * j) for k, (cx, cy) in enumerate(((0, 0), (last, 0), (0, last), (last, last))) for j in range(3)]
    return case("corners", gc.place(rows), nx=MAX_SIDE, ny=MAX_SIDE)


def straddle_case():
    """Five components of two cells each on 96 x 96 cells (3 x 3 tiles): across a vertical border, across a horizontal border, the
    two diagonals of the corner where four tiles meet at (32, 32) -- diagonal contact only -- kept apart by using the corner at
    (64, 64) for the second, and one pair inside a tile."""
    cells = [(31, 5), (32, 5), (5, 31), (5, 32), (31, 31), (32, 32), (64, 63), (63, 64), (10, 10), (11, 11)]
    occupied = np.zeros((96, 96), dtype=bool)
    for cx, cy in cells:
        occupied[cy, cx] = True
    return occupancy_case("straddle", occupied, per_cell=3, seed=4), cells


def serpentine(nx, ny):
    """Every even row full, the odd rows one cell at alternating ends: one component whose cells form one long chain."""
    occupied = np.zeros((ny, nx), dtype=bool)
    occupied[0::2] = True
    for j in range(1, ny, 2):
        occupied[j, nx - 1 if (j // 2) % 2 == 0 else 0] = True
    return occupied


def spiral(n):
    """A square spiral walked inwards from (0, 0), one empty cell between its arms: one component, one long chain."""
    occupied = np.zeros((n, n), dtype=bool)
    x, y, dx, dy = 0, 0, 1, 0
    occupied[0, 0] = True
    turns = 0
    while turns < 2:
        ax, ay, bx, by = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        ahead = 0 <= ax < n and 0 <= ay < n and not occupied[ay, ax]
        clear = not (0 <= bx < n and 0 <= by < n) or not occupied[by, bx]
        if ahead and clear:
            x, y, turns = ax, ay, 0
            occupied[y, x] = True
        else:
            dx, dy, turns = -dy, dx, turns + 1
    return occupied


def shape_cases():
    """A serpentine that fills one tile and one of 33 x 33 (the worst case of the propagation inside a tile), a serpentine and a
    spiral across 3 x 3 tiles (long chains of unions), a fully occupied 64 x 64 grid, and a checkerboard of isolated cells."""
    board = np.zeros((66, 66), dtype=bool)
    board[0::2, 0::2] = True
    return [occupancy_case("serpentine32", serpentine(TILE, TILE)), occupancy_case("serpentine33", serpentine(TILE + 1, TILE + 1)),
            occupancy_case("serpentine96", serpentine(3 * TILE, 3 * TILE)), occupancy_case("spiral96", spiral(3 * TILE)),
            occupancy_case("full64", np.ones((64, 64), dtype=bool), per_cell=2), occupancy_case("checkerboard", board)]


def isolated(k, side=100):
    """k isolated cells (even column, even row) of a side x side grid, in index order."""
    occupied = np.zeros((side, side), dtype=bool)
    slots = [(cy, cx) for cy in range(0, side, 2) for cx in range(0, side, 2)][:k]
    assert len(slots) == k
    for cy, cx in slots:
        occupied[cy, cx] = True
    return occupied


def count_cases():
    """Exactly 1023, 1024 and 1025 cones (n_dropped 0, 0, 1); 2500 components of which none is a cone; 2500 components of which only
    the last ten -- all in the third workgroup of finish and emit -- are cones."""
    out = [occupancy_case(f"cones{k}", isolated(k), seed=k) for k in (MAXD - 1, MAXD, MAXD + 1)]
    out.append(occupancy_case("no_cones", isolated(2500), min_points=2))
    pts = cells_cloud(isolated(2500), seed=6)
    last = [(98 - 2 * j, 98, 0.5) for j in range(10)]                         # a second point in each of the last ten cells
    out.append(case("late_cones", np.concatenate([pts, gc.place(last)]), nx=100, ny=100, min_points=2))
    return out


GATE = dict(min_points=2, max_points=4, min_height=0.125, max_height=0.5, max_width=0.5)


def gate_case():
    """One component per row of `rows`, each in a cell of its own (column 2 * k of row 0 of a 64 x 1 .. grid): two corner points
    (x_lo, y_lo, z_lo) and (x_hi, y_hi, z_hi) plus extra points at the first corner. Each threshold of GATE at equality and one ulp
    beside. Returns the case and, per component, whether it is a cone."""
    w, lo, hi = F(GATE["max_width"]), F(GATE["min_height"]), F(GATE["max_height"])

    def far(v0, kind):
        """the second corner's coordinate: `kind` says where v1 - v0 lies (the corners are exact in fp32, and so is their difference)"""
        return {"in": v0 + F(0.25), "on": v0 + w, "below": ulp(v0 + w, 0), "above": ulp(v0 + w, 1e9), "lo_on": v0 + lo, "lo_below": ulp(v0 + lo, 0),
                "hi_on": v0 + hi, "hi_above": ulp(v0 + hi, 1e9)}[kind]

    rows = [("in", "in", "in", 2, True),
            ("on", "in", "in", 2, True), ("below", "in", "in", 2, True), ("above", "in", "in", 2, False),
            ("in", "on", "in", 2, True), ("in", "below", "in", 2, True), ("in", "above", "in", 2, False),
            ("in", "in", "lo_on", 2, True), ("in", "in", "lo_below", 2, False), ("in", "in", "hi_on", 2, True), ("in", "in", "hi_above", 2, False),
            ("in", "in", "in", 1, False), ("in", "in", "in", 4, True), ("in", "in", "in", 5, False)]
    pts, cones = [], []
    for k, (kx, ky, kz, n, cone) in enumerate(rows):
        x0, y0, z0 = F(2 * k) + F(0.25), F(0.25), F(0.25)
        pts += [(x0, y0, z0)] * max(n - 1, 1)
        if n > 1:
            pts.append((far(x0, kx), far(y0, ky), far(z0, kz)))
        cones.append(cone)
    return case("gate", np.array(pts, dtype=np.float32), nx=2 * len(rows), ny=1, **GATE), cones


# ---------------------------------------------------------------- scenes
SCENE_CLUSTER = dict(x_min=0.0, y_min=-25.6, cell=0.1, nx=512, ny=512, min_points=5, max_points=300, min_height=0.1, max_height=0.45,
                     max_width=0.4, confidence=0.9, class_id=1)
ROW_GROUND = dict(x_min=0.0, y_min=-16.0, cell=1.0, nx=32, ny=32, z_lo=-0.3, z_hi=0.3, rise=0.05, band=0.03, max_height=0.6, reach=1,
                  keep_unknown=0)
ROW_CONES = [(4.0 + 3.0 * k, side * 1.5) for k in range(6) for side in (-1.0, 1.0)]      # (x, y) in the level frame


def two_row_scene(shift=0.0):
    """A level road 0.8 m under the LiDAR with two rows of six cones (0.3 m tall, 0.1 m base radius), a wall 7 m long and 1 m
    tall along y = 6, and a pole 2 m tall at (10, -5), all `shift` metres nearer than their nominal x. The points are in the
    LiDAR frame (gc.LIDAR_TO_LEVEL lifts them by 0.8 m)."""
    rng = np.random.RandomState(21)
    gx, gy = np.meshgrid(np.arange(0.25, 30.0, 0.5), np.arange(-14.75, 15.0, 0.5))
    road = np.stack([gx.reshape(-1), gy.reshape(-1), rng.normal(0.0, 0.005, gx.size)], axis=1)
    parts = [road]
    for cx, cy in ROW_CONES:
        h = rng.uniform(0.05, 0.3, 24)
        r = 0.1 * (1.0 - h / 0.32)
        a = rng.uniform(0.0, 2 * np.pi, 24)
        parts.append(np.stack([cx - shift + r * np.cos(a), cy + r * np.sin(a), h], axis=1))
    wall_x = rng.uniform(5.0, 12.0, 600)
    parts.append(np.stack([wall_x - shift, np.full(600, 6.02), rng.uniform(0.05, 1.0, 600)], axis=1))
    parts.append(np.stack([np.full(300, 10.03 - shift) + rng.uniform(-0.02, 0.02, 300), np.full(300, -5.03) + rng.uniform(-0.02, 0.02, 300),
                           rng.uniform(0.05, 2.0, 300)], axis=1))
    level = np.concatenate(parts)
    pts = level[rng.permutation(len(level))]
    pts[:, 2] -= gc.LIDAR_HEIGHT
    return {"name": "two_rows", "points": pts.astype(np.float32), "m": gc.LIDAR_TO_LEVEL, "params": dict(ROW_GROUND),
            "cluster": dict(SCENE_CLUSTER), "cones": [(cx - shift, cy) for cx, cy in ROW_CONES]}
