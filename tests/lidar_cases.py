"""Inputs shared by tests/test_lidar_cpu.py and tests/test_gpu_lidar.py: clouds built so that every point's pixel and key are
known, boxes, and the named edge cases of unina_locate_lidar_async (include/unina_mi355.h "3-D localisation from a LiDAR sweep").
Pure numpy; nothing here touches the device.

A PLACED cloud is seen through the identity extrinsic by a camera with cx = cy = 0: the point (u + 0.5) * z / fx, (v + 0.5) * z / fy,
z projects to the middle of pixel (u, v) -- the rounding of three fp32 operations moves it by far less than half a pixel -- and
its key is the bit pattern of z itself. tests/test_lidar_cpu.py asserts on the twin that every placed point landed where it was
put."""
import numpy as np

from locate_cases import boxes

MAXD = 1024
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
PLACED_CAM = (64.0, 64.0, 0.0, 0.0)
# LiDAR x forward, y left, z up -> camera x right, y down, z forward; the LiDAR sits 0.3 m above and 0.1 m behind the camera
MOUNTED = (0.0, -1.0, 0.0, 0.02, 0.0, 0.0, -1.0, 0.3, 1.0, 0.0, 0.0, -0.1)
W, H = 100, 70                      # the last cell of each axis is partial for cells of 32 and of 64 pixels
CAM = (70.0, 71.5, 48.25, 30.5)

# the thresholds at which csrc/lidar.hip's select kernel changes path
WAVE_CANDIDATES = 64                # kWave: a record with at most this many candidates (points in the cells its window touches) is a wave's
CACHE_KEYS = 8192                   # kCache: a record with at most this many valid keys keeps them in LDS between the passes


def params(**kw):
    p = dict(sx=1.0, sy=1.0, shrink=1.0, min_depth=0.3, max_depth=40.0, min_valid=1)
    p.update(kw)
    return p


def case(name, dets, points, width, height, count=None, m=IDENTITY, cam=PLACED_CAM, placed=None, **kw):
    """placed: the (u, v, key) rows the points were put at, where the case was built that way."""
    return {"name": name, "dets": dets, "count": len(dets) if count is None else count, "points": np.ascontiguousarray(points, dtype=np.float32),
            "m": m, "cam": cam, "width": width, "height": height, "params": params(**kw), "placed": placed}


def place(rows):
    """(u, v, z) rows -> [n, 3] float32 points for PLACED_CAM and the identity extrinsic, and the (u, v, key) rows they land on."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    z = rows[:, 2].astype(np.float32)
    fx, fy = np.float32(PLACED_CAM[0]), np.float32(PLACED_CAM[1])
    pts = np.stack([(rows[:, 0] + 0.5).astype(np.float32) * z / fx, (rows[:, 1] + 0.5).astype(np.float32) * z / fy, z], axis=1).astype(np.float32)
    want = np.stack([rows[:, 0], rows[:, 1], z.view(np.uint32)], axis=1).astype(np.int64)
    return pts, want


def bits_to_z(words):
    return np.asarray(words, dtype=np.uint32).view(np.float32).astype(np.float64)


class Scene:
    """Points collected region by region; a region is a 64 x 64-pixel square of the image, so it is made of whole cells for a cell
    size of 32 or of 64, and what is put into one region is no candidate of a window in another."""

    def __init__(self, seed, regions_x, regions_y):
        self.rng = np.random.RandomState(seed)
        self.width, self.height = 64 * regions_x, 64 * regions_y
        self.regions_x = regions_x
        self.rows, self.boxes = [], []

    def region(self, name, z_members, z_beside=(), window=(4, 4, 12, 12)):
        """`name` says what the region is for. A record whose window is the pixels `window` (x1, y1, x2, y2, exclusive end) of the next region, with one member per entry
        of z_members at random pixels of the window, and one point per entry of z_beside in the same 32-pixel cell but outside
        the window: a candidate that is no member."""
        j = len(self.boxes)
        ox, oy = 64 * (j % self.regions_x), 64 * (j // self.regions_x)
        assert oy < self.height
        x1, y1, x2, y2 = window
        for z in z_members:
            self.rows.append((ox + self.rng.randint(x1, x2), oy + self.rng.randint(y1, y2), z))
        for z in z_beside:
            self.rows.append((ox + 20 + self.rng.randint(0, 8), oy + 20 + self.rng.randint(0, 8), z))
        self.boxes.append((ox + x1, oy + y1, ox + x2 - 0.5, oy + y2 - 0.5))      # shrink = 1: floor(x2 - 0.5) is the last column

    def case(self, name, shuffle=True, **kw):
        pts, want = place(self.rows)
        if shuffle:
            order = self.rng.permutation(len(pts))
            pts, want = pts[order], want[order]
        return case(name, boxes(self.boxes), pts, self.width, self.height, placed=want, **kw)


def depths(rng, n):
    """n depths of 0.5 .. 30 m whose bit patterns differ in every byte."""
    return rng.uniform(0.5, 30.0, n).astype(np.float32).astype(np.float64)


def members_case(shuffle=True):
    """Members per record of 0, 1, 2, 63, 64, 65; candidates on and beside WAVE_CANDIDATES with few members; valid keys on and beside
    CACHE_KEYS; one record with more than 65 536 members (which is also a cell with more points than a workgroup has threads)."""
    s = Scene(21, 8, 2)
    r = s.rng
    for k in (0, 1, 2, 63, 64, 65):
        s.region(f"members{k}", depths(r, k))
    s.region("candidates64_members10", depths(r, 10), depths(r, WAVE_CANDIDATES - 10))
    s.region("candidates65_members10", depths(r, 10), depths(r, WAVE_CANDIDATES + 1 - 10))
    s.region("candidates100_members0", [], depths(r, 100))
    s.region("candidates64_valid0", [100.0] * 30 + [0.1] * 34)                        # every member out of range
    for k in (CACHE_KEYS - 1, CACHE_KEYS, CACHE_KEYS + 1):
        s.region(f"valid{k}", np.concatenate([depths(r, k), [100.0] * 5]))
    s.region("members66000", depths(r, 66000), window=(0, 0, 64, 64))
    return s.case("members" if shuffle else "members_in_sweep_order", shuffle)     # unshuffled: neighbouring points share a cell


def keys_case():
    """All members equal; two values with an even count; keys that differ only in the top byte and only in the bottom byte; valid and
    out-of-range members mixed. Each once for a wave (at most 64 candidates) and once for the workgroup."""
    s = Scene(22, 8, 2)
    top = bits_to_z([(b << 24) | 0x00123456 for b in (0x3f, 0x40, 0x41, 0x42)])      # 0.57 .. 36.6
    low = bits_to_z([0x41200000 | b for b in range(256)])                              # 10.0 .. 10.0002
    for tag, n in (("wave", 40), ("group", 600)):
        s.region(f"all_equal_{tag}", [12.5] * n)
        s.region(f"two_values_even_{tag}", [7.0] * (n // 2) + [3.0] * (n // 2))       # the lower one is the lower median
        s.region(f"top_byte_{tag}", np.resize(top, n))
        s.region(f"bottom_byte_{tag}", np.resize(low, n))
        s.region(f"mixed_{tag}", np.resize([5.0, 100.0, 9.0, 0.1, 7.0, 0.29999, 40.001], n))
        s.region(f"min_valid_{tag}", np.resize([100.0] * 9 + [6.0], n))               # a tenth of the members is valid
    return s.case("keys", min_valid=5)


def random_cloud(seed, n, width, height, spoiled=0.1, cam=CAM):
    """n points seen by `cam` through MOUNTED: spread over the image and a margin around it, 0.2 .. 50 m deep; `spoiled` of them NaN,
    infinite, behind the camera or at the LiDAR's origin."""
    rng = np.random.RandomState(seed)
    z = rng.uniform(0.2, 50.0, n)
    u, v = rng.uniform(-0.1 * width, 1.1 * width, n), rng.uniform(-0.1 * height, 1.1 * height, n)
    cam_xyz = np.stack([(u - cam[2]) * z / cam[0], (v - cam[3]) * z / cam[1], z], axis=1)
    m = np.asarray(MOUNTED).reshape(3, 4)
    lidar_xyz = (cam_xyz - m[:, 3]) @ m[:, :3]                                         # R is orthonormal: R^-1 = R^T
    pts = lidar_xyz.astype(np.float32)
    bad = rng.rand(n) < spoiled
    marks = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [-5, 0, 0], [0, 0, 0], [np.nan, np.nan, np.nan], [3e38, 3e38, 3e38]],
                     dtype=np.float32)
    pts[bad] = marks[rng.randint(0, len(marks), bad.sum())]
    return pts


def geometry_boxes():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rows = [(5, 5, 20, 20),                                  # inside one cell
            (60, 60, 70, 68), (30, 30, 34, 34), (63.5, 0, 64.5, 70),   # straddling cell corners and a cell edge
            (96, 0, 100, 70), (0, 64, 100, 70), (96, 64, 100, 70),      # along the last partial cell, and its corner
            (0, 0, 100, 70), (-50, -50, 200, 200),                      # the whole image
            (10, 10, 50, 40), (10, 10, 50, 40), (30, 20, 80, 60), (40, 30, 41, 31),   # identical and overlapping records
            (40, 10, 39.875, 30), (10, 30, 20, 29), (nan, 10, 20, 20), (10, 10, inf, 20), (200, 200, 220, 230), (-50, -50, -20, -20),
            (10, 70, 20, 90), (100, 10, 130, 20), (99.5, 69.5, 99.75, 69.75)]
    return boxes(rows)


def geometry_case():
    return case("geometry", geometry_boxes(), random_cloud(31, 3000, W, H), W, H, m=MOUNTED, cam=CAM)


def random_boxes(seed, n, width, height):
    rng = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        big = i % 10 == 9
        bw, bh = (rng.uniform(0.1, 0.6) * width, rng.uniform(0.1, 0.6) * height) if big else (rng.uniform(0, 40), rng.uniform(0, 60))
        x1, y1 = rng.uniform(-20, width), rng.uniform(-20, height)
        rows.append(np.round(np.array([x1, y1, x1 + bw, y1 + bh]) * 8) / 8)
    return boxes(rows)


def large_image_case():
    """4096 x 2048: 8192 cells of 32 x 32 pixels, more than one pass of the scan."""
    w, h = 4096, 2048
    cam = (1400.0, 1400.0, 2047.5, 1023.5)
    rng = np.random.RandomState(41)
    n = 20000
    z = rng.uniform(0.2, 50.0, n)
    u, v = rng.uniform(-50, w + 50, n), rng.uniform(-50, h + 50, n)
    pts = np.stack([(u - cam[2]) * z / cam[0], (v - cam[3]) * z / cam[1], z], axis=1).astype(np.float32)
    dets = np.concatenate([random_boxes(42, 60, w, h), boxes([(0, 0, w, h), (4064, 2016, 4096, 2048), (0, 0, 32, 32)])])
    dets["confidence"] = np.linspace(0.99, 0.05, len(dets)).astype(np.float32)
    return case("image4096x2048", dets, pts, w, h, cam=cam, shrink=0.7)


def random_case(n_boxes=200, n_points=6000, seed=51, **kw):
    return case(f"random{n_boxes}", random_boxes(seed, n_boxes, W, H), random_cloud(seed + 1, n_points, W, H), W, H, m=MOUNTED, cam=CAM,
                shrink=0.6, **kw)


GRID = [(3 * (i % 32) + 0.25, (i // 32) + 0.25, 3 * (i % 32) + 2.75, (i // 32) + 2.75) for i in range(MAXD)]   # 3 x 3 windows, all on the image


def count_cases():
    pts = random_cloud(61, 4000, W, H, spoiled=0.0)
    return [case(name, boxes(GRID[:n_boxes]), pts, W, H, count=count, m=MOUNTED, cam=CAM)
            for name, n_boxes, count in (("count0", 8, 0), ("count1", 8, 1), ("count1024", 1024, 1024), ("count5000", 1024, 5000),
                                         ("count_negative", 8, -3))]


def cloud_size_cases():
    pts = random_cloud(71, 257, W, H, spoiled=0.05)
    dets = boxes([(0, 0, 100, 70), (10, 10, 60, 50), (50, 20, 99, 69), (200, 200, 210, 210)])
    return [case(f"points{n}", dets, pts[:n], W, H, m=MOUNTED, cam=CAM) for n in (0, 1, 63, 64, 65, 255, 256, 257)]


SCAN_CELLS = (1, 1, 4, 15, 4096, 4160)


def scan_edge_cases():
    """Image sizes whose cell counts (SCAN_CELLS) sit on the edges of csrc/lidar.hip's scan, which takes four cells a thread
    (kScanPer) and 4096 a pass (kScanBlock * kScanPer): one cell, four, 15 (a last thread with three cells), 4096 (exactly one
    pass) and 4160 (a second pass of 64 cells)."""
    out = []
    for k, (w, h) in enumerate(((1, 1), (32, 32), (33, 33), (160, 70), (2048, 2048), (2080, 2048))):
        cam = (0.7 * w, 0.7 * w, 0.5 * w - 0.5, 0.5 * h - 0.5)
        dets = np.concatenate([random_boxes(90 + k, 20, w, h), boxes([(0, 0, w, h)])])
        out.append(case(f"image{w}x{h}", dets, random_cloud(95 + k, 3000 if w > 1000 else 300, w, h, cam=cam), w, h, m=MOUNTED, cam=cam))
    return out


def all_cases():
    return [members_case(), keys_case(), geometry_case(), large_image_case(), random_case()]


def tracker_frames():
    """Three frames of eight cones seen 6 .. 20 m ahead, the cloud a dozen points on each cone and clutter; the boxes move by a pixel a
    frame."""
    frames = []
    w, h, cam = 640, 360, (500.0, 500.0, 319.5, 179.5)
    for f in range(3):
        rng = np.random.RandomState(80 + f)
        rows, pts = [], []
        for k in range(8):
            z = 6.0 + 2.0 * k
            uc, vc = 60.0 + 70.0 * k + f, 200.0 - 4.0 * k
            half = 120.0 / z
            rows.append((uc - half, vc - 1.5 * half, uc + half, vc + 1.5 * half))
            u, v = uc + rng.uniform(-0.4, 0.4, 12) * half, vc + rng.uniform(-0.6, 0.6, 12) * half
            zz = z + rng.uniform(-0.05, 0.05, 12)
            pts.append(np.stack([(u - cam[2]) * zz / cam[0], (v - cam[3]) * zz / cam[1], zz], axis=1))
        clutter_z = rng.uniform(1.0, 60.0, 500)
        cu, cv = rng.uniform(0, w, 500), rng.uniform(0, h, 500)
        pts.append(np.stack([(cu - cam[2]) * clutter_z / cam[0], (cv - cam[3]) * clutter_z / cam[1], clutter_z], axis=1))
        cam_xyz = np.concatenate(pts)
        m = np.asarray(MOUNTED).reshape(3, 4)
        lidar = ((cam_xyz - m[:, 3]) @ m[:, :3]).astype(np.float32)
        frames.append(case(f"frame{f}", boxes(rows), lidar[rng.permutation(len(lidar))], w, h, m=MOUNTED, cam=cam, shrink=0.5, min_valid=3))
    return frames
