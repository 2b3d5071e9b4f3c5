"""The constructed inputs of the de-skew tests (tests/test_deskew_cpu.py, tests/test_gpu_deskew.py), each beside the constant of
csrc/deskew.hip or csrc/deskew_math.h it sits on, and the exact motion the physical checks measure against.

A case is a dict: name, points ([n, 3] float32), times (n float32 seconds or n uint32 nanoseconds), fmt, poses (K rows of t, qw,
qx, qy, qz, px, py, pz in float64), t_sweep, t_ref. How the cloud is laid out on the device (stride, base, where the times and
the carried word live) is the GPU test's choice."""
import numpy as np

import cluster_cases as cc
import ground_cases as gc
from clouds import ulp

F = np.float32
WAVE = 64                           # kWave: counts and the shift are folded per wave before the atomics
BLOCK = 256                         # kDeskewBlock: the points of a workgroup, each of which copies the table to LDS
MAX_KEYS = 64                       # kDeskewMaxKeys = UNINA_DESKEW_MAX_KEYS: the bisection's first probe is key 63
F32_S, U32_NS = 0, 1                # UNINA_TIME_F32_S, UNINA_TIME_U32_NS
NAN_WORD = 0x7fc00000

CLOUD_SIZES = (0, 1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 70001)
KEY_COUNTS = (2, 3, MAX_KEYS)
SWEEP = 0.1                         # seconds a sweep takes
SPEED, YAW_RATE = 15.0, 1.5         # m/s, rad/s: the cornering vehicle of the physical checks


# ---------------------------------------------------------------- motion
def arc_pose(t, v=SPEED, w=YAW_RATE, origin=(0.0, 0.0, 0.0), heading=0.0):
    """The exact pose (q as w, x, y, z; p) at time t of a vehicle on a constant-twist arc in the plane: float64."""
    t = np.asarray(t, dtype=np.float64)
    th = heading + w * t
    px = origin[0] + (v / w) * (np.sin(th) - np.sin(heading))
    py = origin[1] - (v / w) * (np.cos(th) - np.cos(heading))
    zero = np.zeros_like(th)
    return np.stack([np.cos(th / 2), zero, zero, np.sin(th / 2)], axis=-1), np.stack([px, py, zero + origin[2]], axis=-1)


def arc_poses(n_keys, t_sweep=0.0, span=SWEEP, **kw):
    """n_keys equally spaced keys of arc_pose over [t_sweep, t_sweep + span] as rows of t, q, p. The motion starts at t_sweep."""
    rel = np.linspace(0.0, span, n_keys)
    q, p = arc_pose(rel, **kw)
    return np.concatenate([(t_sweep + rel)[:, None], q, p], axis=1)


def identity_poses(n_keys, span=SWEEP):
    rows = np.zeros((n_keys, 8))
    rows[:, 0], rows[:, 1] = np.linspace(0.0, span, n_keys), 1.0
    return rows


def rotate(q, v):
    """R(q) v for float64 unit quaternions [n, 4] (or one) and vectors [n, 3]: the textbook matrix, not the code under test."""
    w, x, y, z = np.moveaxis(np.asarray(q, dtype=np.float64), -1, 0)
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    return np.einsum("...ij,...j->...i", R, v)


def conj(q):
    return np.asarray(q, dtype=np.float64) * np.array([1.0, -1.0, -1.0, -1.0])


def measure(at_ref, times, t_ref, **kw):
    """Static points given in the LiDAR frame of time t_ref, as the moving LiDAR measures them at `times` (float64)."""
    q_ref, p_ref = arc_pose(t_ref, **kw)
    q, p = arc_pose(times, **kw)
    world = rotate(q_ref, at_ref) + p_ref
    return rotate(conj(q), world - p)


# ---------------------------------------------------------------- clouds
def case(name, points, times, poses, fmt=F32_S, t_sweep=0.0, t_ref=None):
    poses = np.asarray(poses, dtype=np.float64)
    return {"name": name, "points": np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3), "times": np.ascontiguousarray(times), "fmt": fmt,
            "poses": poses, "t_sweep": t_sweep, "t_ref": poses[-1, 0] if t_ref is None else t_ref}


def random_points(rng, n, reach=30.0):
    return rng.uniform(-reach, reach, (n, 3)).astype(np.float32) * np.array([1.0, 1.0, 0.1], dtype=np.float32)


def random_times(rng, n, fmt, span=SWEEP):
    if fmt == U32_NS:
        return rng.randint(0, int(span * 1e9) + 1, n).astype(np.uint32)
    return rng.uniform(0.0, span, n).astype(np.float32)


def random_case(seed, n, n_keys=11, fmt=F32_S, **kw):
    rng = np.random.RandomState(seed)
    return case(f"random{seed}_{n}_{n_keys}", random_points(rng, n), random_times(rng, n, fmt), arc_poses(n_keys), fmt, **kw)


def cloud_size_cases():
    """0, 1, kWave - 1 | kWave | kWave + 1, kDeskewBlock - 1 | kDeskewBlock | kDeskewBlock + 1 and 70 001 points (274 workgroups, the last
    with 113 points); both formats and K = 2, 3, 64 in turn."""
    return [random_case(300 + i, n, KEY_COUNTS[i % 3], (F32_S, U32_NS)[i % 2], t_ref=(SWEEP, 0.05, 0.0)[i % 3]) for i, n in enumerate(CLOUD_SIZES)]


def key_time_case(n_keys):
    """tau exactly on every key time of the table, one ulp below and above each, two times before t_0 and two after t_{K-1}: the
    probes of deskew_segment on both sides of every `<=`, s == 0 and s == 1 exactly, and both clamps. Returns the case and
    (n_before, n_after)."""
    rng = np.random.RandomState(40 + n_keys)
    poses = arc_poses(n_keys)
    t = poses[:, 0].astype(np.float32)                      # t_sweep = 0: the table's float32 times
    times = np.concatenate([t, [ulp(v, -1.0) for v in t], [ulp(v, 1.0) for v in t], [F(-0.01), F(-1e-30), F(0.1001), F(7.0)]]).astype(np.float32)
    n_before, n_after = int((times < t[0]).sum()), int((times > t[-1]).sum())
    assert (n_before, n_after) == (3, 3)                    # the ulp below t_0 = 0 and above t_{K-1} count too
    return case(f"key_times_{n_keys}", random_points(rng, len(times)), times, poses, t_ref=0.05), (n_before, n_after)


def one_segment_case(n_keys=MAX_KEYS, segment=37, n=3 * BLOCK + 5):
    """Every point inside one segment of the table: every lane of every wave reads the same two rows."""
    rng = np.random.RandomState(44)
    poses = arc_poses(n_keys)
    t = poses[:, 0].astype(np.float32)
    times = rng.uniform(ulp(t[segment], 1.0), ulp(t[segment + 1], 0.0), n).astype(np.float32)
    return case("one_segment", random_points(rng, n), times, poses, t_ref=0.03)


def special_value_case():
    """NaN, +inf and -inf in each coordinate and in the time, -0.0 coordinates, and 200 ordinary points around them. Returns the case
    and the indices of the points that must come out INVALID."""
    rng = np.random.RandomState(45)
    pts, times = random_points(rng, 200), random_times(rng, 200, F32_S)
    bad = []
    at = 3
    for v in (np.nan, np.inf, -np.inf):
        for col in range(3):
            pts[at, col] = v
            bad.append(at)
            at += 7
        times[at] = v
        bad.append(at)
        at += 7
    pts[at] = (-0.0, -0.0, -0.0)
    pts[at + 1, 1] = -0.0
    return case("special_values", pts, times, arc_poses(11), t_ref=0.05), sorted(bad)


def nanosecond_edge_case():
    """uint32 times 0 and 0xffffffff (4.29 s: AFTER), and the nanoseconds around each key of a K = 3 table."""
    rng = np.random.RandomState(46)
    times = np.array([0, 0xffffffff, 1, 49999999, 50000000, 50000001, 99999999, 100000000, 100000001, 0x80000000], dtype=np.uint32)
    return case("nanosecond_edges", random_points(rng, len(times)), times, arc_poses(3), U32_NS, t_ref=0.05)


def identity_case(n=2 * BLOCK + 3):
    """Identity keys: every finite coordinate comes back as the number it was."""
    rng = np.random.RandomState(47)
    pts = random_points(rng, n)
    pts[5] = (-0.0, 0.0, -0.0)
    pts[6] = (1e30, -1e30, 1e-40)                           # far, and a denormal
    return case("identity", pts, random_times(rng, n, F32_S), identity_poses(5), t_ref=0.04)


# ---------------------------------------------------------------- scenes
CONE_AT = (10.0, 2.0)                                        # level frame at t_ref, metres


def cone_points(rng, n=24):
    """n returns of a cone 0.3 m tall with a 0.1 m base radius at CONE_AT, in the LiDAR frame of t_ref (gc.LIDAR_TO_LEVEL lifts it)."""
    h = rng.uniform(0.05, 0.3, n)
    r = 0.1 * (1.0 - h / 0.32)
    a = rng.uniform(0.0, 2 * np.pi, n)
    return np.stack([CONE_AT[0] + r * np.cos(a), CONE_AT[1] + r * np.sin(a), h - gc.LIDAR_HEIGHT], axis=1)


def cornering_cone_scene(with_road=True, t_ref=SWEEP, n_keys=11):
    """A level road and one cone, static, seen by a LiDAR that corners at SPEED and YAW_RATE while the sweep lasts; every return has
    a time of its own. The cone's 24 returns are spread evenly over the sweep, 4.3 ms apart: the vehicle moves 6.5 cm and turns
    6.5 mrad between two of them, so at 10 m neighbours in time lie about 0.13 m apart and any five of them more than the 0.4 m a
    cone may be wide -- as measured, no piece of the smear can pass the clusterer's gate. `truth` holds the points as a LiDAR
    standing still at t_ref would have seen them."""
    rng = np.random.RandomState(48)
    parts, stamps = [cone_points(rng)], [rng.permutation(np.linspace(0.0, SWEEP, 24))]
    if with_road:
        gx, gy = np.meshgrid(np.arange(0.25, 30.0, 0.5), np.arange(-14.75, 15.0, 0.5))
        parts.append(np.stack([gx.reshape(-1), gy.reshape(-1), rng.normal(0.0, 0.005, gx.size) - gc.LIDAR_HEIGHT], axis=1))
        stamps.append(rng.uniform(0.0, SWEEP, gx.size))
    order = rng.permutation(sum(len(p) for p in parts))
    truth = np.concatenate(parts)[order]
    times = np.concatenate(stamps)[order].astype(np.float32)
    c = case("cornering_cone", measure(truth, times.astype(np.float64), t_ref), times, arc_poses(n_keys), t_ref=t_ref)
    c.update(truth=truth, is_cone=order < 24, m=gc.LIDAR_TO_LEVEL, ground=dict(cc.ROW_GROUND), cluster=dict(cc.SCENE_CLUSTER))
    return c
