"""Inputs shared by tests/test_boundary_cpu.py and tests/test_gpu_boundary.py: the named calls of unina_boundary_async
(include/unina_mi355.h "track limits and centre line"), the synthetic oval track and the drive along it. A case is one call: the
tracker's 1024 slots, the device pose (one POSE_RESULT_DTYPE record) or None, and the parameters. Pure numpy; nothing here touches
the device."""
import numpy as np

import pose_cases as pc
import track_cases as tc

MAXD = 1024
F = np.float32
NAN, INF = float("nan"), float("inf")
LIMIT = 32768.0
LEFT, RIGHT, OTHER = 1, 0, 2                  # class ids: blue, yellow, orange
NO_FIRST, NO_NEXT, FULL, NO_HEADING = 0, 1, 2, 3
LEVEL = (1.0, 0.0, 0.0)                       # forward axis of a level frame; with the identity pose: o = (0, 0), h = (1, 0)
PINHOLE_TO_LEVEL = np.array([[0.0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0]])   # camera z forward, x right, y down -> x forward, y left, z up


def params(**kw):
    p = dict(pose=None, forward=LEVEL, first_gate=8.0, step_gate=4.0, cos_turn=0.5, width_gate=6.0, class_left=LEFT, class_right=RIGHT,
             min_hits=3, max_chain=64)
    p.update(kw)
    return p


class Table:
    """The tracker's 1024 slots, filled group by group; ids count from 1 in the order of the adds."""

    def __init__(self):
        from unina_yolo_dla_amd.tracking import TRACK_DTYPE
        self.t = np.zeros(MAXD, dtype=TRACK_DTYPE)
        self.next_id = 1

    def add(self, points, cls, hits=5, slots=None, live=True):
        """points: [m, 2] or [m, 3]. slots: where they go (default: the first free slots). live=False: id stays 0. Returns self."""
        pts = np.asarray(points, dtype=np.float64).reshape(len(points), -1)
        if pts.shape[1] == 2:
            pts = np.concatenate([pts, np.full((len(pts), 1), 0.25)], axis=1)
        free = np.nonzero((self.t["id"] == 0) & (self.t["hits"] == 0))[0]
        s = free[:len(pts)] if slots is None else np.asarray(slots)
        t = self.t
        t["x"][s], t["y"][s], t["z"][s] = pts.astype(np.float32).T
        t["confidence"][s], t["class_id"][s], t["hits"][s] = 0.9, cls, hits
        t["id"][s] = self.next_id + np.arange(len(pts)) if live else 0
        self.next_id += len(pts)
        return self


def call(name, table, dpose=None, **par):
    return {"name": name, "tracks": table.t if isinstance(table, Table) else table, "dpose": dpose, "params": params(**par)}


def straight(n_left, n_right, x0=2.0, step=3.0, half=1.5):
    k = np.arange(max(n_left, n_right))
    return (np.stack([x0 + step * k[:n_left], np.full(n_left, half)], axis=1), np.stack([x0 + step * k[:n_right], np.full(n_right, -half)], axis=1))


def spiral(n, spacing=1.0, r0=5.0, pitch=6.0):
    """n points every `spacing` metres along a spiral whose arms lie `pitch` metres apart, from (0, -r0) onwards, where it heads
    along +x: a chain with a step gate below `pitch` follows it and never leaves it."""
    th = np.linspace(-np.pi / 2, -np.pi / 2 + 2 * np.pi * 40, 400001)
    r = r0 + (th - th[0]) * pitch / (2 * np.pi)
    p = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    s = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(p, axis=0), axis=1))])
    assert s[-1] > spacing * n
    return p[np.searchsorted(s, spacing * np.arange(n))]


def run_twin(c):
    from unina_yolo_dla_amd import boundary
    return boundary.boundary_numpy(c["tracks"], None if c["dpose"] is None else c["dpose"]["pose"][0], c["params"])


def chain_length(points, **par):
    """How many of `points` ([m, 2], left class, in slot order) the left chain takes: the twin's own arithmetic."""
    h, _ = run_twin(call("probe", Table().add(points, LEFT), **par))
    return int(h["n_chain"][0][0])


def turn_bound(a, b, dx, **par):
    """The largest fp32 dy for which the chain o -> a -> b goes on to b + (dx, dy), found on the twin by bisection over the bit
    patterns of dy > 0 and checked at the bound: (dy one ulp inside, dy on the bound, dy one ulp beyond)."""
    def taken(dy):
        return chain_length([a, b, [F(b[0]) + F(dx), F(b[1]) + dy]], **par) == 3
    lo, hi = F(0.0).view(np.uint32), F(100.0).view(np.uint32)
    assert taken(F(0.0)) and not taken(F(100.0))
    while hi - lo > 1:
        mid = np.uint32((int(lo) + int(hi)) // 2)
        lo, hi = (mid, hi) if taken(mid.view(np.float32)) else (lo, mid)
    on = lo.view(np.float32)
    inside, beyond = np.nextafter(on, F(-INF)), np.nextafter(on, F(INF))
    assert taken(inside) and taken(on) and not taken(beyond)
    return inside, on, beyond


def yaw_result(yaw, tx, ty, pinhole=False):
    """A unina_pose_result whose pose stands at (tx, ty) and looks along `yaw`; pinhole: the camera frame is a pinhole camera's."""
    T = pc.yaw_pose(yaw, tx, ty, 0.5)
    return pc.prev_record(pc.compose(T, PINHOLE_TO_LEVEL) if pinhole else T)


def edge_cases():
    out = []
    up = float(np.nextafter(F(LIMIT), F(INF)))
    L8, R8 = straight(8, 8)
    # ---- table contents
    out.append(call("empty", Table()))
    out.append(call("left_only", Table().add(L8[:5], LEFT)))
    out.append(call("plain", Table().add(L8, LEFT).add(R8, RIGHT)))
    out.append(call("id0_with_coordinates", Table().add([[1.0, 1.5]], LEFT, live=False).add(L8[:4], LEFT).add(R8[:4], RIGHT)))
    out.append(call("hits_one_short", Table().add([[1.0, 1.5]], LEFT, hits=2).add(L8[:4], LEFT).add(R8[:4], RIGHT)))
    out.append(call("third_class", Table().add([[1.0, 1.5], [1.0, -1.5], [3.5, 0.0]], OTHER).add(L8[:4], LEFT).add([[6.5, 1.0]], OTHER)
                    .add(R8[:4], RIGHT)))
    out.append(call("non_finite", Table().add([[NAN, 1.5], [1.0, INF], [-INF, 1.5], [1.0, NAN], [INF, INF]], LEFT)
                    .add(np.concatenate([L8[:3], [[INF], [0.25], [-3e38]]], axis=1), LEFT).add(R8[:3], RIGHT)))
    rim = [[LIMIT, 1.0], [-LIMIT, 2.0], [3.0, LIMIT], [4.0, -LIMIT]]
    out.append(call("limit_inside", Table().add(rim, LEFT).add(L8[:2], LEFT)))
    out.append(call("limit_beyond", Table().add([[up, 1.0], [-up, 2.0], [3.0, up], [4.0, -up]], LEFT).add(L8[:2], LEFT)))
    out.append(call("limit_chained", Table().add([[32764.0, 1.5], [LIMIT, 1.5], [up, 1.5]], LEFT), pose=pc.yaw_pose(0.0, 32761.0, 0.0)))
    # ---- the first link
    g1 = 8.0
    out.append(call("first_gate_exact", Table().add([[g1, 0.0]], LEFT), first_gate=g1))
    out.append(call("first_gate_one_ulp_beyond", Table().add([[g1, tc.one_ulp_offset(g1)]], LEFT), first_gate=g1))
    out.append(call("abeam", Table().add([[0.0, 2.0]], LEFT).add([[0.0, -2.0]], RIGHT)))
    out.append(call("behind", Table().add([[-1.0, 1.5], [3.0, 1.5]], LEFT).add([[-0.5, -1.5]], RIGHT)))
    # ---- later links
    gs = 4.0
    out.append(call("step_gate_exact", Table().add([[2.0, 0.0], [2.0 + gs, 0.0]], LEFT), step_gate=gs))
    out.append(call("step_gate_one_ulp_beyond", Table().add([[2.0, 0.0], [2.0 + gs, tc.one_ulp_offset(gs)]], LEFT), step_gate=gs))
    a, b, dx = [2.0, 0.0], [5.0, 1.0], 0.5
    for name, dy in zip(("turn_one_ulp_inside", "turn_on_bound", "turn_one_ulp_beyond"), cached("turn", lambda: turn_bound(a, b, dx))):
        out.append(call(name, Table().add([a, b, [F(b[0]) + F(dx), F(b[1]) + dy]], LEFT)))
    out.append(call("second_track_at_the_same_place", Table().add([[2.0, 1.5], [2.0, 1.5], [5.0, 1.5]], LEFT)))
    ang = np.deg2rad(10.0 + 45.0 * np.arange(8))
    out.append(call("ring8", Table().add(np.stack([4.0 + 3.0 * np.cos(ang), 3.0 * np.sin(ang)], axis=1), LEFT)))
    # ---- ties: the lower slot wins, and the two lie in different waves
    out.append(call("tie_slots_5_and_1000", Table().add([[3.0, 2.0], [3.0, -2.0]], LEFT, slots=[5, 1000])))
    out.append(call("tie_slots_swapped", Table().add([[3.0, -2.0], [3.0, 2.0]], LEFT, slots=[5, 1000])))
    # ---- chain length
    out.append(call("max_chain_1", Table().add(L8, LEFT).add(R8, RIGHT), max_chain=1))
    rng = np.random.RandomState(21)
    for n in (63, 64, 65):
        l, r = straight(n, 64 if n == 64 else 3)
        slots = rng.permutation(MAXD)[:len(l) + len(r)]
        out.append(call(f"line{n}", Table().add(l, LEFT, slots=slots[:len(l)]).add(r, RIGHT, slots=slots[len(l):])))
    out.append(call("all_1024_of_one_class", Table().add(spiral(MAXD), LEFT, slots=rng.permutation(MAXD)), step_gate=3.0,
                    pose=pc.yaw_pose(0.0, -1.0, -5.0)))
    # ---- the ladder
    l, r = straight(1, 64)
    out.append(call("ladder_1_and_64", Table().add(l, LEFT).add(r, RIGHT)))
    wg = 6.0
    out.append(call("width_gate_exact", Table().add([[0.0, 3.0]], LEFT).add([[0.0, -3.0]], RIGHT), width_gate=wg))
    out.append(call("width_gate_one_ulp_beyond", Table().add([[tc.one_ulp_offset(wg), 3.0]], LEFT).add([[0.0, -3.0]], RIGHT), width_gate=wg))
    out.append(call("advance_tie", Table().add(L8[:2], LEFT).add(R8[:2], RIGHT)))
    # ---- the pose
    out.append(call("no_heading_from_forward", Table().add(L8, LEFT).add(R8, RIGHT), forward=(0.0, 0.0, 1.0)))
    bad = yaw_result(0.3, 1.0, 2.0)
    bad["pose"][0][3] = NAN
    out.append(call("no_heading_from_a_nan_device_pose", Table().add(L8, LEFT).add(R8, RIGHT), dpose=bad))
    T = pc.yaw_pose(np.pi / 2, 10.0, -1.0)
    world = lambda pts: (np.concatenate([pts, np.zeros((len(pts), 1))], axis=1) @ T[:, :3].T + T[:, 3])[:, :2]   # noqa: E731
    out.append(call("device_pose_beside_another_pose", Table().add(world(L8), LEFT).add(world(R8), RIGHT), dpose=yaw_result(np.pi / 2, 10.0, -1.0, True),
                    forward=(0.0, 0.0, 1.0), pose=pc.compose(pc.yaw_pose(-0.4, 3.0, 3.0), PINHOLE_TO_LEVEL)))
    return out


# ---------------------------------------------------------------- the oval
OVAL_PAR = dict(first_gate=8.0, step_gate=7.4, cos_turn=float(np.cos(np.deg2rad(70.0))), width_gate=6.0)


def oval_line(a=30.0, b=15.0, n=200000):
    """The centre line, counter-clockwise, sampled densely: (arc length [n], point [n, 2], unit tangent [n, 2], the lap's length)."""
    t = np.linspace(0.0, 2 * np.pi, n + 1)
    p = np.stack([a * np.cos(t), b * np.sin(t)], axis=1)
    s = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(p, axis=0), axis=1))])
    tan = np.stack([-a * np.sin(t), b * np.cos(t)], axis=1)
    return s, p, tan / np.linalg.norm(tan, axis=1)[:, None], s[-1]


def oval_at(line, arc):
    """(points, tangents) of the centre line at the arc lengths `arc`."""
    s, p, tan, lap = line
    i = np.searchsorted(s, np.mod(arc, lap))
    return p[i], tan[i]


def oval_cones(line, spacing=4.0, half=1.5, even=True):
    """(left [m, 2], right [m, 2]): a cone every `spacing` of centre-line arc -- floor(lap / spacing) of them --, `half` to either
    side; the left of a counter-clockwise lap is the inside. even: the cones share the lap evenly (145.3 m / 36 = 4.04 m), as a
    track is laid out; else they stand at exact multiples of `spacing` and the lap closes with one longer gap (5.3 m)."""
    n = int(line[3] // spacing)
    c, t = oval_at(line, (line[3] / n if even else spacing) * np.arange(n))
    normal = np.stack([-t[:, 1], t[:, 0]], axis=1)
    return c + half * normal, c - half * normal


def oval_case(seed, start, a=30.0, b=15.0, half=1.5, spacing=4.0, noise=0.05, step_gate=None, even=True):
    """The oval's table in random slot order with 20 tracks of a third class among it, the vehicle on the centre line a fraction
    `start` of a lap on, heading along it. ids: left ring position r -> 1 + r, right -> 1001 + r. Returns (call, n per side)."""
    line = cached(("line", a, b), lambda: oval_line(a, b))
    left, right = oval_cones(line, spacing, half, even)
    n = len(left)
    rng = np.random.RandomState(seed)
    pts = np.concatenate([left, right]) + rng.normal(0.0, noise, (2 * n, 2))
    other = np.stack([rng.uniform(-a - 5, a + 5, 20), rng.uniform(-b - 5, b + 5, 20)], axis=1)
    slots = rng.permutation(MAXD)[:2 * n + 20]
    tab = Table().add(pts[:n], LEFT, slots=slots[:n])
    tab.next_id = 1001
    tab.add(pts[n:], RIGHT, slots=slots[n:2 * n])
    tab.next_id = 2001
    tab.add(other, OTHER, slots=slots[2 * n:])
    o, t = oval_at(line, np.array([start * line[3]]))
    pose = pc.yaw_pose(np.arctan2(t[0, 1], t[0, 0]), o[0, 0], o[0, 1], 0.5)
    par = dict(OVAL_PAR, pose=pose)
    if step_gate is not None:
        par["step_gate"] = step_gate
    return call(f"oval_seed{seed}_start{start:.2f}", tab, **par), n


def ring_steps(refs, base, n):
    """The ring positions of a chain's refs, as steps from each to the next modulo n: all 1 for a chain in ring order in the
    direction of travel."""
    r = np.asarray(refs) - base
    assert ((r >= 0) & (r < n)).all(), refs
    return np.mod(np.diff(r), n)


def centre_distance(line, pts):
    """Distance of each point [m, 2] to the centre line (its dense sampling, every 2000th of a lap's 200000 samples refined)."""
    p = line[1][::20]
    return np.array([np.sqrt(((p - q) ** 2).sum(axis=1).min()) for q in pts])


def permuted(c, seed=9):
    """The same call with its slots in another order."""
    order = np.random.RandomState(seed).permutation(MAXD)
    return dict(c, tracks=c["tracks"][order], name=c["name"] + "_permuted")


# ---------------------------------------------------------------- the drive: pose -> tracker -> boundary
DRIVE_TRACK = dict(gate=0.5, alpha=0.5, birth_confidence=0.3, class_aware=1, confirm_hits=3, max_missed=3)
DRIVE_POSE = dict(gate=1.0, class_aware=1, min_hits=3, iterations=4, min_pairs=3)
DRIVE_BOUNDARY = dict(OVAL_PAR, forward=LEVEL, min_hits=3)


def drive_inputs(seed=3, n_frames=12, step=1.0, see=20.0, noise=0.02):
    """A vehicle driving the oval's centre line, `step` metres a frame: per frame the records of the cones within `see` metres
    (level camera frame, x forward) with `noise` metres of noise, in random order, and the odometry: the true pose for frame 0, then
    the true increment camera f -> camera f - 1. Returns (frames of tc.frame, increments, true poses, n per side)."""
    line = cached(("line", 30.0, 15.0), oval_line)
    left, right = oval_cones(line)
    n = len(left)
    world = np.concatenate([np.concatenate([left, right]), np.zeros((2 * n, 1))], axis=1)
    cls = np.array([LEFT] * n + [RIGHT] * n)
    rng = np.random.RandomState(seed)
    frames, incs, truth = [], [], []
    for f in range(n_frames):
        o, t = oval_at(line, np.array([step * f]))
        T = pc.yaw_pose(np.arctan2(t[0, 1], t[0, 0]), o[0, 0], o[0, 1], 0.5)
        seen = np.nonzero(np.linalg.norm(world[:, :2] - o[0], axis=1) < see)[0]
        order = rng.permutation(len(seen))
        cam = pc.seen_from(world[seen], T) + rng.normal(0.0, noise, (len(seen), 3))
        frames.append(tc.frame(cam[order], cls=cls[seen][order], **DRIVE_TRACK))
        incs.append(T if f == 0 else pc.compose(pc.inverse(truth[-1]), T))
        truth.append(T)
    return frames, incs, truth, n


def run_drive_twin(seed=3):
    """The three twins chained as the device chains the calls: pose (the earlier result chained, cones moved) -> tracker with the
    identity -> boundary with the pose stage's result. Returns per frame (pose_numpy's dict, tracker state, (header, points))."""
    from unina_yolo_dla_amd import boundary, pose, tracking
    frames, incs, _, _ = drive_inputs(seed)
    state, prev, out = tracking.new_state(), None, []
    for f, inc in zip(frames, incs):
        dets, cones = pc.padded_frame(f)
        r = pose.pose_numpy(dets, f["count"], cones, state["tracks"], prev, dict(DRIVE_POSE, inc=inc))
        prev = r["result"]
        state, _ = tracking.update_numpy(state, dets, f["count"], r["cones"], dict(f["params"], pose=None))
        out.append((r, state, boundary.boundary_numpy(state["tracks"], r["result"]["pose"][0], DRIVE_BOUNDARY)))
    return out


_cache = {}


def cached(key, build):
    """Cases and their twin results are built once per process and shared, unchanged, by every test."""
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def edge_results():
    return cached("edges", lambda: [(c, run_twin(c)) for c in edge_cases()])


def oval_result(seed, start):
    def build():
        c, n = oval_case(seed, start)
        return c, run_twin(c), n
    return cached(("oval", seed, start), build)


def drive_results(seed=3):
    return cached(("drive", seed), lambda: run_drive_twin(seed))
