"""Inputs shared by tests/test_pose_cpu.py and tests/test_gpu_pose.py: the named calls of unina_pose_async (include/unina_mi355.h
"pose from the tracked cones") and the world sequence with a biased odometry. A case is one call: the records and their cones (all
1024 of each, NaN bit patterns behind the records, as the GPU tests upload them), the count word, the tracker's 1024 slots, the
earlier result or None, and the parameters. Pure numpy; nothing here touches the device."""
import numpy as np

import track_cases as tc
from records import padded_words
from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DET_DTYPE

MAXD = 1024
F = np.float32
NAN, INF = float("nan"), float("inf")
LIMIT = 32768.0


def params(**kw):
    p = dict(inc=None, gate=1.0, class_aware=1, min_hits=3, iterations=4, min_pairs=3)
    p.update(kw)
    return p


def table(points, cls=0, hits=5, slots=None):
    """The tracker's 1024 slots with a track at each of `points` ([m, 3]), in `slots` (default: the first m), ids from 1."""
    from unina_yolo_dla_amd.tracking import TRACK_DTYPE
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    tr = np.zeros(MAXD, dtype=TRACK_DTYPE)
    s = np.arange(len(pts)) if slots is None else np.asarray(slots)
    tr["x"][s], tr["y"][s], tr["z"][s] = pts.T
    tr["confidence"][s], tr["id"][s], tr["class_id"][s], tr["hits"][s] = 0.9, 1 + np.arange(len(pts)), cls, hits
    return tr


def prev_record(pose, corr=(1, 0, 0, 0)):
    from unina_yolo_dla_amd.engine import POSE_RESULT_DTYPE
    r = np.zeros(1, dtype=POSE_RESULT_DTYPE)
    r["pose"][0] = np.asarray(pose, dtype=np.float32).reshape(12)
    r["c"], r["s"], r["tx"], r["ty"] = corr
    return r


def call(name, points, tracks, cls=0, valid=1, count=None, prev=None, **par):
    """points: [m, 3] camera-frame positions -> one call; cls / valid broadcast over the records."""
    f = tc.frame(points, cls=cls, valid=valid, count=count)
    return {"name": name, "dets": padded_words(f["dets"], 8 * MAXD).view(DET_DTYPE), "cones": padded_words(f["cones"], 8 * MAXD).view(CONE3D_DTYPE),
            "count": f["count"], "tracks": tracks, "prev": prev, "params": params(**par)}


def yaw_pose(yaw, tx=0.0, ty=0.0, tz=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0, tx], [s, c, 0, ty], [0, 0, 1, tz]])


def inverse(T):
    R, t = T[:, :3], T[:, 3]
    return np.concatenate([R.T, (-R.T @ t)[:, None]], axis=1)


def compose(A, B):
    return np.concatenate([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]], axis=1)


def seen_from(world, T):
    """World points as the camera at pose T (camera -> world) sees them."""
    return (np.asarray(world, dtype=np.float64) - T[:, 3]) @ T[:, :3]


def field(n, seed, half=20.0):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.uniform(-half, half, (n, 2)), rng.uniform(0.0, 0.3, (n, 1))], axis=1)


def fixed_point_edge():
    """1024 landmarks of one class in four 16 x 16 grids of 1 m at the corners of the field, |y| up to 32768 m exactly, |x| up to
    32767 m; the records lie 0.125 m beside them in x."""
    i = np.arange(256)
    gx, gy = 32767.0 - (i % 16), 32768.0 - (i // 16)
    world = np.concatenate([np.stack([sx * gx, sy * gy, np.zeros(256)], axis=1) for sx in (1, -1) for sy in (1, -1)])
    return world, world + np.array([0.125, 0.0, 0.0])


def edge_cases():
    out = []
    w = field(40, 1)
    rng = np.random.RandomState(2)
    truth = yaw_pose(0.3, 2.0, -1.0, 0.5)
    drift = compose(truth, yaw_pose(0.01, 0.2, -0.15))                      # the prior: the truth, wrong by 0.01 rad and 0.25 m
    cam = seen_from(w, truth)
    cls40 = rng.randint(0, 4, 40)
    # counts
    out.append(call("empty_count0", cam[:0], table(w[:0]), inc=drift))
    out.append(call("empty_table", cam, table(w[:0]), cls=cls40, inc=drift))
    out.append(call("count0", cam, table(w, cls40), cls=cls40, count=0, inc=drift))
    out.append(call("count1025", cam, table(w, cls40), cls=cls40, count=1025, inc=drift))
    out.append(call("count_neg1", cam, table(w, cls40), cls=cls40, count=-1, inc=drift))
    # a plain call, also behind an earlier result, class-aware and class-blind
    out.append(call("plain", cam, table(w, cls40), cls=cls40, inc=drift))
    out.append(call("plain_prev", cam, table(w, cls40), cls=cls40, prev=prev_record(drift, (0.9, 0.1, 3, 4)), inc=yaw_pose(0.004, 0.05, 0.0),
                    iterations=8))
    out.append(call("class_blind", cam, table(w, cls40), cls=(cls40 + 1) % 4, inc=drift, class_aware=0))
    out.append(call("class_aware_no_match", cam, table(w, cls40), cls=(cls40 + 1) % 4, inc=drift))
    out.append(call("one_iteration", cam, table(w, cls40), cls=cls40, inc=drift, iterations=1))
    # exactly min_pairs pairs and one fewer: four cones near their landmarks, the others far from every landmark
    few = np.concatenate([w[:4] + [0.1, -0.05, 0.0], w[4:12] + [0.0, 0.0, 30.0]])
    out.append(call("pairs_equal_min", few, table(w), min_pairs=4))
    out.append(call("pairs_below_min", few, table(w), min_pairs=5))
    # three pairs in iteration 1; its correction carries the third record, 0.95 m above its landmark, out of the gate
    tri = np.array([[0.0, 0, 0], [10, 0, 0], [5, 5, 0]])
    out.append(call("too_few_at_iteration_2", tri + [[0.9, 0, 0], [0.9, 0, 0], [0, 0, 0.95]], table(tri)))
    # two pairs at one point of the plane, told apart by their height
    two = np.array([[3.0, 4.0, 0.0], [3.0, 4.0, 5.0]])
    out.append(call("degenerate", two - [0.25, 0.125, 0.0], table(two), min_pairs=2))
    # half a turn: one candidate per record by its class
    tri2 = np.array([[0.25, 0.0, 0.0], [-0.125, 0.25, 0.0], [-0.125, -0.25, 0.0]])
    out.append(call("half_turn", -tri2 * [1, 1, 0], table(tri2, cls=[0, 1, 2]), cls=[0, 1, 2]))
    # two records nearest to one landmark, beside three plain pairs
    base = np.array([[0.0, 0, 0], [8, 0, 0], [0, 8, 0], [8, 8, 0]])
    out.append(call("two_records_one_landmark", np.concatenate([base[:3] + [0.1, 0, 0], [[8.25, 8, 0], [7.5, 8, 0]]]), table(base)))
    # equal d2: a record between two landmarks, a landmark between two records; the index decides
    tie_lm = np.array([[0.0, 0, 0], [1, 0, 0], [20, 0, 0], [0, 20, 0], [20, 20, 0], [10, 10, 0]])
    tie_rec = np.array([[0.5, 0, 0], [20, 0, 0], [0, 20, 0], [20, 20, 0], [10.25, 10, 0], [9.75, 10, 0]])
    out.append(call("ties", tie_rec, table(tie_lm), iterations=1))
    out.append(call("ties_slots_swapped", tie_rec[[0, 1, 2, 3, 5, 4]], table(tie_lm[[1, 0, 2, 3, 4, 5]]), iterations=1))
    # a distance equal to gate * gate and one ulp above, beside two exact pairs
    gate = 0.6
    dy = tc.one_ulp_offset(gate)
    anchor = np.array([[0.0, 0, 0], [16, 0, 0], [0, 16, 0]])
    out.append(call("gate_exact", anchor + [[gate, 0, 0], [0, 0, 0], [0, 0, 0]], table(anchor), gate=gate, iterations=1))
    out.append(call("gate_one_ulp_above", anchor + [[gate, dy, 0], [0, 0, 0], [0, 0, 0]], table(anchor), gate=gate, iterations=1))
    # a slot one hit short, a free slot in the middle of the table, landmarks spread over the waves
    hits = np.full(40, 5)
    hits[:10] = 2
    out.append(call("hits_one_short", cam, table(w, cls40, hits=hits), cls=cls40, inc=drift))
    out.append(call("slots_across_waves", cam, table(w, cls40, slots=np.arange(40) * 25 + 7), cls=cls40, inc=drift))
    # cones that are not usable
    bad = cam.copy()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0] = NAN, INF, -INF, 3e38
    valid = np.ones(40, dtype=np.int32)
    valid[4:8] = 0
    out.append(call("non_finite_and_invalid", bad, table(w, cls40), cls=cls40, valid=valid, inc=drift))
    nan_lm = table(w, cls40)
    nan_lm["x"][0], nan_lm["y"][1], nan_lm["z"][2] = NAN, INF, NAN
    out.append(call("non_finite_landmarks", cam, nan_lm, cls=cls40, inc=drift))
    # the field's limit: a point and a landmark at 32768 m vote, just beyond they do not
    up = float(np.nextafter(F(LIMIT), F(INF)))
    rim = np.array([[LIMIT, 0.0, 0], [-LIMIT, 100.0, 0], [0.0, LIMIT, 0], [100.0, -LIMIT, 0], [0, 0, 0]])
    out.append(call("limit_inside", rim, table(rim), min_pairs=5, iterations=2))
    out.append(call("limit_point_beyond", rim * [[up / LIMIT, 1, 1], [1, 1, 1], [1, up / LIMIT, 1], [1, 1, 1], [1, 1, 1]], table(rim), iterations=2))
    out.append(call("limit_landmark_beyond", rim, table(rim * [[1, 1, 1], [up / LIMIT, 1, 1], [1, 1, 1], [1, up / LIMIT, 1], [1, 1, 1]]), iterations=2))
    lm, rec = fixed_point_edge()
    out.append(call("fixed_point_edge", rec, table(lm), gate=0.4, iterations=2))
    return out


def exact_motion(seed=3):
    """40 cones within 30 m seen without noise; the prior is wrong by an exact planar motion (0.02 rad, 0.3 m). Returns the call
    and the true pose."""
    rng = np.random.RandomState(seed)
    ang, rad = rng.uniform(0, 2 * np.pi, 40), rng.uniform(5, 30, 40)
    truth = yaw_pose(0.7, 3.0, -2.0, 1.0)
    w = np.stack([truth[0, 3] + rad * np.cos(ang), truth[1, 3] + rad * np.sin(ang), np.zeros(40)], axis=1)
    prior = compose(yaw_pose(-0.02, 0.25, -0.17), truth)
    return call("exact_motion", seen_from(w, truth), table(w), inc=prior, gate=1.5), truth


def permuted(c, seed=9):
    """The same call with its records in another order."""
    n = c["count"]
    order = np.random.RandomState(seed).permutation(n)
    d = dict(c, dets=c["dets"].copy(), cones=c["cones"].copy(), name=c["name"] + "_permuted")
    d["dets"][:n], d["cones"][:n] = c["dets"][order], c["cones"][order]
    return d, order


def canon_cones(cones, n=MAXD):
    """A copy whose NaN coordinates in the first n records all carry one bit pattern: the sign and payload of a NaN that an
    operation produced are the processor's (the header says so), everything else is compared byte for byte."""
    out = np.array(cones, dtype=CONE3D_DTYPE)
    for axis in "xyz":
        v = out[axis][:n]
        v.view(np.uint32)[np.isnan(v)] = 0x7fc00000
    return out


def run_twin(c):
    from unina_yolo_dla_amd import pose
    return pose.pose_numpy(c["dets"], c["count"], c["cones"], c["tracks"], c["prev"], c["params"])


# ---------------------------------------------------------------- the world sequence with a biased odometry
YAW_BIAS, STEP_BIAS = 0.004, 0.05            # per frame: radians, metres along the camera's x


def world_chain_inputs(seed):
    """tc.world_sequence(1, seed=seed) and per frame the odometry a drifting source would give: the true pose for frame 0, then the
    increment camera f -> camera f - 1 with YAW_BIAS and STEP_BIAS added. Returns (frames, true poses, increments)."""
    c = tc.world_sequence(1, seed=seed)
    truth = [np.asarray(f["params"]["pose"], dtype=np.float64).reshape(3, 4) for f in c["frames"]]
    incs = [truth[0]]
    for k in range(1, len(truth)):
        incs.append(compose(compose(inverse(truth[k - 1]), truth[k]), yaw_pose(YAW_BIAS, STEP_BIAS, 0.0)))
    return c["frames"], truth, incs


POSE_PAR = dict(gate=1.0, class_aware=1, min_hits=3, iterations=4, min_pairs=3)


def padded_frame(f):
    return padded_words(f["dets"], 8 * MAXD).view(DET_DTYPE), padded_words(f["cones"], 8 * MAXD).view(CONE3D_DTYPE)


def run_chain_twin(seed, with_stage=True):
    """Pose stage (prev chained) -> tracker with the identity, frame by frame. Returns [(pose_numpy's dict or None, tracker state,
    assign, the pose handed on as 12 float64)]. Without the stage the composed odometry goes to the tracker as it is."""
    from unina_yolo_dla_amd import pose, tracking
    frames, _, incs = world_chain_inputs(seed)
    state, prev, out, dead = tracking.new_state(), None, [], None
    for f, inc in zip(frames, incs):
        dets, cones = padded_frame(f)
        tp = dict(f["params"], pose=None)
        if with_stage:
            r = pose.pose_numpy(dets, f["count"], cones, state["tracks"], prev, dict(POSE_PAR, inc=inc))
            prev = r["result"]
            state, assign = tracking.update_numpy(state, dets, f["count"], r["cones"], tp)
            out.append((r, state, assign, r["result"]["pose"][0].astype(np.float64)))
        else:
            dead = inc if dead is None else compose(dead, inc)
            state, assign = tracking.update_numpy(state, dets, f["count"], cones, dict(tp, pose=dead))
            out.append((None, state, assign, dead.reshape(12)))
    return out


def pose_error(pose12, truth):
    """(position error in the plane, |yaw error|) of a 12-value pose against a true [3, 4] pose."""
    p = np.asarray(pose12, dtype=np.float64).reshape(3, 4)
    d = np.arctan2(p[1, 0], p[0, 0]) - np.arctan2(truth[1, 0], truth[0, 0])
    return float(np.hypot(*(p[:2, 3] - truth[:2, 3]))), float(abs((d + np.pi) % (2 * np.pi) - np.pi))


_cache = {}


def cached(key, build):
    """Cases and their twin results are built once per process and shared, unchanged, by every test."""
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def edge_results():
    return cached("edges", lambda: [(c, run_twin(c)) for c in edge_cases()])


def chain_results(seed):
    return cached(("chain", seed), lambda: run_chain_twin(seed))
