"""Inputs shared by tests/test_track_cpu.py and tests/test_gpu_track.py: the named sequences of unina_track_update_async
(include/unina_mi355.h "tracking"). A case is a list of frames run from a reset table; a frame is the records, their points,
the count word and the parameters of one update. Pure numpy; nothing here touches the device."""
import numpy as np

from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DET_DTYPE

MAXD = 1024
F = np.float32
NAN, INF = float("nan"), float("inf")


def params(**kw):
    p = dict(pose=None, gate=0.5, alpha=0.5, birth_confidence=0.3, class_aware=1, confirm_hits=2, max_missed=2)
    p.update(kw)
    return p


def frame(points, cls=0, conf=0.9, valid=1, count=None, **par):
    """points: [m, 3] camera-frame positions (m <= 1024) -> one update. cls / conf / valid broadcast over the records."""
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    m = len(pts)
    dets = np.zeros(m, dtype=DET_DTYPE)
    dets["x1"], dets["y1"], dets["x2"], dets["y2"] = 10, 20, 30, 40
    dets["confidence"], dets["class_id"], dets["valid"] = conf, cls, 1
    cones = np.zeros(m, dtype=CONE3D_DTYPE)
    cones["x"], cones["y"], cones["z"] = pts.T
    cones["u"], cones["v"], cones["n_valid"], cones["n_samples"], cones["valid"] = 20, 30, 5, 9, valid
    return {"dets": dets, "cones": cones, "count": m if count is None else count, "params": params(**par)}


def case(name, *frames):
    return {"name": name, "frames": list(frames)}


def grid(n, step=1.0, z=5.0, cols=32):
    i = np.arange(n)
    return np.stack([(i % cols) * step, (i // cols) * step, np.full(n, z)], axis=1).astype(np.float32)


def chain(n=64):
    """Tracks and records alternating on a line, every gap 0.003 m shorter than the one before, from 0.5 m: each record's
    nearest track and each track's nearest record is its RIGHT neighbour, so only the last pair is mutual and the matching
    takes n rounds. Returns (track points, record points)."""
    gaps = 0.5 - 0.003 * np.arange(2 * n - 1)
    pos = np.concatenate([[0.0], np.cumsum(gaps)])
    line = np.zeros((2 * n, 3))
    line[:, 0] = pos
    line[:, 2] = 4.0
    return line[0::2].astype(np.float32), line[1::2].astype(np.float32)


def one_ulp_offset(gate):
    """dy with (gate * gate + dy * dy) == nextafter(gate * gate) in fp32."""
    g2 = F(gate) * F(gate)
    up = np.nextafter(g2, F(np.inf), dtype=np.float32)
    dy = F(np.sqrt(np.float64(up) - np.float64(g2)))
    assert g2 + dy * dy == up
    return dy


def edge_cases():
    g = grid(1024)
    rng = np.random.RandomState(11)
    jitter = rng.uniform(-0.1, 0.1, (1024, 3)).astype(np.float32)
    out = []
    # counts: 100 tracks, then the first `count` of 1024 records (the first 100 near the tracks, the others found new tracks)
    for c in (0, 1, 63, 64, 65, 1024, 5000, -7):
        out.append(case(f"count{c}", frame(g[:100]), frame(g + F(0.02), count=c), frame(g + F(0.04), count=c)))
    out.append(case("all_invalid", frame(g[:10]), frame(g[:10], valid=0), frame(g[:10] + F(0.01))))
    bad = (g[:8] + F(0.01)).copy()
    bad[0, 0], bad[1, 1], bad[2, 2] = NAN, INF, -INF
    over = g[:8].copy()
    over[:4, 0] = 3e38
    out.append(case("non_finite", frame(g[:8]), frame(bad), frame(over, pose=[1, 0, 0, 3e38, 0, 1, 0, 0, 0, 0, 1, 0]), frame(g[:8])))
    out.append(case("nan_confidence", frame(g[:4]), frame(g[:6] + F(0.01), conf=[NAN, 0.9, NAN, 0.9, NAN, 0.9])))
    out.append(case("empty_table", frame(g[:20], birth_confidence=2.0), frame(g[:0]), frame(g[:20], conf=np.linspace(0.1, 0.9, 20))))
    wide = rng.uniform(-0.5, 0.5, (1024, 3)).astype(np.float32) * np.array([1, 1, 0], dtype=np.float32)
    out.append(case("full_table", frame(g, gate=1.2), frame(g + wide, gate=1.2), frame(g - wide, gate=1.2, class_aware=0)))
    far = grid(24, step=3.0, z=90.0)
    extra = np.concatenate([g[:1000] + F(0.02), far])
    out.append(case("full_table_extra_births", frame(g), frame(extra), frame(extra, max_missed=0), frame(extra)))
    out.append(case("death_birth_reuse", frame(g[:5], max_missed=0),
                    frame(np.concatenate([g[[0, 1, 3, 4]] + F(0.01), [[50, 50, 5]]]), max_missed=0)))
    out.append(case("coast_then_die", frame(g[:3]), frame(g[:0]), frame(g[:0]), frame(g[:0]), frame(g[:3])))
    for a in (1.0, 0.25):
        out.append(case(f"alpha{a}", frame(g[:50], alpha=a), frame(g[:50] + jitter[:50], alpha=a), frame(g[:50] - jitter[:50], alpha=a),
                        frame(g[:50] + jitter[50:100], alpha=a)))
    gate = 0.6
    dy = one_ulp_offset(gate)
    out.append(case("gate_exact", frame([[0, 0, 0]], gate=gate), frame([[gate, 0, 0]], gate=gate)))
    out.append(case("gate_one_ulp_above", frame([[0, 0, 0]], gate=gate), frame([[gate, dy, 0]], gate=gate)))
    two = [[1, 1, 1], [1, 1, 1]]
    near = [[1.01, 1, 1], [1.01, 1, 1]]
    out.append(case("class_aware_pair", frame(two, cls=[0, 1]), frame(near, cls=[1, 0])))
    out.append(case("class_blind_pair", frame(two, cls=[0, 1], class_aware=0), frame(near, cls=[1, 0], class_aware=0)))
    q = grid(64, step=0.25, cols=8)
    out.append(case("grid_ties", frame(q, gate=0.2), frame(q + np.array([0.125, 0.125, 0], dtype=np.float32), gate=0.2),
                    frame(q + np.array([0.125, 0, 0], dtype=np.float32), gate=0.2, class_aware=0)))
    out.append(case("one_record_two_slots", frame([[0, 0, 2], [1, 0, 2]], gate=0.6), frame([[0.5, 0, 2]], gate=0.6)))
    out.append(case("two_records_one_slot", frame([[0, 0, 2]], gate=0.6), frame([[0.5, 0, 2], [-0.5, 0, 2]], gate=0.6)))
    tr, re = chain(64)
    out.append(case("chain64", frame(tr, gate=0.6), frame(re, gate=0.6)))
    fill = grid(32, step=2.0, z=60.0)
    out.append(case("chain64_across_waves", frame(np.concatenate([fill, tr]), gate=0.6),
                    frame(np.concatenate([fill + F(0.01), re]), gate=0.6)))
    return out


def world_sequence(class_aware, n_frames=40, seed=5):
    """150 cones on a 60 m x 60 m field seen from a moving, rotating camera (those within 30 m), 2 cm noise, 15 % dropouts,
    10 false positives per frame; the pose is handed to the tracker as odometry would give it."""
    rng = np.random.RandomState(seed)
    cones = np.concatenate([rng.uniform(-30, 30, (150, 2)), np.zeros((150, 1))], axis=1)
    classes = rng.randint(0, 4, 150)
    frames = []
    for f in range(n_frames):
        yaw = 0.04 * f
        c, s = np.cos(yaw), np.sin(yaw)
        R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        t = np.array([-10 + 0.5 * f, -5 + 0.2 * f, 1.0])
        seen = np.nonzero((np.linalg.norm(cones - t, axis=1) < 30) & (rng.rand(150) > 0.15))[0]
        cam = (cones[seen] - t) @ R + rng.normal(0, 0.02, (len(seen), 3))          # R^T (w - t), row vectors
        false = rng.uniform(-25, 25, (10, 3))
        pts = np.concatenate([cam, false])
        cls = np.concatenate([classes[seen], rng.randint(0, 4, 10)])
        conf = np.concatenate([rng.uniform(0.5, 0.95, len(seen)), rng.uniform(0.3, 0.6, 10)])
        order = rng.permutation(len(pts))
        frames.append(frame(pts[order], cls=cls[order], conf=conf[order], pose=np.concatenate([R, t[:, None]], axis=1),
                            class_aware=class_aware, confirm_hits=3, max_missed=3))
    return case(f"world_class_aware{class_aware}", *frames)


def run_twin(c):
    """[(state, assign)] after each frame of the case, from a reset table."""
    from unina_yolo_dla_amd import tracking
    state, out = tracking.new_state(), []
    for f in c["frames"]:
        state, assign = tracking.update_numpy(state, f["dets"], f["count"], f["cones"], f["params"])
        out.append((state, assign))
    return out


_cache = {}


def cached(key, build):
    """Cases and their twin results are built once per process and shared, unchanged, by every test."""
    if key not in _cache:
        cases = build()
        cases = cases if isinstance(cases, list) else [cases]
        _cache[key] = [(c, run_twin(c)) for c in cases]
    return _cache[key]
