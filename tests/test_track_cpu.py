"""unina_track_update_async without a GPU: tracking.update_numpy (the definition) against an independent brute-force greedy and
against the rounds of mutual nearest neighbours csrc/track.hip computes, csrc/track_math.h compiled for the host
(tests/track_math_host.cpp, also under -fsanitize=address,undefined as the stand-alone program it is) against the numpy twin,
the argument checks of the entry point, the layouts in C, and what each constructed case of tests/track_cases.py contains."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import hostprog
import track_cases as tc

F = np.float32
INT_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------- independent restatements of one update
def gated_pairs(state, f):
    """Every candidate pair of the update as python tuples (d2, s, j), and the usable records' points: scalar loops, no
    vectorised arithmetic, python floats rounded to fp32 after every operation (a double holds the sum, difference or product of two fp32 values
    closely enough that rounding it to fp32 is the fp32 operation)."""
    p, dets, cones, tr = f["params"], f["dets"], f["cones"], state["tracks"]
    pose = [F(v) for v in np.asarray(np.eye(3, 4) if p["pose"] is None else p["pose"], dtype=np.float64).reshape(-1)]
    n = min(max(f["count"], 0), tc.MAXD, len(dets))
    g2 = F(p["gate"]) * F(p["gate"])
    pts, pairs = {}, []
    live = [s for s in range(tc.MAXD) if tr["id"][s] != 0]
    with np.errstate(all="ignore"):
        for j in range(n):
            x, y, z = cones["x"][j], cones["y"][j], cones["z"][j]
            q = [((pose[4 * r] * x + pose[4 * r + 1] * y) + pose[4 * r + 2] * z) + pose[4 * r + 3] for r in range(3)]
            if cones["valid"][j] != 0 and all(math.isfinite(v) for v in q):
                pts[j] = q
        tx, ty, tz, tcls = tr["x"].tolist(), tr["y"].tolist(), tr["z"].tolist(), tr["class_id"].tolist()
        rcls = dets["class_id"].tolist()
        for j, q in pts.items():
            qx, qy, qz = (float(v) for v in q)
            for s in live:
                if p["class_aware"] and tcls[s] != rcls[j]:
                    continue
                dx, dy, dz = float(F(qx - tx[s])), float(F(qy - ty[s])), float(F(qz - tz[s]))
                d2 = float(F(float(F(float(F(dx * dx)) + float(F(dy * dy)))) + float(F(dz * dz))))
                if d2 <= float(g2):
                    pairs.append((d2, s, j))
    return pairs, pts, live


def brute_force(state, f):
    """The definition restated: sort the tuples, greedy loop, then slots, births and header in plain python."""
    from unina_yolo_dla_amd import tracking
    p, dets = f["params"], f["dets"]
    pairs, pts, live = gated_pairs(state, f)
    rec_of, slot_of = {}, {}
    for d2, s, j in sorted(pairs):
        if s not in rec_of and j not in slot_of:
            rec_of[s], slot_of[j] = j, s
    hdr, tr = state["header"].copy(), state["tracks"].copy()
    assign = np.zeros(tc.MAXD, dtype=np.int32)
    alpha = F(p["alpha"])
    died = 0
    with np.errstate(all="ignore"):
        for s in live:
            if s in rec_of:
                j = rec_of[s]
                for a, axis in enumerate("xyz"):
                    d = pts[j][a] - tr[axis][s]
                    tr[axis][s] = tr[axis][s] + alpha * d
                tr["confidence"][s], tr["class_id"][s] = dets["confidence"][j], dets["class_id"][j]
                tr["hits"][s], tr["missed"][s] = min(tr["hits"][s] + 1, 10 ** 9), 0
                assign[j] = tr["id"][s]
            else:
                tr["missed"][s] += 1
                if tr["missed"][s] > p["max_missed"]:
                    tr[s] = np.zeros((), dtype=tracking.TRACK_DTYPE)
                    died += 1
    next_id, born, dropped = int(hdr["next_id"][0]), 0, 0
    for j in sorted(pts):
        if j in slot_of or not dets["confidence"][j] >= F(p["birth_confidence"]):
            continue
        free = [s for s in range(tc.MAXD) if tr["id"][s] == 0]
        if not free or next_id == INT_MAX:
            dropped += 1
            continue
        s = free[0]
        tr[s] = (pts[j][0], pts[j][1], pts[j][2], dets["confidence"][j], next_id, dets["class_id"][j], 1, 0)
        assign[j] = next_id
        next_id, born = next_id + 1, born + 1
    alive = tr["id"] != 0
    hdr[0] = (hdr["frame"][0] + 1, alive.sum(), (alive & (tr["hits"] >= p["confirm_hits"])).sum(), next_id, len(rec_of), born, died, dropped)
    return {"header": hdr, "tracks": tr}, assign, (rec_of, pairs)


def mutual_rounds(pairs):
    """The kernel's association: rounds of mutual nearest neighbours over the free candidate pairs. Returns (slot -> record,
    number of rounds that matched something)."""
    rec_of, slot_of, rounds = {}, {}, 0
    while True:
        free = [(d2, s, j) for d2, s, j in pairs if s not in rec_of and j not in slot_of]
        if not free:
            return rec_of, rounds
        best_slot, best_rec = {}, {}
        for d2, s, j in free:
            best_slot[j] = min(best_slot.get(j, (math.inf, 1 << 30)), (d2, s))
            best_rec[s] = min(best_rec.get(s, (math.inf, 1 << 30)), (d2, j))
        for j, (d2, s) in best_slot.items():
            if best_rec[s] == (d2, j):
                rec_of[s], slot_of[j] = j, s
        rounds += 1


def check_case(c, twin_out):
    """Twin == brute force == mutual rounds on every frame; returns the headers, the assigns and the round counts."""
    from unina_yolo_dla_amd import tracking
    state, rounds = tracking.new_state(), []
    for k, (f, (want_state, want_assign)) in enumerate(zip(c["frames"], twin_out)):
        got_state, got_assign, (rec_of, pairs) = brute_force(state, f)
        where = f"{c['name']} frame {k}"
        assert got_state["header"].tobytes() == want_state["header"].tobytes(), (where, got_state["header"], want_state["header"])
        assert got_state["tracks"].tobytes() == want_state["tracks"].tobytes(), where
        assert got_assign.tobytes() == want_assign.tobytes(), where
        mutual, r = mutual_rounds(pairs)
        assert mutual == rec_of, where
        rounds.append(r)
        state = want_state
    return rounds


@pytest.fixture(scope="module")
def edges(pkg):
    return {c["name"]: (c, out, check_case(c, out)) for c, out in tc.cached("edges", tc.edge_cases)}


def headers(out):
    return [{n: int(s["header"][n][0]) for n in s["header"].dtype.names} for s, _ in out]


def test_twin_equals_brute_force_and_mutual_rounds_on_the_constructed_cases(edges):
    assert len(edges) == 27
    assert edges["chain64"][2][1] == 64 and edges["chain64_across_waves"][2][1] == 64     # one pair per round
    assert edges["full_table"][2][1] >= 2 and edges["full_table"][2][2] >= 3


@pytest.mark.parametrize("class_aware", (1, 0))
def test_twin_equals_brute_force_on_the_world_sequence(pkg, class_aware):
    (c, out), = tc.cached(f"world{class_aware}", lambda: tc.world_sequence(class_aware))
    rounds = check_case(c, out)
    h = headers(out)
    assert len(h) == 40 and [x["frame"] for x in h] == list(range(1, 41))
    assert sum(x["n_matched"] for x in h) > 1500 and sum(x["n_born"] for x in h) > 300
    assert sum(x["n_died"] for x in h) > 200 and h[-1]["n_confirmed"] > 50 and h[-1]["n_live"] > h[-1]["n_confirmed"]
    assert max(rounds) <= 4
    ids = np.concatenate([a[a != 0] for _, a in out])
    assert len(np.unique(ids)) < len(ids) / 3                                               # ids persist across frames


def test_twin_equals_brute_force_on_random_tie_heavy_tables(pkg):
    """300 random configurations on a coarse lattice (many bit-equal distances, shared positions, two classes): the greedy
    loop, the sorted-tuple brute force and the mutual rounds agree, in at most a few rounds each."""
    from unina_yolo_dla_amd import tracking
    rng = np.random.RandomState(2)
    worst = 0
    for trial in range(300):
        lattice = lambda m: rng.randint(0, 6, (m, 3)) * 0.25      # noqa: E731
        kw = dict(gate=float(rng.choice([0.25, 0.3, 0.5, 0.75])), class_aware=int(rng.randint(2)), alpha=float(rng.choice([1.0, 0.5, 0.25])),
                  max_missed=int(rng.randint(3)))
        frames = [tc.frame(lattice(rng.randint(1, 30)), cls=rng.randint(0, 2, 1)[0], **kw)]
        frames += [tc.frame(lattice(m), cls=rng.randint(0, 2, m), conf=rng.choice([0.2, 0.5, 0.9], m), **kw) for m in rng.randint(1, 30, 2)]
        c = tc.case(f"random{trial}", *frames)
        worst = max(worst, max(check_case(c, tc.run_twin(c))))
    assert 2 <= worst <= 8


def test_the_cases_are_what_they_claim(edges):
    h = {k: headers(v[1]) for k, v in edges.items()}
    a = {k: [x[1] for x in v[1]] for k, v in edges.items()}
    t = {k: [x[0]["tracks"] for x in v[1]] for k, v in edges.items()}
    for c, want in ((0, 0), (1, 1), (63, 63), (64, 64), (65, 65), (1024, 100), (5000, 100), (-7, 0)):
        x = h[f"count{c}"]
        n = min(max(c, 0), 1024)
        assert x[1]["n_matched"] == want and x[1]["n_born"] == max(n - 100, 0) and x[2]["n_matched"] == max(n, want), (c, x)
        assert not a[f"count{c}"][1][n:].any() and (a[f"count{c}"][1][:n] != 0).all()
    assert h["count5000"] == h["count1024"] and h["count0"][2]["n_live"] == 100 and h["count-7"] == h["count0"]
    assert (t["count0"][2]["missed"][:100] == 2).all() and not a["count0"][2].any()
    assert h["all_invalid"][1]["n_matched"] == 0 and h["all_invalid"][1]["n_born"] == 0 and h["all_invalid"][2]["n_matched"] == 10
    x = h["non_finite"]
    assert (x[1]["n_matched"], x[1]["n_born"]) == (5, 0) and (x[2]["n_matched"], x[2]["n_born"]) == (0, 4) and x[3]["n_matched"] == 8
    assert a["non_finite"][1][:3].tolist() == [0, 0, 0] and a["non_finite"][2][:4].tolist() == [0] * 4
    x = h["nan_confidence"][1]
    assert (x["n_matched"], x["n_born"], x["n_dropped"]) == (4, 1, 0) and a["nan_confidence"][1][4] == 0
    assert np.isnan(t["nan_confidence"][1]["confidence"][[0, 2]]).all() and t["nan_confidence"][1]["id"][4] == 5
    x = h["empty_table"]
    assert x[0]["n_live"] == 0 and x[0]["next_id"] == 1 and x[1]["frame"] == 2 and 0 < x[2]["n_born"] < 20
    x = h["full_table"]
    assert x[0]["n_born"] == 1024 and x[1]["n_matched"] == 1024 and x[2]["n_confirmed"] == 1024
    assert 900 < x[2]["n_matched"] < 1024 and x[2]["n_dropped"] == 1024 - x[2]["n_matched"] and x[2]["n_born"] == 0
    x = h["full_table_extra_births"]
    assert (x[1]["n_matched"], x[1]["n_dropped"], x[1]["n_born"], x[1]["n_live"]) == (1000, 24, 0, 1024)
    assert (x[2]["n_died"], x[2]["n_born"], x[2]["n_dropped"]) == (24, 24, 0) and x[3]["n_matched"] == 1024
    assert t["full_table_extra_births"][2]["id"][1000:].tolist() == list(range(1025, 1049))
    x = h["death_birth_reuse"][1]
    assert (x["n_matched"], x["n_died"], x["n_born"]) == (4, 1, 1)
    assert t["death_birth_reuse"][1]["id"][:6].tolist() == [1, 2, 6, 4, 5, 0] and a["death_birth_reuse"][1][4] == 6
    x = h["coast_then_die"]
    assert [y["n_live"] for y in x] == [3, 3, 3, 0, 3] and x[3]["n_died"] == 3 and t["coast_then_die"][4]["id"][:3].tolist() == [4, 5, 6]
    assert not t["coast_then_die"][3].view(np.uint8).any()
    for k, alpha in (("alpha1.0", 1.0), ("alpha0.25", 0.25)):
        assert [y["n_matched"] for y in h[k]] == [0, 50, 50, 50]
    moved = edges["alpha1.0"][0]["frames"][3]["cones"]
    assert t["alpha1.0"][3]["x"][:50].tobytes() == moved["x"].tobytes() and t["alpha0.25"][3]["x"][:50].tobytes() != moved["x"].tobytes()
    assert h["gate_exact"][1]["n_matched"] == 1 and h["gate_one_ulp_above"][1]["n_matched"] == 0 and h["gate_one_ulp_above"][1]["n_born"] == 1
    pairs = gated_pairs(edges["gate_exact"][1][0][0], edges["gate_exact"][0]["frames"][1])[0]
    assert len(pairs) == 1 and F(pairs[0][0]).view(np.uint32) == (F(0.6) * F(0.6)).view(np.uint32)
    f = edges["gate_one_ulp_above"][0]["frames"][1]["cones"]
    above = F(f["x"][0]) * F(f["x"][0]) + F(f["y"][0]) * F(f["y"][0])
    assert int(above.view(np.uint32)) == int((F(0.6) * F(0.6)).view(np.uint32)) + 1
    assert a["class_aware_pair"][1][:2].tolist() == [2, 1] and a["class_blind_pair"][1][:2].tolist() == [1, 2]
    assert t["class_blind_pair"][1]["class_id"][:2].tolist() == [1, 0] and t["class_aware_pair"][1]["class_id"][:2].tolist() == [0, 1]
    pairs = gated_pairs(edges["grid_ties"][1][0][0], edges["grid_ties"][0]["frames"][1])[0]
    assert len(pairs) > 150 and len({p[0] for p in pairs}) == 1 and h["grid_ties"][1]["n_matched"] > 40      # every distance bit-equal
    assert a["one_record_two_slots"][1][0] == 1 and a["two_records_one_slot"][1][:2].tolist() == [1, 2]
    assert h["chain64"][1]["n_matched"] == 64 and a["chain64"][1][:64].tolist() == list(range(1, 65))
    assert a["chain64_across_waves"][1][:96].tolist() == list(range(1, 97))
    full = gated_pairs(edges["full_table"][1][0][0], edges["full_table"][0]["frames"][1])[0]
    assert len(full) > 3 * 1024                                                                             # gated to several slots


def test_next_id_stops_at_int_max(pkg):
    from unina_yolo_dla_amd import tracking
    state = tracking.new_state()
    state["header"]["next_id"] = INT_MAX - 2
    f = tc.frame(tc.grid(5))
    got, assign = tracking.update_numpy(state, f["dets"], f["count"], f["cones"], f["params"])
    want, want_assign, _ = brute_force(state, f)
    assert got["header"].tobytes() == want["header"].tobytes() and got["tracks"].tobytes() == want["tracks"].tobytes()
    assert assign[:5].tolist() == [INT_MAX - 2, INT_MAX - 1, 0, 0, 0] == want_assign[:5].tolist()
    h = got["header"][0]
    assert (h["n_born"], h["n_dropped"], h["next_id"]) == (2, 3, INT_MAX)


# ---------------------------------------------------------------- csrc/track_math.h on the host
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("track_math_host")
    return hostprog.build_pair(d, "track_math_host.cpp"), d


def run_host(drivers, mode, words, float_cols):
    """Both builds on one input ([n, 16] uint32 words); the sanitised build must exit 0 and give the same words (a NaN in a
    float column is compared as a NaN: its sign differs between a folded constant and the FPU's result)."""
    def canon(g):
        assert g.size == 4 * len(words)
        g = g.reshape(-1, 4)
        for col in float_cols:
            g[np.isnan(g[:, col].view(np.float32)), col] = 0x7fc00000
        return g

    payload = struct.pack("<3i", 0x54524b31, mode, len(words)) + np.ascontiguousarray(words, dtype=np.uint32).tobytes()
    return hostprog.run_pair(*drivers, payload, dtype=np.uint32, canon=canon)


SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, 0.25, 0.6, 1e-45, 1e-38, 3e38, -3e38, 3.4028235e38, np.inf, -np.inf, np.nan, 100.0, 0.1],
                   dtype=np.float32)


def sweep(rng, n, k):
    """[n, k] fp32: specials, lattice values (ties) and random magnitudes mixed."""
    lattice = (rng.randint(-8, 9, (n, k)) * 0.25).astype(np.float32)
    wild = (rng.standard_normal((n, k)) * 10.0 ** rng.randint(-3, 4, (n, k))).astype(np.float32)
    pick = rng.randint(0, 4, (n, k))
    return np.where(pick == 0, SPECIAL[rng.randint(0, len(SPECIAL), (n, k))], np.where(pick == 1, wild, lattice)).astype(np.float32)


def test_host_math_equals_the_twin_over_a_sweep(pkg, drivers):
    from unina_yolo_dla_amd import tracking
    rng = np.random.RandomState(4)
    n = 20000
    with np.errstate(all="ignore"):
        # the pose transform
        w = np.zeros((n, 16), dtype=np.uint32)
        vals = sweep(rng, n, 15)
        w[:, :15] = vals.view(np.uint32)
        w[:, 15] = rng.randint(-1, 2, n).astype(np.int32).view(np.uint32)
        got = run_host(drivers, 0, w, (0, 1, 2))
        px, py, pz = tracking.point_numpy([vals[:, i] for i in range(12)], vals[:, 12], vals[:, 13], vals[:, 14])
        usable = (w[:, 15] != 0) & np.isfinite(px) & np.isfinite(py) & np.isfinite(pz)
        finite = np.isfinite(px) & np.isfinite(py) & np.isfinite(pz)       # NaN payloads may differ between compilers: compare the values
        for col, v in enumerate((px, py, pz)):
            ok = ~np.isnan(v)
            assert (got[ok, col] == v.view(np.uint32)[ok]).all() and np.isnan(got[~ok, col].view(np.float32)).all()
        assert (got[:, 3] == usable).all() and 0.05 < usable.mean() < 0.95 and (~finite).sum() > 1000
        # the gated distance and the key
        w = np.zeros((n, 16), dtype=np.uint32)
        vals = sweep(rng, n, 6)
        g2 = (F(0.25) * rng.randint(1, 9, n).astype(np.float32)) ** 2
        idx = rng.randint(0, 1024, n).astype(np.uint32)
        w[:, :6], w[:, 6], w[:, 7] = vals.view(np.uint32), g2.view(np.uint32), idx
        got = run_host(drivers, 1, w, (0, 3))
        d2 = tracking.d2_numpy(*[vals[:, i] for i in range(6)])
        ok = ~np.isnan(d2)
        assert (got[ok, 0] == d2.view(np.uint32)[ok]).all() and np.isnan(got[~ok, 0].view(np.float32)).all()
        assert (got[:, 1] == (d2 <= g2)).all() and 0.01 < (d2 <= g2).mean() < 0.95
        assert (got[:, 2] == idx).all() and (got[:, 3] == got[:, 0]).all()
        assert not (d2[ok].view(np.uint32) >> 31).any()                                        # never negative: the bits order
        order = np.argsort(d2[ok].view(np.uint32), kind="stable")
        by_bits = d2[ok][order]
        assert (by_bits[1:] >= by_bits[:-1]).all() and (np.diff(d2[ok].view(np.uint32)[order]) == 0).sum() > 100     # and ties exist
        # the slot update and the counters
        w = np.zeros((n, 16), dtype=np.uint32)
        vals = sweep(rng, n, 3)
        vals[:, 1] = rng.choice(np.array([1.0, 0.5, 0.25, 0.1, 0.7], dtype=np.float32), n)
        ints = np.stack([rng.choice([0, 1, 5, 10 ** 9 - 1, 10 ** 9], n), rng.choice([0, 1, 7, INT_MAX - 1, INT_MAX], n),
                         rng.randint(0, 1025, n), rng.randint(0, 1025, n), rng.choice([1, 2, 1000, INT_MAX - 1000, INT_MAX - 3, INT_MAX - 1, INT_MAX], n)],
                        axis=1).astype(np.int64)
        w[:, :3], w[:, 3:8] = vals.view(np.uint32), ints.astype(np.int32).view(np.uint32)
        got = run_host(drivers, 2, w, (0,))
        step = tracking.step_numpy(vals[:, 0], vals[:, 1], vals[:, 2])
        ok = ~np.isnan(step)
        assert (got[ok, 0] == step.view(np.uint32)[ok]).all() and np.isnan(got[~ok, 0].view(np.float32)).all()
        assert (got[:, 1] == np.minimum(ints[:, 0] + 1, 10 ** 9)).all() and (got[:, 2] == np.minimum(ints[:, 1] + 1, INT_MAX)).all()
        assert (got[:, 3] == np.minimum(np.minimum(ints[:, 2], ints[:, 3]), INT_MAX - ints[:, 4])).all()


# ---------------------------------------------------------------- the entry points' argument checks
def test_every_bad_argument_is_refused_before_any_hip_call(pkg):
    """UNINA_ERR_ARG (4) for each refusal the header lists, in a process that has no device: a HIP call in front of the
    checks would answer 3 (UNINA_ERR_HIP) instead. The pointers are never dereferenced by a refused call."""
    from unina_yolo_dla_amd import build, engine, tracking
    build.build_native()
    L = engine.load_library()
    nan, inf = float("nan"), float("inf")
    DETS, COUNT, CONES, ASSIGN = 0x10000, 0x20000, 0x30000, 0x40000
    h = C.c_void_p()
    assert L.unina_track_create(0, None) == 4 and L.unina_track_create(-1, C.byref(h)) == 4 and not h
    assert L.unina_track_create(0, C.byref(h)) == 0 and h
    try:
        def call(t=h, dets=DETS, count=COUNT, cones=CONES, par=True, assign=ASSIGN, pose=None, **kw):
            p = dict(gate=0.5, alpha=0.5, birth_confidence=0.3, class_aware=1, confirm_hits=2, max_missed=2)
            p.update(kw)
            pp = tracking.make_params(pose=pose, **p)
            return L.unina_track_update_async(t, dets, count, cones, C.byref(pp) if par else None, assign, None)

        def pose_with(i, v):
            q = list(tracking.IDENTITY)
            q[i] = v
            return q

        bad = [dict(t=None), dict(dets=None), dict(count=None), dict(cones=None), dict(par=False),
               dict(dets=DETS + 8), dict(cones=CONES + 4), dict(cones=CONES + 8), dict(assign=ASSIGN + 2), dict(assign=ASSIGN + 1),
               *[dict(pose=pose_with(i, v)) for i in range(12) for v in (nan, inf, -inf)],
               *[dict(gate=v) for v in (0.0, -1.0, nan, inf, 2e19)], *[dict(alpha=v) for v in (0.0, -0.5, 1.0001, nan, inf)],
               dict(birth_confidence=nan), dict(confirm_hits=0), dict(confirm_hits=-3), dict(max_missed=-1)]
        for kw in bad:
            assert call(**kw) == 4, kw
        assert L.unina_track_reset_async(None, None) == 4 and L.unina_track_buffers(None, None, None) == 4
        assert L.unina_track_read(None, None, None, 0, None) == 4 and L.unina_track_read(h, None, None, 0, None) == 4
        hdr = np.zeros(1, dtype=tracking.TRACK_HEADER_DTYPE)
        assert L.unina_track_read(h, hdr.ctypes.data, None, 5, None) == 4
        a, b = C.c_void_p(), C.c_void_p()
        assert L.unina_track_buffers(h, C.byref(a), C.byref(b)) == 5                  # UNINA_ERR_STATE: nothing enqueued yet
        import torch
        if not torch.cuda.is_available():
            # the good calls reach HIP, which has no device here: the checks above sit in front of it
            assert call() == 3 and call(assign=None) == 3 and call(birth_confidence=inf, alpha=1.0, max_missed=0, confirm_hits=1) == 3
            assert L.unina_track_buffers(h, C.byref(a), C.byref(b)) == 5
    finally:
        L.unina_track_destroy(h)
    L.unina_track_destroy(None)


def test_layouts_and_the_header_stays_plain_c(pkg, tmp_path):
    from unina_yolo_dla_amd import engine, tracking
    assert [tracking.TRACK_DTYPE.fields[n][1] for n in ("x", "y", "z", "confidence", "id", "class_id", "hits", "missed")] == list(range(0, 32, 4))
    assert [tracking.TRACK_HEADER_DTYPE.fields[n][1] for n in ("frame", "n_live", "n_confirmed", "next_id", "n_matched", "n_born", "n_died",
                                                               "n_dropped")] == list(range(0, 32, 4))
    assert C.sizeof(engine.TrackParams) == 72 and engine.TrackParams.gate.offset == 48 and engine.TrackParams.max_missed.offset == 68
    assert set(n for n in engine.ABI_SYMBOLS if n.startswith("unina_track_")) == {
        "unina_track_create", "unina_track_destroy", "unina_track_reset_async", "unina_track_update_async", "unina_track_buffers",
        "unina_track_read"}
    hostprog.assert_header_is_c99()
    hostprog.compile_c99(tmp_path, 'typedef char track32[(sizeof(unina_track) == 32) ? 1 : -1];\n'
                                   'typedef char id16[(offsetof(unina_track, id) == 16) ? 1 : -1];\n'
                                   'typedef char conf12[(offsetof(unina_track, confidence) == 12) ? 1 : -1];\n'
                                   'typedef char missed28[(offsetof(unina_track, missed) == 28) ? 1 : -1];\n'
                                   'typedef char head32[(sizeof(unina_track_header) == 32) ? 1 : -1];\n'
                                   'typedef char next12[(offsetof(unina_track_header, next_id) == 12) ? 1 : -1];\n'
                                   'typedef char dropped28[(offsetof(unina_track_header, n_dropped) == 28) ? 1 : -1];\n'
                                   'typedef char par72[(sizeof(unina_track_params) == 72) ? 1 : -1];\n'
                                   'typedef char gate48[(offsetof(unina_track_params, gate) == 48) ? 1 : -1];\n'
                                   'typedef char aware60[(offsetof(unina_track_params, class_aware) == 60) ? 1 : -1];\n'
                                   'typedef char max1024[(UNINA_TRACK_MAX == 1024) ? 1 : -1];\n'
                                   'int use(const GpuDetection *d, const int *n, const unina_cone3d *c, int *assign) {\n'
                                   '  unina_tracker_t *t = 0;\n'
                                   '  unina_track_params p = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, 0.5f, 0.5f, 0.3f, 1, 3, 5};\n'
                                   '  unina_track_header h;\n  unina_track tr[4];\n'
                                   '  const unina_track *dt;\n  const unina_track_header *dh;\n'
                                   '  if (unina_track_create(0, &t)) return 1;\n'
                                   '  if (unina_track_reset_async(t, 0) || unina_track_update_async(t, d, n, c, &p, assign, 0)) return 2;\n'
                                   '  if (unina_track_buffers(t, &dt, &dh) || unina_track_read(t, &h, tr, 4, 0)) return 3;\n'
                                   '  unina_track_destroy(t);\n  return h.n_live + tr[0].id;\n}\n')
