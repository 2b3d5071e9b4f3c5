"""unina_pose_async without a GPU: pose.pose_numpy (the definition) against an independent scalar restatement, csrc/pose_math.h
compiled for the host (tests/pose_math_host.cpp, also under -fsanitize=address,undefined as the stand-alone program it is) against
the numpy twin, the argument checks of the entry point, the layouts in C, what each constructed case of tests/pose_cases.py
contains, the recovery of an exact planar motion and the world sequence with a biased odometry."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import hostprog
import pose_cases as pc

F = np.float32


def f32(v):
    """A python float rounded to fp32: a double holds the sum, difference or product of two fp32 values closely enough that
    rounding it to fp32 is the fp32 operation."""
    return float(F(v))


def bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


# ---------------------------------------------------------------- an independent restatement of one call
def scalar_pose(c):
    """The header's definition in python ints and floats, one scalar operation at a time; no vectorised arithmetic."""
    from unina_yolo_dla_amd.engine import POSE_HEADER_DTYPE, POSE_RESULT_DTYPE
    p, dets, cones, tr = c["params"], c["dets"], c["cones"], c["tracks"]
    inc = [f32(v) for v in np.asarray(np.eye(3, 4) if p["inc"] is None else p["inc"], dtype=np.float64).reshape(-1)]
    with np.errstate(all="ignore"):
        if c["prev"] is None:
            P = inc
        else:
            a = [float(v) for v in c["prev"]["pose"][0]]
            P = [0.0] * 12
            for r in range(3):
                for k in range(4):
                    v = f32(f32(f32(a[4 * r] * inc[k]) + f32(a[4 * r + 1] * inc[4 + k])) + f32(a[4 * r + 2] * inc[8 + k]))
                    P[4 * r + k] = f32(v + a[4 * r + 3]) if k == 3 else v
        n = min(max(c["count"], 0), pc.MAXD)
        g2 = f32(f32(p["gate"]) * f32(p["gate"]))
        pts = []
        for j in range(n):
            x, y, z = float(cones["x"][j]), float(cones["y"][j]), float(cones["z"][j])
            pts.append([f32(f32(f32(f32(P[4 * r] * x) + f32(P[4 * r + 1] * y)) + f32(P[4 * r + 2] * z)) + P[4 * r + 3]) for r in range(3)])
        use = [j for j in range(n) if cones["valid"][j] != 0 and all(math.isfinite(v) for v in pts[j]) and abs(pts[j][0]) <= 32768.0
               and abs(pts[j][1]) <= 32768.0]
        lms = [s for s in range(pc.MAXD) if tr["id"][s] != 0 and tr["hits"][s] >= p["min_hits"] and abs(float(tr["x"][s])) <= 32768.0
               and abs(float(tr["y"][s])) <= 32768.0]
        lx, ly, lz, lc = (tr[k].tolist() for k in ("x", "y", "z", "class_id"))
        rc = dets["class_id"].tolist()
        c_, s_, tx, ty = 1.0, 0.0, 0.0, 0.0
        status, updates, n_pairs, max_bits = 0, 0, 0, 0

        def moved(q):
            return f32(f32(f32(c_ * q[0]) - f32(s_ * q[1])) + tx), f32(f32(f32(s_ * q[0]) + f32(c_ * q[1])) + ty)

        for _ in range(p["iterations"]):
            of_rec, of_lm = {}, {}                                          # record -> (d2 bits, slot), slot -> (d2 bits, record)
            for j in use:
                qx, qy = moved(pts[j])
                qz = pts[j][2]
                for s in lms:
                    if p["class_aware"] and lc[s] != rc[j]:
                        continue
                    dx = f32(qx - lx[s])
                    if dx * dx > 2.0 * g2:                                  # d2 >= fl(dx * dx): far outside the gate (a NaN goes on)
                        continue
                    dy, dz = f32(qy - ly[s]), f32(qz - lz[s])
                    d2 = f32(f32(f32(dx * dx) + f32(dy * dy)) + f32(dz * dz))
                    if d2 <= g2:
                        b = bits(d2)
                        of_rec[j] = min(of_rec.get(j, (1 << 40, 0)), (b, s))
                        of_lm[s] = min(of_lm.get(s, (1 << 40, 0)), (b, j))
            pairs = [(j, s, b) for j, (b, s) in of_rec.items() if of_lm[s] == (b, j)]
            n_pairs = len(pairs)
            max_bits = max([b for _, _, b in pairs], default=0)
            if n_pairs < p["min_pairs"]:
                status = 1
                break
            fx = lambda v: int(round(v * 1024.0))                           # noqa: E731  the product is exact in a double; round() takes halves to even, as rint does
            spx = spy = smx = smy = sdot = scross = 0
            for j, s, _ in pairs:
                ipx, ipy, imx, imy = fx(pts[j][0]), fx(pts[j][1]), fx(lx[s]), fx(ly[s])
                spx, spy, smx, smy = spx + ipx, spy + ipy, smx + imx, smy + imy
                sdot, scross = sdot + ipx * imx + ipy * imy, scross + ipx * imy - ipy * imx
            assert max(abs(sdot), abs(scross)) < 2 ** 62
            nn = float(n_pairs)
            A = float(sdot) - (float(spx) * float(smx) + float(spy) * float(smy)) / nn
            B = float(scross) - (float(spx) * float(smy) - float(spy) * float(smx)) / nn
            af, bf = f32(A), f32(B)
            h = f32(math.sqrt(f32(f32(af * af) + f32(bf * bf))))            # sqrt of an fp32 value, rounded once more: the fp32 root
            if math.isfinite(h) and h > 0:
                c_, s_, status = f32(af / h), f32(bf / h), 0
            else:
                c_, s_, status = 1.0, 0.0, 2
            tx = f32(((float(smx) - (c_ * float(spx) - s_ * float(spy))) / nn) / 1024.0)
            ty = f32(((float(smy) - (s_ * float(spx) + c_ * float(spy))) / nn) / 1024.0)
            updates += 1
        out = cones.copy()
        for j in range(n):
            out["x"][j], out["y"][j] = moved(pts[j])
            out["z"][j] = pts[j][2]
        result, header = np.zeros(1, dtype=POSE_RESULT_DTYPE), np.zeros(1, dtype=POSE_HEADER_DTYPE)
        for k in range(4):
            a, b = f32(f32(c_ * P[k]) - f32(s_ * P[4 + k])), f32(f32(s_ * P[k]) + f32(c_ * P[4 + k]))
            result["pose"][0][k], result["pose"][0][4 + k] = (f32(a + tx), f32(b + ty)) if k == 3 else (a, b)
            result["pose"][0][8 + k] = P[8 + k]
    result["c"], result["s"], result["tx"], result["ty"] = c_, s_, tx, ty
    header[0] = (n, len(use), len(lms), n_pairs, updates, status, max_bits, 0)
    return {"header": header, "result": result, "cones": out}


def assert_same(name, got, want, n=pc.MAXD):
    assert got["header"].tobytes() == want["header"].tobytes(), (name, got["header"], want["header"])
    assert got["result"].tobytes() == want["result"].tobytes(), (name, got["result"], want["result"])
    from records import assert_records_equal
    assert_records_equal(pc.canon_cones(got["cones"], n), pc.canon_cones(want["cones"], n), name, "cone")


@pytest.fixture(scope="module")
def edges(pkg):
    return {c["name"]: (c, r) for c, r in pc.edge_results()}


def head(r):
    return {n: int(r["header"][n][0]) for n in r["header"].dtype.names}


def test_twin_equals_the_scalar_restatement_on_the_constructed_cases(edges):
    assert len(edges) == 28
    for name, (c, want) in edges.items():
        assert_same(name, scalar_pose(c), want, head(want)["n_records"])
    c, _ = pc.exact_motion()
    assert_same("exact_motion", scalar_pose(c), pc.run_twin(c))
    p, order = pc.permuted(edges["plain"][0])
    assert_same("permuted", scalar_pose(p), pc.run_twin(p))


def test_what_the_constructed_cases_contain(edges, pkg):
    from unina_yolo_dla_amd import tracking
    OK, FEW, DEG = 0, 1, 2
    h = {k: head(r) for k, (_, r) in edges.items()}
    res = {k: r["result"][0] for k, (_, r) in edges.items()}
    ident = (1.0, 0.0, 0.0, 0.0)
    corr = lambda k: tuple(float(res[k][n]) for n in ("c", "s", "tx", "ty"))              # noqa: E731
    for k in ("empty_count0", "empty_table", "count0", "count_neg1"):
        assert (h[k]["status"], h[k]["iterations"], h[k]["n_pairs"], corr(k)) == (FEW, 0, 0, ident), k
    assert [h[k]["n_records"] for k in ("empty_count0", "count0", "count1025", "count_neg1", "plain")] == [0, 0, 1024, 0, 40]
    # an identity correction: the out cones are track_point of the prior, the pose is the prior
    c, r = edges["empty_table"]
    pose = [F(v) for v in np.asarray(c["params"]["inc"]).reshape(-1)]
    px, py, pz = tracking.point_numpy(pose, c["cones"]["x"][:40], c["cones"]["y"][:40], c["cones"]["z"][:40])
    assert (r["cones"]["x"][:40] == px).all() and (r["cones"]["y"][:40] == py).all() and (r["cones"]["z"][:40] == pz).all()
    assert r["cones"][40:].tobytes() == c["cones"][40:].tobytes() and (r["result"]["pose"][0] == np.array(pose)).all()
    assert all(r["cones"][n].tobytes() == c["cones"][n].tobytes() for n in ("u", "v", "n_valid", "n_samples", "valid"))
    # the plain call finds all 40 pairs and undoes the prior's error of 0.01 rad; the counts beyond 1024 change nothing
    assert (h["plain"]["status"], h["plain"]["iterations"], h["plain"]["n_pairs"]) == (OK, 4, 40) and abs(corr("plain")[1] + 0.01) < 1e-4
    assert edges["count1025"][1]["result"].tobytes() == edges["plain"][1]["result"].tobytes()
    assert edges["slots_across_waves"][1]["result"].tobytes() == edges["plain"][1]["result"].tobytes()
    assert h["plain_prev"]["iterations"] == 8 and h["plain_prev"]["n_pairs"] == 40
    assert h["class_blind"]["n_pairs"] == 40 and h["class_aware_no_match"]["status"] == FEW and h["class_aware_no_match"]["n_pairs"] < 3
    assert h["one_iteration"]["iterations"] == 1 and h["one_iteration"]["n_pairs"] < 40       # the drift hides a pair at first
    assert (h["pairs_equal_min"]["status"], h["pairs_equal_min"]["n_pairs"], h["pairs_equal_min"]["iterations"]) == (OK, 4, 4)
    assert (h["pairs_below_min"]["status"], h["pairs_below_min"]["n_pairs"], h["pairs_below_min"]["iterations"]) == (FEW, 4, 0)
    assert corr("pairs_below_min") == ident
    k = "too_few_at_iteration_2"
    assert (h[k]["status"], h[k]["iterations"], h[k]["n_pairs"]) == (FEW, 1, 2) and corr(k) != ident and abs(corr(k)[2] + 0.6) < 0.1
    assert (h["degenerate"]["status"], h["degenerate"]["n_pairs"], h["degenerate"]["iterations"]) == (DEG, 2, 4)
    assert corr("degenerate") == (1.0, 0.0, 0.25, 0.125)
    assert h["half_turn"]["status"] == OK and corr("half_turn")[0] == -1.0 and abs(corr("half_turn")[1]) == 0.0
    assert (h["two_records_one_landmark"]["n_usable"], h["two_records_one_landmark"]["n_pairs"]) == (5, 4)
    assert h["ties"]["n_pairs"] == 5 and h["ties_slots_swapped"]["n_pairs"] == 5
    assert edges["ties"][1]["result"].tobytes() != edges["ties_slots_swapped"][1]["result"].tobytes()        # the index decided
    assert corr("ties")[2] < 0 < corr("ties_slots_swapped")[2]
    g2 = F(0.6) * F(0.6)
    assert (h["gate_exact"]["n_pairs"], h["gate_exact"]["max_d2_bits"]) == (3, int(g2.view(np.uint32)))
    assert (h["gate_one_ulp_above"]["n_pairs"], h["gate_one_ulp_above"]["status"]) == (2, FEW)
    assert (h["hits_one_short"]["n_landmarks"], h["hits_one_short"]["n_pairs"]) == (30, 30)
    assert (h["non_finite_and_invalid"]["n_usable"], h["non_finite_and_invalid"]["n_pairs"]) == (32, 32)
    out = edges["non_finite_and_invalid"][1]["cones"]
    assert np.isnan(out["x"][0]) and not np.isfinite(out["y"][1]) and np.isinf(out["z"][2]) and np.isfinite(out["x"][4:8]).all()
    assert h["non_finite_landmarks"]["n_landmarks"] == 38 and h["non_finite_landmarks"]["n_pairs"] == 37    # a NaN z: a landmark without a candidate
    assert [(h[k]["n_usable"], h[k]["n_landmarks"], h[k]["n_pairs"]) for k in ("limit_inside", "limit_point_beyond", "limit_landmark_beyond")] == \
        [(5, 5, 5), (3, 5, 3), (5, 3, 3)]
    k = "fixed_point_edge"
    assert (h[k]["n_pairs"], h[k]["iterations"], h[k]["status"]) == (1024, 2, OK) and corr(k) == (1.0, 0.0, -0.125, 0.0)
    c = edges[k][0]
    ix, iy = np.rint(c["tracks"]["x"] * F(1024)).astype(np.int64), np.rint(c["tracks"]["y"] * F(1024)).astype(np.int64)
    assert abs(iy).max() == 2 ** 25 and 2 ** 60 < int((ix * ix + iy * iy).sum()) < 2 ** 62               # the sums reach their design size


# ---------------------------------------------------------------- csrc/pose_math.h on the host
def host_payload(c):
    p = c["params"]
    w = np.zeros(40, dtype=np.int32)
    w[:12] = np.asarray(np.eye(3, 4) if p["inc"] is None else p["inc"], dtype=np.float32).reshape(-1).view(np.int32)
    w[12] = F(p["gate"]).view(np.int32)
    w[13:17] = p["class_aware"], p["min_hits"], p["iterations"], p["min_pairs"]
    if c["prev"] is not None:
        w[17] = 1
        w[18:34] = c["prev"].view(np.int32).reshape(-1)
    w[34] = c["count"]
    return struct.pack("<3i", 0x504f5331, 0, 1) + w.tobytes() + c["dets"].tobytes() + c["cones"].tobytes() + c["tracks"].tobytes()


def host_result(words):
    from unina_yolo_dla_amd.engine import CONE3D_DTYPE, POSE_HEADER_DTYPE, POSE_RESULT_DTYPE
    assert len(words) == 8 * pc.MAXD + 16 + 8
    return {"cones": words[:8 * pc.MAXD].view(CONE3D_DTYPE), "result": words[8 * pc.MAXD:8 * pc.MAXD + 16].view(POSE_RESULT_DTYPE),
            "header": words[8 * pc.MAXD + 16:].view(POSE_HEADER_DTYPE)}


def canon_host(words):
    words = words.copy()
    words[:8 * pc.MAXD] = pc.canon_cones(words[:8 * pc.MAXD].view(host_cone_dtype())).view(np.int32)
    return words


def host_cone_dtype():
    from unina_yolo_dla_amd.engine import CONE3D_DTYPE
    return CONE3D_DTYPE


def test_pose_math_header_on_the_host_equals_the_twin(edges, tmp_path):
    """The whole stage as loops over csrc/pose_math.h on every constructed case, the exact motion and a permuted call; then 20 000
    seeded sets of sums through pose_solve alone, degenerate ones and sums of the design size among them."""
    from unina_yolo_dla_amd import pose
    drivers = hostprog.build_pair(tmp_path, "pose_math_host.cpp")
    cases = [v for v in edges.values()] + [(c, pc.run_twin(c)) for c in (pc.exact_motion()[0], pc.permuted(edges["plain"][0])[0])]
    for c, want in cases:
        got = host_result(hostprog.run_pair(drivers, tmp_path, host_payload(c), canon=canon_host))
        assert_same(c["name"], got, want)
    rng = np.random.RandomState(4)
    n = 20000
    sums = np.zeros((n, 7), dtype=np.int64)
    sums[:, 0] = rng.randint(1, 1025, n)
    scale = 2 ** rng.randint(4, 26, n).astype(np.int64)
    for col in (1, 2, 3, 4):
        sums[:, col] = (rng.uniform(-1, 1, n) * scale * sums[:, 0]).astype(np.int64)
    for col in (5, 6):
        sums[:, col] = (rng.uniform(-1, 1, n) * scale.astype(np.float64) ** 2 * sums[:, 0]).astype(np.int64)
    sums[:200, 5] = sums[:200, 6] = 0                                       # all pairs at the origin: degenerate
    sums[:200, 1:5] = 0
    sums[200:400, 5] = rng.choice([-1, 1], 200) * (2 ** 61 - rng.randint(0, 1000, 200))
    got = hostprog.run_pair(drivers, tmp_path, struct.pack("<3i", 0x504f5331, 1, n) + sums.tobytes()).reshape(n, 8)
    want = np.zeros((n, 8), dtype=np.int32)
    for i, row in enumerate(sums.tolist()):
        corr, status = pose.solve_numpy(*row)
        want[i, :4] = np.array(corr, dtype=np.float32).view(np.int32)
        want[i, 4] = status
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
    assert (want[:200, 4] == 2).all() and (want[200:, 4] == 0).mean() > 0.99
    # c * c + s * s == 1 to fp32 rounding wherever the rotation was taken
    cs = want[200:, :2].copy().view(np.float32).astype(np.float64)
    assert np.abs((cs ** 2).sum(axis=1) - 1.0).max() < 4e-7


# ---------------------------------------------------------------- the entry point's argument checks
def test_every_bad_argument_is_refused_before_any_hip_call(pkg):
    """UNINA_ERR_ARG (4) for each refusal the header lists, in a process that has no device: a HIP call in front of the checks
    would answer 3 (UNINA_ERR_HIP) instead. The pointers are never dereferenced by a refused call."""
    from unina_yolo_dla_amd import build, engine, pose
    build.build_native()
    L = engine.load_library()
    nan, inf = float("nan"), float("inf")
    DETS, COUNT, CONES, TRACKS, PREV, OUT, RES, HDR = (0x10000 * k for k in range(1, 9))

    def call(dets=DETS, count=COUNT, cones=CONES, tracks=TRACKS, prev=None, par=True, out=OUT, res=RES, hdr=HDR, **kw):
        pp = pose.make_params(**kw)
        return L.unina_pose_async(dets, count, cones, tracks, prev, C.byref(pp) if par else None, out, res, hdr, None)

    def inc_with(i, v):
        q = list(pose.IDENTITY)
        q[i] = v
        return q

    bad = [dict(dets=None), dict(count=None), dict(cones=None), dict(tracks=None), dict(par=False), dict(out=None), dict(res=None), dict(hdr=None),
           dict(dets=DETS + 8), dict(count=COUNT + 2), dict(cones=CONES + 4), dict(cones=CONES + 8), dict(tracks=TRACKS + 8), dict(tracks=TRACKS + 4),
           dict(prev=PREV + 8), dict(prev=PREV + 4), dict(out=OUT + 8), dict(res=RES + 8), dict(res=RES + 4), dict(hdr=HDR + 8), dict(hdr=HDR + 4),
           dict(out=CONES + 32), dict(out=CONES - 32), dict(out=CONES + 32 * 1023), dict(prev=PREV, res=PREV + 16), dict(prev=PREV, res=PREV - 48),
           *[dict(inc=inc_with(i, v)) for i in range(12) for v in (nan, inf, -inf)],
           *[dict(gate=v) for v in (0.0, -1.0, nan, inf, 2e19)], dict(min_hits=0), dict(min_hits=-2), dict(iterations=0), dict(iterations=9),
           dict(iterations=-1), dict(min_pairs=1), dict(min_pairs=0), dict(min_pairs=-5)]
    for kw in bad:
        assert call(**kw) == 4, kw
    import torch
    if not torch.cuda.is_available():
        # the good calls reach HIP, which has no device here: the checks above sit in front of it
        good = [dict(), dict(out=CONES), dict(prev=PREV), dict(prev=PREV, res=PREV), dict(out=CONES + 32 * 1024), dict(prev=PREV, res=PREV + 64),
                dict(iterations=8, min_pairs=2, min_hits=1, class_aware=0, gate=1e19)]
        for kw in good:
            assert call(**kw) == 3, kw
    for kw in (dict(gate=nan), dict(min_hits=0), dict(iterations=9), dict(min_pairs=1), dict(inc=inc_with(3, inf))):
        with pytest.raises(ValueError):
            pose.check_params(pose.make_params(**kw))


def test_layouts_and_the_header_stays_plain_c(pkg, tmp_path):
    from unina_yolo_dla_amd import engine, pose
    assert C.sizeof(engine.PoseParams) == 68 and engine.PoseParams.gate.offset == 48 and engine.PoseParams.min_pairs.offset == 64
    assert engine.POSE_RESULT_DTYPE.itemsize == 64 and [engine.POSE_RESULT_DTYPE.fields[n][1] for n in ("pose", "c", "s", "tx", "ty")] == [0, 48, 52, 56, 60]
    assert engine.POSE_HEADER_DTYPE.itemsize == 32 and [engine.POSE_HEADER_DTYPE.fields[n][1] for n in engine.POSE_HEADER_DTYPE.names] == list(range(0, 32, 4))
    assert (engine.POSE_OK, engine.POSE_TOO_FEW, engine.POSE_DEGENERATE) == (0, 1, 2) and "unina_pose_async" in engine.ABI_SYMBOLS
    assert pose.TRACK_MAX == 1024
    hostprog.assert_header_is_c99()
    hostprog.compile_c99(tmp_path, 'typedef char par68[(sizeof(unina_pose_params) == 68) ? 1 : -1];\n'
                                   'typedef char gate48[(offsetof(unina_pose_params, gate) == 48) ? 1 : -1];\n'
                                   'typedef char pairs64[(offsetof(unina_pose_params, min_pairs) == 64) ? 1 : -1];\n'
                                   'typedef char res64[(sizeof(unina_pose_result) == 64) ? 1 : -1];\n'
                                   'typedef char c48[(offsetof(unina_pose_result, c) == 48) ? 1 : -1];\n'
                                   'typedef char ty60[(offsetof(unina_pose_result, ty) == 60) ? 1 : -1];\n'
                                   'typedef char head32[(sizeof(unina_pose_header) == 32) ? 1 : -1];\n'
                                   'typedef char status20[(offsetof(unina_pose_header, status) == 20) ? 1 : -1];\n'
                                   'typedef char bits24[(offsetof(unina_pose_header, max_d2_bits) == 24) ? 1 : -1];\n'
                                   'typedef char codes[(UNINA_POSE_OK == 0 && UNINA_POSE_TOO_FEW == 1 && UNINA_POSE_DEGENERATE == 2) ? 1 : -1];\n'
                                   'typedef char its[(UNINA_POSE_MAX_ITERATIONS == 8) ? 1 : -1];\n'
                                   'int use(const GpuDetection *d, const int *n, unina_cone3d *c, unina_tracker_t *t, unina_pose_result *r,\n'
                                   '        unina_pose_header *h, int *assign) {\n'
                                   '  unina_pose_params p = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, 1.0f, 1, 3, 4, 3};\n'
                                   '  unina_track_params tp = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, 0.5f, 0.5f, 0.3f, 1, 3, 5};\n'
                                   '  const unina_track *slots;\n'
                                   '  if (unina_track_buffers(t, &slots, 0)) return 1;\n'
                                   '  if (unina_pose_async(d, n, c, slots, r, &p, c, r, h, 0)) return 2;\n'
                                   '  return unina_track_update_async(t, d, n, c, &tp, assign, 0);\n}\n')


# ---------------------------------------------------------------- what the stage is for
def test_an_exact_planar_motion_is_recovered_to_the_fixed_point_step(pkg):
    """40 cones at 5 .. 30 m, no noise, a prior wrong by 0.02 rad and 0.3 m: the corrected pose is the true one to |dt| <= 2 mm and
    |dyaw| <= 1e-4 rad. Measured on the twin: 0.038 mm and 6.0e-6 rad, after one iteration as after eight (every iteration solves
    for the whole correction from the unmoved points; the step of the sums is 1 mm)."""
    c, truth = pc.exact_motion()
    for it in (1, 4, 8):
        r = pc.run_twin(dict(c, params=dict(c["params"], iterations=it)))
        dt, dyaw = pc.pose_error(r["result"]["pose"][0], truth)
        print(f"iterations {it}: |dt| = {dt * 1e3:.4f} mm, |dyaw| = {dyaw:.3e} rad, header {r['header'][0]}")
        assert head(r)["n_pairs"] == 40 and head(r)["status"] == 0
        assert dt <= 2e-3 and dyaw <= 1e-4
    prior_dt, prior_dyaw = pc.pose_error(np.asarray(c["params"]["inc"]).reshape(-1), truth)
    assert prior_dt > 0.25 and prior_dyaw > 0.019


@pytest.mark.parametrize("seed", (5, 6, 7))
def test_world_sequence_with_a_biased_odometry(pkg, seed):
    """150 cones, 40 frames, 2 cm noise, 15 % dropouts, 10 false positives per frame, an odometry wrong by 0.004 rad and 0.05 m per
    frame. Handed to the tracker as it is, the pose is wrong by 2.80 m and 0.156 rad after 40 frames; with the stage in front
    (the earlier result chained, gate 1.0, min_hits 3, 4 iterations, min_pairs 3) by 0.106 / 0.096 / 0.090 m and 0.0052 / 0.0048 /
    0.0047 rad for seeds 5 / 6 / 7, at most 0.106 m and 0.0080 rad over the frames (the first three frames have no confirmed
    track yet and take the odometry as it is)."""
    _, truth, _ = pc.world_chain_inputs(seed)
    out = pc.chain_results(seed)
    errs = [pc.pose_error(o[3], T) for o, T in zip(out, truth)]
    dead = pc.run_chain_twin(seed, with_stage=False)
    dead_dt, dead_dyaw = pc.pose_error(dead[-1][3], truth[-1])
    print(f"seed {seed}: final {errs[-1]}, largest {max(e[0] for e in errs)}, {max(e[1] for e in errs)}; without the stage {dead_dt}, {dead_dyaw}")
    assert dead_dt > 2.5 and dead_dyaw > 0.15
    assert errs[-1][0] <= 0.25 and errs[-1][1] <= 0.02
    heads = [head(o[0]) for o in out]
    assert [h["status"] for h in heads[:3]] == [1, 1, 1] and all(h["status"] == 0 and h["n_pairs"] > 40 for h in heads[3:])
    # the table the stage keeps together: more confirmed tracks than the smeared one
    assert out[-1][1]["header"]["n_confirmed"][0] > dead[-1][1]["header"]["n_confirmed"][0]
