"""unina_boundary_async without a GPU: boundary.boundary_numpy (the definition) against an independent scalar restatement,
csrc/boundary_math.h compiled for the host (tests/boundary_math_host.cpp, also under -fsanitize=address,undefined as the stand-alone
program it is) against the numpy twin, the argument checks of the entry point, the layouts in C, what each constructed case of
tests/boundary_cases.py contains, and the quality of the chains and of the centre line on a synthetic oval track."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import boundary_cases as bc
import hostprog
from records import assert_records_equal

F = np.float32
NO_FIRST, NO_NEXT, FULL, NO_HEADING = bc.NO_FIRST, bc.NO_NEXT, bc.FULL, bc.NO_HEADING


def f32(v):
    """A python float rounded to fp32: a double holds the sum, difference or product of two fp32 values closely enough that
    rounding it to fp32 is the fp32 operation."""
    return float(F(v))


def bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


# ---------------------------------------------------------------- an independent restatement of one call
def scalar_boundary(c):
    """The header's definition in python ints and floats, one scalar operation at a time; no vectorised arithmetic."""
    from unina_yolo_dla_amd.engine import BOUNDARY_HEADER_DTYPE, BOUNDARY_POINT_DTYPE
    p, tr = c["params"], c["tracks"]
    pose = np.eye(3, 4) if p["pose"] is None else p["pose"]
    P = [f32(v) for v in (np.asarray(pose, dtype=np.float64).reshape(-1) if c["dpose"] is None else c["dpose"]["pose"][0])]
    f = [f32(v) for v in p["forward"]]
    header, points = np.zeros(1, dtype=BOUNDARY_HEADER_DTYPE), np.zeros(256, dtype=BOUNDARY_POINT_DTYPE)
    sq = lambda v: f32(f32(v) * f32(v))                                                    # noqa: E731
    first2, step2, cos2, width2 = sq(p["first_gate"]), sq(p["step_gate"]), sq(p["cos_turn"]), sq(p["width_gate"])
    with np.errstate(all="ignore"):
        ox, oy = P[3], P[7]
        hx = f32(f32(f32(P[0] * f[0]) + f32(P[1] * f[1])) + f32(P[2] * f[2]))
        hy = f32(f32(f32(P[4] * f[0]) + f32(P[5] * f[1])) + f32(P[6] * f[2]))
        n2 = f32(f32(hx * hx) + f32(hy * hy))
    if not (math.isfinite(ox) and math.isfinite(oy) and math.isfinite(n2) and n2 > 0):
        header["end"][0] = NO_HEADING
        return header, points
    x, y, z, ids, cls, hits = (tr[k].tolist() for k in ("x", "y", "z", "id", "class_id", "hits"))

    def plane_d2(ax, ay, bx, by):
        dx, dy = f32(ax - bx), f32(ay - by)
        return f32(f32(dx * dx) + f32(dy * dy))

    chains = []
    for k, want in enumerate((p["class_left"], p["class_right"])):
        cand = [s for s in range(bc.MAXD) if ids[s] != 0 and hits[s] >= p["min_hits"] and cls[s] == want and abs(x[s]) <= 32768.0 and abs(y[s]) <= 32768.0]
        chain, end = [], None
        cx, cy, dirx, diry = ox, oy, hx, hy
        while end is None:
            m = len(chain)
            if m == p["max_chain"]:
                end = FULL
                break
            best = None
            for s in cand:
                if s in chain:
                    continue
                dx, dy = f32(x[s] - cx), f32(y[s] - cy)
                d2 = f32(f32(dx * dx) + f32(dy * dy))
                dot = f32(f32(dx * dirx) + f32(dy * diry))
                if m == 0:
                    ok = d2 <= first2 and dot >= 0
                else:
                    ok = d2 <= step2 and dot > 0 and f32(dot * dot) >= f32(cos2 * f32(d2 * f32(f32(dirx * dirx) + f32(diry * diry))))
                if ok and (best is None or (bits(d2), s) < best):
                    best = (bits(d2), s)
            if best is None:
                end = NO_FIRST if m == 0 else NO_NEXT
                break
            s = best[1]
            if m >= 1:
                dirx, diry = f32(x[s] - cx), f32(y[s] - cy)
            cx, cy = x[s], y[s]
            chain.append(s)
        for m, s in enumerate(chain):
            points[64 * k + m] = (x[s], y[s], z[s], ids[s])
        header["n_candidates"][0][k], header["n_chain"][0][k], header["end"][0][k] = len(cand), len(chain), end
        chains.append(chain)
    L, R = chains
    n_centre = n_wide = 0
    if L and R:
        i = j = 0
        while True:
            l, r = L[i], R[j]
            if plane_d2(x[l], y[l], x[r], y[r]) <= width2:
                points[128 + n_centre] = (f32(f32(x[l] + x[r]) * 0.5), f32(f32(y[l] + y[r]) * 0.5), f32(f32(z[l] + z[r]) * 0.5), i | j << 16)
                n_centre += 1
            else:
                n_wide += 1
            has_i, has_j = i + 1 < len(L), j + 1 < len(R)
            if not has_i and not has_j:
                break
            if has_i and (not has_j or plane_d2(x[L[i + 1]], y[L[i + 1]], x[r], y[r]) <= plane_d2(x[l], y[l], x[R[j + 1]], y[R[j + 1]])):
                i += 1
            else:
                j += 1
    header["n_centre"], header["n_wide"] = n_centre, n_wide
    return header, points


def assert_same(name, got, want):
    assert got[0].tobytes() == want[0].tobytes(), (name, got[0], want[0])
    assert_records_equal(got[1], want[1], name, "point")


@pytest.fixture(scope="module")
def edges(pkg):
    return {c["name"]: (c, r) for c, r in bc.edge_results()}


def head(r):
    h = r[0][0]
    return {"cand": h["n_candidates"].tolist(), "chain": h["n_chain"].tolist(), "end": h["end"].tolist(), "centre": int(h["n_centre"]),
            "wide": int(h["n_wide"])}


def sides(r):
    from unina_yolo_dla_amd import boundary
    return boundary.split(*r)


def test_twin_equals_the_scalar_restatement_on_the_constructed_cases(edges):
    assert len(edges) == 35
    for name, (c, want) in edges.items():
        assert_same(name, scalar_boundary(c), want)
    c, want, _ = bc.oval_result(0, 1 / 3)
    assert_same(c["name"], scalar_boundary(c), want)
    p = bc.permuted(c)
    assert_same(p["name"], scalar_boundary(p), bc.run_twin(p))


def test_what_the_constructed_cases_contain(edges):
    h = {k: head(r) for k, (_, r) in edges.items()}
    assert h["empty"] == dict(cand=[0, 0], chain=[0, 0], end=[NO_FIRST, NO_FIRST], centre=0, wide=0)
    assert all(not r[1].tobytes().strip(b"\0") for r in (edges["empty"][1], edges["no_heading_from_forward"][1]))
    assert h["left_only"] == dict(cand=[5, 0], chain=[5, 0], end=[NO_NEXT, NO_FIRST], centre=0, wide=0)
    assert h["plain"] == dict(cand=[8, 8], chain=[8, 8], end=[NO_NEXT, NO_NEXT], centre=15, wide=0)
    L, R, Cn = sides(edges["plain"][1])
    assert L["x"].tolist() == R["x"].tolist() == [2.0 + 3 * k for k in range(8)] and set(L["y"]) == {1.5} and set(R["y"]) == {-1.5}
    assert L["ref"].tolist() == list(range(1, 9)) and R["ref"].tolist() == list(range(9, 17))
    assert set(Cn["y"]) == {0.0} and set(Cn["z"]) == {0.25} and (np.diff(Cn["x"]) == 1.5).all() and Cn["ref"][1] == 1 and Cn["ref"][2] == 1 | 1 << 16
    assert edges["plain"][1][1][8:64].tobytes() == bytes(56 * 16)                            # behind the count: zero bytes
    # a free slot with coordinates, a slot one hit short and a third class would each have been the first link at (1, +-1.5)
    for k in ("id0_with_coordinates", "hits_one_short", "third_class"):
        assert h[k] == dict(cand=[4, 4], chain=[4, 4], end=[NO_NEXT, NO_NEXT], centre=7, wide=0), k
        assert sides(edges[k][1])[0]["x"][0] == 2.0
    assert h["non_finite"]["cand"] == [3, 3] and h["non_finite"]["chain"] == [3, 3]
    L, _, Cn = sides(edges["non_finite"][1])
    assert np.isinf(L["z"][0]) and np.isinf(Cn["z"][0]) and L["z"][2] == F(-3e38)            # z is carried, never tested
    assert h["limit_inside"]["cand"] == [6, 0] and h["limit_beyond"]["cand"] == [2, 0]
    assert h["limit_chained"] == dict(cand=[2, 0], chain=[2, 0], end=[NO_NEXT, NO_FIRST], centre=0, wide=0)
    assert sides(edges["limit_chained"][1])[0]["x"].tolist() == [32764.0, 32768.0]
    # the first link
    assert (h["first_gate_exact"]["chain"], h["first_gate_exact"]["end"][0]) == ([1, 0], NO_NEXT)
    assert (h["first_gate_one_ulp_beyond"]["cand"], h["first_gate_one_ulp_beyond"]["chain"], h["first_gate_one_ulp_beyond"]["end"][0]) == ([1, 0], [0, 0], NO_FIRST)
    assert h["abeam"]["chain"] == [1, 1] and h["abeam"]["centre"] == 1
    assert h["behind"] == dict(cand=[2, 1], chain=[1, 0], end=[NO_NEXT, NO_FIRST], centre=0, wide=0) and sides(edges["behind"][1])[0]["x"][0] == 3.0
    # later links
    assert h["step_gate_exact"]["chain"] == [2, 0] and h["step_gate_one_ulp_beyond"]["chain"] == [1, 0]
    assert h["turn_one_ulp_inside"]["chain"] == [3, 0] and h["turn_on_bound"]["chain"] == [3, 0] and h["turn_one_ulp_beyond"]["chain"] == [2, 0]
    ys = [float(edges[k][0]["tracks"]["y"][2]) for k in ("turn_one_ulp_inside", "turn_on_bound", "turn_one_ulp_beyond")]
    assert ys[0] < ys[1] < ys[2] and ys[2] == float(np.nextafter(F(ys[1]), F(np.inf))) and abs(math.degrees(math.atan2(ys[1] - 1.0, 0.5) - math.atan2(1, 3)) - 60.0) < 1e-3
    k = "second_track_at_the_same_place"
    assert h[k]["cand"] == [3, 0] and h[k]["chain"] == [2, 0] and sides(edges[k][1])[0]["ref"].tolist() == [1, 3]
    assert h["ring8"] == dict(cand=[8, 0], chain=[8, 0], end=[NO_NEXT, NO_FIRST], centre=0, wide=0)
    assert sorted(sides(edges["ring8"][1])[0]["ref"].tolist()) == list(range(1, 9))           # no revisit
    # ties: the lower slot
    a, b = sides(edges["tie_slots_5_and_1000"][1])[0], sides(edges["tie_slots_swapped"][1])[0]
    assert (len(a), len(b), float(a["y"][0]), float(b["y"][0]), int(a["ref"][0]), int(b["ref"][0])) == (1, 1, 2.0, -2.0, 1, 1)
    # chain length
    assert h["max_chain_1"] == dict(cand=[8, 8], chain=[1, 1], end=[FULL, FULL], centre=1, wide=0)
    assert [(h[k]["cand"][0], h[k]["chain"][0], h[k]["end"][0]) for k in ("line63", "line64", "line65")] == [(63, 63, NO_NEXT), (64, 64, FULL), (65, 64, FULL)]
    k = "all_1024_of_one_class"
    assert h[k] == dict(cand=[1024, 0], chain=[64, 0], end=[FULL, NO_FIRST], centre=0, wide=0)
    refs = sides(edges[k][1])[0]["ref"]
    assert refs.tolist() == list(range(1, 65))                                               # along the spiral, from its start
    slots = np.array([int(np.nonzero(edges[k][0]["tracks"]["id"] == r)[0][0]) for r in refs])
    assert len(set((slots // 64).tolist())) == 16 and (np.bincount(slots % 64, minlength=64) > 0).sum() > 30   # every wave's share of the list, many lanes
    # the ladder
    assert h["line64"]["centre"] == 127 and h["line64"]["wide"] == 0
    assert h["ladder_1_and_64"]["chain"] == [1, 64] and h["ladder_1_and_64"]["centre"] + h["ladder_1_and_64"]["wide"] == 64
    assert (h["width_gate_exact"]["centre"], h["width_gate_exact"]["wide"]) == (1, 0)
    assert (h["width_gate_one_ulp_beyond"]["centre"], h["width_gate_one_ulp_beyond"]["wide"]) == (0, 1)
    assert sides(edges["advance_tie"][1])[2]["ref"].tolist() == [0, 1, 1 | 1 << 16]              # i moved on the tie
    # the pose
    for k in ("no_heading_from_forward", "no_heading_from_a_nan_device_pose"):
        assert h[k] == dict(cand=[0, 0], chain=[0, 0], end=[NO_HEADING, NO_HEADING], centre=0, wide=0), k
    c, r = edges["device_pose_beside_another_pose"]
    assert h[c["name"]] == h["plain"] and sides(r)[0]["ref"].tolist() == list(range(1, 9))
    assert head(bc.run_twin(dict(c, dpose=None)))["chain"] != [8, 8]                          # the parameters' pose would have given another answer
    np.testing.assert_allclose(sides(r)[2]["x"], 10.0, atol=1e-5)


def test_permuted_slots_give_the_same_points_and_header():
    c, want, _ = bc.oval_result(0, 1 / 3)
    got = bc.run_twin(bc.permuted(c))
    assert_same("permuted", got, want)


# ---------------------------------------------------------------- csrc/boundary_math.h on the host
def host_payload(c):
    from unina_yolo_dla_amd import boundary
    p = boundary.as_params(c["params"])
    assert C.sizeof(p) == 92
    dpose = np.zeros(12, dtype=np.float32) if c["dpose"] is None else c["dpose"]["pose"][0]
    return (struct.pack("<i", 0x424e4431) + bytes(p) + struct.pack("<i", 0 if c["dpose"] is None else 1) + np.asarray(dpose, dtype=np.float32).tobytes()
            + np.ascontiguousarray(c["tracks"]).tobytes())


def test_boundary_math_header_on_the_host_equals_the_twin(edges, tmp_path):
    """The whole stage as loops over csrc/boundary_math.h on every constructed case, the oval and a permuted oval."""
    from unina_yolo_dla_amd.engine import BOUNDARY_HEADER_DTYPE, BOUNDARY_POINT_DTYPE
    drivers = hostprog.build_pair(tmp_path, "boundary_math_host.cpp")
    c, want, _ = bc.oval_result(0, 1 / 3)
    p = bc.permuted(c)
    for c, want in list(edges.values()) + [(c, want), (p, bc.run_twin(p))]:
        words = hostprog.run_pair(drivers, tmp_path, host_payload(c))
        assert len(words) == 8 + 4 * 256
        assert_same(c["name"], (words[:8].view(BOUNDARY_HEADER_DTYPE), words[8:].view(BOUNDARY_POINT_DTYPE)), want)


# ---------------------------------------------------------------- the entry point's argument checks
def test_every_bad_argument_is_refused_before_any_hip_call(pkg):
    """UNINA_ERR_ARG (4) for each refusal the header lists, in a process that has no device: a HIP call in front of the checks
    would answer 3 (UNINA_ERR_HIP) instead. The pointers are never dereferenced by a refused call."""
    from unina_yolo_dla_amd import boundary, build, engine
    build.build_native()
    L = engine.load_library()
    nan, inf = float("nan"), float("inf")
    TRACKS, POSE, POINTS, HDR = (0x10000 * k for k in range(1, 5))

    def call(tracks=TRACKS, dpose=None, par=True, points=POINTS, hdr=HDR, **kw):
        pp = boundary.params(**kw)
        return L.unina_boundary_async(tracks, dpose, C.byref(pp) if par else None, points, hdr, None)

    def with_value(base, i, v):
        q = list(base)
        q[i] = v
        return q

    ident = list(boundary.IDENTITY)
    bad = [dict(tracks=None), dict(par=False), dict(points=None), dict(hdr=None),
           dict(tracks=TRACKS + 8), dict(tracks=TRACKS + 4), dict(dpose=POSE + 8), dict(dpose=POSE + 4), dict(points=POINTS + 8), dict(points=POINTS + 4),
           dict(hdr=HDR + 8), dict(hdr=HDR + 4),
           *[dict(pose=with_value(ident, i, v)) for i in range(12) for v in (nan, inf, -inf)],
           *[dict(forward=with_value((1.0, 0.0, 0.0), i, v)) for i in range(3) for v in (nan, inf, -inf)],
           *[dict(dpose=POSE, forward=with_value((1.0, 0.0, 0.0), i, nan)) for i in range(3)],
           *[{g: v} for g in ("first_gate", "step_gate", "width_gate") for v in (0.0, -1.0, nan, inf, 2e19)],
           *[dict(cos_turn=v) for v in (nan, -0.01, 1.0, 1.5, inf, -inf)], dict(min_hits=0), dict(min_hits=-3), dict(max_chain=0), dict(max_chain=65),
           dict(max_chain=-1), dict(class_left=-1), dict(class_right=-1), dict(class_left=2, class_right=2), dict(class_left=0, class_right=0),
           dict(points=HDR), dict(points=HDR + 16), dict(points=HDR - 4096 + 16), dict(hdr=POINTS + 16), dict(hdr=POINTS + 4080), dict(hdr=POINTS - 16)]
    for kw in bad:
        assert call(**kw) == 4, kw
    import torch
    if not torch.cuda.is_available():
        # the good calls reach HIP, which has no device here: the checks above sit in front of it
        good = [dict(), dict(dpose=POSE), dict(dpose=POSE, pose=with_value(ident, 3, nan)), dict(dpose=POSE, pose=with_value(ident, 0, inf)),
                dict(points=HDR + 32), dict(points=HDR - 4096), dict(cos_turn=0.0), dict(cos_turn=0.999), dict(max_chain=1), dict(max_chain=64),
                dict(first_gate=1e19, step_gate=0.001, width_gate=1e19), dict(class_left=0, class_right=7, min_hits=1)]
        for kw in good:
            assert call(**kw) == 3, kw
    for kw in (dict(first_gate=nan), dict(step_gate=0.0), dict(width_gate=2e19), dict(cos_turn=1.0), dict(min_hits=0), dict(max_chain=65),
               dict(class_left=3, class_right=3), dict(pose=with_value(ident, 3, inf)), dict(forward=(nan, 0.0, 0.0))):
        with pytest.raises(ValueError):
            boundary.check_params(boundary.params(**kw))
    boundary.check_params(boundary.params(pose=with_value(ident, 3, inf)), device_pose=True)


def test_layouts_and_the_header_stays_plain_c(pkg, tmp_path):
    from unina_yolo_dla_amd import boundary, engine
    P = engine.BoundaryParams
    assert C.sizeof(P) == 92 and (P.forward.offset, P.first_gate.offset, P.cos_turn.offset, P.class_left.offset, P.max_chain.offset) == (48, 60, 68, 76, 88)
    assert engine.BOUNDARY_POINT_DTYPE.itemsize == 16 and [engine.BOUNDARY_POINT_DTYPE.fields[n][1] for n in ("x", "y", "z", "ref")] == [0, 4, 8, 12]
    H = engine.BOUNDARY_HEADER_DTYPE
    assert H.itemsize == 32 and [H.fields[n][1] for n in ("n_candidates", "n_chain", "end", "n_centre", "n_wide")] == [0, 8, 16, 24, 28]
    assert (engine.BOUNDARY_NO_FIRST, engine.BOUNDARY_NO_NEXT, engine.BOUNDARY_FULL, engine.BOUNDARY_NO_HEADING) == (0, 1, 2, 3)
    assert engine.BOUNDARY_MAX_CHAIN == 64 and boundary.N_POINTS == 256 and boundary.TRACK_MAX == 1024
    assert "unina_boundary_async" in engine.ABI_SYMBOLS and hasattr(engine.load_library(), "unina_boundary_async")
    hostprog.assert_header_is_c99()
    hostprog.compile_c99(tmp_path, 'typedef char par92[(sizeof(unina_boundary_params) == 92) ? 1 : -1];\n'
                                   'typedef char fwd48[(offsetof(unina_boundary_params, forward) == 48) ? 1 : -1];\n'
                                   'typedef char gate60[(offsetof(unina_boundary_params, first_gate) == 60) ? 1 : -1];\n'
                                   'typedef char left76[(offsetof(unina_boundary_params, class_left) == 76) ? 1 : -1];\n'
                                   'typedef char point16[(sizeof(unina_boundary_point) == 16) ? 1 : -1];\n'
                                   'typedef char head32[(sizeof(unina_boundary_header) == 32) ? 1 : -1];\n'
                                   'typedef char end16[(offsetof(unina_boundary_header, end) == 16) ? 1 : -1];\n'
                                   'typedef char centre24[(offsetof(unina_boundary_header, n_centre) == 24) ? 1 : -1];\n'
                                   'typedef char codes[(UNINA_BOUNDARY_NO_FIRST == 0 && UNINA_BOUNDARY_NO_NEXT == 1 && UNINA_BOUNDARY_FULL == 2 &&\n'
                                   '                    UNINA_BOUNDARY_NO_HEADING == 3 && UNINA_BOUNDARY_MAX_CHAIN == 64) ? 1 : -1];\n'
                                   'int use(const GpuDetection *d, const int *n, unina_cone3d *c, unina_tracker_t *t, unina_pose_result *r,\n'
                                   '        unina_pose_header *h, unina_boundary_point *pts, unina_boundary_header *bh) {\n'
                                   '  unina_pose_params pp = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, 1.0f, 1, 3, 4, 3};\n'
                                   '  unina_track_params tp = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, 0.5f, 0.5f, 0.3f, 1, 3, 5};\n'
                                   '  unina_boundary_params bp = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {0, 0, 1}, 8.0f, 7.4f, 0.342f, 6.0f, 1, 0, 3,\n'
                                   '                              UNINA_BOUNDARY_MAX_CHAIN};\n'
                                   '  const unina_track *slots;\n'
                                   '  if (unina_track_buffers(t, &slots, 0)) return 1;\n'
                                   '  if (unina_pose_async(d, n, c, slots, r, &pp, c, r, h, 0)) return 2;\n'
                                   '  if (unina_track_update_async(t, d, n, c, &tp, 0, 0)) return 3;\n'
                                   '  return unina_boundary_async(slots, r, &bp, pts, bh, 0);\n}\n')


# ---------------------------------------------------------------- what the stage is for
def check_oval(c, r, n):
    """Both chains hold all n cones of their side in ring order in the direction of travel and end NO_NEXT."""
    h = head(r)
    assert h["cand"] == [n, n] and h["chain"] == [n, n] and h["end"] == [NO_NEXT, NO_NEXT], (c["name"], h)
    L, R, Cn = sides(r)
    assert (bc.ring_steps(L["ref"], 1, n) == 1).all() and (bc.ring_steps(R["ref"], 1001, n) == 1).all(), c["name"]
    o, fwd = np.asarray(c["params"]["pose"])[:2, 3], np.asarray(c["params"]["pose"])[:2, 0]
    for side in (L, R):                                                                      # it starts beside the vehicle, not behind it
        first = np.array([side["x"][0], side["y"][0]]) - o
        assert first @ fwd > -0.2 and np.linalg.norm(first) < 6.0, c["name"]
    return h, Cn


@pytest.mark.parametrize("seed", range(5))
def test_oval_track_both_limits_in_ring_order_and_the_centre_line_within_half_a_metre(pkg, seed):
    """An ellipse of 30 m x 15 m as the centre line, the limits 1.5 m to either side, 36 cones per side (one every 4 m of arc,
    sharing the lap evenly), 0.05 m noise, random slot order, 20 tracks of a third class; the vehicle on the centre line at three
    places a third of a lap apart. Measured on the twin over the 15 cases: the largest distance of a centre point from the true
    centre line is 0.23 .. 0.32 m (the chord's sagitta in the tight end plus the noise)."""
    line = bc.cached(("line", 30.0, 15.0), bc.oval_line)
    for start in (0.0, 1 / 3, 2 / 3):
        c, r, n = bc.oval_result(seed, start)
        assert n == 36
        h, Cn = check_oval(c, r, n)
        assert h["wide"] == 0 and h["centre"] == 2 * n - 1
        off = bc.centre_distance(line, np.stack([Cn["x"], Cn["y"]], axis=1)).max()
        print(f"seed {seed} start {start:.2f}: centre line off by at most {off:.3f} m")
        assert off <= 0.5


def test_other_ovals_and_a_lap_that_closes_with_a_longer_gap(pkg):
    """25 m x 10 m with a cone every 3 m and 40 m x 20 m with one every 5 m, step_gate = 1.6 * spacing + 1: ring order as well. With
    the cones of the 30 m x 15 m oval at exact multiples of 4 m the lap closes with a gap of 5.3 m: the chains are the same 36 in
    ring order, and the one rung that crosses the gap slantwise (3 m across, 5.3 m along: 6.0 .. 6.1 m) may exceed width_gate = 6 m."""
    for a, b, spacing in ((25.0, 10.0, 3.0), (40.0, 20.0, 5.0)):
        for seed in range(5):
            c, n = bc.oval_case(seed, seed / 5.0, a=a, b=b, spacing=spacing, step_gate=1.6 * spacing + 1.0)
            check_oval(c, bc.run_twin(c), n)
    for seed in range(5):
        c, n = bc.oval_case(seed, 1 / 3, even=False)
        h, _ = check_oval(c, bc.run_twin(c), n)
        assert h["wide"] <= 1 and h["centre"] + h["wide"] == 2 * n - 1


def test_the_drive_keeps_both_chains_in_ring_order(pkg):
    """12 frames along the oval through the three twins chained (pose -> tracker -> boundary): from the frame on in which the
    cones are confirmed both chains are in ring order and start beside the vehicle."""
    out = bc.drive_results()
    _, _, truth, n = bc.drive_inputs()
    assert head(out[0][2])["cand"] == [0, 0] and head(out[1][2])["end"] == [NO_FIRST, NO_FIRST]
    for k in range(2, len(out)):
        r, state = out[k][2], out[k][1]
        h = head(r)
        ids = {int(t["id"]): t for t in state["tracks"] if t["id"] != 0}
        assert min(h["chain"]) >= 4 and h["wide"] == 0 and h["centre"] == sum(h["chain"]) - 1, (k, h)
        for side, cls in zip(sides(r)[:2], (bc.LEFT, bc.RIGHT)):
            assert all(ids[int(ref)]["class_id"] == cls for ref in side["ref"])
            along = [bc_arc(p) for p in side]
            assert (np.diff(along) > 2.0).all() and (np.diff(along) < 6.5).all(), (k, along)    # ring order, no cone skipped


def bc_arc(p):
    """The arc length (counter-clockwise from (30, 0), the first quarter of the lap) of the centre-line point nearest to p."""
    s, pts, _, _ = bc.cached(("line", 30.0, 15.0), bc.oval_line)
    q = slice(0, len(s) // 4, 20)
    return float(s[q][((pts[q] - np.array([p["x"], p["y"]])) ** 2).sum(axis=1).argmin()])
