"""unina_fuse_async without a GPU: fusion.fuse_numpy (the definition) against an independent brute-force greedy and against the
rounds of mutual nearest neighbours csrc/fuse.hip computes, csrc/fuse_math.h compiled for the host (tests/fuse_math_host.cpp, also
under -fsanitize=address,undefined as the stand-alone program it is) against the numpy twin, the argument checks of the entry
point, the layouts in C, and what each constructed case of tests/fuse_cases.py contains.

unina_fuse_params is 100 bytes: twelve transform values, four pinhole values and nine scalars, 25 floats, as the header lists them
(a figure of 76 bytes cannot hold those fields)."""
import ctypes as C
import math
import struct
from types import SimpleNamespace as Fields

import numpy as np
import pytest

import fuse_cases as fc
import hostprog

F = np.float32
NAMES = ("header", "count", "dets", "cones", "links", "lidar_slot")


def r(v):
    """A python float rounded to fp32: a double holds the sum, difference, product or quotient of two fp32 values closely enough
    that rounding it to fp32 is the fp32 operation."""
    return float(F(v))


# ---------------------------------------------------------------- independent restatements of one call
def brute_pairs(c):
    """Every candidate pair as python tuples (d2, i, j), the usable cones' points and pixels, and the two counts: scalar loops, no
    vectorised arithmetic."""
    p = c["params"]
    m = [float(F(v)) for v in p["level_to_cam"]]
    fx, fy, cx, cy = (float(F(v)) for v in p["cam"])
    sx, sy, lift, grow, pad = (float(F(p[k])) for k in ("sx", "sy", "lift", "grow", "pad"))
    zmin, zmax, ra, rr = (float(F(p[k])) for k in ("min_depth", "max_depth", "range_abs", "range_rel"))
    nc = min(max(c["count"], 0), fc.MAXD, len(c["dets"]))
    nl = min(max(c["lcount"], 0), fc.MAXD, len(c["ldets"]))
    row = lambda k, x, y, z: r(r(r(r(m[k] * x) + r(m[k + 1] * y)) + r(m[k + 2] * z)) + m[k + 3])   # noqa: E731
    cones, pixels = {}, {}
    with np.errstate(all="ignore"):
        for j in range(nl):
            x, y, z = (float(c["lcones"][n][j]) for n in "xyz")
            zl = r(z + lift)
            q = (row(0, x, y, zl), row(4, x, y, zl), row(8, x, y, zl))
            if c["lcones"]["valid"][j] == 0 or not all(math.isfinite(v) for v in q):
                continue
            cones[j] = q
            if zmin <= q[2] <= zmax:
                pixels[j] = (r(r(r(fx * q[0]) / q[2]) + cx), r(r(r(fy * q[1]) / q[2]) + cy))
        pairs = []
        plist = sorted(pixels.items())
        for i in range(nc):
            d = c["dets"][i]
            X1, X2, Y1, Y2 = r(float(d["x1"]) * sx), r(float(d["x2"]) * sx), r(float(d["y1"]) * sy), r(float(d["y2"]) * sy)
            if not all(math.isfinite(v) for v in (X1, X2, Y1, Y2)) or X2 < X1 or Y2 < Y1:
                continue
            uc, vc = r(0.5 * r(X1 + X2)), r(0.5 * r(Y1 + Y2))
            hg = r(0.5 * grow)
            hw, hh = r(r(hg * r(X2 - X1)) + pad), r(r(hg * r(Y2 - Y1)) + pad)
            gated, cz = c["cones"]["valid"][i] != 0, float(c["cones"]["z"][i])
            for j, (u, v) in plist:
                du = r(u - uc)
                if not abs(du) <= hw:
                    continue
                dv = r(v - vc)
                if not abs(dv) <= hh:
                    continue
                zc = cones[j][2]
                if gated and not abs(r(zc - cz)) <= r(ra + r(rr * zc)):
                    continue
                pairs.append((r(r(du * du) + r(dv * dv)), i, j))
    return pairs, cones, pixels, nc, nl


def brute_force(c):
    """The definition restated: sort the tuples, greedy loop, then the records in plain python."""
    from unina_yolo_dla_amd import engine
    p = c["params"]
    pairs, cones, pixels, nc, nl = brute_pairs(c)
    lidar_of, camera_of = {}, {}
    for d2, i, j in sorted(pairs):
        if i not in lidar_of and j not in camera_of:
            lidar_of[i], camera_of[j] = (j, d2), i
    dets, out_cones = np.zeros(fc.MAXD, dtype=engine.DET_DTYPE), np.zeros(fc.MAXD, dtype=engine.CONE3D_DTYPE)
    links, slot = np.zeros(fc.MAXD, dtype=engine.FUSE_LINK_DTYPE), np.full(fc.MAXD, -1, dtype=np.int32)

    def cone_of(j):
        u, v = pixels.get(j, (0.0, 0.0))
        return (*cones[j], u, v, c["lcones"]["n_valid"][j], c["lcones"]["n_samples"][j], 1)

    for i in range(nc):
        dets[i] = c["dets"][i]
        if i in lidar_of:
            j, d2 = lidar_of[i]
            out_cones[i], links[i], slot[j] = cone_of(j), (i, j, d2, 1), i
        else:
            out_cones[i], links[i] = c["cones"][i], (i, -1, 0.0, 2)
    only = [j for j in sorted(cones) if j not in camera_of]
    written = nc
    for j in only:
        if written == fc.MAXD:
            break
        with np.errstate(all="ignore"):
            bx, by = (r(pixels[j][0] / float(F(p["sx"]))), r(pixels[j][1] / float(F(p["sy"])))) if j in pixels else (0.0, 0.0)
        dets[written] = (bx, by, bx, by, 0, c["ldets"]["class_id"][j], 1, 0)
        dets["confidence"][written:written + 1] = c["ldets"]["confidence"][j:j + 1]
        out_cones[written], links[written], slot[j] = cone_of(j), (-1, j, 0.0, 3), written
        written += 1
    header = np.zeros(1, dtype=engine.FUSE_HEADER_DTYPE)
    header[0] = (nc, nl, len(pixels), len(lidar_of), nc - len(lidar_of), len(only), written, len(only) - (written - nc))
    out = {"header": header, "count": np.array([written], dtype=np.int32), "dets": dets, "cones": out_cones, "links": links, "lidar_slot": slot}
    return out, {i: j for i, (j, _) in lidar_of.items()}, pairs


def mutual_rounds(pairs):
    """The kernel's association: rounds of mutual nearest neighbours over the free candidate pairs. Returns (camera record -> cone,
    number of rounds that matched something)."""
    lidar_of, camera_of, rounds = {}, {}, 0
    while True:
        free = [(d2, i, j) for d2, i, j in pairs if i not in lidar_of and j not in camera_of]
        if not free:
            return lidar_of, rounds
        best_cone, best_rec = {}, {}
        for d2, i, j in free:
            best_cone[i] = min(best_cone.get(i, (math.inf, 1 << 30)), (d2, j))       # the record's own minimum, a register
            best_rec[j] = min(best_rec.get(j, (math.inf, 1 << 30)), (d2, i))         # the list entry's 64-bit minimum
        for i, (d2, j) in best_cone.items():
            if best_rec[j] == (d2, i):
                lidar_of[i], camera_of[j] = j, i
        rounds += 1


def check_case(c, want):
    """Twin == brute force == mutual rounds; returns the number of rounds."""
    got, matched, pairs = brute_force(c)
    for name in NAMES:
        assert got[name].tobytes() == want[name].tobytes(), (c["name"], name, got["header"], want["header"])
    mutual, rounds = mutual_rounds(pairs)
    assert mutual == matched, c["name"]
    return rounds, pairs


def head(out):
    return {n: int(out["header"][n][0]) for n in out["header"].dtype.names}


@pytest.fixture(scope="module")
def edges(pkg):
    return {c["name"]: (c, out, *check_case(c, out)) for c, out in fc.cached("edges", fc.edge_cases)}


def test_twin_equals_brute_force_and_mutual_rounds_on_the_constructed_cases(edges):
    assert len(edges) == 42
    assert edges["chain64"][2] == 64 and edges["chain64_across_waves"][2] == 64          # one pair per round
    assert edges["grid_ties"][2] >= 2


def test_the_cases_are_what_they_claim(edges):
    h = {k: head(v[1]) for k, v in edges.items()}
    o = {k: v[1] for k, v in edges.items()}
    for c in (0, 1, 63, 64, 65, 1024, 5000, -7):
        n = min(max(c, 0), 1024)
        x = h[f"camera{c}"]
        assert (x["n_camera"], x["n_lidar"], x["n_projected"], x["n_matched"], x["n_lidar_only"]) == (n, 100, 100, min(n, 100), 100 - min(n, 100)), x
        assert x["n_written"] == min(n + x["n_lidar_only"], 1024) and x["n_dropped"] == 0 and x["n_camera_only"] == n - min(n, 100)
        x = h[f"lidar{c}"]
        assert (x["n_camera"], x["n_lidar"], x["n_projected"], x["n_matched"]) == (100, n, n, min(n, 100)), x
        assert x["n_written"] == max(n, 100) and x["n_dropped"] == 0 and x["n_lidar_only"] == max(n - 100, 0)
        assert not o[f"lidar{c}"]["dets"][x["n_written"]:].view(np.uint8).any() and (o[f"lidar{c}"]["lidar_slot"][n:] == -1).all()
    assert h["camera5000"] == h["camera1024"] and h["lidar5000"] == h["lidar1024"] and h["camera-7"] == h["camera0"]
    assert h["lidar1024"]["n_written"] == 1024 and (o["lidar1024"]["links"]["kind"] == np.r_[[1] * 100, [3] * 924]).all()
    assert o["lidar1024"]["lidar_slot"].tolist() == list(range(1024))
    assert (o["camera0"]["links"]["kind"][:100] == 3).all() and o["camera0"]["links"]["lidar"][:100].tolist() == list(range(100))
    assert all(v == 0 for v in h["both_empty"].values()) and not any(o["both_empty"][n].view(np.uint8).any() for n in ("dets", "cones", "links"))
    x = h["room_for_24"]
    assert (x["n_camera"], x["n_matched"], x["n_lidar_only"], x["n_written"], x["n_dropped"]) == (1000, 0, 100, 1024, 76)
    assert o["room_for_24"]["lidar_slot"][:100].tolist() == list(range(1000, 1024)) + [-1] * 76
    x = h["no_room"]
    assert (x["n_camera"], x["n_lidar_only"], x["n_written"], x["n_dropped"]) == (1024, 10, 1024, 10) and (o["no_room"]["lidar_slot"] == -1).all()
    x = h["all_lidar_invalid"]
    assert (x["n_projected"], x["n_matched"], x["n_lidar_only"], x["n_written"]) == (0, 0, 0, 10)
    x = h["non_finite_points"]
    assert (x["n_projected"], x["n_matched"], x["n_lidar_only"], x["n_written"]) == (4, 4, 0, 8)
    assert o["non_finite_points"]["lidar_slot"][:8].tolist() == [-1] * 4 + [4, 5, 6, 7]
    x = h["transform_overflows"]                    # 3e38 + 3e38 overflows: four cones unusable; the others land at u = inf
    assert (x["n_projected"], x["n_matched"], x["n_lidar_only"]) == (4, 0, 4) and np.isinf(o["transform_overflows"]["dets"]["x1"][8:12]).all()
    x = h["behind_the_camera"]
    assert (x["n_projected"], x["n_matched"], x["n_lidar_only"], x["n_written"]) == (2, 2, 2, 6)
    far = o["behind_the_camera"]
    assert all((far["dets"][n][4:6] == 0).all() for n in ("x1", "y1", "x2", "y2")) and (far["cones"]["z"][4:6] == -4).all()
    assert (far["cones"]["u"][4:6] == 0).all() and far["links"]["kind"][:6].tolist() == [2, 2, 1, 1, 3, 3]
    assert (h["depth_range_bounds"]["n_projected"], h["depth_range_bounds"]["n_lidar_only"]) == (2, 4)
    assert (o["depth_range_bounds"]["cones"]["u"][:4] != 0).tolist() == [True, False, True, False]
    for axis in "uv":
        assert h[f"border_{axis}_on"]["n_matched"] == 1 and h[f"border_{axis}_outside"]["n_matched"] == 0
        assert h[f"border_{axis}_outside"]["n_projected"] == 1
        assert o[f"border_{axis}_on"]["links"]["d2"][0] == 100.0
        near = o[f"border_{axis}_outside"]["cones"][axis][1]
        assert near == np.nextafter(F(300), F(np.inf)), near
    assert h["depth_gate_equal"]["n_matched"] == 1 and h["depth_gate_one_ulp_over"]["n_matched"] == 0
    assert o["depth_gate_one_ulp_over"]["cones"]["z"][1] == np.nextafter(F(4.5), F(np.inf))
    assert h["no_depth_no_gate"]["n_matched"] == 1 and h["nan_depth_fails_the_gate"]["n_matched"] == 0
    x = o["no_depth_no_gate"]
    assert x["cones"]["z"][0] == 4.5 and x["cones"]["valid"][0] == 1 and x["dets"]["class_id"][0] == 1 and x["links"][0].tolist() == (0, 0, 0.0, 1)
    x = h["inverted_and_nan_boxes"]
    assert (x["n_matched"], x["n_camera_only"], x["n_lidar_only"]) == (1, 4, 1) and o["inverted_and_nan_boxes"]["links"]["lidar"][:5].tolist() == [-1] * 4 + [0]
    assert edges["inverted_and_nan_boxes"][0]["dets"][:4].tobytes() == o["inverted_and_nan_boxes"]["dets"][:4].tobytes()
    assert h["centre_hit_only"]["n_matched"] == 1 and o["centre_hit_only"]["links"]["lidar"][:2].tolist() == [0, -1]
    pairs = edges["grid_ties"][3]
    assert len(pairs) == 4 * 49 + 2 * 2 * 7 + 1 and {p[0] for p in pairs} == {128.0} and h["grid_ties"]["n_matched"] == 64
    assert o["grid_ties"]["links"]["lidar"][:64].tolist() == list(range(64))     # (i, j) decides: record 9 could have 0, 1, 8 or 9; 0, 1 and 8 go to lower records
    assert o["one_cone_two_boxes"]["links"]["lidar"][:2].tolist() == [0, -1] and o["one_cone_two_boxes_depth"]["links"]["lidar"][:2].tolist() == [-1, 0]
    assert o["one_cone_two_boxes_depth"]["links"]["d2"][1] == 36.0 and o["one_cone_two_boxes"]["links"]["d2"][0] == 16.0
    x = o["two_cones_one_box"]
    assert x["links"][0].tolist() == (0, 1, 9.0, 1) and x["links"][1].tolist() == (-1, 0, 0.0, 3) and x["lidar_slot"][:2].tolist() == [1, 0]
    assert h["chain64"]["n_matched"] == 64 and o["chain64"]["links"]["lidar"][:64].tolist() == list(range(64))
    assert o["chain64_across_waves"]["links"]["lidar"][:96].tolist() == list(range(96))
    x = o["nan_confidence"]
    assert np.isnan(x["dets"]["confidence"][[0, 2, 4]]).all() and x["links"]["kind"][:6].tolist() == [1, 1, 2, 2, 3, 3]
    assert x["dets"]["class_id"][:6].tolist() == [1, 1, 1, 1, fc.UNKNOWN, fc.UNKNOWN] and x["dets"]["confidence"][5] == 0.5
    x = h["scaled_records"]
    assert (x["n_matched"], x["n_lidar_only"]) == (50, 10)
    s = o["scaled_records"]
    assert (s["dets"]["x1"][50:60] == s["cones"]["u"][50:60] / F(2.0)).all() and (s["dets"]["y2"][50:60] == s["cones"]["v"][50:60] / F(1.5)).all()


def test_twin_equals_brute_force_on_random_tie_heavy_inputs(pkg):
    """300 random configurations with integer-valued pixels and box corners (many bit-equal distances, shared pixels, depths on
    and off): the greedy loop, the sorted-tuple brute force and the mutual rounds agree, in at most a few rounds each."""
    rng = np.random.RandomState(3)
    worst = 0
    for trial in range(300):
        nc, nl = rng.randint(0, 25), rng.randint(0, 25)
        cu, cv = rng.randint(100, 130, nc) * 1.0, rng.randint(100, 120, nc) * 1.0
        half = rng.randint(0, 8, (nc, 1)) * 1.0
        boxes = np.concatenate([np.stack([cu, cv], axis=1) - half, np.stack([cu, cv], axis=1) + half], axis=1)
        depth = None if rng.rand() < 0.3 else np.where(rng.rand(nc) < 0.5, rng.choice([4.0, 4.5, 8.0], nc), np.nan)
        cam = fc.camera(boxes, depth=depth, cls=rng.randint(0, 3, nc))
        if depth is not None:
            cam[1]["valid"] = ~np.isnan(depth)
        z = rng.choice([4.0, 8.0], nl)
        pts = np.stack([fc.at_pixel(u, v, zz) for u, v, zz in zip(rng.randint(98, 134, nl), rng.randint(98, 124, nl), z)]) if nl else np.zeros((0, 3))
        c = fc.case(f"random{trial}", cam, fc.lidar(pts, valid=rng.randint(0, 5, nl) > 0), pad=float(rng.choice([0.0, 1.0, 3.0])),
                    grow=float(rng.choice([0.0, 1.0, 2.0])), range_abs=float(rng.choice([0.25, 0.5, 4.0])))
        worst = max(worst, check_case(c, fc.run_twin(c))[0])
    assert 2 <= worst <= 10


@pytest.fixture(scope="module")
def scenes(pkg):
    return fc.cached("scene", fc.scene_cases)


def joins(c, out):
    """(BOTH links, those that join records of one truth cone)."""
    both = out["links"][out["links"]["kind"] == 1]
    right = sum(1 for l in both if c["truth"][l["camera"]] >= 0 and c["truth"][l["camera"]] == c["ltruth"][l["lidar"]])
    return len(both), right


def test_scene_equals_brute_force_and_joins_the_right_records(scenes):
    """All three kinds of link; on the noise-free variant every BOTH link joins the two records of one cone. The share of correct
    joins of the noisy variants is printed, not bounded."""
    for c, out in scenes:
        rounds, _ = check_case(c, out)
        h = head(out)
        kinds = out["links"]["kind"][:h["n_written"]]
        assert {1, 2, 3} == set(kinds.tolist()) and rounds <= 4, (c["name"], h, rounds)
        print(c["name"], h)
        assert h["n_camera"] > 40 and h["n_lidar"] > 40 and h["n_matched"] > 15 and h["n_lidar_only"] > 20 and h["n_camera_only"] > 10
        n_both, right = joins(c, out)
        seen_by_both = len(set(c["truth"][c["truth"] >= 0]) & set(c["ltruth"][c["ltruth"] >= 0]))
        print(f"{c['name']}: {h}, rounds {rounds}, BOTH {n_both}, correct {right} ({100.0 * right / max(n_both, 1):.1f} %), seen by both {seen_by_both}")
        if c["name"].startswith("scene_exact"):
            assert right == n_both == seen_by_both
        matched = out["links"][:h["n_camera"]]
        i = np.nonzero(matched["kind"] == 1)[0]
        assert (out["dets"][i].tobytes() == c["dets"][i].tobytes()) and (out["cones"]["valid"][i] == 1).all()       # the camera's class, the LiDAR's point
        assert np.allclose(out["cones"]["z"][i], c["lcones"]["x"][matched["lidar"][i]], atol=1e-5)                  # zc is the level frame's x


# ---------------------------------------------------------------- csrc/fuse_math.h on the host
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("fuse_math_host")
    return hostprog.build_pair(d, "fuse_math_host.cpp"), d


def run_host(drivers, mode, words, float_cols):
    """Both builds on one input ([n, 24] uint32 words); the sanitised build must exit 0 and give the same words (a NaN in a float
    column is compared as a NaN: its sign differs between a folded constant and the FPU's result)."""
    def canon(g):
        assert g.size == 8 * len(words)
        g = g.reshape(-1, 8)
        for col in float_cols:
            g[np.isnan(g[:, col].view(np.float32)), col] = 0x7fc00000
        return g

    payload = struct.pack("<3i", 0x46555331, mode, len(words)) + np.ascontiguousarray(words, dtype=np.uint32).tobytes()
    return hostprog.run_pair(*drivers, payload, dtype=np.uint32, canon=canon)


SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, 0.25, 0.5, 1e-45, 1e-38, 3e38, -3e38, 3.4028235e38, np.inf, -np.inf, np.nan, 100.0, 0.1], dtype=np.float32)


def sweep(rng, n, k):
    """[n, k] fp32: specials, lattice values (ties) and random magnitudes mixed."""
    lattice = (rng.randint(-8, 9, (n, k)) * 0.25).astype(np.float32)
    wild = (rng.standard_normal((n, k)) * 10.0 ** rng.randint(-3, 4, (n, k))).astype(np.float32)
    pick = rng.randint(0, 4, (n, k))
    return np.where(pick == 0, SPECIAL[rng.randint(0, len(SPECIAL), (n, k))], np.where(pick == 1, wild, lattice)).astype(np.float32)


def same(got, want):
    """A column of float bits against the twin's values: equal bits, or both NaN."""
    ok = ~np.isnan(want)
    return (got[ok] == want.view(np.uint32)[ok]).all() and np.isnan(got[~ok].view(np.float32)).all()


def test_host_math_equals_the_twin_over_a_sweep(pkg, drivers):
    from unina_yolo_dla_amd import fusion
    rng = np.random.RandomState(6)
    n = 20000
    positive = lambda m: np.abs(sweep(rng, m, 1)[:, 0]) + F(0.125)      # noqa: E731
    with np.errstate(all="ignore"):
        # the point and the pixel
        w = np.zeros((n, 24), dtype=np.uint32)
        vals = sweep(rng, n, 22)
        vals[:, 17] = rng.choice(np.array([0.25, 0.5, 1.0], dtype=np.float32), n)                      # min_depth > 0
        vals[:, 18] = vals[:, 17] + np.abs(vals[:, 18])
        w[:, :22] = vals.view(np.uint32)
        w[:, 22] = rng.randint(-1, 2, n).astype(np.int32).view(np.uint32)
        got = run_host(drivers, 0, w, (0, 1, 2, 3, 4))
        # the twin reads its parameters as fields: a column of the sweep per field gives every row its own set
        p = Fields(level_to_cam=[vals[:, k] for k in range(12)], cam=Fields(fx=vals[:, 12], fy=vals[:, 13], cx=vals[:, 14], cy=vals[:, 15]),
                   lift=vals[:, 16], min_depth=vals[:, 17], max_depth=vals[:, 18])
        *floats, usable, projected = fusion.point_numpy(p, vals[:, 19], vals[:, 20], vals[:, 21], w[:, 22].view(np.int32))
        for col, want in enumerate(floats):
            assert same(got[:, col], want), col
        assert (got[:, 5] == usable).all() and (got[:, 6] == projected).all()
        assert 0.02 < usable.mean() < 0.9 and 0.01 < projected.mean() < usable.mean()
        # the box
        w = np.zeros((n, 24), dtype=np.uint32)
        vals = sweep(rng, n, 8)
        vals[:, 4], vals[:, 5] = positive(n), positive(n)
        w[:, :8] = vals.view(np.uint32)
        got = run_host(drivers, 1, w, (0, 1, 2, 3))
        p = Fields(sx=vals[:, 4], sy=vals[:, 5], grow=vals[:, 6], pad=vals[:, 7])
        *floats, boxed = fusion.box_numpy(p, vals[:, 0], vals[:, 1], vals[:, 2], vals[:, 3])
        for col, want in enumerate(floats):
            assert same(got[:, col], want), col
        assert (got[:, 4] == boxed).all() and 0.05 < boxed.mean() < 0.95
        # the gated pair and its key
        w = np.zeros((n, 24), dtype=np.uint32)
        vals = sweep(rng, n, 11)
        vals[:, 5:7] = np.abs(vals[:, 5:7])
        has_depth = rng.randint(0, 2, n)
        ra, rr = rng.choice(np.array([0.0, 0.25, 0.5, 2.0], dtype=np.float32), n), rng.choice(np.array([0.0, 0.125, 0.1], dtype=np.float32), n)
        vals[:, 9], vals[:, 10] = ra, rr
        idx = rng.randint(0, 1024, n).astype(np.uint32)
        w[:, :7], w[:, 7], w[:, 8:11], w[:, 11] = vals[:, :7].view(np.uint32), has_depth, vals[:, 8:11].view(np.uint32), idx
        got = run_host(drivers, 2, w, (0, 3))
        cand, d2 = fusion.candidate_numpy(Fields(range_abs=ra, range_rel=rr), *[vals[:, k] for k in range(7)], has_depth != 0, vals[:, 8])
        assert same(got[:, 0], d2) and (got[:, 1] == cand).all() and 0.01 < cand.mean() < 0.9
        assert (got[:, 2] == idx).all() and (got[:, 3] == got[:, 0]).all()
        ok = cand
        assert not (d2[ok].view(np.uint32) >> 31).any() and not np.isnan(d2[ok]).any()          # never negative, never NaN: the bits order
        order = np.argsort(d2[ok].view(np.uint32), kind="stable")
        assert (d2[ok][order][1:] >= d2[ok][order][:-1]).all() and (np.diff(d2[ok].view(np.uint32)[order]) == 0).sum() > 100     # and ties exist
        # the output expressions
        w = np.zeros((n, 24), dtype=np.uint32)
        vals = sweep(rng, n, 2)
        vals[:, 1] = positive(n)
        ints = np.stack([rng.randint(0, 1025, n), rng.choice([0, 1, 23, 24, 25, 1024, 5000], n), np.full(n, 1024)], axis=1)
        w[:, :2], w[:, 2:5] = vals.view(np.uint32), ints.astype(np.uint32)
        got = run_host(drivers, 3, w, (0,))
        assert same(got[:, 0], vals[:, 0] / vals[:, 1])
        assert (got[:, 1] == np.minimum(ints[:, 0] + ints[:, 1], 1024)).all()


# ---------------------------------------------------------------- the entry point's argument checks
def test_every_bad_argument_is_refused_before_any_hip_call(pkg):
    """UNINA_ERR_ARG (4) for each refusal the header lists, in a process that has no device: a HIP call in front of the checks
    would answer 3 (UNINA_ERR_HIP) instead. The pointers are never dereferenced by a refused call."""
    from unina_yolo_dla_amd import build, engine, fusion
    build.build_native()
    L = engine.load_library()
    nan, inf = float("nan"), float("inf")
    names = ("dets", "count", "cones", "ldets", "lcount", "lcones", "out_dets", "out_count", "out_cones", "links", "slot", "header")
    good = {n: 0x100000 * (k + 1) for k, n in enumerate(names)}                    # 1 MiB apart: nothing overlaps
    aligned16 = ("dets", "cones", "ldets", "lcones", "out_dets", "out_cones", "links", "header")

    def call(par=True, m=fc.IDENTITY, cam=fc.CAM, **kw):
        a = dict(good)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        p = dict(sx=1.0, sy=1.0, lift=0.15, min_depth=0.3, max_depth=40.0, grow=1.0, pad=4.0, range_abs=0.5, range_rel=0.1)
        p.update(kw)
        pp = fusion.make_fuse_params(m, cam, **p)
        return L.unina_fuse_async(a["dets"], a["count"], a["cones"], a["ldets"], a["lcount"], a["lcones"], C.byref(pp) if par else None,
                                  a["out_dets"], a["out_count"], a["out_cones"], a["links"], a["slot"], a["header"], None)

    def with_value(values, i, v):
        q = list(values)
        q[i] = v
        return q

    bad = [dict(par=False), *[{n: None} for n in names if n != "slot"],
           *[{n: good[n] + off} for n in aligned16 for off in (4, 8)], *[{n: good[n] + off} for n in ("count", "lcount", "out_count", "slot") for off in (1, 2)],
           *[dict(m=with_value(fc.IDENTITY, i, v)) for i in range(12) for v in (nan, inf, -inf)],
           *[dict(cam=with_value(fc.CAM, i, v)) for i in range(4) for v in (nan, inf, -inf)], dict(cam=with_value(fc.CAM, 0, 0.0)),
           dict(cam=with_value(fc.CAM, 1, -0.0)),
           *[{k: v} for k in ("sx", "sy", "min_depth") for v in (0.0, -1.0, nan, inf)], *[dict(lift=v) for v in (nan, inf, -inf)],
           *[dict(max_depth=v) for v in (nan, inf, 0.2)],
           *[{k: v} for k in ("grow", "pad", "range_abs", "range_rel") for v in (-0.5, nan, inf, -inf)]]
    # every output against every input and every other output: the same base, and an overlap of the last / first bytes
    size = dict(dets=32768, count=4, cones=32768, ldets=32768, lcount=4, lcones=32768, out_dets=32768, out_count=4, out_cones=32768,
                links=16384, slot=4096, header=32)
    outputs = names[6:]
    for o in outputs:
        for other in names:
            if other == o:
                continue
            if other in outputs and outputs.index(other) < outputs.index(o):
                continue
            bad.append({o: good[other]})
            bad.append({o: good[other] + size[other] - 16} if size[other] >= 32 else {other: good[o] + size[o] - (16 if other in aligned16 else 4)})
    for kw in bad:
        assert call(**kw) == 4, kw
    import torch
    if not torch.cuda.is_available():
        # the good calls reach HIP, which has no device here: the checks above sit in front of it
        assert call() == 3 and call(slot=None) == 3 and call(grow=0.0, pad=0.0, range_abs=0.0, range_rel=0.0, max_depth=0.3, lift=-0.5) == 3
        assert call(out_count=good["out_dets"] - 32) == 3                  # Engine.infer_async's layout: the count 32 bytes in front of the records


def test_layouts_and_the_header_stays_plain_c(pkg, tmp_path):
    from unina_yolo_dla_amd import engine, fusion
    assert [fusion.FUSE_LINK_DTYPE.fields[n][1] for n in ("camera", "lidar", "d2", "kind")] == [0, 4, 8, 12]
    assert [fusion.FUSE_HEADER_DTYPE.fields[n][1] for n in ("n_camera", "n_lidar", "n_projected", "n_matched", "n_camera_only", "n_lidar_only",
                                                             "n_written", "n_dropped")] == list(range(0, 32, 4))
    assert fusion.FUSE_LINK_DTYPE.itemsize == 16 and fusion.FUSE_HEADER_DTYPE.itemsize == 32
    assert C.sizeof(engine.FuseParams) == 100 and engine.FuseParams.cam.offset == 48 and engine.FuseParams.sx.offset == 64
    assert engine.FuseParams.range_rel.offset == 96
    assert (engine.FUSE_BOTH, engine.FUSE_CAMERA, engine.FUSE_LIDAR) == (1, 2, 3) and "unina_fuse_async" in engine.ABI_SYMBOLS
    hostprog.assert_header_is_c99()
    hostprog.compile_c99(tmp_path, 'typedef char par100[(sizeof(unina_fuse_params) == 100) ? 1 : -1];\n'
                                   'typedef char cam48[(offsetof(unina_fuse_params, cam) == 48) ? 1 : -1];\n'
                                   'typedef char lift72[(offsetof(unina_fuse_params, lift) == 72) ? 1 : -1];\n'
                                   'typedef char rel96[(offsetof(unina_fuse_params, range_rel) == 96) ? 1 : -1];\n'
                                   'typedef char link16[(sizeof(unina_fuse_link) == 16) ? 1 : -1];\n'
                                   'typedef char d2at8[(offsetof(unina_fuse_link, d2) == 8) ? 1 : -1];\n'
                                   'typedef char head32[(sizeof(unina_fuse_header) == 32) ? 1 : -1];\n'
                                   'typedef char dropped28[(offsetof(unina_fuse_header, n_dropped) == 28) ? 1 : -1];\n'
                                   'typedef char kinds[(UNINA_FUSE_BOTH == 1 && UNINA_FUSE_CAMERA == 2 && UNINA_FUSE_LIDAR == 3) ? 1 : -1];\n'
                                   'int use(const GpuDetection *d, const int *n, const unina_cone3d *c, GpuDetection *od, int *on, unina_cone3d *oc,\n'
                                   '        unina_fuse_link *l, int *slot, unina_fuse_header *h) {\n'
                                   '  unina_fuse_params p = {{0, -1, 0, 0, 0, 0, -1, 1, 1, 0, 0, 0}, {600, 600, 640, 360}, 1, 1, 0.15f, 0.5f, 40, 1, 4, 0.5f, 0.1f};\n'
                                   '  return unina_fuse_async(d, n, c, d, n, c, &p, od, on, oc, l, slot, h, 0);\n}\n')


def test_level_to_camera_of_a_known_pair(pkg):
    """The LiDAR 0.8 m above the level frame's origin and yawed by 90 degrees; the camera 0.2 m in front of and 0.1 m above the
    LiDAR, looking along the LiDAR's x. A level point is carried to the optical frame as the two extrinsics say."""
    from unina_yolo_dla_amd import fusion
    lidar_to_level = [0, -1, 0, 0.0, 1, 0, 0, 0.0, 0, 0, 1, 0.8]                   # level = Rz(90) * lidar + (0, 0, 0.8)
    lidar_to_cam = [0, -1, 0, 0.0, 0, 0, -1, 0.1, 1, 0, 0, -0.2]                   # optical x = -y, y = -z + 0.1, z = x - 0.2
    m = fusion.level_to_camera(lidar_to_level, lidar_to_cam)
    assert m.dtype == np.float32 and m.shape == (12,)
    # lidar = Rz(-90) * (level - t): lidar x = level y, lidar y = -level x, lidar z = level z - 0.8
    want = [1, 0, 0, 0.0, 0, 0, -1, 0.9, 0, 1, 0, -0.2]
    assert np.allclose(m, want, atol=1e-7) and m.tolist() == [float(F(v)) for v in want]
    rng = np.random.RandomState(1)
    a, b = rng.standard_normal((3, 3)), rng.standard_normal((3, 3))
    ra, rb = np.linalg.qr(a)[0], np.linalg.qr(b)[0]
    ta, tb = rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3)
    m = fusion.level_to_camera(np.concatenate([ra, ta[:, None]], axis=1), np.concatenate([rb, tb[:, None]], axis=1)).astype(np.float64).reshape(3, 4)
    p = rng.uniform(-5, 5, (20, 3))                                                 # points of the LiDAR frame
    level, cam = p @ ra.T + ta, p @ rb.T + tb
    assert np.abs(level @ m[:, :3].T + m[:, 3] - cam).max() < 1e-5
    assert fusion.level_to_camera(fc.IDENTITY, fc.LEVEL_TO_CAM).tolist() == list(fc.LEVEL_TO_CAM)
