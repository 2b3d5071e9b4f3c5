"""unina_locate_stereo_async without a GPU: localize.locate_stereo_numpy (the definition) on scenes whose answer is known by
construction, on rejections and on boundaries built so that equality occurs; csrc/stereo_match.h compiled for the host
(tests/stereo_match_host.cpp, also under -fsanitize=address,undefined as the stand-alone program it is) against the numpy
twin; the argument checks of the entry point; the record layouts in C."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import hostprog
import stereo_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def twin(c):
    from unina_yolo_dla_amd import localize
    return localize.locate_stereo_numpy(c["dets"], c["count"], c["left"], c["right"], c["cam"], c["baseline"], c["params"])


def brute_costs(c, i):
    """cost(d) of record i with python loops over the sampled pixels: {d: cost}, d over the record's range."""
    from unina_yolo_dla_amd import localize
    p = c["params"]
    h, w = c["left"].shape
    d = c["dets"][i]
    win = localize.window_numpy((d["x1"], d["y1"], d["x2"], d["y2"]), p["sx"], p["sy"], p["shrink"], w, h, p["max_side"])
    _, d_lo, d_hi_all = localize.stereo_range_numpy(c["cam"][0], c["baseline"], p["min_depth"], p["max_depth"], w)
    out = {}
    for dd in range(d_lo, min(d_hi_all, win["u0"]) + 1):
        out[dd] = sum(abs(int(c["left"][v, u]) - int(c["right"][v, u - dd]))
                      for v in range(win["v0"], win["v1"] + 1, win["stride_y"]) for u in range(win["u0"], win["u1"] + 1, win["stride_x"]))
    return out


# ---------------------------------------------------------------- scenes whose answer is known
def test_integer_shifts_are_found_exactly(pkg):
    """Every window inside one rectangle: d_best is the rectangle's disparity, the cost there is 0, the record is valid, the
    refined disparity is within half a pixel, and z is fxB / disparity to the bit."""
    c, truth = sc.integer_case()
    cones, m = twin(c)
    n = len(truth)
    assert n == 48 and (m["d_best"][:n] == truth).all() and (m["cost_best"][:n] == 0).all() and (cones["valid"][:n] == 1).all()
    assert (np.abs(m["disparity"][:n] - truth) <= 0.5).all()
    fxB = F(c["cam"][0]) * F(c["baseline"])
    assert (fxB / m["disparity"][:n]).astype(np.float32).tobytes() == cones["z"][:n].tobytes()
    assert (cones["n_valid"][:n] == np.minimum(70, np.floor(c["dets"]["x1"])).astype(int)).all()      # d_lo = 1, d_hi = min(70, u0)
    assert not cones[n:].view(np.uint8).any() and not m[n:].view(np.uint8).any()


def test_costs_equal_a_pixel_loop(pkg):
    """The vectorised costs of the twin against a loop over the sampled pixels: unstrided, strided on one axis and on both,
    clipped at the image's edge."""
    from unina_yolo_dla_amd import localize
    left, right = sc.integer_scene()
    rows = [sc.cell(70, 18, 9, 7), sc.cell(63, 17, 31, 8), sc.cell(64, 16, 7, 14), sc.cell(63, 16, 31, 14), (80.5, 40.5, 120.0, 75.0), sc.cell(5, 5, 3, 3)]
    c = sc.case("loop", sc.boxes(rows), left, right, max_side=8)
    cones, m = twin(c)
    for i in range(len(rows)):
        want = brute_costs(c, i)
        assert len(want) == cones["n_valid"][i] > 0
        best = min(want.items(), key=lambda kv: (kv[1], kv[0]))
        far = [v for d, v in want.items() if abs(d - best[0]) > 1]
        assert (m["d_best"][i], m["cost_best"][i]) == best and m["cost_second"][i] == (min(far) if far else sc.NONE)
    p = c["params"]
    w = localize.window_numpy(rows[3], 1.0, 1.0, 1.0, sc.W, sc.H, 8)
    assert (w["stride_x"], w["stride_y"]) == (4, 2)
    assert localize.stereo_costs_numpy(left, right, w, 1, 63).tolist() == list(brute_costs(c, 3).values()) and p["max_side"] == 8


def test_fractional_shifts_land_beside_the_truth(pkg):
    """200 windows of 3 .. 30 px on planes at fractional disparities 3 .. 90 (a smoothed texture, the right image interpolated
    linearly, -2 .. +2 grey levels of noise): all valid, and |disparity - true| <= 0.5, which holds exactly when the integer
    minimum is one of the two integers beside the truth -- a condition on the matcher, not a measured tolerance. The worst error is
    printed and kept in profiles/r04/stereo_subpixel.txt (0.238 px)."""
    worst, n_total = 0.0, 0
    for c, true in sc.fractional_cases():
        cones, m = twin(c)
        n = c["count"]
        assert (cones["valid"][:n] == 1).all(), c["name"]
        err = np.abs(m["disparity"][:n].astype(np.float64) - true)
        assert (err <= 0.5).all(), (c["name"], err.max())
        assert (np.abs(m["d_best"][:n] - true) < 1).all()
        worst, n_total = max(worst, float(err.max())), n_total + n
    assert n_total == 200
    print(f"stereo sub-pixel: {n_total} records, worst |disparity - true| = {worst:.4f} px")
    stored = open(os.path.join(ROOT, "profiles", "r04", "stereo_subpixel.txt")).read()
    assert f"{worst:.4f}" in stored


# ---------------------------------------------------------------- rejections
def test_rejections(pkg):
    cones, m = twin(sc.flat_case())                      # all costs equal: the second best ties the best
    assert (cones["valid"][:2] == 0).all() and (cones["n_samples"][:2] == [81, 900]).all()
    assert (m["cost_best"][:2] == 0).all() and (m["cost_second"][:2] == 0).all() and (m["d_best"][:2] == 1).all()
    assert (cones["z"][:2] == 0).all() and (m["disparity"][:2] == 0).all() and (cones["u"][:2] == [74.5, 55.0]).all()
    cones, m = twin(sc.periodic_case())                  # minima at 3, 11, 19, ...: two separated disparities tie
    assert (cones["valid"][:2] == 0).all() and (m["d_best"][:2] == 3).all() and (m["cost_best"][:2] == 0).all() and (m["cost_second"][:2] == 0).all()
    cones, m = twin(sc.outside_case())
    assert not cones[:4].view(np.uint8).any() and not m[:4].view(np.uint8).any()                 # off the map, NaN, inverted: empty
    assert cones["n_samples"][4] == 16 and cones["n_valid"][4] == 0 and cones["valid"][4] == 0   # u0 = 0 < d_lo = 1: nd == 0
    assert m[4].tolist() == (0.0, 0, sc.NONE, sc.NONE) and cones["u"][4] == 2.0
    assert cones["valid"][5] == 1 and m["d_best"][5] == 12
    # a legal range that holds nothing: d_hi_all < d_lo
    c = sc.case("no_range", sc.boxes([sc.cell(70, 20, 5, 5)]), *sc.integer_scene(), min_depth=38.0, max_depth=39.0)   # fxB / 38 < 1
    cones, m = twin(c)
    assert cones["n_valid"][0] == 0 and cones["n_samples"][0] == 25 and m[0].tolist() == (0.0, 0, sc.NONE, sc.NONE)


# ---------------------------------------------------------------- boundaries, built so that equality occurs
def test_boundaries(pkg):
    """One-column windows, so that every cost is a chosen number: cost_best at max_mean_sad * n_samples and one above;
    cost_second * 100 at cost_best * (100 + uniqueness) and one grey level more; the best at d_lo, at d_hi and at u0; equal
    bests at two adjacent disparities and at two separated ones; ranges of 0, 1, 2 and 3 disparities."""
    fxB = F(sc.CAM[0]) * F(sc.BASELINE)
    for name, (c, want) in sc.boundary_cases().items():
        cones, m = twin(c)
        got = dict(valid=cones["valid"][0], d_best=m["d_best"][0], cost_best=m["cost_best"][0], cost_second=m["cost_second"][0],
                   disparity=m["disparity"][0], n_valid=cones["n_valid"][0])
        for k, v in want.items():
            assert got[k] == (F(v) if k == "disparity" else v), (name, k, got[k], v)
        assert cones["n_samples"][0] == 10
        if got["valid"]:
            assert cones["z"][0] == fxB / got["disparity"] and abs(got["disparity"] - got["d_best"]) <= 0.5
        else:
            assert got["disparity"] == 0 and cones["x"][0] == cones["y"][0] == cones["z"][0] == 0
    assert len(sc.boundary_cases()) >= 25


def test_maximal_cost_and_the_last_index(pkg):
    """64 x 64 samples of |255 - 0| against 1024 disparities: every cost is 4096 * 255 and the first disparity is the best; with
    one right pixel raised, the best is the LAST disparity at 4096 * 255 - 1: the key (cost << 10 | 1023) still orders."""
    from unina_yolo_dla_amd import localize
    big = 4096 * 255
    for dent, want in ((0, (0, 1, big, big, 0.0)), (1, (1, 1024, big - 1, big, 1024.0))):
        c = sc.wide_case("max", [sc.cell(1100, 8, 64, 64)], scene=sc.max_cost_scene(dent), max_mean_sad=255, uniqueness=0)
        assert localize.stereo_range_numpy(700.0, 0.5, c["params"]["min_depth"], 400.0, sc.WIDE_W)[1:] == (1, 1024)
        cones, m = twin(c)
        assert (cones["valid"][0], m["d_best"][0], m["cost_best"][0], m["cost_second"][0], m["disparity"][0]) == want
        assert cones["n_samples"][0] == 4096 and cones["n_valid"][0] == 1024
    assert (big << 10 | 1023) < 2 ** 32


# ---------------------------------------------------------------- csrc/stereo_match.h on the host
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("stereo_match_host")
    return hostprog.build_pair(d, "stereo_match_host.cpp"), d


def run_host(drivers, payload, n_words):
    got = hostprog.run_pair(*drivers, payload)
    assert got.size == n_words
    return got


def test_host_range_equals_the_twin_over_a_sweep(pkg, drivers):
    """fx * baseline from tiny to overflowing, depths whose quotients fall on and beside integers, widths 1 .. 2^24: the same
    (fxB, d_lo, d_hi_all), and a refusal exactly where the twin raises."""
    from unina_yolo_dla_amd import localize
    cases = []
    for width in (1, 2, 97, 1300, 1920, 1 << 24):
        for fx in (0.5, 70.0, 700.0, 1400.0, 3e4, 1e30):
            for baseline in (1e-3, 0.12, 0.5, 1.0, 1e9):
                for lo, hi in ((0.3, 40.0), (0.5, 0.75), (1.0, 35.0), (35.0, 70.0), (1e-30, 1.0), (350 / 1024.5, 400.0), (350 / 1025.5, 400.0),
                               (0.34, 0.35), (2.0, 3e38), (1e-42, 1e-40)):
                    cases.append((fx, baseline, lo, hi, width))
    payload = struct.pack("<3i", 0x53544d31, 0, len(cases)) + b"".join(struct.pack("<4fi", *c) for c in cases)
    got = run_host(drivers, payload, 4 * len(cases)).reshape(-1, 4)
    n_ok = n_refused = n_nothing = 0
    for c, g in zip(cases, got):
        try:
            fxB, d_lo, d_hi_all = localize.stereo_range_numpy(*c)
        except ValueError:
            assert g[0] in (1, 2), c
            n_refused += 1
            continue
        assert g.tolist() == [0, int(np.array(fxB).view(np.int32)), d_lo, d_hi_all], c
        assert 1 <= d_lo and d_hi_all <= c[4] - 1 and d_hi_all - d_lo + 1 <= 1024
        n_ok += 1
        n_nothing += d_hi_all < d_lo
    assert n_ok > 500 and n_refused > 100 and n_nothing > 100


def test_host_match_functions_equal_the_twin_over_a_table(pkg, drivers):
    """The packed key, the acceptance test (both inequalities at, one below and one above equality, with products past 2^32), the
    sub-pixel step (den == 0, which a whole record cannot reach because the smaller of two equal neighbours wins; the ends of the
    range; cm - cp = +-den) and the point, on a table written by the twin's own functions."""
    from unina_yolo_dla_amd import localize
    rng = np.random.RandomState(8)
    big = 4096 * 255
    rows = []
    for n_samples, sad, uniq, best in ((10, 20, 10, 200), (10, 20, 10, 201), (4096, 255, 1000, big), (4096, 255, 0, big), (4096, 254, 0, big),
                                       (1, 0, 0, 0), (1, 0, 0, 1), (64, 20, 10, 100), (4096, 200, 999, 819200)):
        for second in (sc.NONE, best, best + 1, best * (100 + uniq) // 100, best * (100 + uniq) // 100 + 1, big):
            for nd in (0, 1, 5):
                rows.append((n_samples, sad, uniq, nd, 1, 70, 30, best, second, best, best))
    for d_best, d_lo, d_hi in ((30, 1, 70), (1, 1, 70), (70, 1, 70), (5, 5, 5), (1023 + 7, 7, 1023 + 7), (1024, 1, 1024)):
        for c0, cm, cp in ((10, 10, 10), (10, 40, 20), (10, 11, 12), (10, 10, 500), (10, 500, 10), (0, 1, 0), (0, 0, 1), (big - 2, big, big - 1),
                           (0, big, big), (0, big, 0), (7, 8, 8)):
            rows.append((64, 255, 0, d_hi - d_lo + 1, d_lo, d_hi, d_best, c0, sc.NONE, cm, cp))
    for _ in range(300):
        c0 = int(rng.randint(0, big))
        d_lo = int(rng.randint(1, 50))
        d_hi = d_lo + int(rng.randint(0, 1024))
        rows.append((int(rng.randint(1, 4097)), int(rng.randint(0, 256)), int(rng.randint(0, 1001)), d_hi - d_lo + 1, d_lo, d_hi,
                     int(rng.randint(d_lo, d_hi + 1)), c0, int(rng.randint(c0, big + 1)), int(rng.randint(c0, big + 1)), int(rng.randint(c0, big + 1))))
    cams = [(F(35.0), F(48.5), F(30.25), F(70.0), F(71.5), F(48.25), F(30.5)), (F(350.0), F(1132.0), F(40.0), F(700.0), F(700.0), F(650.0), F(40.0)),
            (F(0.06), F(3.125), F(900.5), F(1400.0), F(1399.0), F(959.5), F(539.5))]
    payload = struct.pack("<3i", 0x53544d31, 1, len(rows))
    for i, r in enumerate(rows):
        payload += struct.pack("<7i4I7f", *r, *cams[i % 3])
    got = run_host(drivers, payload, 8 * len(rows)).reshape(-1, 8)
    n_accept = n_refined = 0
    for i, (r, g) in enumerate(zip(rows, got)):
        n_samples, sad, uniq, nd, d_lo, d_hi, d_best, c0, second, cm, cp = r
        key = (c0 << 10) | (d_best - d_lo)
        assert key < 2 ** 32 and int(g[0]) & 0xFFFFFFFF == key and (g[1], g[2]) == (c0, d_best - d_lo), r
        ok = localize.stereo_accept_numpy(nd, c0, second, n_samples, sad, uniq)
        assert bool(g[3]) == ok, r
        with np.errstate(all="ignore"):
            disparity = localize.stereo_disparity_numpy(d_best, d_lo, d_hi, cm, c0, cp)
            point = localize.stereo_point_numpy(cams[i % 3][0], disparity, *cams[i % 3][1:])
        assert g[4:].tobytes() == np.array([disparity, *point], dtype=np.float32).tobytes(), r
        assert abs(float(disparity) - d_best) <= 0.5 and (d_lo < d_best < d_hi or disparity == d_best)
        n_accept += ok
        n_refined += disparity != d_best
    assert 50 < n_accept < len(rows) - 50 and n_refined > 100
    assert localize.stereo_disparity_numpy(30, 1, 70, 10, 10, 10) == 30 and localize.stereo_disparity_numpy(30, 1, 70, 500, 10, 10) == 30.5


# ---------------------------------------------------------------- the entry point's argument checks
def test_every_bad_argument_is_refused_before_any_hip_call(pkg):
    """UNINA_ERR_ARG (4) for each refusal the header lists, in a process that has no device: a HIP call in front of the checks
    would answer 3 (UNINA_ERR_HIP) instead. The pointers are never dereferenced by a refused call."""
    from unina_yolo_dla_amd import build, engine
    build.build_native()
    L = engine.load_library()
    nan, inf = float("nan"), float("inf")
    DETS, COUNT, LEFT, RIGHT, OUT, MATCH = 0x10000, 0x20000, 0x30001, 0x40003, 0x50000, 0x60000

    def call(dets=DETS, count=COUNT, out=OUT, match=MATCH, pair=True, cam=True, par=True, baseline=0.5, **kw):
        s = dict(width=97, height=61, pitch=97, left=LEFT, right=RIGHT)
        c = dict(fx=70.0, fy=70.0, cx=48.0, cy=30.0)
        p = dict(sx=1.0, sy=1.0, shrink=0.5, min_depth=0.5, max_depth=40.0, max_side=64, max_mean_sad=20, uniqueness=10)
        for k, v in kw.items():
            next(t for t in (s, c, p) if k in t)[k] = v
        ss, cc, pp = engine.StereoPair(**s), engine.Pinhole(**c), engine.StereoParams(**p)
        return L.unina_locate_stereo_async(dets, count, C.byref(ss) if pair else None, C.byref(cc) if cam else None, baseline,
                                           C.byref(pp) if par else None, out, match, None)

    bad = [dict(dets=None), dict(count=None), dict(out=None), dict(pair=False), dict(cam=False), dict(par=False), dict(left=None), dict(right=None),
           dict(out=OUT + 8), dict(dets=DETS + 4), dict(match=MATCH + 8), dict(match=MATCH + 4), dict(count=COUNT + 2),
           dict(width=0), dict(height=0), dict(width=-5), dict(height=-1), dict(width=(1 << 24) + 1, pitch=1 << 25), dict(height=(1 << 24) + 1),
           dict(pitch=96), dict(pitch=0), dict(pitch=-97),
           *[{k: v} for k in ("fx", "fy", "baseline", "sx", "sy") for v in (0.0, -1.0, nan, inf)],
           *[{k: v} for k in ("cx", "cy") for v in (nan, inf, -inf)],
           dict(fx=3e38, baseline=3.0),                                  # fxB overflows
           dict(fx=3e30, baseline=1.0, min_depth=1e-30, max_depth=1.0),  # fxB / min_depth overflows
           dict(shrink=0.0), dict(shrink=-0.5), dict(shrink=1.0001), dict(shrink=nan),
           dict(max_side=0), dict(max_side=65), dict(max_side=256), dict(max_side=-1),
           dict(max_mean_sad=-1), dict(max_mean_sad=256), dict(uniqueness=-1), dict(uniqueness=1001),
           dict(min_depth=0.0), dict(min_depth=-1.0), dict(min_depth=nan), dict(min_depth=40.0), dict(min_depth=50.0),
           dict(max_depth=inf), dict(max_depth=nan),
           dict(width=1300, pitch=1300, fx=700.0, min_depth=350 / 1025.5, max_depth=400.0),        # 1025 disparities
           dict(width=4000, pitch=4000, fx=1400.0, baseline=1.0, min_depth=0.5, max_depth=1.4)]    # 1000 .. 2800
    for kw in bad:
        assert call(**kw) == 4, kw
    import torch
    if not torch.cuda.is_available():
        # good calls reach HIP, which has no device here: the checks above sit in front of it
        assert call() == 3 and call(match=None) == 3
        assert call(width=1300, pitch=1301, fx=700.0, min_depth=350 / 1024.5, max_depth=400.0) == 3                # exactly 1024 disparities
        assert call(min_depth=38.0, max_depth=39.0) == 3 and call(max_side=1, max_mean_sad=0, uniqueness=1000) == 3  # an empty range is legal


def test_twin_refuses_what_the_entry_point_refuses(pkg):
    left, right = sc.integer_scene()
    dets = sc.boxes([sc.cell(70, 20, 5, 5)])
    for kw in (dict(max_side=65), dict(max_side=0)):
        with pytest.raises(ValueError):
            twin(sc.case("refused", dets, left, right, **kw))
    with pytest.raises(ValueError, match="1025 disparities"):
        twin(sc.wide_case("refused", [sc.cell(1100, 8, 4, 4)], min_depth=350 / 1025.5))
    # a nearer min_depth than the image can show is not an error: d_hi_all is clipped to width - 1, d_hi to u0
    assert twin(sc.case("near", dets, left, right, min_depth=0.03))[0]["n_valid"][0] == 70


def test_records_are_plain_c_of_the_stated_sizes(pkg, tmp_path):
    from unina_yolo_dla_amd import engine
    assert engine.STEREO_MATCH_DTYPE.itemsize == 16
    assert [engine.STEREO_MATCH_DTYPE.fields[n][1] for n in ("disparity", "d_best", "cost_best", "cost_second")] == [0, 4, 8, 12]
    assert C.sizeof(engine.StereoParams) == 32 and C.sizeof(engine.StereoPair) == 32
    assert (engine.STEREO_MAX_DISPARITIES, engine.STEREO_MAX_SIDE) == (1024, 64)
    hostprog.compile_c99(tmp_path, 'typedef char match16[(sizeof(unina_stereo_match) == 16) ? 1 : -1];\n'
                                   'typedef char second12[(offsetof(unina_stereo_match, cost_second) == 12) ? 1 : -1];\n'
                                   'typedef char par32[(sizeof(unina_stereo_params) == 32) ? 1 : -1];\n'
                                   'typedef char left16[(offsetof(unina_stereo_pair, left) == 16) ? 1 : -1];\n'
                                   'typedef char lim[(UNINA_STEREO_MAX_DISPARITIES == 1024 && UNINA_STEREO_MAX_SIDE == 64) ? 1 : -1];\n'
                                   'int use(const GpuDetection *d, const int *n, const uint8_t *y, unina_cone3d *o, unina_stereo_match *m) {\n'
                                   '  unina_stereo_pair s = {640, 360, 1280, 0, 0};\n'
                                   '  unina_pinhole c = {700.0f, 700.0f, 320.0f, 180.0f};\n'
                                   '  unina_stereo_params p = {1.0f, 1.0f, 0.5f, 0.5f, 40.0f, 64, 20, 10};\n'
                                   '  s.left = y; s.right = y + 640;\n'
                                   '  return unina_locate_stereo_async(d, n, &s, &c, 0.12f, &p, o, m, 0);\n}\n')
