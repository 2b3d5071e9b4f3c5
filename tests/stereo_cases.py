"""Inputs shared by tests/test_stereo_cpu.py and tests/test_gpu_stereo.py: rectified pairs built from one texture by column
shifts, boxes, and the named edge cases of unina_locate_stereo_async (include/unina_mi355.h "3-D localisation from a stereo
pair"). Pure numpy, seeded by the package's counter-based rng; nothing here touches the device.

Geometry of the small pairs: 97 x 61, fx = 70, baseline = 0.5 m, so fxB = 35: with min_depth = 0.5 m and max_depth = 40 m the
searched disparities are 1 .. 70. The wide pair is 1300 x 80 with fxB = 350 and disparities 1 .. 1024."""
import numpy as np

from unina_yolo_dla_amd import rng
from unina_yolo_dla_amd.engine import DET_DTYPE

W, H = 97, 61
CAM = (70.0, 71.5, 48.25, 30.5)
BASELINE = 0.5
WIDE_W, WIDE_H = 1300, 80
WIDE_CAM = (700.0, 700.0, 650.0, 40.0)
WIDE_MIN_DEPTH = 350.0 / 1024.5          # floorf(fxB / min_depth) = 1024
MAXD = 1024
NONE = 0xFFFFFFFF


def params(**kw):
    p = dict(sx=1.0, sy=1.0, shrink=1.0, min_depth=0.5, max_depth=40.0, max_side=64, max_mean_sad=20, uniqueness=10)
    p.update(kw)
    return p


def wide_params(**kw):
    return params(**{"min_depth": WIDE_MIN_DEPTH, "max_depth": 400.0, **kw})


def boxes(rows):
    """(x1, y1, x2, y2) rows -> DET_DTYPE records as the engine writes them: compact, confidence descending, valid = 1."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    d = np.zeros(len(rows), dtype=DET_DTYPE)
    d["x1"], d["y1"], d["x2"], d["y2"] = rows.T
    d["confidence"] = np.linspace(0.99, 0.05, len(rows)).astype(np.float32)
    d["class_id"] = np.arange(len(rows)) % 4
    d["valid"] = 1
    return d


def cell(u0, v0, cols=1, rows=1):
    """The box whose window (shrink = 1) is exactly columns u0 .. u0 + cols - 1 and rows v0 .. v0 + rows - 1."""
    return (u0 + 0.25, v0 + 0.25, u0 + cols - 0.25, v0 + rows - 0.25)


def texture(seed, h=H, w=W, name="left"):
    """White noise, 0 .. 255."""
    return np.floor(rng.uniform(seed, name, h * w, 0.0, 256.0)).astype(np.uint8).reshape(h, w)


def shifted_scene(seed, bg, rects, h=H, w=W):
    """left: noise. right: what a second camera would see of a background plane at disparity `bg` and fronto-parallel
    rectangles (x0, y0, x1, y1, d) of the left image, exclusive ends, each at its own disparity d > bg: right[v, u - d] =
    left[v, u], the nearer surface in front. The background hidden behind a rectangle in the left image, and the columns nothing
    maps to, are other noise: no window can match there."""
    left = texture(seed, h, w)
    right = texture(seed, h, w, "filler")
    seen = np.ones((h, w), dtype=bool)                                       # left pixels that show the background
    for x0, y0, x1, y1, d in rects:
        seen[y0:y1, x0:x1] = False
    right[:, :w - bg] = np.where(seen[:, bg:], left[:, bg:], right[:, :w - bg])
    for x0, y0, x1, y1, d in sorted(rects, key=lambda r: r[4]):
        assert x0 - d >= 0 and d > bg
        right[y0:y1, x0 - d:x1 - d] = left[y0:y1, x0:x1]
    return left, right


def case(name, dets, left, right, count=None, cam=CAM, baseline=BASELINE, **kw):
    return {"name": name, "dets": dets, "count": len(dets) if count is None else count, "left": left, "right": right, "cam": cam,
            "baseline": baseline, "params": params(**kw)}


# ---------------------------------------------------------------- integer shifts
RECTS = [(30, 1, 60, 15, 12), (62, 16, 95, 30, 40), (20, 31, 50, 45, 7), (70, 46, 96, 60, 66)]
BG = 3


def integer_scene(seed=21):
    return shifted_scene(seed, BG, RECTS)


def inside_boxes(seed=5, per_rect=12):
    """Boxes whose windows (shrink = 1) lie inside one rectangle of RECTS, and the disparity each must find."""
    r = np.random.RandomState(seed)
    rows, truth = [], []
    for x0, y0, x1, y1, d in RECTS:
        for _ in range(per_rect):
            cw, ch = r.randint(1, min(12, x1 - x0) + 1), r.randint(1, min(12, y1 - y0) + 1)
            u0, v0 = r.randint(x0, x1 - cw + 1), r.randint(y0, y1 - ch + 1)
            rows.append(cell(u0, v0, cw, ch))
            truth.append(d)
    return boxes(rows), np.array(truth)


def integer_case():
    left, right = integer_scene()
    dets, truth = inside_boxes()
    return case("integer_shifts", dets, left, right), truth


# ---------------------------------------------------------------- fractional shifts
def smooth(img, passes=2):
    """`passes` of the 5-point average (a pixel and its four neighbours, edges replicated), in float64."""
    a = img.astype(np.float64)
    for _ in range(passes):
        p = np.pad(a, 1, mode="edge")
        a = (p[1:-1, 1:-1] + p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:]) / 5.0
    return a


def fractional_scene(seed, disparity, h=H, w=W):
    """One plane at a fractional disparity: left = the smoothed texture rounded to bytes; right[v, x] = that texture linearly
    interpolated at x + disparity (the last column repeated beyond the edge), plus -2 .. +2 grey levels of noise."""
    t = smooth(texture(seed, h, w + 2))
    left = np.clip(np.rint(t[:, :w]), 0, 255).astype(np.uint8)
    x = np.arange(w) + disparity
    i = np.floor(x).astype(int)
    f = x - np.floor(x)
    tt = np.concatenate([t, np.repeat(t[:, -1:], w, axis=1)], axis=1)
    interp = tt[:, i] * (1.0 - f) + tt[:, i + 1] * f
    noise = np.floor(rng.uniform(seed, "noise", h * w, -2.0, 3.0)).reshape(h, w)
    right = np.clip(np.rint(interp + noise), 0, 255).astype(np.uint8)
    return left, right


def fractional_cases(n_scenes=20, per_scene=10):
    """Scenes at disparities 3 .. 90, windows of 3 .. 30 px whose both neighbouring integer disparities are in the range
    (u0 >= ceil(disparity) + 1). fxB = 47.25, min_depth = 0.5, max_depth = 40: disparities 2 .. 94."""
    r = np.random.RandomState(12)
    out = []
    for k in range(n_scenes):
        jitter = r.uniform(-0.5, 0.5)
        true = float(np.round(3.0 + (90.0 - 3.0) * k / (n_scenes - 1) + jitter, 3))
        true = {0: 3.25, n_scenes - 1: 89.75}.get(k, true)                        # the two ends stay inside 3 .. 90
        left, right = fractional_scene(400 + k, true)
        first = int(np.ceil(true)) + 1
        rows = []
        for _ in range(per_scene):
            cw = r.randint(3, min(30, W - first) + 1)
            ch = r.randint(3, 31)
            u0, v0 = r.randint(first, W - cw + 1), r.randint(0, H - ch + 1)
            rows.append(cell(u0, v0, cw, ch))
        c = case(f"fractional_{true}", boxes(rows), left, right, baseline=0.675)
        out.append((c, true))
    return out


# ---------------------------------------------------------------- chosen costs
def column_case(name, costs, default, u=80, v0=4, rows=10, left_value=0, d_range=(1, 70), **kw):
    """A window of one column and `rows` rows at column u: cost(d) touches right column u - d alone, so every cost is set on its
    own. `costs` maps d -> cost, every other d in d_range costs `default`. left is `left_value` everywhere; each right column
    holds its cost spread over the rows (all rows floor(cost / rows), the first cost % rows one more)."""
    left = np.full((H, W), left_value, dtype=np.uint8)
    right = np.full((H, W), left_value, dtype=np.uint8)
    for d in range(d_range[0], min(d_range[1], u) + 1):
        c = costs.get(d, default)
        col = np.full(rows, c // rows) + (np.arange(rows) < c % rows)
        assert col.max() <= 255
        right[v0:v0 + rows, u - d] = np.abs(left_value - col)
    return case(name, boxes([cell(u, v0, 1, rows)]), left, right, **kw)


def boundary_cases():
    """name -> (case, expected fields of record 0: valid, d_best, cost_best, cost_second, disparity or None)."""
    out = {}

    def add(name, costs, default, want, **kw):
        out[name] = (column_case(name, costs, default, **kw), want)
    # cost_best against max_mean_sad * n_samples = 20 * 10
    add("sad_at_limit", {30: 200}, 2000, dict(valid=1, d_best=30, cost_best=200, cost_second=2000))
    add("sad_above_limit", {30: 201}, 2000, dict(valid=0, d_best=30, cost_best=201, cost_second=2000))
    add("sad_zero_limit_zero_cost", {30: 0}, 50, dict(valid=1, d_best=30, cost_best=0, cost_second=50), max_mean_sad=0)
    # cost_second * 100 against cost_best * (100 + 10)
    add("unique_at_limit", {30: 100}, 110, dict(valid=0, d_best=30, cost_best=100, cost_second=110))
    add("unique_one_more", {30: 100}, 111, dict(valid=1, d_best=30, cost_best=100, cost_second=111))
    add("neighbours_do_not_count", {29: 101, 30: 100, 31: 101}, 111, dict(valid=1, d_best=30, cost_best=100, cost_second=111, disparity=30.0))
    add("unique_zero_tie", {30: 100, 40: 100}, 500, dict(valid=0, d_best=30, cost_best=100, cost_second=100), uniqueness=0)
    add("unique_zero_one_more", {30: 100, 40: 101}, 500, dict(valid=1, d_best=30, cost_best=100, cost_second=101), uniqueness=0)
    add("unique_1000", {30: 10}, 110, dict(valid=0, d_best=30, cost_best=10, cost_second=110), uniqueness=1000)
    add("unique_1000_one_more", {30: 10}, 111, dict(valid=1, d_best=30, cost_best=10, cost_second=111), uniqueness=1000)
    # the ends of the range: no refinement, whatever the one neighbour says
    add("best_at_d_lo", {1: 10, 2: 11}, 900, dict(valid=1, d_best=1, cost_best=10, cost_second=900, disparity=1.0))
    add("best_at_d_hi", {70: 10, 69: 11}, 900, dict(valid=1, d_best=70, cost_best=10, cost_second=900, disparity=70.0))
    add("best_at_u0", {50: 10, 49: 400}, 900, dict(valid=1, d_best=50, cost_best=10, cost_second=900, disparity=50.0), u=50)   # d_hi = u0
    # the parabola: (cm - cp) / (2 * (cm - 2 c0 + cp))
    add("refined", {29: 40, 30: 10, 31: 20}, 900, dict(valid=1, d_best=30, cost_best=10, cost_second=900, disparity=30.0 + 20.0 / 80.0))
    add("refined_thirds", {29: 11, 30: 10, 31: 12}, 900,
        dict(valid=1, d_best=30, cost_best=10, cost_second=900, disparity=float(np.float32(30) + np.float32(-1) / np.float32(6))))
    # equal best at two adjacent disparities: the smaller wins, the step is exactly +0.5; at two separated ones: ambiguous
    add("tie_adjacent", {30: 10, 31: 10}, 900, dict(valid=1, d_best=30, cost_best=10, cost_second=900, disparity=30.5))
    add("tie_adjacent_below", {29: 10, 30: 10, 31: 900}, 900, dict(valid=1, d_best=29, cost_best=10, cost_second=900, disparity=29.5))
    add("tie_separated", {30: 10, 32: 10}, 900, dict(valid=0, d_best=30, cost_best=10, cost_second=10))
    add("flat", {}, 0, dict(valid=0, d_best=1, cost_best=0, cost_second=0))
    add("flat_grey", {}, 150, dict(valid=0, d_best=1, cost_best=150, cost_second=150))
    # the shortest ranges: nothing is two away from the best
    add("nd1", {}, 50, dict(valid=1, d_best=1, cost_best=50, cost_second=NONE, disparity=1.0, n_valid=1), u=1)
    add("nd2", {2: 40}, 50, dict(valid=1, d_best=2, cost_best=40, cost_second=NONE, disparity=2.0, n_valid=2), u=2)
    add("nd3_middle", {2: 40}, 50, dict(valid=1, d_best=2, cost_best=40, cost_second=NONE, disparity=2.0, n_valid=3), u=3)
    add("nd3_end", {3: 40, 2: 41, 1: 44}, 50, dict(valid=0, d_best=3, cost_best=40, cost_second=44, n_valid=3), u=3)
    add("nd3_end_one_more", {3: 40, 2: 41, 1: 45}, 50, dict(valid=1, d_best=3, cost_best=40, cost_second=45, disparity=3.0, n_valid=3), u=3)
    add("nd0", {}, 0, dict(valid=0, d_best=0, cost_best=NONE, cost_second=NONE, n_valid=0), u=0)
    return out


def periodic_case(period=8):
    """A texture periodic along the row with a period inside the range: the minima at d and d + period tie exactly."""
    base = texture(31, H, period)
    left = np.tile(base, (1, W // period + 1))[:, :W]
    right = np.roll(left, -3, axis=1)                                           # period-exact, so the roll is a pure shift
    return case("periodic", boxes([cell(70, 20, 9, 9), cell(60, 30, 5, 7)]), left, right)


def flat_case():
    left = np.full((H, W), 77, dtype=np.uint8)
    return case("flat_patch", boxes([cell(70, 20, 9, 9), cell(40, 3, 30, 30)]), left, left.copy())


def outside_case():
    left, right = integer_scene()
    rows = [(200, 200, 220, 230), (-50, -50, -20, -20), (np.nan, 10, 20, 20), (40, 10, 39.875, 30), cell(0, 5, 4, 4), cell(30, 6, 5, 5)]
    return case("outside_and_nd0", boxes(rows), left, right)


# ---------------------------------------------------------------- the wide pair: 1024 disparities, 64 x stride windows
def wide_scene(seed=77):
    """1300 x 80: background at disparity 5, one rectangle at disparity 1000 and one at 300."""
    return shifted_scene(seed, 5, [(1030, 10, 1290, 78, 1000), (400, 8, 800, 74, 300)], WIDE_H, WIDE_W)


def wide_case(name, rows, scene=None, **kw):
    left, right = wide_scene() if scene is None else scene
    c = case(name, boxes(rows), left, right, cam=WIDE_CAM, baseline=0.5)
    c["params"] = wide_params(**kw)
    return c


def max_cost_scene(dent):
    """left = 255, right = 0: every cost of a 64 x 64 window is 4096 * 255. With `dent` the one right pixel that only the
    LAST disparity of the window at u0 = 1100 reads is 1, so the best is (4096 * 255 - 1, d - d_lo = 1023)."""
    left = np.full((WIDE_H, WIDE_W), 255, dtype=np.uint8)
    right = np.zeros((WIDE_H, WIDE_W), dtype=np.uint8)
    if dent:
        right[8, 1100 - 1024] = 1
    return left, right


def gpu_shape_cases():
    """Cases whose point is the kernel's path: nd of 1, 2, 3, 63, 64, 65 (small pair) and 256, 257, 1024 (wide pair); n_samples
    of 1, 63, 64, 65 and 4096; strides on one axis and on both; 64 x stride windows whose strip stays on chip and does not."""
    left, right = shifted_scene(23, 1, [])                                     # everything at disparity 1: found from u0 = 1 on
    out = [case("nd_small", boxes([cell(u0, 3 + i, 4, 5) for i, u0 in enumerate((1, 2, 3, 63, 64, 65))]), left, right)]
    sl, sr = integer_scene()
    out.append(case("n_samples", boxes([cell(75, 18), cell(70, 18, 9, 7), cell(70, 18, 8, 8), cell(70, 18, 13, 5), cell(63, 16, 31, 14), cell(64, 9, 31, 30)]), sl, sr))
    out.append(case("stride_one_axis", boxes([cell(63, 17, 31, 8), cell(64, 16, 7, 14)]), sl, sr, max_side=8))
    out.append(case("stride_both_axes", boxes([cell(63, 16, 31, 14), cell(30, 5, 30, 25)]), sl, sr, max_side=8))
    out.append(wide_case("nd_wide", [cell(256, 2, 6, 6), cell(257, 2, 6, 6), cell(1030, 30, 6, 6), cell(1024, 40, 3, 3), cell(1200, 12, 64, 64)]))
    out.append(wide_case("samples4096", [cell(1100, 12, 64, 64), cell(620, 10, 64, 64), cell(70, 10, 64, 64)]))
    # 128 columns at stride 2: at u0 = 1040 the strip is 64 x (126 + 1024) bytes and is read through L2; at u0 = 600 it stays on chip
    out.append(wide_case("stride2_wide", [cell(1040, 12, 128, 64), cell(600, 8, 128, 64), cell(1040, 10, 256, 68)]))
    out.append(wide_case("stride_both_wide", [cell(1040, 10, 250, 68), cell(595, 10, 200, 60)], max_side=32))
    for dent in (0, 1):
        out.append(wide_case(f"max_cost_dent{dent}", [cell(1100, 8, 64, 64)], scene=max_cost_scene(dent), max_mean_sad=255, uniqueness=0))
    return out


def random_boxes(seed, n, w=W, h=H, big_every=25):
    """Cone-sized boxes (2 .. 20 px) all over the pair and past every edge, on a 1/8-pixel grid; every `big_every`-th one large."""
    r = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        big = big_every and i % big_every == big_every - 1
        bw, bh = (r.uniform(55, 70), r.uniform(50, 60)) if big else (r.uniform(0, 20), r.uniform(0, 20))
        x1, y1 = (r.uniform(0, w - bw), r.uniform(0, h - bh)) if big else (r.uniform(-8, w), r.uniform(-8, h))
        rows.append(np.round(np.array([x1, y1, x1 + bw, y1 + bh]) * 8) / 8)
    return boxes(rows)


def random_case(n=200, seed=11):
    left, right = shifted_scene(41, BG, [(45, 0, 97, 61, 30)])
    return case(f"random{n}", random_boxes(seed, n), left, right, shrink=0.8)


def all_cases():
    """Every case the CPU tests pin, for the GPU test to compare byte for byte."""
    out = [integer_case()[0], periodic_case(), flat_case(), outside_case()]
    out += [c for c, _ in boundary_cases().values()]
    out += [c for c, _ in fractional_cases()]
    return out + gpu_shape_cases()
