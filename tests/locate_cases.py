"""Inputs shared by tests/test_locate_cpu.py and tests/test_gpu_locate.py: depth maps with holes, boxes, and the named edge
cases of unina_locate_async (include/unina_mi355.h "3-D localisation"). Pure numpy; nothing here touches the device."""
import numpy as np

from unina_yolo_dla_amd.engine import DEPTH_F32, DEPTH_U16, DET_DTYPE

W, H = 97, 61
CAM = (70.0, 71.5, 48.25, 30.5)
UNIT = {DEPTH_F32: 1.0, DEPTH_U16: 0.001}          # metres; millimetres
FORMATS = (DEPTH_F32, DEPTH_U16)
MAXD = 1024


def params(**kw):
    p = dict(sx=1.0, sy=1.0, shrink=0.5, min_depth=0.3, max_depth=40.0, max_side=64, min_valid=1)
    p.update(kw)
    return p


def depth_map(seed, fmt, h=H, w=W, holes=0.3):
    """Depths of 0.5 .. 30 m with `holes` of the pixels marked the ways a camera marks them, or out of range on either side."""
    rng = np.random.RandomState(seed)
    metres = rng.uniform(0.5, 30.0, (h, w))
    hole = rng.rand(h, w) < holes
    kind = rng.randint(0, 8, (h, w))
    if fmt == DEPTH_F32:
        d = metres.astype(np.float32)
        marks = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 100.0, 0.01], dtype=np.float32)
        return np.where(hole, marks[kind], d)
    d = np.round(metres * 1000).astype(np.uint16)
    marks = np.array([0, 0, 0, 100, 65000, 0, 299, 40001], dtype=np.uint16)       # 0.1 m, 65 m, just under, just over
    return np.where(hole, marks[kind], d)


def boxes(rows):
    """(x1, y1, x2, y2) rows -> DET_DTYPE records as the engine writes them: compact, confidence descending, valid = 1."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    d = np.zeros(len(rows), dtype=DET_DTYPE)
    d["x1"], d["y1"], d["x2"], d["y2"] = rows.T
    d["confidence"] = np.linspace(0.99, 0.05, len(rows)).astype(np.float32)
    d["class_id"] = np.arange(len(rows)) % 4
    d["valid"] = 1
    return d


def random_boxes(seed, n, w=W, h=H, big_every=25):
    """Cone-sized boxes (2 .. 20 px) all over the map and past every edge, on a 1/8-pixel grid; every `big_every`-th one large."""
    rng = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        big = big_every and i % big_every == big_every - 1
        bw, bh = (rng.uniform(20, 70), rng.uniform(20, 60)) if big else (rng.uniform(0, 20), rng.uniform(0, 20))
        x1, y1 = rng.uniform(-12, w + 4), rng.uniform(-12, h + 4)
        rows.append(np.round(np.array([x1, y1, x1 + bw, y1 + bh]) * 8) / 8)
    return boxes(rows)


def _const(fmt, metres, h=H, w=W):
    return np.full((h, w), metres if fmt == DEPTH_F32 else int(round(metres * 1000)), dtype=np.float32 if fmt == DEPTH_F32 else np.uint16)


def _from_bits(fmt, words, h=H, w=W):
    """A map tiled from a list of raw words (uint32 bit patterns for f32, values for u16)."""
    words = np.asarray(words, dtype=np.uint32)
    flat = np.resize(words, h * w)
    flat = flat[np.random.RandomState(7).permutation(h * w)]
    return flat.view(np.float32).reshape(h, w) if fmt == DEPTH_F32 else flat.astype(np.uint16).reshape(h, w)


def case(name, fmt, dets, depth, count=None, **kw):
    return {"name": name, "fmt": fmt, "dets": dets, "count": len(dets) if count is None else count, "depth": depth,
            "unit": UNIT[fmt], "cam": CAM, "params": params(**kw)}


def edge_cases(fmt):
    """The named cases, one format. Maps are 97 x 61 unless the name says otherwise."""
    dm = depth_map(100 + fmt, fmt)
    out = []
    add = lambda *a, **kw: out.append(case(*a, **kw))                                  # noqa: E731
    grid = [(3 * (i % 32) + 0.25, (i // 32) + 0.25, 3 * (i % 32) + 2.75, (i // 32) + 2.75) for i in range(MAXD)]   # 3 x 3 windows, all on the map
    add("count0", fmt, boxes(grid[:8]), dm, count=0)
    add("count1", fmt, boxes(grid[:8]), dm, count=1)
    add("count1024_3x3", fmt, boxes(grid), dm, shrink=1.0)
    add("count5000_clamped", fmt, boxes(grid), dm, count=5000, shrink=1.0)
    add("count_negative", fmt, boxes(grid[:8]), dm, count=-3)
    add("outside", fmt, boxes([(200, 200, 220, 230), (-50, -50, -20, -20), (10, 70, 20, 90), (120, 10, 130, 20)]), dm)
    add("clipped_edges", fmt, boxes([(-10, 20, 10, 40), (85, 20, 120, 40), (30, -15, 50, 12), (30, 50, 50, 80), (-20, -20, 130, 90)]), dm,
        shrink=1.0)
    add("degenerate_x2_eq_x1", fmt, boxes([(40.5, 10, 40.5, 30), (40, 10, 40, 30), (12, 33.5, 30, 33.5), (5.5, 5.5, 5.5, 5.5)]), dm, shrink=1.0)
    add("inverted", fmt, boxes([(40, 10, 39.875, 30), (10, 30, 20, 29), (10, 10, 20, 20)]), dm)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    add("non_finite_box", fmt, boxes([(nan, 10, 20, 20), (10, 10, inf, 20), (-inf, 10, inf, 20), (10, nan, 20, nan), (3e38, 1, 3.2e38, 2),
                                      (10, 10, 20, 20)]), dm, sx=4.0)
    add("one_sample", fmt, boxes([(10.25, 10.25, 10.5, 10.5)]), dm)
    add("samples63", fmt, boxes([(10.125, 20.125, 18.875, 26.875)]), dm, shrink=1.0)            # 9 x 7
    add("samples64", fmt, boxes([(10.125, 20.125, 17.875, 27.875)]), dm, shrink=1.0)            # 8 x 8
    add("samples65", fmt, boxes([(10.125, 20.125, 22.875, 24.875)]), dm, shrink=1.0)            # 13 x 5
    add("stride2_one_axis", fmt, boxes([(10.125, 20.125, 22.875, 24.875), (20.125, 10.125, 24.875, 22.875)]), dm, shrink=1.0, max_side=8)
    add("max_side1", fmt, boxes([(10, 10, 40, 40), (50, 5, 90, 55)]), dm, shrink=1.0, max_side=1)
    big = depth_map(300 + fmt, fmt, 600, 600)
    add("map600_256x256", fmt, boxes([(40.125, 30.125, 551.875, 541.875)]), big, shrink=1.0, max_side=256)
    # 8192 samples are the most the kernel keeps on chip between its passes: exactly that, and one column more
    add("map600_128x64_129x64", fmt, boxes([(40.125, 30.125, 167.875, 93.875), (40.125, 130.125, 168.875, 193.875),
                                            (300.125, 300.125, 390.875, 390.875)]), big, shrink=1.0, max_side=256)
    if fmt == DEPTH_F32:
        marks = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 0.29, 40.5, 1e-40, 3e38], dtype=np.float32)
    else:
        marks = np.array([0, 0, 299, 40001, 65535, 1], dtype=np.uint16)
    holes = np.resize(marks, H * W).reshape(H, W)
    add("all_holes", fmt, random_boxes(5, 40), holes)
    few = holes.copy()
    few[30, 40:43] = _const(fmt, 5.0)[0, :3]                                                  # three valid samples in one window
    add("min_valid_one_above", fmt, boxes([(38, 28, 46, 33), (38, 28, 46, 33)]), few, shrink=1.0, min_valid=4)
    add("min_valid_met", fmt, boxes([(38, 28, 46, 33)]), few, shrink=1.0, min_valid=3)
    ev = holes.copy()
    ev[30, 40:44] = (np.array([7.0, 3.0, 5.0, 9.0]) * (1 if fmt == DEPTH_F32 else 1000)).astype(ev.dtype)   # lower median: 5
    add("even_n_valid", fmt, boxes([(38, 28, 46, 33), (5, 5, 60, 50)]), ev, shrink=1.0)
    add("all_equal", fmt, boxes([(10, 10, 12, 12), (5, 5, 60, 50), (0, 0, 97, 61)]), _const(fmt, 12.5), shrink=1.0)
    if fmt == DEPTH_F32:
        low = [0x41200000 | b for b in range(256)]                                             # 10.0 .. 10.0002
        high = [(b << 24) | 0x00123456 for b in (0x3f, 0x40, 0x41, 0x42)]                      # 0.57 .. 36.6
    else:
        low = [0x1200 | b for b in range(256)]
        high = [(b << 8) | 0x34 for b in range(2, 0x9c)]
    wide = [(10, 10, 12, 12), (5, 5, 60, 50), (0, 0, 97, 61), (20.125, 20.125, 27.875, 27.875)]
    add("lowest_byte_only", fmt, boxes(wide), _from_bits(fmt, low), shrink=1.0)
    add("highest_byte_only", fmt, boxes(wide), _from_bits(fmt, high), shrink=1.0)
    ties = [1000] * 5 + [2000] * 9 + [2001] * 2 + [3000] * 7 + [0] * 3
    ties = ties if fmt == DEPTH_U16 else np.array([t / 1000 for t in ties], dtype=np.float32).view(np.uint32).tolist()
    add("heavy_ties", fmt, boxes(wide), _from_bits(fmt, ties), shrink=1.0)
    return out


def random_case(fmt, n=200, seed=11):
    return case(f"random{n}", fmt, random_boxes(seed + fmt, n), depth_map(50 + fmt, fmt), shrink=0.6, max_side=16)
