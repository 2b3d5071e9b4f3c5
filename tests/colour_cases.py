"""Inputs shared by tests/test_colour_cpu.py and tests/test_gpu_colour.py: the named calls of unina_colour_async
(include/unina_mi355.h "class from pixels"), the renderer of the cone table, and a scalar restatement of the pixel's class. A case
is the records, their count word, their cones (or None), an image with its layout in memory, the pinhole and the parameters of
one call. Pure numpy; nothing here touches the device. tests/test_colour_cpu.py asserts on the twin what each case contains.

A window is placed with box_over(u0, v0, u1, v1): the box (u0 + 0.25, v0 + 0.25, u1 + 0.75, v1 + 0.75) covers, at shrink = 1,
exactly the pixels u0..u1 x v0..v1 (floorf(c - h) = u0, floorf(c + h) = u1, every value a short binary fraction).
A PAINTED window is a small matrix of letters, one pixel each: Y, B, O the three body colours, W white, K black, G a grey that is
OTHER, M a magenta that is COLOURED but in no hue range.
Images are at most 256 x 192, so a 64 x 64 grid has stride 1, or 4 x 3 over the whole image; stride 5 is reached with
max_side = 48 (a span of 240)."""
import numpy as np

from unina_yolo_dla_amd.engine import CONE3D_DTYPE, DET_DTYPE

MAXD = 1024
F = np.float32
NAN, INF = float("nan"), float("inf")
CAM = (256.0, 256.0, 128.0, 96.0)
UNKNOWN = 9                       # the class_id the LiDAR-only records carry
CLASS_OF = (0, 1, 2, 3)
PAINT = {"Y": (230, 210, 40), "B": (30, 80, 200), "O": (240, 110, 30), "W": (235, 235, 235), "K": (25, 25, 25), "G": (100, 100, 100),
         "M": (200, 40, 120)}     # R, G, B
DEFAULTS = dict(sx=1.0, sy=1.0, shrink=1.0, half_width=0.114, above=0.175, below=0.15, max_side=64, order=1, only_class=-1, class_of=CLASS_OF,
                black_max=50, sat_min=96, val_min=60, white_min=150, hue_lo=(171, 850, 20), hue_hi=(300, 1110, 170), taper=64, min_pixels=12,
                min_share=96, max_rival=128, require_stripe=0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ---------------------------------------------------------------- the pixel's class, scalar python integers
def scalar_hue(R, G, B):
    mx, mn = max(R, G, B), min(R, G, B)
    d = mx - mn
    if mx == R:
        return 256 * (G - B) // d if G >= B else (1536 - 256 * (B - G) // d) % 1536
    if mx == G:
        return 512 + 256 * (B - R) // d if B >= R else 512 - 256 * (R - B) // d
    return 1024 + 256 * (R - G) // d if R >= G else 1024 - 256 * (G - R) // d


def scalar_pixel(p, R, G, B):
    """The bin of a pixel: 0, 1, 2 a colour, 3 white, 4 black, -1 other. p: a dict of the parameters."""
    mx, mn = max(R, G, B), min(R, G, B)
    d = mx - mn
    if mx <= p["black_max"]:
        return 4
    if d * 256 >= p["sat_min"] * mx and mx >= p["val_min"]:
        h = scalar_hue(R, G, B)
        for c in range(3):
            lo, hi = p["hue_lo"][c], p["hue_hi"][c]
            if (lo <= h <= hi) if lo <= hi else (h >= lo or h <= hi):
                return c
        return -1
    return 3 if mx >= p["white_min"] else -1


_by_hue = {}


def pixel_with_hue(h):
    """A saturated, bright (R, G, B) whose hue is exactly h: max = 220, found by a search over the other two channels."""
    if not _by_hue:
        for a in range(0, 120):
            for b in range(a, 221):
                for rgb in ((220, b, a), (220, a, b), (b, 220, a), (a, 220, b), (b, a, 220), (a, b, 220)):
                    _by_hue.setdefault(scalar_hue(*rgb), rgb)
    return _by_hue[h]


# ---------------------------------------------------------------- records, cones, images
def box_over(u0, v0, u1, v1):
    return (u0 + 0.25, v0 + 0.25, u1 + 0.75, v1 + 0.75)


def records(boxes, cls=UNKNOWN, conf=0.5):
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    dets = np.zeros(len(b), dtype=DET_DTYPE)
    dets["x1"], dets["y1"], dets["x2"], dets["y2"] = b.T
    dets["confidence"], dets["class_id"], dets["valid"] = conf, cls, 1
    return dets


def cones_at(u, v, z, valid=1):
    u = np.atleast_1d(np.asarray(u, dtype=np.float32))
    cones = np.zeros(len(u), dtype=CONE3D_DTYPE)
    cones["u"], cones["v"], cones["z"], cones["valid"] = u, v, z, valid
    cones["x"], cones["y"] = (cones["u"] - F(CAM[2])) * cones["z"] / F(CAM[0]), (cones["v"] - F(CAM[3])) * cones["z"] / F(CAM[1])
    cones["n_valid"] = cones["n_samples"] = 12
    return cones


def case(name, dets, image, cones=None, count=None, pitch=None, offset=0, cam=CAM, **par):
    """image: uint8 [H, W, C] in the byte order par['order'] names (default RGB); pitch / offset: its layout in a buffer of exactly
    offset + (H - 1) * pitch + W * C bytes."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    h, w, ch = image.shape
    return {"name": name, "dets": dets, "count": len(dets) if count is None else count, "cones": cones, "image": image,
            "pitch": w * ch if pitch is None else pitch, "offset": offset, "cam": cam, "params": params(**par)}


def image_bytes(c) -> np.ndarray:
    """The case's image as it lies in memory: uint8 [offset + (H - 1) * pitch + W * C], 0xA5 where no pixel is."""
    h, w, ch = c["image"].shape
    buf = np.full(c["offset"] + (h - 1) * c["pitch"] + w * ch, 0xA5, dtype=np.uint8)
    for r in range(h):
        at = c["offset"] + r * c["pitch"]
        buf[at:at + w * ch] = c["image"][r].reshape(-1)
    return buf


def in_order(rgb, channels=3, order=1):
    """uint8 [H, W, 3] R, G, B -> the image in `order` (0 = BGR, 1 = RGB) with `channels` channels, the fourth 0x5A."""
    rgb = np.asarray(rgb, dtype=np.uint8)
    img = rgb if order == 1 else rgb[..., ::-1]
    if channels == 4:
        img = np.concatenate([img, np.full(img.shape[:2] + (1,), 0x5A, dtype=np.uint8)], axis=2)
    return np.ascontiguousarray(img)


def scene_rgb(height=192, width=256, seed=5):
    """Blocks of 8 x 6 pixels of the seven paints with +-12 noise: every window sees several bins."""
    rng = np.random.default_rng(seed)
    keys = list(PAINT)
    pick = rng.integers(0, len(keys), (height // 6 + 1, width // 8 + 1))
    base = np.array([PAINT[k] for k in keys], dtype=np.int64)[pick]
    img = np.repeat(np.repeat(base, 6, axis=0), 8, axis=1)[:height, :width]
    return np.clip(img + rng.integers(-12, 13, img.shape), 0, 255).astype(np.uint8)


def painted(windows, gap=2, width=256):
    """windows: a list of lists of equally long strings of PAINT letters -> (uint8 [H, W, 3] RGB on a background of G, the boxes
    that cover each window exactly), the windows laid out left to right, top to bottom."""
    boxes, x, y, row_h, placed = [], gap, gap, 0, []
    for wnd in windows:
        rows, cols = len(wnd), len(wnd[0])
        assert all(len(r) == cols for r in wnd) and cols + 2 * gap <= width
        if x + cols + gap > width:
            x, y, row_h = gap, y + row_h + gap, 0
        placed.append((x, y, wnd))
        boxes.append(box_over(x, y, x + cols - 1, y + rows - 1))
        x, row_h = x + cols + gap, max(row_h, rows)
    height = y + row_h + gap
    assert height <= 192
    img = np.empty((height, width, 3), dtype=np.uint8)
    img[:] = PAINT["G"]
    for x, y, wnd in placed:
        for k, r in enumerate(wnd):
            for c, letter in enumerate(r):
                img[y + k, x + c] = PAINT[letter]
    return img, boxes


def column(letters):
    """A window one pixel wide, a row per letter."""
    return [ch for ch in letters]


def block(counts, cols):
    """A window of `cols` columns filled row by row with counts = {letter: pixels}, in the dict's order."""
    s = "".join(k * v for k, v in counts.items())
    assert len(s) % cols == 0
    return [s[i:i + cols] for i in range(0, len(s), cols)]


# ---------------------------------------------------------------- the rendered cones
BACKGROUNDS = {"asphalt": (95, 95, 100), "grass": (60, 140, 50), "sky": (150, 195, 240), "night": (20, 20, 22)}
CONE_KINDS = {"yellow": ((230, 210, 40), (25, 25, 25), 1, 0), "blue": ((30, 80, 200), (235, 235, 235), 1, 1),
              "orange": ((240, 110, 30), (235, 235, 235), 1, 2), "large_orange": ((240, 110, 30), (235, 235, 235), 2, 3)}   # body, stripe, stripes, index
CONE_SIZES = ((6, 9), (10, 14), (20, 28), (40, 56))


def render_cone(img, u, v, w, h, kind):
    """A trapezoid whose top is 20 % of its base, w x h pixels with its top left at (u, v): one stripe over 35-60 % of the height
    from the top, or two over 25-40 % and 60-75 %. A pixel belongs to a shape where its centre does."""
    body, stripe, n, _ = CONE_KINDS[kind]
    bands = ((0.35, 0.60),) if n == 1 else ((0.25, 0.40), (0.60, 0.75))
    for k in range(h):
        t = (k + 0.5) / h
        half = 0.5 * w * (0.2 + 0.8 * t)
        paint = stripe if any(lo <= t < hi for lo, hi in bands) else body
        for c in range(w):
            if abs(c + 0.5 - 0.5 * w) <= half:
                img[v + k, u + c] = paint


def rendered_cases(sizes=CONE_SIZES):
    """One case per background: the four kinds at every size, +-12 uniform noise from default_rng(0), default parameters. The
    case carries `truth`: (colour index, stripes) per record."""
    out = []
    rng = np.random.default_rng(0)
    for bg_name, bg in BACKGROUNDS.items():
        img = np.empty((192, 256, 3), dtype=np.int64)
        img[:] = bg
        boxes, truth, y = [], [], 3
        for w, h in sizes:
            x = 3
            for kind in CONE_KINDS:
                render_cone(img, x, y, w, h, kind)
                boxes.append(box_over(x, y, x + w - 1, y + h - 1))
                truth.append((CONE_KINDS[kind][3], CONE_KINDS[kind][2]))
                x += w + 6
            y += h + 4
        img = np.clip(img + rng.integers(-12, 13, img.shape), 0, 255).astype(np.uint8)
        c = case(f"rendered_{bg_name}", records(boxes), img)
        c["truth"] = truth
        out.append(c)
    return out


# ---------------------------------------------------------------- the constructed cases
def grid_boxes(n=MAXD, cols=32, w=8, h=6):
    i = np.arange(n)
    return [box_over(x, y, x + w - 1, y + h - 1) for x, y in zip((i % cols) * w, (i // cols) * h)]


WINDOW_BOXES = {
    "one_pixel": box_over(17, 23, 17, 23), "column_1x64": box_over(40, 10, 40, 73), "row_64x1": box_over(100, 5, 163, 5),
    "full_64x64": box_over(150, 100, 213, 163), "whole_image_stride_4x3": box_over(0, 0, 255, 191), "wide_65_stride_2": box_over(3, 3, 67, 40),
    "clip_left": (-10.5, 20.25, 12.75, 40.75), "clip_right": (240.25, 20.25, 300.5, 40.75), "clip_top": (30.25, -20.0, 50.75, 9.75),
    "clip_bottom": (30.25, 180.25, 50.75, 260.0), "outside_right": (300.0, 20.0, 320.0, 40.0), "outside_above": (30.0, -40.0, 50.0, -2.0),
    "nan_box": (NAN, 20.0, 40.0, 40.0), "inf_box": (10.0, 20.0, INF, 40.0), "inverted_x": (60.0, 20.0, 40.0, 40.0), "inverted_y": (40.0, 60.0, 60.0, 20.0),
    "last_pixel": box_over(250, 188, 255, 191), "first_pixel": box_over(0, 0, 0, 0),
}
# the zero-area boxes the fuser writes, with the cone beside them: u, v, z, valid
SIZE_CONES = {
    "size_near": (128.0, 96.0, 2.0, 1), "size_far": (60.5, 100.25, 20.0, 1), "size_one_pixel": (200.5, 50.5, 400.0, 1), "size_invalid": (128.0, 96.0, 2.0, 0),
    "size_z_zero": (128.0, 96.0, 0.0, 1), "size_z_negative": (128.0, 96.0, -2.0, 1), "size_z_nan": (128.0, 96.0, NAN, 1), "size_u_nan": (NAN, 96.0, 2.0, 1),
    "size_v_inf": (128.0, INF, 2.0, 1), "size_clipped": (2.0, 190.0, 1.0, 1), "size_outside": (-400.0, 96.0, 2.0, 1), "size_overflows": (128.0, 96.0, 1e-38, 1), "size_huge": (128.0, 96.0, 1e-30, 1),
}


def window_records():
    """The BOX windows, then the SIZE windows (point boxes at the cone's pixel, NaN for a cone without one) -> dets, cones."""
    names = list(WINDOW_BOXES) + list(SIZE_CONES)
    cones = np.concatenate([cones_at(np.zeros(len(WINDOW_BOXES)), 0.0, 0.0, valid=0), *[cones_at(u, v, z, ok) for u, v, z, ok in SIZE_CONES.values()]])
    pts = [(u, v, u, v) if np.isfinite(u) and np.isfinite(v) else (0.0, 0.0, 0.0, 0.0) for u, v, _, _ in SIZE_CONES.values()]
    return names, records(list(WINDOW_BOXES.values()) + pts), cones


PIXELS = {   # R, G, B under the default thresholds -> the bin
    "black_on_bound": ((50, 50, 50), 4), "black_one_above": ((51, 51, 51), -1), "black_coloured": ((50, 10, 10), 4),
    "sat_on_bound": ((128, 100, 80), 2), "sat_one_below": ((128, 100, 81), -1), "val_on_bound": ((60, 40, 10), 2), "val_one_below": ((59, 40, 10), -1),
    "white_on_bound": ((150, 150, 150), 3), "white_one_below": ((149, 149, 149), -1), "grey_equal_channels": ((200, 200, 200), 3),
    "max_is_r_and_g": ((200, 200, 40), 0), "max_is_all": ((255, 255, 255), 3), "zero": ((0, 0, 0), 4),
    "branch_r_g_ge_b": ((240, 110, 30), 2), "branch_r_g_lt_b": ((200, 40, 120), -1), "branch_g_b_ge_r": ((40, 200, 120), -1),
    "branch_g_b_lt_r": ((230, 240, 40), 0), "branch_b_r_ge_g": ((120, 40, 200), -1), "branch_b_r_lt_g": ((30, 80, 200), 1),
}
HUE_BOUNDS = {170: 2, 171: 0, 300: 0, 301: -1, 849: -1, 850: 1, 1110: 1, 1111: -1, 19: -1, 20: 2}   # hue -> the bin under the default ranges
WRAP = dict(hue_lo=(171, 850, 1500), hue_hi=(300, 1110, 170))          # orange across 0
WRAP_HUES = {1499: -1, 1500: 2, 1535: 2, 0: 2, 10: 2, 170: 2, 171: 0}
OVERLAP = dict(hue_lo=(100, 850, 20), hue_hi=(300, 1110, 170))        # yellow and orange share 100..170: yellow wins
OVERLAP_HUES = {99: 2, 100: 0, 150: 0, 170: 0, 301: -1}


def pixel_row(rgbs, **par):
    """One record per pixel, each a 1 x 1 window on a row image; min_pixels = 1, every share accepted: the record's colour entry
    shows the pixel's bin."""
    img = np.array([list(rgbs)], dtype=np.uint8)
    return records([box_over(i, 0, i, 0) for i in range(len(rgbs))]), img, dict(taper=256, min_pixels=1, min_share=0, max_rival=256, **par)


STRIPE_STRINGS = {   # a column of paints -> (row string, stripes); body O, stripe W
    "OWO": ("BSB", 1), "WO": ("SB", 0), "OW": ("BS", 0), "OWGWO": ("BSSB", 1), "OWOWO": ("BSBSB", 2), "OW" * 32: ("BS" * 32, 31), "WOWGO": ("SBSB", 1),
    "OOWWWOO": ("BBSSSBB", 1), "OGO": ("BB", 0), "W": ("", 0), "OWOWOWO": ("BSBSBSB", 3),
}
DECISION = dict(taper=256, min_pixels=16, min_share=96, max_rival=128)


def decision_windows():
    """name -> (window, expected decided): 16 pixels each unless the name says otherwise."""
    return {
        "mask_on_min_pixels": (block({"Y": 16}, 4), True), "mask_one_below": (block({"Y": 15}, 5), False),
        "share_equal": (block({"Y": 6, "G": 10}, 4), True), "share_one_vote_short": (block({"Y": 5, "G": 11}, 4), False),
        "rival_equal": (block({"Y": 6, "B": 3, "G": 7}, 4), True), "rival_one_vote_over": (block({"Y": 6, "B": 4, "G": 6}, 4), False),
        "two_equal": (block({"B": 6, "O": 6, "G": 4}, 4), False), "three_equal": (block({"Y": 5, "B": 5, "O": 5, "G": 1}, 4), False),
        "no_coloured_pixel": (block({"W": 6, "K": 5, "G": 5}, 4), False), "magenta_only": (block({"M": 16}, 4), False),
    }


def edge_cases():
    out = []
    rgb = scene_rgb()
    # counts: the first `count` of 1024 records on a grid of 8 x 6 windows, every one of them the unknown class
    grid = records(grid_boxes())
    for n in (0, 1, 63, 64, 65, 1024, 5000, -7):
        out.append(case(f"count{n}", grid, rgb, count=n, min_pixels=1))
    # windows, BOX and SIZE; then the same records without the cones array
    names, dets, cones = window_records()
    out.append(dict(case("windows", dets, rgb, cones=cones), names=names))
    out.append(dict(case("windows_no_cones", dets, rgb), names=names))
    out.append(dict(case("windows_shrunk_scaled", dets, rgb, cones=cones, shrink=0.5, sx=0.5, sy=1.5), names=names))
    out.append(case("stride5", records([box_over(0, 0, 239, 191), box_over(8, 0, 247, 100)]), rgb, max_side=48))
    out.append(case("max_side_1", records([box_over(10, 10, 40, 50), box_over(0, 0, 255, 191)]), rgb, max_side=1, min_pixels=1))
    out.append(case("image_1x1", records([box_over(0, 0, 0, 0), (-5.0, -5.0, 5.0, 5.0), (3.0, 3.0, 5.0, 5.0)]), np.array([[PAINT["Y"]]]), min_pixels=1))
    # images: 3 and 4 channels, both orders, odd pitches and addresses; every buffer ends with the last pixel's last byte
    for ch in (3, 4):
        for order in (0, 1):
            img = in_order(rgb, ch, order)
            out.append(dict(case(f"scene_c{ch}_o{order}", dets, img, cones=cones, order=order), names=names))
            out.append(dict(case(f"scene_c{ch}_o{order}_odd", dets, img, cones=cones, order=order, pitch=256 * ch + (5 if ch == 3 else 6), offset=1), names=names))
    out.append(dict(case("scene_c4_pitch_aligned_offset_2", dets, in_order(rgb, 4, 0), cones=cones, order=0, pitch=1028, offset=2), names=names))
    out.append(dict(case("scene_c3_width_253", dets, in_order(rgb[:, :253], 3, 1), cones=cones, pitch=253 * 3 + 1), names=names))
    # the pixel's class, one record per pixel
    d, img, par = pixel_row([v[0] for v in PIXELS.values()])
    out.append(case("pixels", d, img, **par))
    for ch, order in ((3, 0), (4, 0), (4, 1)):
        out.append(case(f"pixels_c{ch}_o{order}", d, in_order(img, ch, order), order=order, **par))
    d, img, par = pixel_row([pixel_with_hue(h) for h in HUE_BOUNDS])
    out.append(case("hue_bounds", d, img, **par))
    d, img, par = pixel_row([pixel_with_hue(h) for h in WRAP_HUES], **WRAP)
    out.append(case("hue_wrap", d, img, **par))
    d, img, par = pixel_row([pixel_with_hue(h) for h in OVERLAP_HUES], **OVERLAP)
    out.append(case("hue_overlap", d, img, **par))
    # the silhouette
    sil = records([box_over(10, 10, 49, 65), box_over(60, 10, 60, 73), box_over(70, 10, 133, 10), box_over(140, 10, 146, 18), box_over(150, 10, 151, 11)])
    for taper in (0, 64, 256):
        out.append(case(f"taper{taper}", sil, rgb, taper=taper, min_pixels=1))
    # the decision
    dw = decision_windows()
    img, boxes = painted([w for w, _ in dw.values()])
    out.append(dict(case("decision", records(boxes), img, **DECISION), names=list(dw)))
    out.append(dict(case("decision_rival_256", records(boxes), img, **dict(DECISION, max_rival=256, min_share=64)), names=list(dw)))
    stripes_img, stripes_boxes = painted([column(s) for s in STRIPE_STRINGS] + [["OW", "OO", "WW", "OW", "OO"], column("YKY"), column("YWY"), column("BWB"),
                                                                                  column("BKB")])
    for name, par in (("stripes", {}), ("stripes_required", dict(require_stripe=1)), ("stripes_no_body_class", dict(class_of=(0, 1, -1, 3))),
                      ("stripes_no_large_class", dict(class_of=(0, 1, 2, -1))), ("stripes_no_class_at_all", dict(class_of=(-1, -1, -1, -1)))):
        out.append(case(name, records(stripes_boxes), stripes_img, taper=256, min_pixels=1, **par))
    # selection: an unknown id among coloured records; the others carry NaN payloads and come back byte for byte
    sel = records(grid_boxes(64), cls=np.where(np.arange(64) % 3 == 0, UNKNOWN, np.arange(64) % 3))
    words = sel.view(np.uint32).reshape(-1, 8)
    words[1::3, :5] = 0x7fc12345                                                   # NaN box and confidence with a payload
    words[2::3, 6:] = 0xdeadbeef                                                   # valid and _pad are not read either
    out.append(case("only_unknown", sel, rgb, only_class=UNKNOWN, min_pixels=1))
    out.append(case("every_record", sel, rgb, only_class=-1, min_pixels=1))
    out.append(case("only_class_absent", sel, rgb, only_class=77, min_pixels=1))
    return out


def run_twin(c):
    from unina_yolo_dla_amd import colour
    return colour.colour_numpy(c["dets"], c["count"], c["cones"], c["image"], c["cam"], c["params"])


_cache = {}


def cached(key, build):
    """Cases and their twin results are built once per process and shared, unchanged, by every test."""
    if key not in _cache:
        _cache[key] = [(c, run_twin(c)) for c in build()]
    return _cache[key]
