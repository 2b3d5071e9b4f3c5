"""unina_colour_async without a GPU: colour.colour_numpy (the definition) against an independent scalar restatement -- plain python
loops over the pixels -- on every constructed case, the rendered cones and 200 random cases with tie-heavy pixel values;
csrc/colour_math.h compiled for the host (tests/colour_math_host.cpp, also under -fsanitize=address,undefined as the stand-alone
program it is, the image in a heap buffer of exactly its size) against the twin on the same cases; the table of rendered cones
under the default parameters; the argument checks of the entry point; the layouts in C; and what each constructed case of
tests/colour_cases.py contains."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import colour_cases as cc
import hostprog

F = np.float32
NAMES = ("header", "dets", "colours")
WINDOW, SELECTED, DECIDED, LARGE, SIZE = 1, 2, 4, 8, 16


def r(v):
    """A python float rounded to fp32: a double holds the sum, difference, product or quotient of two fp32 values closely enough
    that rounding it to fp32 is the fp32 operation."""
    return float(F(v))


# ---------------------------------------------------------------- an independent restatement of one call
def brute_axis(c, h, n, max_side):
    lo, hi = r(c - h), r(c + h)
    if not (math.isfinite(lo) and math.isfinite(hi)):
        return None
    lo, hi = math.floor(lo), math.floor(hi)
    if hi < 0 or lo > n - 1:
        return None
    lo, hi = max(lo, 0), min(hi, n - 1)
    stride = -(-(hi - lo + 1) // max_side)
    return [lo + k * stride for k in range((hi - lo) // stride + 1)]


def brute_grid(box, sx, sy, shrink, width, height, max_side):
    """The sampled columns and rows of a box, or None: python floats rounded after every operation."""
    with np.errstate(all="ignore"):
        X1, Y1, X2, Y2 = r(box[0] * sx), r(box[1] * sy), r(box[2] * sx), r(box[3] * sy)
        if not all(math.isfinite(v) for v in (X1, Y1, X2, Y2)) or X2 < X1 or Y2 < Y1:
            return None
        hs = r(0.5 * shrink)
        us = brute_axis(r(0.5 * r(X1 + X2)), r(hs * r(X2 - X1)), width, max_side)
        vs = brute_axis(r(0.5 * r(Y1 + Y2)), r(hs * r(Y2 - Y1)), height, max_side)
    return None if us is None or vs is None else (us, vs)


def brute_window(c, i):
    """(columns, rows, size) of record i, or None."""
    p, d = c["params"], c["dets"][i]
    sx, sy, shrink = (float(F(p[k])) for k in ("sx", "sy", "shrink"))
    h, w = c["image"].shape[:2]
    box = [float(d[k]) for k in ("x1", "y1", "x2", "y2")]
    with np.errstate(all="ignore"):
        X = [r(box[0] * sx), r(box[1] * sy), r(box[2] * sx), r(box[3] * sy)]
        if all(math.isfinite(v) for v in X) and X[2] > X[0] and X[3] > X[1]:
            g = brute_grid(box, sx, sy, shrink, w, h, p["max_side"])
            return None if g is None else (*g, 0)
        if c["cones"] is None or c["cones"]["valid"][i] == 0:
            return None
        u, v, z = (float(c["cones"][k][i]) for k in "uvz")
        if not (math.isfinite(u) and math.isfinite(v) and math.isfinite(z) and z > 0):
            return None
        fx, fy = float(F(c["cam"][0])), float(F(c["cam"][1]))
        hw, up, down = (r(r(f * float(F(p[k]))) / z) for f, k in ((fx, "half_width"), (fy, "above"), (fy, "below")))
        g = brute_grid([r(u - hw), r(v - up), r(u + hw), r(v + down)], 1.0, 1.0, shrink, w, h, p["max_side"])
        return None if g is None else (*g, 1)


def brute_force(c):
    """The definition restated: a python loop over every sampled pixel, strings for the rows."""
    from unina_yolo_dla_amd import engine
    p = c["params"]
    n = min(max(c["count"], 0), cc.MAXD, len(c["dets"]))
    dets, colours = np.zeros(cc.MAXD, dtype=engine.DET_DTYPE), np.zeros(cc.MAXD, dtype=engine.COLOUR_DTYPE)
    head = dict(n_records=n, n_selected=0, n_window=0, n_decided=0, n_class=[0, 0, 0, 0])
    img = c["image"]
    for i in range(n):
        dets[i] = c["dets"][i]
        if p["only_class"] >= 0 and int(c["dets"]["class_id"][i]) != p["only_class"]:
            continue
        head["n_selected"] += 1
        colours["status"][i] = SELECTED
        win = brute_window(c, i)
        if win is None:
            continue
        head["n_window"] += 1
        us, vs, size = win
        cols, rows, taper = len(us), len(vs), p["taper"]
        votes, white, black, n_mask, letters_of = [0, 0, 0], 0, 0, 0, []
        per_row = []
        for k, v in enumerate(vs):
            row = [0, 0, 0, 0, 0, 0]
            for col, u in enumerate(us):
                if abs(2 * col - (cols - 1)) * 256 * rows > cols * (taper * rows + (256 - taper) * (k + 1)):
                    continue
                px = [int(x) for x in img[v, u][:3]]
                R, G, B = (px[2], px[1], px[0]) if p["order"] == 0 else px
                b = cc.scalar_pixel(p, R, G, B)
                if b >= 0:
                    row[b] += 1
                row[5] += 1
            per_row.append(row)
            for b in range(3):
                votes[b] += row[b]
            white, black, n_mask = white + row[3], black + row[4], n_mask + row[5]
        order = sorted(range(3), key=lambda b: (-votes[b], b))
        best, second = order[0], order[1]
        for row in per_row:
            stripe = row[4] if best == 0 else row[3]
            if row[5] > 0 and 2 * row[best] >= row[5]:
                letters_of.append("B")
            elif row[5] > 0 and 2 * stripe >= row[5]:
                letters_of.append("S")
        s = "".join(letters_of)
        n_stripes, seen_b, in_run = 0, False, False
        for k, ch in enumerate(s):                       # a run is counted when it starts behind a B and a B follows somewhere
            if ch == "B":
                seen_b, in_run = True, False
            elif not in_run:
                in_run = True
                n_stripes += 1 if seen_b and "B" in s[k:] else 0
        large = best == 2 and n_stripes >= 2 and p["class_of"][3] >= 0
        index = 3 if large else best
        decided = (n_mask >= p["min_pixels"] and votes[best] * 256 >= p["min_share"] * n_mask and votes[second] * 256 <= p["max_rival"] * votes[best]
                   and votes[best] > 0 and (not p["require_stripe"] or n_stripes >= 1) and p["class_of"][index] >= 0)
        status = WINDOW | SELECTED | (DECIDED if decided else 0) | (LARGE if decided and large else 0) | (SIZE if size else 0) | (best << 8)
        colours[i] = (votes, white, black, n_mask, n_stripes, status)
        if decided:
            dets["class_id"][i] = p["class_of"][index]
            head["n_decided"] += 1
            head["n_class"][index] += 1
    header = np.zeros(1, dtype=engine.COLOUR_HEADER_DTYPE)
    header[0] = (head["n_records"], head["n_selected"], head["n_window"], head["n_decided"], head["n_class"])
    return {"header": header, "dets": dets, "colours": colours}


def check_case(c, want):
    got = brute_force(c)
    for name in NAMES:
        assert got[name].tobytes() == want[name].tobytes(), (c["name"], name, got["header"], want["header"])


def head(out):
    h = out["header"][0]
    return {n: (h[n].tolist() if n == "n_class" else int(h[n])) for n in out["header"].dtype.names}


def random_case(rng, trial):
    """A small image of few distinct channel values (every threshold met exactly, equal channels, equal votes), boxes on a quarter-
    pixel lattice, cones for some point boxes, and parameters drawn per case."""
    h, w, ch = int(rng.integers(1, 40)), int(rng.integers(1, 48)), int(rng.choice([3, 4]))
    values = np.array([0, 25, 50, 51, 59, 60, 96, 128, 149, 150, 200, 220, 255], dtype=np.uint8)
    img = values[rng.integers(0, len(values), (h, w, ch))]
    banded = rng.random() < 0.5
    if banded:                                                                      # rows of one paint each, a pixel in eight left as it was: stripes
        body = "YBO"[int(rng.integers(0, 3))]
        bands = np.array([cc.PAINT[k] for k in body * 4 + "WKG"], dtype=np.uint8)[rng.integers(0, 7, h)]
        keep = rng.random((h, w)) < 0.125
        img[..., :3] = np.where(keep[..., None], img[..., :3], bands[:, None, :])
    m = int(rng.integers(0, 12))
    x1, y1 = rng.integers(-8, 4 * w, m) * 0.25, rng.integers(-8, 4 * h, m) * 0.25
    bw, bh = rng.integers(-2, 4 * w, m) * 0.25, rng.integers(-2, 4 * h, m) * 0.25
    point = rng.random(m) < 0.3
    bw[point], bh[point] = 0.0, 0.0
    dets = cc.records(np.stack([x1, y1, x1 + bw, y1 + bh], axis=1) if m else np.zeros((0, 4)), cls=rng.choice([cc.UNKNOWN, 1], m))
    cones = None if rng.random() < 0.2 else cc.cones_at(x1, y1, rng.choice([0.5, 1.0, 2.0, 8.0, 0.0, cc.NAN], m), valid=rng.integers(0, 3, m))
    lo = rng.integers(0, 1536, 3)
    par = dict(shrink=float(rng.choice([1.0, 0.5, 0.75])), max_side=int(rng.choice([1, 3, 8, 64])), order=int(rng.integers(0, 2)),
               only_class=int(rng.choice([-1, cc.UNKNOWN])), class_of=tuple(int(v) for v in rng.choice([-1, 0, 1, 2, 3], 4)),
               black_max=int(rng.choice([0, 25, 50])), sat_min=int(rng.choice([1, 96, 256])), val_min=int(rng.choice([0, 60, 128])),
               white_min=int(rng.choice([0, 150, 255])), hue_lo=tuple(int(v) for v in lo), hue_hi=tuple(int(v) for v in (lo + rng.integers(-200, 600, 3)) % 1536),
               taper=int(rng.choice([0, 64, 128, 256])), min_pixels=int(rng.choice([1, 4, 12])), min_share=int(rng.choice([0, 96, 128, 256])),
               max_rival=int(rng.choice([0, 128, 256])), require_stripe=int(rng.integers(0, 2)))
    if banded:                                                                      # the default thresholds and ranges read the paints as they are meant
        par = dict(shrink=par["shrink"], max_side=int(rng.choice([8, 64])), only_class=par["only_class"], taper=par["taper"], min_pixels=par["min_pixels"],
                   require_stripe=par["require_stripe"])
    return cc.case(f"random{trial}", dets, img, cones=cones, count=int(rng.choice([m, m, m + 3, max(m - 1, 0)])), pitch=w * ch + int(rng.integers(0, 4)),
                   offset=int(rng.integers(0, 4)), **par)


def random_cases():
    rng = np.random.default_rng(11)
    return [random_case(rng, t) for t in range(200)]


@pytest.fixture(scope="module")
def edges(pkg):
    return {c["name"]: (c, out) for c, out in cc.cached("edges", cc.edge_cases)}


@pytest.fixture(scope="module")
def rendered(pkg):
    return cc.cached("rendered", cc.rendered_cases)


@pytest.fixture(scope="module")
def randoms(pkg):
    return cc.cached("random", random_cases)


def test_twin_equals_the_scalar_restatement_on_the_constructed_cases(edges, rendered):
    assert len(edges) == 44
    for c, out in list(edges.values()) + rendered:
        check_case(c, out)


def test_twin_equals_the_scalar_restatement_on_random_tie_heavy_inputs(randoms):
    seen = dict(window=0, size=0, decided=0, large=0, stripes=0, undecided=0)
    for c, out in randoms:
        check_case(c, out)
        st = out["colours"]["status"]
        seen["window"] += int(((st & WINDOW) != 0).sum())
        seen["size"] += int(((st & SIZE) != 0).sum())
        seen["decided"] += int(((st & DECIDED) != 0).sum())
        seen["large"] += int(((st & LARGE) != 0).sum())
        seen["stripes"] += int((out["colours"]["n_stripes"] > 0).sum())
        seen["undecided"] += int((((st & WINDOW) != 0) & ((st & DECIDED) == 0)).sum())
    assert seen["window"] > 300 and seen["size"] > 30 and seen["decided"] > 30 and seen["undecided"] > 100 and seen["stripes"] > 30 and seen["large"] > 0, seen


def test_the_cases_are_what_they_claim(edges):
    h = {k: head(v[1]) for k, v in edges.items()}
    o = {k: v[1] for k, v in edges.items()}
    col = {k: v[1]["colours"] for k, v in edges.items()}
    status = lambda name, i: int(col[name]["status"][i])                                          # noqa: E731
    # counts
    for n in (0, 1, 63, 64, 65, 1024, 5000, -7):
        m = min(max(n, 0), 1024)
        x = h[f"count{n}"]
        assert (x["n_records"], x["n_selected"], x["n_window"]) == (m, m, m), x
        assert (col[f"count{n}"]["n_mask"][:m] > 0).all() and not col[f"count{n}"][m:].view(np.uint8).any() and not o[f"count{n}"]["dets"][m:].view(np.uint8).any()
    assert h["count1024"]["n_decided"] > 300 and all(v > 30 for v in h["count1024"]["n_class"][:3]) and h["count5000"] == h["count1024"]
    # windows
    names = edges["windows"][0]["names"]
    at = {n: i for i, n in enumerate(names)}
    w = col["windows"]
    mask_of = lambda n: int(w["n_mask"][at[n]])                                                    # noqa: E731
    full = dict(edges["windows"][0]["params"], taper=256)
    wide = cc.run_twin(dict(edges["windows"][0], params=full))["colours"]["n_mask"]                # taper = 256: n_mask = cols * rows
    assert [int(wide[at[n]]) for n in ("one_pixel", "column_1x64", "row_64x1", "full_64x64", "whole_image_stride_4x3", "wide_65_stride_2", "last_pixel",
                                       "first_pixel")] == [1, 64, 64, 4096, 4096, 33 * 38, 24, 1]
    assert [int(wide[at[n]]) for n in ("clip_left", "clip_right", "clip_top", "clip_bottom")] == [13 * 21, 16 * 21, 21 * 10, 21 * 12]
    for n in ("outside_right", "outside_above", "nan_box", "inf_box", "inverted_x", "inverted_y", "size_invalid", "size_z_zero", "size_z_negative", "size_z_nan",
              "size_u_nan", "size_v_inf", "size_outside", "size_overflows"):
        assert status("windows", at[n]) == SELECTED and not w[at[n]].tobytes()[:28].strip(b"\0"), n
        assert o["windows"]["dets"][at[n]].tobytes() == edges["windows"][0]["dets"][at[n]].tobytes()
    for n in ("size_near", "size_far", "size_one_pixel", "size_clipped", "size_huge"):
        assert status("windows", at[n]) & (WINDOW | SIZE) == WINDOW | SIZE and mask_of(n) > 0, n
        assert status("windows_no_cones", at[n]) == SELECTED
    assert int(wide[at["size_near"]]) == 30 * 43 and int(wide[at["size_one_pixel"]]) == 1     # columns 113..142, rows 73..115: half width 14.592, 22.4 up and 19.2 down at 2 m
    assert all(status("windows", at[n]) & SIZE == 0 for n in cc.WINDOW_BOXES)
    assert h["windows"]["n_window"] == 17 and h["windows_no_cones"]["n_window"] == 12 and h["windows"]["n_selected"] == 31
    assert int(wide[at["size_huge"]]) == 4096                                                      # half extents of 2.9e31 pixels, clipped to the image
    x = cc.run_twin(dict(edges["stride5"][0], params=dict(edges["stride5"][0]["params"], taper=256)))["colours"]["n_mask"]
    assert x[:2].tolist() == [48 * 48, 48 * 34]                                                    # strides 5 x 4 (192 rows) and 5 x 3 (101 rows)
    assert col["max_side_1"]["n_mask"][:2].tolist() == [1, 1]
    assert [status("image_1x1", i) & WINDOW for i in range(3)] == [1, 1, 0] and col["image_1x1"]["votes"][:2, 0].tolist() == [1, 1]
    # images: the same pixels in every layout give the same answers
    ref = o["scene_c3_o1"]
    for ch in (3, 4):
        for order in (0, 1):
            for tail in ("", "_odd"):
                name = f"scene_c{ch}_o{order}{tail}"
                c = edges[name][0]
                assert all(o[name][k].tobytes() == ref[k].tobytes() for k in NAMES), name
                assert c["image"].shape[2] == ch and c["params"]["order"] == order
                assert (c["pitch"] % 4 != 0 and c["offset"] % 2 == 1) == bool(tail)
    assert ref["header"].tobytes() == o["windows"]["header"].tobytes() and h["scene_c3_o1"]["n_decided"] >= 3
    assert all(o["scene_c4_pitch_aligned_offset_2"][k].tobytes() == ref[k].tobytes() for k in NAMES)
    c = edges["scene_c3_width_253"][0]
    assert len(cc.image_bytes(c)) == 191 * 760 + 253 * 3 and (cc.image_bytes(c)[-3:] == c["image"][-1, -1]).all()
    assert len(cc.image_bytes(edges["scene_c4_o0_odd"][0])) == 1 + 191 * 1030 + 1024
    # the pixel's class
    bins = lambda rec: [int(v) for v in (*rec["votes"], rec["n_white"], rec["n_black"])]          # noqa: E731
    def bin_of(rec):                                                                                # noqa: E306
        b = bins(rec)
        assert sum(b) <= 1 and rec["n_mask"] == 1
        return b.index(1) if 1 in b else -1
    for name in ("pixels", "pixels_c3_o0", "pixels_c4_o0", "pixels_c4_o1"):
        assert [bin_of(col[name][i]) for i in range(len(cc.PIXELS))] == [v[1] for v in cc.PIXELS.values()], name
    assert [cc.scalar_hue(*cc.PIXELS[k][0]) for k in ("branch_r_g_ge_b", "branch_r_g_lt_b", "branch_g_b_ge_r", "branch_g_b_lt_r", "branch_b_r_ge_g",
                                                     "branch_b_r_lt_g", "max_is_r_and_g")] == [97, 1408, 640, 269, 1152, 949, 256]
    R, G, B = cc.PIXELS["sat_on_bound"][0]
    assert (R - B) * 256 == 96 * R and (cc.PIXELS["sat_one_below"][0][0] - cc.PIXELS["sat_one_below"][0][2]) * 256 == 96 * R - 256
    for name, table in (("hue_bounds", cc.HUE_BOUNDS), ("hue_wrap", cc.WRAP_HUES), ("hue_overlap", cc.OVERLAP_HUES)):
        assert [cc.scalar_hue(*cc.pixel_with_hue(hh)) for hh in table] == list(table)
        assert [bin_of(col[name][i]) for i in range(len(table))] == list(table.values()), name
    # the silhouette
    assert col["taper256"]["n_mask"][:5].tolist() == [40 * 56, 64, 64, 63, 4]
    assert col["taper0"]["n_mask"][1:3].tolist() == [64, 64] and col["taper64"]["n_mask"][1:3].tolist() == [64, 64]    # cols = 1: every row; rows = 1: the base
    assert col["taper0"]["n_mask"][0] < col["taper64"]["n_mask"][0] < 40 * 56 and abs(int(col["taper0"]["n_mask"][0]) - 20 * 57) <= 60
    # the decision
    dw = cc.decision_windows()
    assert [bool(status("decision", i) & DECIDED) for i in range(len(dw))] == [v[1] for v in dw.values()]
    d = {n: col["decision"][i] for i, n in enumerate(dw)}
    assert d["mask_on_min_pixels"]["n_mask"] == 16 and d["mask_one_below"]["n_mask"] == 15
    assert d["share_equal"]["votes"][0] * 256 == 96 * 16 and d["rival_equal"]["votes"][1] * 256 == 128 * d["rival_equal"]["votes"][0]
    assert d["two_equal"]["votes"].tolist() == [0, 6, 6] and d["two_equal"]["status"] >> 8 == 1                       # blue before orange
    assert d["three_equal"]["votes"].tolist() == [5, 5, 5] and d["three_equal"]["status"] >> 8 == 0
    assert d["no_coloured_pixel"]["votes"].tolist() == [0, 0, 0] and (d["no_coloured_pixel"]["n_white"], d["no_coloured_pixel"]["n_black"]) == (6, 5)
    assert d["magenta_only"]["votes"].tolist() == [0, 0, 0] and d["magenta_only"]["n_mask"] == 16
    loose = {n: int(col["decision_rival_256"]["status"][i]) for i, n in enumerate(dw)}
    assert loose["two_equal"] & DECIDED and loose["three_equal"] & DECIDED and loose["rival_one_vote_over"] & DECIDED
    got = o["decision_rival_256"]["dets"]["class_id"]
    assert got[list(dw).index("two_equal")] == 1 and got[list(dw).index("three_equal")] == 0 and got[list(dw).index("no_coloured_pixel")] == cc.UNKNOWN
    # the stripes
    ns = len(cc.STRIPE_STRINGS)
    assert col["stripes"]["n_stripes"][:ns].tolist() == [v[1] for v in cc.STRIPE_STRINGS.values()]
    from unina_yolo_dla_amd import colour
    assert [colour.stripes_numpy(v[0]) for v in cc.STRIPE_STRINGS.values()] == [v[1] for v in cc.STRIPE_STRINGS.values()]
    half = col["stripes"][ns]                                                                     # rows OW OO WW OW OO: B B S B B
    assert half["n_stripes"] == 1 and (half["votes"][2], half["n_white"]) == (6, 4)
    assert col["stripes"]["n_stripes"][ns + 1:ns + 5].tolist() == [1, 0, 1, 0]                     # yellow: black stripes; blue: white ones
    cls = o["stripes"]["dets"]["class_id"][:ns].tolist()
    assert cls == [3 if v[1] >= 2 else (2 if "B" in v[0] else cc.UNKNOWN) for v in cc.STRIPE_STRINGS.values()]
    large = (col["stripes"]["status"][:ns] & LARGE) != 0
    assert large.tolist() == [v[1] >= 2 for v in cc.STRIPE_STRINGS.values()] and h["stripes"]["n_class"][3] == 3
    req = col["stripes_required"]["status"][:ns]
    assert ((req & DECIDED) != 0).tolist() == [v[1] >= 1 for v in cc.STRIPE_STRINGS.values()]
    assert ((col["stripes_required"]["status"][ns + 1:ns + 5] & DECIDED) != 0).tolist() == [True, False, True, False]
    nb = o["stripes_no_body_class"]
    assert nb["dets"]["class_id"][:ns].tolist() == [3 if v[1] >= 2 else cc.UNKNOWN for v in cc.STRIPE_STRINGS.values()]
    nl = o["stripes_no_large_class"]
    assert nl["dets"]["class_id"][:ns].tolist() == [2 if "B" in v[0] else cc.UNKNOWN for v in cc.STRIPE_STRINGS.values()] and not (nl["colours"]["status"] & LARGE).any()
    assert h["stripes_no_class_at_all"]["n_decided"] == 0 and h["stripes_no_class_at_all"]["n_window"] == 16
    assert o["stripes_no_class_at_all"]["dets"].tobytes()[:32 * 16] == edges["stripes"][0]["dets"].tobytes()
    # selection
    src = edges["only_unknown"][0]["dets"]
    x = o["only_unknown"]
    chosen = np.arange(64) % 3 == 0
    assert h["only_unknown"]["n_selected"] == 22 and ((x["colours"]["status"][:64] & SELECTED) != 0).tolist() == chosen.tolist()
    assert x["dets"][:64][~chosen].tobytes() == src[~chosen].tobytes() and not x["colours"][:64][~chosen].view(np.uint8).any()
    assert np.isnan(src["x1"][1]) and src.view(np.uint32).reshape(-1, 8)[1, 0] == 0x7fc12345 and h["only_unknown"]["n_decided"] > 5
    assert (x["dets"]["class_id"][:64][chosen] != cc.UNKNOWN).sum() == h["only_unknown"]["n_decided"]
    assert h["every_record"]["n_selected"] == 64 and h["every_record"]["n_window"] == 43 and h["only_class_absent"]["n_selected"] == 0
    assert o["only_class_absent"]["dets"][:64].tobytes() == src.tobytes()


def test_rendered_cones_are_decided_with_the_right_class_and_stripe_count(rendered):
    """The table the defaults were chosen on: yellow, blue, orange and large orange cones of 6 x 9 up to 40 x 56 pixels on asphalt,
    grass, sky and near-black, +-12 noise: all 64 DECIDED with the right class and stripe count. A 4 x 6 large cone shows one
    stripe, as a 6-row raster must."""
    n = 0
    for c, out in rendered:
        assert len(c["truth"]) == 16
        for i, (index, stripes) in enumerate(c["truth"]):
            rec = out["colours"][i]
            assert rec["status"] & DECIDED and out["dets"]["class_id"][i] == cc.CLASS_OF[index] and rec["n_stripes"] == stripes, (c["name"], i, rec)
            assert bool(rec["status"] & LARGE) == (index == 3)
            n += 1
    assert n == 64
    small, = cc.rendered_cases(sizes=((4, 6),))[:1]
    out = cc.run_twin(small)
    assert out["colours"]["n_stripes"][3] == 1 and small["truth"][3] == (3, 2)


# ---------------------------------------------------------------- csrc/colour_math.h on the host
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("colour_math_host")
    return hostprog.build_pair(d, "colour_math_host.cpp"), d


def payload(c):
    from unina_yolo_dla_amd import colour, engine
    h, w, ch = c["image"].shape
    img = cc.image_bytes(c)
    m = len(c["dets"])
    head = struct.pack("<10i2f", 0x434f4c31, c["count"], m, int(c["cones"] is not None), w, h, c["pitch"], ch, c["offset"], len(img), c["cam"][0], c["cam"][1])
    cones = b"" if c["cones"] is None else np.ascontiguousarray(c["cones"], dtype=engine.CONE3D_DTYPE).tobytes()
    return head + bytes(colour.make_colour_params(**c["params"])) + np.ascontiguousarray(c["dets"]).tobytes() + cones + img.tobytes()


def test_host_math_equals_the_twin_on_every_case(edges, rendered, randoms, drivers):
    """Both builds of the stand-alone program, the sanitised one included, on the constructed cases (odd pitches and addresses,
    3-channel images whose last pixel ends the buffer), the rendered cones and the random cases."""
    for c, want in list(edges.values()) + rendered + randoms:
        got = hostprog.run_pair(*drivers, payload(c), dtype=np.uint8)
        assert got.tobytes() == want["header"].tobytes() + want["dets"].tobytes() + want["colours"].tobytes(), c["name"]


# ---------------------------------------------------------------- the entry point's argument checks
def test_every_bad_argument_is_refused_before_any_hip_call(pkg):
    """UNINA_ERR_ARG (4) for each refusal the header lists, in a process that has no device: a HIP call in front of the checks
    would answer 3 (UNINA_ERR_HIP) instead. The pointers are never dereferenced by a refused call."""
    from unina_yolo_dla_amd import build, colour, engine
    build.build_native()
    L = engine.load_library()
    nan, inf = float("nan"), float("inf")
    names = ("dets", "count", "cones", "data", "out_dets", "colours", "header")
    good = {n: 0x100000 * (k + 1) for k, n in enumerate(names)}                    # 1 MiB apart: nothing overlaps

    def call(img=True, cam=cc.CAM, par=True, width=256, height=192, pitch=768, channels=3, **kw):
        a = dict(good)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        image = engine.Image(width, height, pitch, channels, a["data"])
        pin = engine.Pinhole(*cam) if cam is not None else None
        pp = colour.make_colour_params(**cc.params(**kw))
        return L.unina_colour_async(a["dets"], a["count"], a["cones"], C.byref(image) if img else None, C.byref(pin) if pin is not None else None,
                                    C.byref(pp) if par else None, a["out_dets"], a["colours"], a["header"], None)

    def with_value(values, i, v):
        q = list(values)
        q[i] = v
        return tuple(q)

    bad = [dict(img=False), dict(cam=None), dict(par=False), *[{n: None} for n in names if n != "cones"],
           *[{n: good[n] + off} for n in ("dets", "cones", "out_dets", "colours", "header") for off in (4, 8)], *[dict(count=good["count"] + off) for off in (1, 2)],
           dict(channels=1), dict(channels=2), dict(channels=5), dict(width=0), dict(width=16385, pitch=16385 * 3), dict(height=0), dict(height=16385),
           dict(pitch=767), dict(channels=4, pitch=1023), dict(pitch=-768),
           *[dict(cam=with_value(cc.CAM, i, v)) for i in range(4) for v in (nan, inf, -inf)], dict(cam=with_value(cc.CAM, 0, 0.0)),
           dict(cam=with_value(cc.CAM, 1, -256.0)),
           *[{k: v} for k in ("sx", "sy") for v in (0.0, -1.0, nan, inf)], *[dict(shrink=v) for v in (0.0, -0.5, 1.5, nan, inf)],
           *[{k: v} for k in ("half_width", "above", "below") for v in (-0.5, nan, inf, -inf)],
           dict(max_side=0), dict(max_side=65), dict(max_side=-1), dict(order=2), dict(order=-1),
           *[{k: v} for k in ("black_max", "val_min", "white_min") for v in (-1, 256)], dict(sat_min=0), dict(sat_min=257),
           *[{k: with_value(cc.DEFAULTS[k], i, v)} for k in ("hue_lo", "hue_hi") for i in range(3) for v in (-1, 1536)],
           *[{k: v} for k in ("taper", "min_share", "max_rival") for v in (-1, 257)], dict(min_pixels=0), dict(min_pixels=-3),
           # partial overlaps over the MAX_DETECTIONS extents; d_out_dets == d_dets alone is allowed
           dict(out_dets=good["dets"] + 32), dict(out_dets=good["dets"] + 32768 - 32), dict(dets=good["out_dets"] + 32768 - 32),
           dict(colours=good["dets"]), dict(colours=good["dets"] + 32768 - 32), dict(dets=good["colours"] + 32768 - 32),
           dict(colours=good["out_dets"]), dict(colours=good["out_dets"] + 32768 - 32), dict(out_dets=good["colours"] + 32768 - 32),
           dict(out_dets=good["dets"], colours=good["dets"])]
    for kw in bad:
        assert call(**kw) == 4, kw
    import torch
    if not torch.cuda.is_available():
        # the good calls reach HIP, which has no device here: the checks above sit in front of it
        assert call() == 3 and call(cones=None) == 3 and call(out_dets=good["dets"]) == 3
        assert call(data=good["data"] + 1, pitch=771) == 3 and call(channels=4, pitch=1025, data=good["data"] + 3) == 3      # no alignment of data or pitch
        assert call(width=16384, height=16384, pitch=16384 * 3) == 3 and call(width=1, height=1, pitch=3) == 3
        assert call(shrink=1.0, half_width=0.0, above=0.0, below=0.0, max_side=1, sat_min=256, taper=0, min_share=0, max_rival=0, only_class=-5,
                    class_of=(-1, -1, -1, -1)) == 3


def test_layouts_and_the_header_stays_plain_c(pkg, tmp_path):
    from unina_yolo_dla_amd import colour, engine
    P = engine.ColourParams
    assert C.sizeof(P) == 112 and (P.sx.offset, P.below.offset, P.max_side.offset, P.order.offset, P.only_class.offset, P.class_of.offset) == (0, 20, 24, 28, 32, 36)
    assert (P.black_max.offset, P.white_min.offset, P.hue_lo.offset, P.hue_hi.offset, P.taper.offset, P.require_stripe.offset) == (52, 64, 68, 80, 92, 108)
    d = colour.COLOUR_DTYPE
    assert d.itemsize == 32 and [d.fields[n][1] for n in ("votes", "n_white", "n_black", "n_mask", "n_stripes", "status")] == [0, 12, 16, 20, 24, 28]
    d = colour.COLOUR_HEADER_DTYPE
    assert d.itemsize == 32 and [d.fields[n][1] for n in ("n_records", "n_selected", "n_window", "n_decided", "n_class")] == [0, 4, 8, 12, 16]
    assert (engine.COLOUR_BGR, engine.COLOUR_RGB) == (0, 1) and "unina_colour_async" in engine.ABI_SYMBOLS
    assert (engine.COLOUR_WINDOW, engine.COLOUR_SELECTED, engine.COLOUR_DECIDED, engine.COLOUR_LARGE, engine.COLOUR_SIZE_WINDOW) == (1, 2, 4, 8, 16)
    p = colour.make_colour_params()
    assert (p.black_max, p.sat_min, p.val_min, p.white_min, p.taper, p.min_pixels, p.min_share, p.max_rival, p.require_stripe) == (50, 96, 60, 150, 64, 12, 96, 128, 0)
    assert (list(p.hue_lo), list(p.hue_hi)) == ([171, 850, 20], [300, 1110, 170])
    assert [round(v, 6) for v in (p.half_width, p.above, p.below)] == [0.114, 0.175, 0.15]
    hostprog.assert_header_is_c99()
    hostprog.compile_c99(tmp_path, 'typedef char par112[(sizeof(unina_colour_params) == 112) ? 1 : -1];\n'
                                   'typedef char side24[(offsetof(unina_colour_params, max_side) == 24) ? 1 : -1];\n'
                                   'typedef char class36[(offsetof(unina_colour_params, class_of) == 36) ? 1 : -1];\n'
                                   'typedef char lo68[(offsetof(unina_colour_params, hue_lo) == 68) ? 1 : -1];\n'
                                   'typedef char stripe108[(offsetof(unina_colour_params, require_stripe) == 108) ? 1 : -1];\n'
                                   'typedef char rec32[(sizeof(unina_colour) == 32) ? 1 : -1];\n'
                                   'typedef char status28[(offsetof(unina_colour, status) == 28) ? 1 : -1];\n'
                                   'typedef char head32[(sizeof(unina_colour_header) == 32) ? 1 : -1];\n'
                                   'typedef char class16[(offsetof(unina_colour_header, n_class) == 16) ? 1 : -1];\n'
                                   'typedef char codes[(UNINA_COLOUR_BGR == 0 && UNINA_COLOUR_RGB == 1 && UNINA_COLOUR_WINDOW == 1 && UNINA_COLOUR_SELECTED == 2 &&\n'
                                   '                    UNINA_COLOUR_DECIDED == 4 && UNINA_COLOUR_LARGE == 8 && UNINA_COLOUR_SIZE_WINDOW == 16) ? 1 : -1];\n'
                                   'int use(GpuDetection *d, const int *n, const unina_cone3d *c, const uint8_t *pixels, unina_colour *col, unina_colour_header *h) {\n'
                                   '  unina_colour_params p = {1, 1, 1, 0.114f, 0.175f, 0.15f, 64, UNINA_COLOUR_BGR, 9, {0, 1, 2, 3}, 50, 96, 60, 150,\n'
                                   '                           {171, 850, 20}, {300, 1110, 170}, 64, 12, 96, 128, 0};\n'
                                   '  unina_image img = {1280, 720, 3840, 3, 0};\n'
                                   '  unina_pinhole cam = {600, 600, 640, 360};\n'
                                   '  img.data = pixels;\n'
                                   '  return unina_colour_async(d, n, c, &img, &cam, &p, d, col, h, 0);\n}\n')
