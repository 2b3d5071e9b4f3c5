"""The cases of tests/stem_source_cases.py without a GPU: that each is what its name says (the CameraKind frame_kind chooses, the
partial-tile arithmetic, odd origins, the letterbox rectangles on non-square destinations), that the numpy twins they are held
to equal the scalar CPU oracle where the oracle defines the operation, that the thresholds of tests/test_gpu_stem_sources.py keep a
record on every compared tensor (a condition on the CPU oracle, not a measurement of an engine), and camera.unmap_boxes on
non-square networks against a float64 inversion of the letterbox."""
import ctypes as C

import numpy as np
import pytest

import hostprog
import stem_source_cases as S
from frame_child import BGRA, NV12


@pytest.fixture(scope="module")
def twin(pkg):
    from unina_yolo_dla_amd import camera
    return camera


@pytest.fixture(scope="module")
def mine(pkg):
    from unina_yolo_dla_amd import mine
    return mine


@pytest.fixture(scope="module")
def engine(pkg):
    from unina_yolo_dla_amd import engine
    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def slicing(pkg):
    from unina_yolo_dla_amd import slicing
    return slicing


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("stem_sources_host")
    return hostprog.build_pair(d, "stem_sources_host.cpp"), d


# ------------------------------------------------------------------------------------ the cases are what their names say

def test_sizes_cover_the_partial_tile_arithmetic():
    """(columns of the last stem tile, footprint columns beyond W): nothing whole at 16 x 16, one partial tile at 80 x 112, a
    whole tile then 16 columns at 96 x 160 (footprint columns 124..255 of 160), two whole tiles and 8 columns at 32 x 272."""
    assert S.SIZES == ((16, 16), (80, 112), (96, 160), (32, 272))
    assert [S.partial_tile(s) for s in S.SIZES] == [(8, 112), (56, 16), (16, 96), (8, 112)]
    for H, W in S.SIZES:
        wo, ho = W // 2, H // 2
        assert H % 16 == 0 and W % 16 == 0 and ho % S.TILE_H == 0           # the 2-row tile is never partial
        assert wo % S.TILE_W != 0                                           # the last tile column always is
        assert wo % S.TILE_W == S.partial_tile((H, W))[0]
    assert [(W // 2) // S.TILE_W for _H, W in S.SIZES] == [0, 0, 1, 2]      # whole tile columns in front of it
    H, W = 96, 160
    tx0 = 64
    assert (2 * tx0 - 4, 2 * tx0 - 4 + 131) == (124, 255)


def test_frame_kind_chooses_the_named_kind(drivers, mine, engine):
    """frame_kind (csrc/camera_source.h, compiled for the host) on every case's geometry, the letterbox rectangle from
    unina_letterbox_geometry, which equals mine.letterbox_geometry's on these non-square destinations."""
    L = engine.load_library()
    rows, want, names = [], [], []
    for size in S.SIZES:
        H, W = size
        for c in S.cases(size):
            if c.geometry == "tiled":
                regions = [(w, h) for _x, _y, w, h in c.tiles]
                box = None
            else:
                regions = [(c.w, c.h)]
                box = None
                if c.geometry == "letterbox":
                    lb = engine.Letterbox()
                    assert L.unina_letterbox_geometry(c.w, c.h, W, H, C.byref(lb)) == 0
                    box = (lb.new_w, lb.new_h, lb.left, lb.top)
                    assert box == mine.letterbox_geometry(c.w, c.h, W, H), S.case_id(c)
            for (w, h), k in zip(regions, S.expected_kinds(c)):
                rows.append([c.fmt, w, h, W, H, int(box is not None), *(box or (0, 0, 0, 0))])
                want.append(k)
                names.append(S.case_id(c))
    payload = np.int32(len(rows)).tobytes() + np.asarray(rows, dtype=np.int32).tobytes()
    got = hostprog.run_pair(*drivers, payload)
    bad = [(n, int(g), w) for n, g, w in zip(names, got, want) if g != w]
    assert len(got) == len(want) and not bad, bad[:8]
    assert set(want) == set(range(1, 10))                                   # every camera kind is among the cases


@pytest.mark.parametrize("size", S.SIZES, ids=S.SIZE_ID)
def test_cameras_are_what_their_names_say(mine, size):
    H, W = size
    cams = S.cameras(size)
    assert all((h, w) == (H, W) for _n, h, w, _m in cams["tap"])
    assert [m for _n, _h, _w, m in cams["tap"]] == [False, True]            # wide loads | byte loads
    (_d, dh, dw, _), (_u, uh, uw, _) = cams["resize"]
    assert dh > H and dw > W and dw * H != dh * W                            # down-scale, the ratios differ
    assert uh < H and uw < W and uh % 2 == 1 and uw % 2 == 1 and uw * H != uh * W    # up-scale, odd both ways, another aspect
    boxes = {n: mine.letterbox_geometry(w, h, W, H) for n, h, w, _m in cams["letterbox"]}
    new_w, new_h, left, top = boxes["wide"]
    assert new_w == W and left == 0 and top > 0 and new_h < H                # bars above and below
    new_w, new_h, left, top = boxes["tall"]
    assert new_h == H and top == 0 and left > 0 and new_w < W                # bars left and right
    new_w, new_h, left, top = boxes["r1"]
    r1 = [c for c in cams["letterbox"] if c[0] == "r1"][0]
    assert (new_w, new_h) == (r1[2], r1[1]) and left == 0                    # r == 1: the frame is tapped, not resized
    assert (H - new_h) % 2 == 1 and top != H - new_h - top                   # an odd remainder: top != bottom
    for n, (new_w, new_h, _l, _t) in boxes.items():
        assert new_w * H != new_h * W, n                                     # no inner rectangle has the network's aspect
    (_o, fh, fw, _), = cams["tiled"]
    assert fh % 2 == 1 and fw % 2 == 1
    a, b, c = S.tiles_of(size)
    assert a[2:] == (W, H) and a[0] % 2 == 1 and a[1] % 2 == 1               # the network's size at an odd origin
    assert b[2] * H != b[3] * W and b[2:] != (W, H)                          # resized, w / W != h / H
    assert c[2:] == (W, H) and (c[0] + c[2], c[1] + c[3]) == (fw, fh)        # ends at the frame's corner
    for x, y, w, h in (a, b, c):
        assert x >= 0 and y >= 0 and x + w <= fw and y + h <= fh


def test_formats_and_case_counts():
    from frame_child import BGGR, GBRG, GRBG, RGB, RGBA, RGGB, UYVY, YUYV
    assert set(S.ALL_FORMATS) == {BGRA, NV12, YUYV, UYVY, RGB, RGBA, RGGB, BGGR, GRBG, GBRG}
    for fmts in (S.BOX_FORMATS, S.TILED_FORMATS):
        assert {BGRA, NV12} <= set(fmts) and set(fmts) & {YUYV, UYVY} and set(fmts) & {RGGB, BGGR, GRBG, GBRG}
    for size in S.SIZES:
        assert len(S.cases(size)) == 2 * 10 + 2 * 10 + 3 * 4 + 4
        assert len({S.case_id(c) for c in S.cases(size)}) == len(S.cases(size))
    child = S.child_cases()
    assert len(child) * 3 >= sum(len(S.cases(s)) for s in S.SIZES) - 8
    assert {(c.size, c.geometry) for c in child} == {(s, g) for s in S.SIZES for g in S.GEOMETRIES}
    assert {c.fmt for c in child} == set(S.ALL_FORMATS)


# ------------------------------------------------------------------------------------ twin against oracle

@pytest.mark.parametrize("size", S.SIZES, ids=S.SIZE_ID)
def test_twin_tensors_equal_the_oracle_where_it_defines_the_operation(twin, oracle_mod, size):
    """Plain and resized whole BGRA frames against oracle.preprocess_bgra, plain NV12 frames against oracle.preprocess_nv12 (the
    reference has no NV12 resize), byte for byte."""
    n = 0
    for c in S.cases(size, formats=(BGRA, NV12)):
        if c.geometry not in ("tap", "resize"):
            continue
        p = S.planes(twin, c)
        x, = S.reference_tensors(twin, c, p)
        assert x.shape == (3,) + size and x.dtype == np.float32
        if c.fmt == BGRA:
            want = oracle_mod.preprocess_bgra(p) if c.geometry == "tap" else oracle_mod.preprocess_bgra(p, dst_hw=size)
        elif c.geometry == "tap":
            want = oracle_mod.preprocess_nv12(*p)
        else:
            continue
        assert x.tobytes() == want.tobytes(), S.case_id(c)
        n += 1
    assert n == 2 + 2 + 2                                                   # BGRA tap x 2, BGRA resize x 2, NV12 tap x 2


# ------------------------------------------------------------------------------------ the threshold is a condition

def _oracle_records(pkg, oracle_mod, oracle_sd7, x, conf):
    heads = oracle_mod.forward(oracle_sd7, x)
    return oracle_mod.postprocess([heads[n] for n in pkg.graph.OUTPUT_NAMES], conf, S.IOU, S.Q)[0]


@pytest.mark.parametrize("size", S.SIZES, ids=S.SIZE_ID)
def test_the_oracle_alone_keeps_records_on_every_compared_tensor(pkg, twin, slicing, oracle_mod, oracle_sd7, size):
    """On every tensor whose record list tests/test_gpu_stem_sources.py compares -- every case, every tile of a tiled one --
    oracle.forward + oracle.postprocess (fp32) keep between 1 and 1024 records at CONF[size], the strongest at least 0.03 above
    the threshold; so every tile's count fits its slot. On the CPU oracle's own records, the tiled cases' merge has at least two
    contributing tiles and suppresses at least one record (the GPU test asserts the same on the engine's counts)."""
    conf = S.CONF[size]
    lo = (None, 9.0)
    kept = []
    for c in S.cases(size):
        xs = S.reference_tensors(twin, c)
        assert len(xs) == (3 if c.geometry == "tiled" else 1)
        per_tile = []
        for t, x in enumerate(xs):
            assert x.shape == (3,) + size
            d = _oracle_records(pkg, oracle_mod, oracle_sd7, x, conf)
            top = float(d["confidence"].max()) if len(d) else 0.0
            if top < lo[1]:
                lo = (S.case_id(c), top)
            kept.append(len(d))
            assert 1 <= len(d) <= S.MAXD and top >= conf + 0.03, (S.case_id(c), t, len(d), top)
            per_tile.append(d)
        if c.geometry == "tiled":
            slots = np.zeros((len(xs), S.MAXD), dtype=slicing.DET_DTYPE)
            for t, d in enumerate(per_tile):
                slots[t, :len(d)] = d
            counts = [len(d) for d in per_tile]
            merged = slicing.merge_numpy(slots, counts, c.tiles, S.MERGE, net_w=size[1], net_h=size[0])
            print(S.case_id(c), "oracle per-tile counts", counts, "merged", len(merged))
            assert sum(n > 0 for n in counts) >= 2 and len(merged) < sum(counts), (S.case_id(c), counts, len(merged))
    print(S.SIZE_ID(size), "records per tensor", min(kept), "..", max(kept), "weakest strongest record", lo)


# ------------------------------------------------------------------------------------ the box map on non-square networks

@pytest.mark.parametrize("size", S.SIZES[1:], ids=S.SIZE_ID)
def test_unmap_boxes_inverts_the_letterbox_on_non_square_networks(twin, mine, engine, size):
    """camera.unmap_boxes(dets, src_w, src_h, W, H) against the inversion of the paste in float64: X = (x - left) * src_w / new_w,
    Y = (y - top) * src_h / new_h. The fp32 form rounds three times per coordinate (the difference, the scale, the product),
    each by at most 2^-24 relative: |X32 - X| <= 3 * 2^-24 * |X| (+ second-order terms, covered by the factor 3.001). Hand-placed
    records: the inner rectangle itself, one on each bar edge, one over the padding, one at fractional positions."""
    H, W = size
    for name, h, w, _m in S.cameras(size)["letterbox"]:
        new_w, new_h, left, top = mine.letterbox_geometry(w, h, W, H)
        recs = [(left, top, left + new_w, top + new_h),                                # the inner rectangle: the whole frame
                (left, top + 1.5, left + 0.375 * new_w, top + 0.5 * new_h),            # on the left bar's edge
                (left + 0.25 * new_w, top + 2.0, left + new_w, top + 0.75 * new_h),    # on the right bar's edge
                (left + 1.0, top, left + 0.5 * new_w, top + 3.25),                     # on the upper bar's edge
                (left + 2.5, top + 0.125 * new_h, left + 7.0, top + new_h),            # on the lower bar's edge
                (-3.5, -1.25, W + 2.0, H + 6.5),                                       # over the padding: no clamp
                (left + 1.0 / 3.0, top + 2.0 / 7.0, left + new_w / 3.0, top + new_h / 1.7)]
        d = np.zeros(len(recs), dtype=engine.DET_DTYPE)
        for i, r in enumerate(recs):
            d[i] = (*r, 0.5, i % 4, 1, 0)
        m = twin.unmap_boxes(d, w, h, W, H)
        for i in range(len(d)):
            for k, off, num, den in (("x1", left, w, new_w), ("y1", top, h, new_h), ("x2", left, w, new_w), ("y2", top, h, new_h)):
                want = (float(d[i][k]) - off) * num / den                              # float64 on the stored fp32 coordinate
                assert abs(float(m[i][k]) - want) <= 3.001 * 2.0 ** -24 * abs(want), (name, i, k, float(m[i][k]), want)
        assert m[0]["x1"] == 0.0 and m[0]["y1"] == 0.0
        assert left != top                                   # the two axes' offsets differ: a swapped pair is far outside the bound
        for k in ("confidence", "class_id", "valid", "_pad"):
            assert np.array_equal(m[k], d[k])
