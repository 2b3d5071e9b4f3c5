"""Sliced inference without a GPU: the slicing (Python and C ABI) and the numpy merge against the reference's recorded
results (tests/golden/tiled_slices.npz, made by tests/golden/make_golden_tiled.py from auto_labeler.py), the numpy merge
against the oracle's uo_sort_nms byte for byte, and the argument checks of the three engine entry points."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

MAXD = 1024


@pytest.fixture(scope="module")
def gold():
    return load_golden("tiled_slices.npz")


@pytest.fixture(scope="module")
def lib(pkg):
    from unina_yolo_dla_amd import build, engine
    build.build_native()
    return engine.load_library()


@pytest.fixture(scope="module")
def slicing(pkg):
    from unina_yolo_dla_amd import slicing
    return slicing


def _cases(gold):
    for i, (h, w, sh, sw, oh, ow) in enumerate(gold["cases"]):
        raw = [tuple(int(v) for v in r) for r in gold[f"slices/{i}"]]
        yield (int(h), int(w), int(sh), int(sw), float(oh), float(ow)), raw, list(dict.fromkeys(raw))


def oracle_sort_nms(oracle_mod, dets, iou_thr):
    """uo_sort_nms (oracle/postprocess_oracle.c:102) with the engine's semantics on records in enumeration order."""
    L = oracle_mod.lib()
    L.uo_sort_nms.restype = C.c_int
    L.uo_sort_nms.argtypes = [C.c_void_p, C.c_int, C.c_float, C.POINTER(oracle_mod.Semantics), C.c_void_p]
    work = np.array(dets, dtype=oracle_mod.DET_DTYPE)          # (sorted in place)
    out = np.zeros(max(len(work), 1), dtype=oracle_mod.DET_DTYPE)
    sem = oracle_mod.semantics("engine")
    k = L.uo_sort_nms(work.ctypes.data, len(work), iou_thr, C.byref(sem), out.ctypes.data)
    return out[:k].copy()


def seeded_union(slicing, seed, n_tiles, per_tile, tiles=None, equal_conf=True):
    """Records clustered so that tiles overlap heavily; confidences drawn from a small set so that many are bit-equal across
    tiles (tile order then decides), boxes on a 1/8-pixel grid."""
    rng = np.random.RandomState(seed)
    if tiles is None:
        tiles = [(int(64 * (t % 8)), int(48 * (t // 8)), 640, 640) for t in range(n_tiles)]
    slots = np.zeros((n_tiles, MAXD), dtype=slicing.DET_DTYPE)
    counts = np.zeros(n_tiles, dtype=np.int32)
    levels = (rng.randint(1, 4096, 600) / 4096.0).astype(np.float32) if equal_conf else None
    centres = rng.uniform(40, 600, (96, 2))
    for t in range(n_tiles):
        n = per_tile if np.isscalar(per_tile) else per_tile[t]
        c = centres[rng.randint(0, len(centres), n)] + rng.uniform(-6, 6, (n, 2))
        wh = rng.uniform(8, 40, (n, 2))
        r = slots[t][:n]
        r["x1"], r["y1"] = np.round((c[:, 0] - wh[:, 0]) * 8) / 8, np.round((c[:, 1] - wh[:, 1]) * 8) / 8
        r["x2"], r["y2"] = np.round((c[:, 0] + wh[:, 0]) * 8) / 8, np.round((c[:, 1] + wh[:, 1]) * 8) / 8
        conf = levels[rng.randint(0, len(levels), n)] if equal_conf else rng.uniform(0.05, 0.99, n).astype(np.float32)
        r["confidence"] = -np.sort(-conf)                     # a slot is sorted, as the engine leaves it
        r["class_id"] = rng.randint(0, 4, n)
        r["valid"] = 1
        counts[t] = n
    return slots, counts, tiles


# ---------------------------------------------------------------------------------------------- slicing

def test_get_slices_matches_the_reference(gold, slicing):
    n = 0
    for (h, w, sh, sw, oh, ow), raw, dedup in _cases(gold):
        assert slicing.get_slices(h, w, sh, sw, oh, ow, raw=True) == raw
        assert slicing.get_slices(h, w, sh, sw, oh, ow) == dedup
        n += 1
    assert n >= 12
    assert slicing.get_slices(1080, 1920) == [(0, 0, 640, 640), (512, 0, 640, 640), (1024, 0, 640, 640), (1280, 0, 640, 640),
                                              (0, 440, 640, 640), (512, 440, 640, 640), (1024, 440, 640, 640), (1280, 440, 640, 640)]
    assert slicing.get_slices(400, 500) == [(0, 0, 500, 400)]                       # smaller than a slice: the whole frame
    assert {t[2:] for t in slicing.get_slices(480, 1936)} == {(640, 480)}           # smaller in one dimension: non-square


def test_unina_slice_tiles_matches_the_reference(gold, lib, pkg):
    from unina_yolo_dla_amd import engine
    for (h, w, sh, sw, oh, ow), _raw, dedup in _cases(gold):
        n, tiles = engine.slice_tiles(w, h, sw, sh, ow, oh)
        assert n == len(dedup) and tiles == dedup, (h, w, sh, sw, oh, ow)
        # cap smaller than the count: the count comes back, `cap` tiles are written and nothing behind them
        cap = max(len(dedup) - 3, 0)
        arr = (engine.Tile * (cap + 2))()
        for t in arr:
            t.x = t.y = t.w = t.h = -7
        assert lib.unina_slice_tiles(w, h, sw, sh, ow, oh, arr, cap) == len(dedup)
        assert [(t.x, t.y, t.w, t.h) for t in arr[:cap]] == dedup[:cap]
        assert all((t.x, t.y, t.w, t.h) == (-7, -7, -7, -7) for t in arr[cap:])
    assert lib.unina_slice_tiles(1920, 1200, 640, 640, 0.2, 0.2, None, 0) == 12
    for bad in ((0, 1200, 640, 640, 0.2, 0.2), (1920, 1200, 0, 640, 0.2, 0.2), (1920, 1200, 640, 640, 1.0, 0.2),
                (1920, 1200, 640, 640, 0.2, float("nan"))):
        assert lib.unina_slice_tiles(*bad, None, 0) == -4                           # -UNINA_ERR_ARG
    assert lib.unina_slice_tiles(1920, 1200, 640, 640, 0.2, 0.2, None, 3) == -4     # cap > 0 needs a buffer


def test_map_boxes_to_global_matches_the_reference(gold, slicing):
    boxes = gold["map/boxes"]
    for (x, y), want in zip(gold["map/offsets"], gold["map/global"]):
        got = slicing.map_boxes_to_global(boxes, int(x), int(y))
        assert got.dtype == want.dtype and np.array_equal(got, want)
    empty = np.zeros((0, 4), dtype=np.float32)
    assert slicing.map_boxes_to_global(empty, 3, 4) is empty
    assert boxes[0, 0] == 0.0                                                        # the input is not written


# ---------------------------------------------------------------------------------------------- merge

def _gold_union(gold, slicing):
    tiles = [tuple(int(v) for v in r) for r in gold["union/tiles"]]
    slots = np.zeros((len(tiles), MAXD), dtype=slicing.DET_DTYPE)
    part = gold["union/slots"].view(slicing.DET_DTYPE)
    slots[:, :part.shape[1]] = part
    return slots, gold["union/counts"], tiles, float(gold["union/merge_iou"])


def test_merge_numpy_keeps_the_reference_kept_set(gold, slicing):
    slots, counts, tiles, iou = _gold_union(gold, slicing)
    union = slicing.map_records(slots, counts, tiles)
    want = union[gold["union/kept"]]                          # the reference's kept records, by descending confidence
    got = slicing.merge_numpy(slots, counts, tiles, iou)
    assert 0 < len(got) < len(union)
    for k in ("x1", "y1", "x2", "y2", "confidence", "class_id"):
        assert np.array_equal(got[k], want[k]), k
    assert np.all(got["valid"] == 1) and np.all(got["_pad"] == 0)


def test_merge_numpy_equals_the_oracle_byte_for_byte(gold, slicing, oracle_mod):
    slots, counts, tiles, iou = _gold_union(gold, slicing)
    got = slicing.merge_numpy(slots, counts, tiles, iou)
    want = oracle_sort_nms(oracle_mod, slicing.map_records(slots, counts, tiles), iou)
    assert len(want) > 0 and got.tobytes() == want.tobytes()
    # more than 1024 records, equal confidences across tiles, a non-square tile (scale != 1) among them
    tiles = [(int(64 * (t % 8)), int(48 * (t // 8)), 640, 640) for t in range(12)]
    tiles[5] = (100, 20, 500, 333)
    slots, counts, tiles = seeded_union(slicing, 31, 12, 300, tiles)
    union = slicing.map_records(slots, counts, tiles)
    conf = union["confidence"]
    assert len(union) == 3600 and len(np.unique(conf)) < len(conf)
    cut = np.sort(conf)[::-1][MAXD - 1]
    assert (conf == cut).sum() > 1                            # the cap falls inside a run of equal confidences
    got = slicing.merge_numpy(slots, counts, tiles, 0.45)
    want = oracle_sort_nms(oracle_mod, union, 0.45)
    assert 0 < len(want) < MAXD and got.tobytes() == want.tobytes()


def test_merging_one_tile_at_the_origin_is_the_identity(slicing, oracle_mod):
    slots, counts, tiles = seeded_union(slicing, 5, 1, 700, [(0, 0, 640, 640)], equal_conf=False)
    kept = oracle_sort_nms(oracle_mod, slots[0][:counts[0]], 0.45)             # records that already passed NMS at 0.45
    assert 0 < len(kept) < 700
    one = np.zeros((1, MAXD), dtype=slicing.DET_DTYPE)
    one[0, :len(kept)] = kept
    assert slicing.merge_numpy(one, [len(kept)], tiles, 0.45).tobytes() == kept.tobytes()


# ---------------------------------------------------------------------------------------------- argument checks

def test_tiled_entry_points_reject_bad_arguments_without_a_device(lib, pkg):
    from unina_yolo_dla_amd import engine
    tiles = (engine.Tile * 2)(engine.Tile(0, 0, 640, 640), engine.Tile(512, 0, 640, 640))
    norm = lib.create_norm_params_imagenet()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    n = C.c_int()
    ARG = 4
    assert lib.unina_infer_tiled_bgra(None, p, 1920, 1200, 7680, tiles, 2, C.byref(norm), 0.3, 0.45, 0.1, 0.45, p, C.byref(n), None) == ARG
    assert lib.unina_infer_tiled_bgra_async(None, p, 1920, 1200, 7680, tiles, 2, C.byref(norm), 0.3, 0.45, 0.1, 0.45, p, p, None) == ARG
    assert lib.unina_merge_tiles_async(None, p, p, tiles, 2, 0.45, p, p, None) == ARG
