"""Sliced inference on the GPU (unina_infer_tiled_bgra / unina_merge_tiles_async: csrc/postprocess.hip tile_gather_kernel +
the frame's own post_nms_kernel). Every comparison is byte-exact: against the oracle's uo_sort_nms on the union mapped in
numpy, and against the existing unina_infer_bgra on each crop."""
import ctypes as C

import numpy as np
import pytest

from test_tiled_cpu import MAXD, oracle_sort_nms, seeded_union

pytestmark = pytest.mark.gpu

CONF, IOU, Q, MERGE = 0.3, 0.45, 0.1, 0.45
FRAME_SEED = 23


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import engine, slicing
    return torch, engine, slicing


@pytest.fixture(scope="module")
def eng(env, sd7):
    _torch, engine, _s = env
    e = engine.Engine.from_state_dict(sd7)
    yield e
    e.close()


def gpu_merge(env, eng, slots, counts, tiles, iou):
    torch, engine, _s = env
    d_slots = torch.from_numpy(np.ascontiguousarray(slots).view(np.int32).reshape(len(slots), -1)).cuda()
    d_counts = torch.from_numpy(np.asarray(counts, dtype=np.int32)).cuda()
    out = torch.full((MAXD * 8 + 8,), -1, dtype=torch.int32, device="cuda")
    eng.merge_tiles(d_slots, d_counts, tiles, iou, out=out)
    torch.cuda.synchronize()
    return engine.Engine.unpack(out)


def check_merge(env, eng, oracle_mod, slots, counts, tiles, iou=MERGE):
    slicing = env[2]
    union = slicing.map_records(slots, counts, tiles)
    want = oracle_sort_nms(oracle_mod, union, iou)
    for _ in range(2):                                        # twice: the workspace must be back at rest after a merge
        got = gpu_merge(env, eng, slots, counts, tiles, iou)
        assert got.tobytes() == want.tobytes(), (len(got), len(want))
    return union, want


def test_merge_heavy_cross_tile_overlap(env, eng, oracle_mod):
    slots, counts, tiles = seeded_union(env[2], 41, 12, 80, equal_conf=False)
    union, want = check_merge(env, eng, oracle_mod, slots, counts, tiles)
    assert len(union) == 960 and 0 < len(want) < len(union)


def test_merge_empty_tiles_and_one_tile(env, eng, oracle_mod):
    slicing = env[2]
    slots, counts, tiles = seeded_union(slicing, 42, 6, [0, 50, 0, 0, 70, 0], equal_conf=False)
    _u, want = check_merge(env, eng, oracle_mod, slots, counts, tiles)
    assert len(want) > 0
    slots, counts, tiles = seeded_union(slicing, 43, 3, 0)
    _u, want = check_merge(env, eng, oracle_mod, slots, counts, tiles)   # nothing at all
    assert len(want) == 0
    slots, counts, tiles = seeded_union(slicing, 44, 1, 900, [(128, 64, 640, 640)], equal_conf=False)
    _u, want = check_merge(env, eng, oracle_mod, slots, counts, tiles)
    assert 0 < len(want) < 900


@pytest.mark.parametrize("levels", [600, 3])
def test_merge_64_full_tiles(env, eng, oracle_mod, levels):
    """65 536 candidates: the histogram cut. 600 confidence levels: the cut bin holds ~100 equal keys; 3 levels: ~21 000 equal
    keys, so the 1024 best are chosen by enumeration index alone (tile order)."""
    slicing = env[2]
    slots, counts, tiles = seeded_union(slicing, 45, 64, MAXD)
    if levels == 3:
        rng = np.random.RandomState(46)
        for t in range(64):
            slots[t]["confidence"] = -np.sort(-np.array([0.75, 0.5, 0.40625], dtype=np.float32)[rng.randint(0, 3, MAXD)])
    union, want = check_merge(env, eng, oracle_mod, slots, counts, tiles)
    assert len(union) == 64 * MAXD and 0 < len(want) <= MAXD


def test_merge_equal_confidences_tile_order_decides(env, eng, oracle_mod):
    """The same record in two tiles with bit-equal confidence: neither suppresses the other, the lower tile comes first; a
    third copy with a lower confidence is suppressed."""
    slicing = env[2]
    slots = np.zeros((3, MAXD), dtype=slicing.DET_DTYPE)
    tiles = [(512, 0, 640, 640), (0, 0, 640, 640), (256, 0, 640, 640)]
    for t, (x0, conf) in enumerate(((10.0, 0.8), (522.0, 0.8), (266.5, 0.7))):
        r = slots[t][0]
        r["x1"], r["y1"], r["x2"], r["y2"], r["confidence"], r["class_id"], r["valid"] = x0, 20.0, x0 + 30.0, 60.0, conf, 2, 1
    _u, want = check_merge(env, eng, oracle_mod, slots, [1, 1, 1], tiles)
    assert len(want) == 2 and want["x1"].tolist() == [522.0, 522.0] and np.all(want["confidence"] == np.float32(0.8))
    slots2, counts, tiles2 = seeded_union(slicing, 47, 8, 100)   # many ties across tiles
    check_merge(env, eng, oracle_mod, slots2, counts, tiles2)


def test_merge_non_square_tile_scales(env, eng, oracle_mod):
    slicing = env[2]
    tiles = [(0, 0, 500, 400), (300, 100, 640, 480), (1280, 560, 333, 640), (64, 48, 640, 640)]
    slots, counts, tiles = seeded_union(slicing, 48, 4, 200, tiles, equal_conf=False)
    union, want = check_merge(env, eng, oracle_mod, slots, counts, tiles)
    assert not np.array_equal(union["x1"][:200], slots[0]["x1"][:200]) and len(want) > 0


def test_bad_arguments_are_rejected_with_a_message(env, eng):
    torch, engine, _s = env
    cam = torch.zeros((64, 64 * 4), dtype=torch.uint8, device="cuda")
    for kw in (dict(tiles=[]), dict(tiles=[(0, 0, 64, 64)] * 65), dict(tiles=[(1, 0, 64, 64)]), dict(tiles=[(0, 0, 0, 64)]),
               dict(tiles=[(0, -1, 64, 64)]), dict(pitch=63 * 4), dict(pitch=64 * 4 + 2)):
        args = dict(tiles=[(0, 0, 64, 64)], pitch=64 * 4)
        args.update(kw)
        with pytest.raises(engine.EngineError, match=r"\[ARG\] unina_infer_tiled_bgra"):
            eng.infer_tiled_bgra(cam, 64, 64, args["pitch"], args["tiles"])
    slots = torch.zeros((1, 8 * MAXD), dtype=torch.int32, device="cuda")
    counts = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(engine.EngineError, match=r"\[ARG\] unina_merge_tiles_async"):
        eng.merge_tiles(slots, counts, [(0, 0, 0, 0)])
    L = eng.L
    t1 = (engine.Tile * 1)(engine.Tile(0, 0, 64, 64))
    assert L.unina_merge_tiles_async(eng.h, None, counts.data_ptr(), t1, 1, 0.45, slots.data_ptr(), counts.data_ptr(), None) == 4
    assert L.unina_merge_tiles_async(eng.h, slots.data_ptr(), counts.data_ptr(), t1, 0, 0.45, slots.data_ptr(), counts.data_ptr(), None) == 4
    n = C.c_int()
    norm = L.create_norm_params_imagenet()
    assert L.unina_infer_tiled_bgra(eng.h, cam.data_ptr(), 64, 64, 256, t1, 1, C.byref(norm), 0.3, 0.45, 0.1, 0.45, None, C.byref(n), None) == 4
    assert L.unina_infer_tiled_bgra_async(eng.h, None, 64, 64, 256, t1, 1, C.byref(norm), 0.3, 0.45, 0.1, 0.45, slots.data_ptr(), counts.data_ptr(), None) == 4


# ---------------------------------------------------------------------------------------------- end to end

def camera(torch, seed, h, w):
    """Seeded random pitched BGRA frame. Low-contrast noise, bytes in [104, 152): on full-range noise the seed-7 network
    passes ~950 cells per 640x640 tile at conf 0.3 (a union of 11 366 for 1920x1200), on this range 17..34 per tile."""
    pitch = w * 4 + 64
    host = np.random.default_rng(seed).integers(104, 152, (h, pitch), dtype=np.uint8)
    return torch.from_numpy(host).cuda(), pitch


def per_crop(env, eng, cam, pitch, tiles):
    """The form possible without the feature: unina_infer_bgra on every crop (a pointer-offset view of the frame)."""
    slicing = env[2]
    flat = cam.view(-1)
    slots = np.zeros((len(tiles), MAXD), dtype=slicing.DET_DTYPE)
    counts = []
    for t, (x, y, w, h) in enumerate(tiles):
        d = eng.infer_bgra(flat[y * pitch + 4 * x:], w, h, pitch, None, CONF, IOU, Q)
        slots[t, :len(d)] = d
        counts.append(len(d))
    return slots, counts


def test_tiled_frame_equals_per_crop_inference_then_merge(env, eng, oracle_mod):
    """1920x1200 pitched BGRA noise (camera(): bytes in [104, 152)), frame seed 23, seed-7 weights, conf 0.3: the tiled call
    against unina_infer_bgra on each of the 12 default tiles, the numpy map and uo_sort_nms.
    The seed and the byte range were chosen with the CPU oracle (oracle.preprocess_bgra + oracle.forward + oracle.postprocess
    per crop, fp32): per-tile counts 27 28 33 34 23 17 26 28 29 30 26 30, union 331, merged 240 -- every tile detects
    something, the union fits 1024 and the merge suppresses 91 records across tiles. (Seed 24 at 1920x1080: 8 tiles, union
    192, merged 150; seed 25 at 500x400: 15.) The three conditions are asserted below on the engine's own figures, so the
    comparison cannot pass on an empty or a trivially disjoint union."""
    torch, engine, slicing = env
    cam, pitch = camera(torch, FRAME_SEED, 1200, 1920)
    tiles = eng.default_tiles(1920, 1200)
    assert len(tiles) == 12 and tiles == engine.slice_tiles(1920, 1200)[1]
    images = torch.from_numpy(np.random.default_rng(3).standard_normal((1, 3, 640, 640)).astype(np.float32)).cuda()
    before = eng.infer(images, CONF, IOU, Q)
    slots, counts = per_crop(env, eng, cam, pitch, tiles)
    want = oracle_sort_nms(oracle_mod, slicing.map_records(slots, counts, tiles), MERGE)
    print("per-tile counts", counts, "union", sum(counts), "merged", len(want))
    assert min(counts) >= 1 and sum(counts) <= MAXD and len(want) < sum(counts)
    got = eng.infer_tiled_bgra(cam, 1920, 1200, pitch, tiles, None, CONF, IOU, Q, MERGE)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() == slicing.merge_numpy(slots, counts, tiles, MERGE).tobytes()
    # two consecutive calls; tiles=None slices the same way
    assert eng.infer_tiled_bgra(cam, 1920, 1200, pitch, None, None, CONF, IOU, Q, MERGE).tobytes() == want.tobytes()
    # the async form + a device -> host copy
    out = torch.full((MAXD * 8 + 8,), -1, dtype=torch.int32, device="cuda")
    eng.infer_tiled_bgra(cam, 1920, 1200, pitch, tiles, None, CONF, IOU, Q, MERGE, out=out)
    torch.cuda.synchronize()
    assert engine.Engine.unpack(out).tobytes() == want.tobytes()
    # the handle's other paths still return what they returned before (the stem node is re-pointed back)
    assert eng.infer(images, CONF, IOU, Q).tobytes() == before.tobytes()
    t0 = tiles[0]
    assert eng.infer_bgra(cam, t0[2], t0[3], pitch, None, CONF, IOU, Q).tobytes() == slots[0][:counts[0]].tobytes()
    assert eng.infer_tiled_bgra(cam, 1920, 1200, pitch, tiles, None, CONF, IOU, Q, MERGE).tobytes() == want.tobytes()


def test_1080p_deduplicated_tiles_equal_default_slicing(env, eng, oracle_mod):
    torch, engine, slicing = env
    cam, pitch = camera(torch, FRAME_SEED + 1, 1080, 1920)
    n, tiles = engine.slice_tiles(1920, 1080)
    assert n == 8 and len(slicing.get_slices(1080, 1920, raw=True)) == 12
    a = eng.infer_tiled_bgra(cam, 1920, 1080, pitch, tiles, None, CONF, IOU, Q, MERGE)
    b = eng.infer_tiled_bgra(cam, 1920, 1080, pitch, None, None, CONF, IOU, Q, MERGE)
    slots, counts = per_crop(env, eng, cam, pitch, tiles)
    want = oracle_sort_nms(oracle_mod, slicing.map_records(slots, counts, tiles), MERGE)
    assert len(want) > 0 and a.tobytes() == want.tobytes() and b.tobytes() == want.tobytes()


def test_small_frame_is_one_tile_with_boxes_scaled_back(env, eng):
    torch, _engine, slicing = env
    cam, pitch = camera(torch, FRAME_SEED + 2, 400, 500)
    whole = eng.infer_bgra(cam, 500, 400, pitch, None, CONF, IOU, Q)
    got = eng.infer_tiled_bgra(cam, 500, 400, pitch, None, None, CONF, IOU, Q, MERGE)
    assert eng.default_tiles(500, 400) == [(0, 0, 500, 400)] and len(whole) > 0
    one = np.zeros((1, MAXD), dtype=slicing.DET_DTYPE)
    one[0, :len(whole)] = whole
    scaled = slicing.map_records(one, [len(whole)], [(0, 0, 500, 400)])
    assert got.tobytes() == scaled.tobytes()
    assert np.array_equal(got["x1"], (whole["x1"] * (np.float32(500) / np.float32(640))).astype(np.float32))
