"""The letterbox without a GPU: unina_letterbox_geometry (host-only C) against mine.letterbox_geometry, and the numpy twins
camera.letterbox_bgra_to_tensor / letterbox_nv12_to_tensor / unmap_boxes against the scalar oracle's BGRA resize (the path
tests/test_camera_cpu.py uses) and against the definition in include/unina_mi355.h written out on np.float32 scalars."""
import ctypes as C

import numpy as np
import pytest

from letterbox_child import CAMERAS, NET, PAD, host_camera, visible

F = np.float32


@pytest.fixture(scope="module")
def engine(pkg):
    from unina_yolo_dla_amd import engine
    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def camera(pkg):
    from unina_yolo_dla_amd import camera
    return camera


@pytest.fixture(scope="module")
def mine(pkg):
    from unina_yolo_dla_amd import mine
    return mine


# ------------------------------------------------------------------------------------ geometry

@pytest.mark.parametrize("dst_w,dst_h", [(64, 64), (96, 64), (64, 96)])
def test_c_geometry_equals_mine_for_every_small_frame(engine, mine, dst_w, dst_h):
    L = engine.load_library()
    box = engine.Letterbox()
    bad = []
    for src_h in range(1, 161):
        for src_w in range(1, 161):
            assert L.unina_letterbox_geometry(src_w, src_h, dst_w, dst_h, C.byref(box)) == 0
            got = (box.new_w, box.new_h, box.left, box.top)
            if got != mine.letterbox_geometry(src_w, src_h, dst_w, dst_h):
                bad.append((src_w, src_h, got))
            assert box.new_w >= 1 and box.new_h >= 1 and box.left >= 0 and box.top >= 0
            assert box.left + box.new_w <= dst_w and box.top + box.new_h <= dst_h
    assert not bad, bad[:5]


@pytest.mark.parametrize("src,dst,want", [
    ((1920, 1080), (640, 640), (640, 360, 0, 140)),
    ((640, 481), (640, 640), (640, 481, 0, 79)),       # odd remainder: 79 above, 80 below
    ((333, 500), (640, 640), (426, 640, 107, 0)),
    ((5, 128), (64, 64), (2, 64, 31, 0)),              # r = 0.5: round(2.5) is 2 (half to even); lround gives (3, 64, 30, 0)
])
def test_geometry_pins(engine, mine, src, dst, want):
    assert engine.letterbox_geometry(*src, *dst) == want
    assert mine.letterbox_geometry(*src, *dst) == want
    if src == (640, 481):
        assert dst[1] - want[3] - want[1] == 80


def test_geometry_rejects_non_positive_sizes(engine):
    L = engine.load_library()
    box = engine.Letterbox()
    for args in ((0, 10, 64, 64), (10, 0, 64, 64), (10, 10, 0, 64), (10, 10, 64, 0), (-3, 10, 64, 64), (10, 10, 64, -1)):
        assert L.unina_letterbox_geometry(*args, C.byref(box)) == -4          # -UNINA_ERR_ARG
        with pytest.raises(engine.EngineError, match="ARG"):
            engine.letterbox_geometry(*args)
    assert L.unina_letterbox_geometry(10, 10, 64, 64, None) == -4


# ------------------------------------------------------------------------------------ the twins

def pad_pixel(camera):
    n = [F(v) for v in camera.IMAGENET]
    return [((F(PAD) / F(255.0)) - n[c]) / n[3 + c] for c in range(3)]


def split(t, box):
    """(inner rectangle, mask of the border) of a letterboxed tensor."""
    new_w, new_h, left, top = box
    border = np.ones(t.shape[1:], dtype=bool)
    border[top:top + new_h, left:left + new_w] = False
    return t[:, top:top + new_h, left:left + new_w], border


@pytest.mark.parametrize("name", list(CAMERAS))
def test_bgra_twin_is_the_oracle_resize_inside_and_the_pad_outside(camera, mine, oracle_mod, name):
    c = host_camera(name)
    img, _y, _uv = visible(c)
    box = mine.letterbox_geometry(c["w"], c["h"], NET, NET)
    new_w, new_h = box[:2]
    t = camera.letterbox_bgra_to_tensor(img, (NET, NET), PAD)
    assert t.dtype == np.float32 and t.shape == (3, NET, NET)
    inner, border = split(t, box)
    if (new_w, new_h) == (c["w"], c["h"]):                 # r == 1: the plain tap
        want = oracle_mod.preprocess_bgra(img)
    else:
        want = oracle_mod.preprocess_bgra(img, dst_hw=(new_h, new_w))
    assert inner.tobytes() == want.tobytes()
    pad = pad_pixel(camera)
    for ch in range(3):
        assert np.all(t[ch][border] == pad[ch]) and t[ch][border].dtype == np.float32
    assert border.any() == (name != "64x64_identity")
    assert len(np.unique(inner)) > 50                      # (not a constant picture)


def test_r1_frames_take_the_plain_tap(camera, mine, oracle_mod):
    c = host_camera("64x37_r1")
    img, y, uv = visible(c)
    assert mine.letterbox_geometry(64, 37, NET, NET) == (64, 37, 0, 13)
    a = camera.letterbox_bgra_to_tensor(img, (NET, NET), PAD)
    assert a[:, 13:50].tobytes() == oracle_mod.preprocess_bgra(img).tobytes()
    b = camera.letterbox_nv12_to_tensor(y, uv, (NET, NET), PAD)
    assert b[:, 13:50].tobytes() == camera.nv12_to_tensor(y, uv).tobytes()
    assert np.all(b[0, :13] == pad_pixel(camera)[0]) and np.all(b[2, 50:] == pad_pixel(camera)[2])


@pytest.mark.parametrize("name", list(CAMERAS))
def test_nv12_twin_on_a_grey_frame_is_the_bgra_twin(camera, name):
    """All chroma bytes 128: r = g = b = Y exactly, so the NV12 letterbox equals the BGRA one of B = G = R = Y."""
    c = host_camera(name)
    _img, y, uv = visible(c)
    uv = np.full_like(uv, 128)
    img = np.empty((c["h"], c["w"], 4), dtype=np.uint8)
    img[..., :3] = y[..., None]
    img[..., 3] = 7
    a = camera.letterbox_nv12_to_tensor(y, uv, (NET, NET), PAD)
    b = camera.letterbox_bgra_to_tensor(img, (NET, NET), PAD)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["128x72_down", "40x30_up", "5x128_even"])
def test_nv12_twin_inside_is_the_nv12_resize_twin(camera, mine, name):
    """... and on a coloured frame the inner rectangle is nv12_to_tensor (pinned by tests/test_camera_cpu.py) at new_w x new_h."""
    c = host_camera(name)
    _img, y, uv = visible(c)
    box = mine.letterbox_geometry(c["w"], c["h"], NET, NET)
    inner, border = split(camera.letterbox_nv12_to_tensor(y, uv, (NET, NET), PAD), box)
    assert inner.tobytes() == camera.nv12_to_tensor(y, uv, dst_hw=(box[1], box[0])).tobytes()
    assert border.any()


def test_twins_refuse_bad_sizes(camera):
    img = np.zeros((4, 4, 4), dtype=np.uint8)
    with pytest.raises(ValueError):
        camera.letterbox_bgra_to_tensor(img, (0, 8))
    with pytest.raises(ValueError):
        camera.letterbox_nv12_to_tensor(np.zeros((4, 4), np.uint8), np.zeros((1, 4), np.uint8), (8, 8))   # a chroma row short


# ------------------------------------------------------------------------------------ the box map

@pytest.mark.parametrize("src", [(1920, 1080), (128, 72), (40, 30), (64, 37), (5, 128), (200, 23), (333, 500)])
def test_unmap_boxes_inverts_the_paste_on_the_rectangle_corners(engine, camera, mine, src):
    """The inner rectangle's corners (left, top, left + new_w, top + new_h) are where the frame's corners (0, 0, src_w, src_h) were
    pasted. x - left is exact (small integers), the scale fl(src_w / new_w) is off by at most 2^-24 relative, the product rounds
    once more: |X - src_w| <= src_w * 2^-23."""
    dst = (640, 640) if max(src) > 200 else (NET, NET)
    new_w, new_h, left, top = mine.letterbox_geometry(*src, *dst)
    d = np.zeros(2, dtype=engine.DET_DTYPE)
    d[0] = (left, top, left + new_w, top + new_h, 0.5, 1, 1, 0)
    d[1] = (left + 1.25, top - 3.5, left + 0.75 * new_w, dst[1] + 10.0, 0.25, 2, 1, 0)      # over the padding: no clamp
    m = camera.unmap_boxes(d, *src, *dst)
    assert m.dtype == d.dtype and d[0]["x1"] == left                                      # (a copy: the input is untouched)
    assert m[0]["x1"] == 0.0 and m[0]["y1"] == 0.0
    assert abs(float(m[0]["x2"]) - src[0]) <= src[0] * 2.0 ** -23
    assert abs(float(m[0]["y2"]) - src[1]) <= src[1] * 2.0 ** -23
    for k in ("confidence", "class_id", "valid", "_pad"):
        assert np.array_equal(m[k], d[k])
    # the definition on scalars, bit for bit
    sx, sy = F(src[0]) / F(new_w), F(src[1]) / F(new_h)
    for i in range(2):
        want = [(F(d[i]["x1"]) - F(left)) * sx, (F(d[i]["y1"]) - F(top)) * sy, (F(d[i]["x2"]) - F(left)) * sx, (F(d[i]["y2"]) - F(top)) * sy]
        assert all(type(v) is np.float32 for v in want)
        assert [m[i][k] for k in ("x1", "y1", "x2", "y2")] == want
    assert m[1]["y2"] > src[1] and m[1]["y1"] < 0                                          # outside the camera frame, kept as is


# ------------------------------------------------------------------------------------ the consumers' switches

def test_evaluate_skips_the_host_rescale_for_mapped_boxes(engine, pkg, tmp_path):
    from unina_yolo_dla_amd import evaluate
    root = tmp_path / "ds"
    (root / "images").mkdir(parents=True)
    (root / "labels").mkdir()
    np.save(root / "images" / "a.npy", np.zeros((72, 128, 4), dtype=np.uint8))
    (root / "labels" / "a.txt").write_text("0 0.5 0.5 0.1 0.2\n")
    d = np.zeros(1, dtype=engine.DET_DTYPE)
    d[0] = (10, 20, 30, 50, 0.9, 0, 1, 0)
    detect = lambda frame, conf, iou, q: d.copy()
    mapped = evaluate.evaluate(detect, str(root), 64, net_size=(NET, NET), camera_pixels=True)
    stretched = evaluate.evaluate(detect, str(root), 64, net_size=(NET, NET))
    assert mapped["predictions"][0]["bbox"] == pytest.approx([10, 20, 20, 30])              # the frame's own pixels already
    assert stretched["predictions"][0]["bbox"] == pytest.approx([20, 22.5, 40, 33.75])      # 128 / 64 and 72 / 64, as before


def test_cli_switches_default_to_off(mine):
    base = ["--engine", "m.une", "--data", "d"]
    assert mine.parser().parse_args(base).device_letterbox is False
    assert mine.parser().parse_args(base + ["--device-letterbox"]).device_letterbox is True
