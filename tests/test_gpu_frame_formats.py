"""The frame descriptor on the GPU: RGB, RGBA, YUYV, UYVY and Bayer frames straight into the stem, whole, letterboxed and tiled
(unina_infer_frame, unina_infer_letterbox_frame, unina_infer_tiled_frame, unina_preprocess_frame, unina_preprocess_letterbox_frame),
and BGRA / NV12 through the same calls. Every comparison is byte-exact: the stand-alone pre-process against camera.frame_to_tensor
(the numpy twin, pinned to the oracle and the NV12 twin by tests/test_frame_formats_cpu.py), the in-stem form against the two-step
form, the tiled call against twin tensor per tile -> unina_infer_async -> unina_merge_tiles_async."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from frame_child import (BGGR, BGRA, CAMERAS, CHILD_CASES, GBRG, GRBG, NAMES, NEW_FORMATS, NV12, RGB, RGBA, RGGB, UYVY, YUYV, camera,
                         make_frame)
from nv12_child import CONF, IOU, Q, ROOT

pytestmark = pytest.mark.gpu

MERGE = 0.45
MAXD = 1024
PAD = 114.0
ids = lambda fmts: [NAMES[f] for f in fmts]


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import camera as twin, engine, export, slicing
    return torch, engine, twin, slicing, export


@pytest.fixture(scope="module")
def eng(env, sd7):
    e = env[1].Engine.from_state_dict(sd7)
    yield e
    e.close()


def preprocess(env, c, dst_hw, region=None):
    torch, engine = env[0], env[1]
    out = torch.full((3,) + tuple(dst_hw), float("nan"), dtype=torch.float32, device="cuda")
    engine.preprocess_frame(c["frame"], out, region=region)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def twin_tensor(env, c, dst_hw, origin=(0, 0), region=None):
    return env[2].frame_to_tensor(c["fmt"], c["planes"], dst_hw=dst_hw, origin=origin, region=region or (c["w"], c["h"]))


# ------------------------------------------------------------------------------------ 1. the stand-alone pre-process

ALL_FORMATS = (BGRA, NV12) + NEW_FORMATS


@pytest.mark.parametrize("fmt", ALL_FORMATS, ids=ids(ALL_FORMATS))
def test_preprocess_frame_equals_the_twin(env, fmt):
    """Every format, the two the named calls serve included (their kernels meet a region's origin only through this call). The
    aligned 64 x 64 tap is the quad loaders' wide loads against the twin, the misaligned one their byte loads."""
    torch, engine, twin = env[:3]
    for seed, (h, w), dst, misaligned in ((81, (50, 70), (64, 64), False), (82, (7, 9), (16, 16), False), (83, (64, 64), (64, 64), True),
                                          (80, (64, 64), (64, 64), False)):
        c = make_frame(torch, engine, twin, fmt, seed, h, w, misaligned)
        if misaligned and fmt in (BGRA, RGBA):
            assert c["pitch"] == 4 * w + 4
        elif misaligned:
            assert c["pitch"] % 2 == 1 and c["d"].data_ptr() % 4 == 1
        else:
            assert c["d"].data_ptr() % 16 == 0
        got = preprocess(env, c, dst)
        assert got.tobytes() == twin_tensor(env, c, dst).tobytes(), (NAMES[fmt], h, w, dst, misaligned)
        assert len(np.unique(got)) > 50
    c = make_frame(torch, engine, twin, fmt, 84, 120, 160)
    for dst in ((13, 21), (16, 20)):                                          # a region at an odd origin, tapped | resized
        got = preprocess(env, c, dst, region=(33, 17, 21, 13))
        assert got.tobytes() == twin_tensor(env, c, dst, origin=(33, 17), region=(21, 13)).tobytes(), (NAMES[fmt], dst)
    for dst in ((20, 52), (32, 40)):                                          # at an aligned even origin (wide loads), tapped | resized
        got = preprocess(env, c, dst, region=(36, 18, 52, 20))
        assert got.tobytes() == twin_tensor(env, c, dst, origin=(36, 18), region=(52, 20)).tobytes(), (NAMES[fmt], dst)
    # a tapped region of more than one quad per row that ends at the frame's corner (Bayer: reflected at the FRAME's border)
    got = preprocess(env, c, (20, 51), region=(160 - 51, 100, 51, 20))
    assert got.tobytes() == twin_tensor(env, c, (20, 51), origin=(160 - 51, 100), region=(51, 20)).tobytes()
    # regions of a misaligned frame (an odd pitch, the plane one byte off an aligned address)
    c = make_frame(torch, engine, twin, fmt, 79, 120, 160, True)
    for region in ((3, 17, 52, 20), (33, 18, 21, 13)):
        dst = (region[3], region[2])
        got = preprocess(env, c, dst, region=region)
        assert got.tobytes() == twin_tensor(env, c, dst, origin=region[:2], region=region[2:]).tobytes(), (NAMES[fmt], region)


def test_preprocess_frame_nv12_region_on_skewed_planes(env):
    """NV12 planes whose pitch is a multiple of 4 but whose base is not: the region's origin decides whether plane + x0 is aligned
    again (dword loads of luma and, at an even origin, of chroma) or not (bytes). Tapped regions, against the twin."""
    torch, engine, twin = env[:3]
    from nv12_child import nv12_planes, upload
    h, w, pitch = 120, 160, 164
    y, uv = nv12_planes(78, h, w, pitch, pitch)
    planes = (y[:, :w], uv[:, :w])
    for off, region in ((1, (3, 17, 52, 20)), (1, (4, 17, 52, 20)), (2, (2, 18, 52, 20)), (2, (6, 5, 50, 21)), (0, (36, 18, 52, 20)),
                        (3, (33, 17, 21, 13))):
        d_y, d_uv = upload(torch, y, off), upload(torch, uv, off)
        frame = engine.Frame.from_tensors(NV12, w, h, d_y, pitch, d_uv, pitch)
        out = torch.full((3, region[3], region[2]), float("nan"), dtype=torch.float32, device="cuda")
        engine.preprocess_frame(frame, out, region=region)
        torch.cuda.synchronize()
        want = twin.frame_to_tensor(NV12, planes, origin=region[:2], region=region[2:])
        assert out.cpu().numpy().tobytes() == want.tobytes(), (off, region)


def test_preprocess_letterbox_frame_equals_the_twin(env):
    torch, engine, twin = env[:3]
    for fmt, (w, h) in ((UYVY, (5, 128)), (RGB, (128, 72)), (GBRG, (128, 72)), (RGGB, (64, 40)), (YUYV, (64, 64)), (RGBA, (5, 128))):
        c = make_frame(torch, engine, twin, fmt, 85, h, w)
        out = torch.full((3, 64, 64), float("nan"), dtype=torch.float32, device="cuda")
        engine.preprocess_letterbox_frame(c["frame"], out, PAD)
        torch.cuda.synchronize()
        want = twin.letterbox_frame_to_tensor(fmt, c["planes"], (64, 64), PAD, size=(w, h))
        assert out.cpu().numpy().tobytes() == want.tobytes(), (NAMES[fmt], w, h)


# ------------------------------------------------------------------------------------ 2. whole frames in the stem

def two_step_tensor(env, e, c):
    torch, engine = env[0], env[1]
    images = torch.empty((1, 3, e.height, e.width), dtype=torch.float32, device="cuda")
    engine.preprocess_frame(c["frame"], images)
    torch.cuda.synchronize()
    return images


def run_frame(e, c):
    return e.infer_frame(c["frame"], None, CONF, IOU, Q)


def check_in_stem_equals_two_step(env, e, c):
    images = two_step_tensor(env, e, c)
    want = e.infer(images, CONF, IOU, Q)
    e.set_fusion(False)
    e.forward(images)
    stem_want = e.read_buffer("backbone.stem")
    e.set_fusion(True)
    got = run_frame(e, c)
    stem_got = e.read_buffer("backbone.stem")
    print(NAMES[c["fmt"]], c["w"], c["h"], "detections", len(want), "stem mismatches", int(np.count_nonzero(stem_got != stem_want)))
    assert np.array_equal(stem_got, stem_want)
    assert len(want) > 0 and got.tobytes() == want.tobytes()
    assert run_frame(e, c).tobytes() == want.tobytes()          # twice: the stem node is re-pointed per call
    return images, want


@pytest.mark.parametrize("fmt", NEW_FORMATS, ids=ids(NEW_FORMATS))
def test_frame_in_the_stem_kernel_is_bit_identical(env, eng, fmt):
    """unina_infer_frame against unina_preprocess_frame + unina_infer: the network's size aligned (the quad loaders' wide loads)
    and misaligned (their byte loads), 720p (down-scale) and 45 x 77 (up-scale, odd both ways)."""
    torch, engine, twin = env[:3]
    for name in CAMERAS:
        c = camera(torch, engine, twin, fmt, name)
        images, _ = check_in_stem_equals_two_step(env, eng, c)
        if name == "45x77_up":                                  # the two-step form itself against the twin, once per format
            assert images.cpu().numpy()[0].tobytes() == twin_tensor(env, c, (eng.height, eng.width)).tobytes()


@pytest.mark.parametrize("precision", ["FP32", "STRICT"])
def test_frame_in_the_other_stem_instantiations(env, sd7, precision):
    """The fp32 and the split-fp16 stem kernels on one 4:2:2 and one Bayer camera (the fp16 one: the test above)."""
    torch, engine, twin, _s, export = env
    e = engine.Engine.from_state_dict(sd7, precision=getattr(export, precision))
    try:
        for fmt, name in ((YUYV, "640_wide"), (UYVY, "640_bytes"), (GRBG, "640_wide"), (RGGB, "640_bytes"), (BGGR, "45x77_up")):
            check_in_stem_equals_two_step(env, e, camera(torch, engine, twin, fmt, name))
    finally:
        e.close()


# ------------------------------------------------------------------------------------ 3. BGRA / NV12 through the new calls

TILES_OLD = [(64, 32, 640, 640), (33, 17, 640, 640), (101, 61, 320, 480)]


def test_bgra_and_nv12_through_the_frame_calls_are_the_named_calls(env, eng):
    torch, engine, twin = env[:3]
    images = torch.from_numpy(np.random.default_rng(86).standard_normal((1, 3, 640, 640)).astype(np.float32)).cuda()
    before = eng.infer(images, CONF, IOU, Q)
    assert len(before) > 0
    for h, w, misaligned in ((640, 640, False), (720, 1280, True)):
        b = make_frame(torch, engine, twin, BGRA, 87, h, w, misaligned)
        n = make_frame(torch, engine, twin, NV12, 88, h, w, misaligned)
        want = eng.infer_bgra(b["d"], w, h, b["pitch"], None, CONF, IOU, Q)
        assert len(want) > 0 and eng.infer_frame(b["frame"], None, CONF, IOU, Q).tobytes() == want.tobytes()
        want = eng.infer_nv12(n["d"], n["d_uv"], w, h, n["pitch"], n["uv_pitch"], None, CONF, IOU, Q)
        assert len(want) > 0 and eng.infer_frame(n["frame"], None, CONF, IOU, Q).tobytes() == want.tobytes()
        for map_boxes in (False, True):
            want = eng.infer_letterbox_bgra(b["d"], w, h, b["pitch"], None, CONF, IOU, Q, PAD, map_boxes)
            assert eng.infer_letterbox_frame(b["frame"], None, CONF, IOU, Q, PAD, map_boxes).tobytes() == want.tobytes()
            want = eng.infer_letterbox_nv12(n["d"], n["d_uv"], w, h, n["pitch"], n["uv_pitch"], None, CONF, IOU, Q, PAD, map_boxes)
            assert eng.infer_letterbox_frame(n["frame"], None, CONF, IOU, Q, PAD, map_boxes).tobytes() == want.tobytes()
    b = make_frame(torch, engine, twin, BGRA, 89, 720, 1280, lo=104, hi=152)
    n = make_frame(torch, engine, twin, NV12, 90, 720, 1280, lo=104, hi=152)
    want = eng.infer_tiled_bgra(b["d"], 1280, 720, b["pitch"], TILES_OLD, None, CONF, IOU, Q, MERGE)
    assert len(want) > 0 and eng.infer_tiled_frame(b["frame"], TILES_OLD, None, CONF, IOU, Q, MERGE).tobytes() == want.tobytes()
    want = eng.infer_tiled_nv12(n["d"], n["d_uv"], 1280, 720, n["pitch"], n["uv_pitch"], TILES_OLD, None, CONF, IOU, Q, MERGE)
    assert len(want) > 0 and eng.infer_tiled_frame(n["frame"], TILES_OLD, None, CONF, IOU, Q, MERGE).tobytes() == want.tobytes()
    # the pre-process of the old formats through the descriptor is the named pre-process
    L, s, norm = eng.L, torch.cuda.current_stream().cuda_stream, eng.L.create_norm_params_imagenet()
    a = torch.full((3, 640, 640), float("nan"), dtype=torch.float32, device="cuda")
    z = torch.full((3, 640, 640), float("nan"), dtype=torch.float32, device="cuda")
    assert L.preprocess_bgra_resize(b["d"].data_ptr(), a.data_ptr(), 1280, 720, b["pitch"], 640, 640, norm, s) == 0
    engine.preprocess_frame(b["frame"], z)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == z.cpu().numpy().tobytes()
    assert L.unina_preprocess_nv12_resize(n["d"].data_ptr(), n["d_uv"].data_ptr(), a.data_ptr(), 1280, 720, n["pitch"], n["uv_pitch"], 640, 640, norm, s) == 0
    engine.preprocess_frame(n["frame"], z)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == z.cpu().numpy().tobytes()
    # a tensor frame after a run of frame calls gives its earlier bytes
    assert eng.infer(images, CONF, IOU, Q).tobytes() == before.tobytes()


# ------------------------------------------------------------------------------------ 4. letterbox

@pytest.mark.parametrize("fmt", [UYVY, GBRG], ids=ids([UYVY, GBRG]))
def test_letterboxed_frame_equals_two_step_and_unmap(env, eng, fmt):
    torch, engine, twin = env[:3]
    w, h = 1280, 720
    c = make_frame(torch, engine, twin, fmt, 91, h, w)
    images = torch.full((1, 3, eng.height, eng.width), float("nan"), dtype=torch.float32, device="cuda")
    engine.preprocess_letterbox_frame(c["frame"], images, PAD)
    torch.cuda.synchronize()
    assert images.cpu().numpy()[0].tobytes() == twin.letterbox_frame_to_tensor(fmt, c["planes"], (eng.height, eng.width), PAD).tobytes()
    want = eng.infer(images, CONF, IOU, Q)
    assert len(want) > 0
    got = eng.infer_letterbox_frame(c["frame"], None, CONF, IOU, Q, PAD, False)
    assert got.tobytes() == want.tobytes()
    mapped = eng.infer_letterbox_frame(c["frame"], None, CONF, IOU, Q, PAD, True)
    assert mapped.tobytes() == twin.unmap_boxes(want, w, h, eng.width, eng.height).tobytes()
    out = torch.full((MAXD * 8 + 8,), -1, dtype=torch.int32, device="cuda")            # the async form
    eng.infer_letterbox_frame(c["frame"], None, CONF, IOU, Q, PAD, True, out=out)
    torch.cuda.synchronize()
    assert engine.Engine.unpack(out).tobytes() == mapped.tobytes()


# ------------------------------------------------------------------------------------ 5. tiles

FRAME_W, FRAME_H = 1001, 803                                                            # odd both ways
TILES = [(0, 0, 640, 640), (181, 77, 640, 640), (361, 163, 640, 640), (500, 300, 320, 400)]


@pytest.mark.parametrize("fmt", [YUYV, GRBG, RGB], ids=ids([YUYV, GRBG, RGB]))
def test_tiled_frame_equals_twin_per_tile_then_merge(env, eng, fmt):
    torch, engine, twin, slicing, _x = env
    c = make_frame(torch, engine, twin, fmt, 92, FRAME_H, FRAME_W, lo=104, hi=152)    # low contrast: a tile's records fit its slot
    slots = np.zeros((len(TILES), MAXD), dtype=slicing.DET_DTYPE)
    counts = []
    buf = torch.zeros((MAXD * 8 + 8,), dtype=torch.int32, device="cuda")
    for t, (x0, y0, w, h) in enumerate(TILES):
        x = twin_tensor(env, c, (640, 640), origin=(x0, y0), region=(w, h))
        eng.infer_async(torch.from_numpy(x[None]).cuda(), CONF, IOU, Q, out=buf)
        torch.cuda.synchronize()
        d = engine.Engine.unpack(buf)
        slots[t, :len(d)] = d
        counts.append(len(d))
    d_slots = torch.from_numpy(slots.view(np.int32).reshape(len(TILES), -1)).cuda()
    d_counts = torch.from_numpy(np.asarray(counts, dtype=np.int32)).cuda()
    out = torch.full((MAXD * 8 + 8,), -1, dtype=torch.int32, device="cuda")
    eng.merge_tiles(d_slots, d_counts, TILES, MERGE, out=out)
    torch.cuda.synchronize()
    want = engine.Engine.unpack(out)
    print(NAMES[fmt], "per-tile counts", counts, "merged", len(want))
    assert min(counts) >= 1 and len(want) > 0
    got = eng.infer_tiled_frame(c["frame"], TILES, None, CONF, IOU, Q, MERGE)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() == slicing.merge_numpy(slots, counts, TILES, MERGE).tobytes()
    out2 = torch.full((MAXD * 8 + 8,), -1, dtype=torch.int32, device="cuda")            # the async form
    eng.infer_tiled_frame(c["frame"], TILES, None, CONF, IOU, Q, MERGE, out=out2)
    torch.cuda.synchronize()
    assert engine.Engine.unpack(out2).tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------ 6. the one-thread-per-pixel stem

def test_one_thread_per_pixel_stem_gives_the_same_bytes(env, eng, tmp_path):
    """UNINA_STEM_V1=1 is read once per process: one fresh child runs CHILD_CASES through stem_conv_kernel; the parent's default
    (tiled) run must give the same records and the same stem buffer."""
    torch, engine, twin = env[:3]
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "frame_child.py"), out], capture_output=True, text=True,
                       timeout=240, env=dict(os.environ, UNINA_STEM_V1="1"))
    assert r.returncode == 0 and "FRAME_CHILD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.load(out, allow_pickle=False)
    assert str(got["kernel"]).startswith("stem_conv_kernel")
    assert [o["kernel"] for o in eng.op_infos() if o["kernel"].startswith("stem_")][0].startswith("stem_tile_kernel")
    for k, (fmt, name) in enumerate(CHILD_CASES):
        want = run_frame(eng, camera(torch, engine, twin, fmt, name))
        assert len(want) > 0 and got[f"det{k}"].tobytes() == want.tobytes(), (NAMES[fmt], name)
        assert np.array_equal(got[f"stem{k}"], eng.read_buffer("backbone.stem")), (NAMES[fmt], name)


# ------------------------------------------------------------------------------------ 7. rejections

def test_bad_frames_are_rejected_and_leave_the_handle_intact(env, eng):
    torch, engine, twin = env[:3]
    images = torch.from_numpy(np.random.default_rng(93).standard_normal((1, 3, 640, 640)).astype(np.float32)).cuda()
    before = eng.infer(images, CONF, IOU, Q)
    assert len(before) > 0
    good = make_frame(torch, engine, twin, YUYV, 94, 45, 77)
    d, F = good["d"], engine.Frame.from_tensors
    bad = [
        F(10, 77, 45, d, 156), F(-1, 77, 45, d, 156),           # format outside 0..9
        F(YUYV, 77, 45, None, 156),                             # null plane
        F(YUYV, 77, 45, d, 155),                                # 4 * ((77 + 1) / 2) = 156
        F(RGB, 77, 45, d, 230),                                 # 3 * 77 = 231
        F(GBRG, 1, 45, d, 4), F(RGGB, 77, 1, d, 77),            # a Bayer frame of width / height 1
        F(RGBA, 8, 8, d.data_ptr() + 1, 32), F(RGBA, 8, 8, d, 34),   # misaligned RGBA
        F(NV12, 77, 45, d, 77),                                 # no chroma plane
    ]
    whole = [(0, 0, 77, 45)]
    out = torch.zeros((MAXD * 8 + 8,), dtype=torch.int32, device="cuda")
    calls = []
    for f in bad:
        calls += [lambda f=f: eng.infer_frame(f, None, CONF, IOU, Q), lambda f=f: eng.infer_frame(f, None, CONF, IOU, Q, out=out),
                  lambda f=f: eng.infer_letterbox_frame(f, None, CONF, IOU, Q), lambda f=f: eng.infer_tiled_frame(f, whole)]
    calls += [lambda: eng.infer_tiled_frame(good["frame"], [(1, 0, 77, 45)]), lambda: eng.infer_tiled_frame(good["frame"], []),
              lambda: eng.infer_tiled_frame(good["frame"], whole * 65), lambda: eng.infer_tiled_frame(good["frame"], [(1, 0, 77, 45)], out=out),
              lambda: eng.infer_letterbox_frame(good["frame"], None, CONF, IOU, Q, PAD, 2)]
    for i, call in enumerate(calls):
        with pytest.raises(engine.EngineError, match=r"\[ARG\] unina_infer(_letterbox|_tiled)?_frame(_async)?: \S") as err:
            call()
        assert eng.L.unina_last_error(eng.h), i
        if i % 4 == 3 or i >= 4 * len(bad):
            assert eng.infer(images, CONF, IOU, Q).tobytes() == before.tobytes(), (i, str(err.value))
    n = C.c_int()
    norm = eng.L.create_norm_params_imagenet()
    host = np.zeros(MAXD, dtype=engine.DET_DTYPE)
    assert eng.L.unina_infer_frame(eng.h, C.byref(bad[0]), C.byref(norm), CONF, IOU, Q, host.ctypes.data, C.byref(n), None) == 4
    assert eng.L.unina_infer_frame(eng.h, None, C.byref(norm), CONF, IOU, Q, host.ctypes.data, C.byref(n), None) == 4
    with pytest.raises(engine.EngineError):
        engine.preprocess_frame(bad[3], torch.empty((3, 8, 8), dtype=torch.float32, device="cuda"))
    # the good call still works afterwards
    assert len(run_frame(eng, good)) > 0
    assert eng.infer(images, CONF, IOU, Q).tobytes() == before.tobytes()
