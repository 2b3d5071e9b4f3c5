"""NV12 camera frames straight into the stem, whole and tiled (unina_infer_nv12, unina_infer_tiled_nv12[_async],
unina_preprocess_nv12_resize). Every comparison is byte-exact: the stand-alone pre-process against camera.nv12_to_tensor (the
numpy twin, itself pinned to the oracle by tests/test_camera_cpu.py), the in-stem form against the two-step form, the tiled
call against twin tensor per tile -> unina_infer_async -> unina_merge_tiles_async."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from nv12_child import CAMERAS, CHILD_CAMERAS, CONF, IOU, Q, ROOT, camera, nv12_planes, upload

pytestmark = pytest.mark.gpu

MERGE = 0.45
MAXD = 1024


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


def visible(c):
    """The planes without their padding, as the twin takes them."""
    return c["y"][:, :c["w"]], c["uv"][:, :2 * ((c["w"] + 1) // 2)]


def two_step_tensor(env, e, c):
    """preprocess_nv12 (the network's size) or unina_preprocess_nv12_resize into an fp32 tensor."""
    torch, L = env[0], e.L
    images = torch.empty((1, 3, e.height, e.width), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    norm = L.create_norm_params_imagenet()
    if (c["h"], c["w"]) == (e.height, e.width):
        assert L.preprocess_nv12(c["d_y"].data_ptr(), c["d_uv"].data_ptr(), images.data_ptr(), c["w"], c["h"], c["y_pitch"],
                                 c["uv_pitch"], norm, s) == 0
    else:
        assert L.unina_preprocess_nv12_resize(c["d_y"].data_ptr(), c["d_uv"].data_ptr(), images.data_ptr(), c["w"], c["h"],
                                              c["y_pitch"], c["uv_pitch"], e.width, e.height, norm, s) == 0
    torch.cuda.synchronize()
    return images


def run_nv12(e, c):
    return e.infer_nv12(c["d_y"], c["d_uv"], c["w"], c["h"], c["y_pitch"], c["uv_pitch"], None, CONF, IOU, Q)


def check_in_stem_equals_two_step(env, e, c):
    images = two_step_tensor(env, e, c)
    want = e.infer(images, CONF, IOU, Q)
    e.set_fusion(False)
    e.forward(images)
    stem_want = e.read_buffer("backbone.stem")
    e.set_fusion(True)
    got = run_nv12(e, c)
    stem_got = e.read_buffer("backbone.stem")
    print("detections", len(want), "stem mismatches", int(np.count_nonzero(stem_got != stem_want)))
    assert np.array_equal(stem_got, stem_want)
    assert len(want) > 0 and got.tobytes() == want.tobytes()
    assert run_nv12(e, c).tobytes() == want.tobytes()          # twice: the stem node is re-pointed per call
    return images, want, stem_want


# ------------------------------------------------------------------------------------ 1. the stand-alone pre-process

@pytest.mark.parametrize("h,w,y_pitch,uv_pitch,dst", [(50, 70, 74, 74, (64, 64)), (360, 640, 768, 768, (64, 96)), (7, 9, 9, 10, (16, 16))])
def test_preprocess_nv12_resize_equals_the_twin(env, h, w, y_pitch, uv_pitch, dst):
    torch, engine, twin, _s, _x = env
    L = engine.load_library()
    y, uv = nv12_planes(71, h, w, y_pitch, uv_pitch)
    dy, duv = upload(torch, y), upload(torch, uv)
    s = torch.cuda.current_stream().cuda_stream
    norm = L.create_norm_params_imagenet()
    out = torch.full((3,) + dst, float("nan"), dtype=torch.float32, device="cuda")
    assert L.unina_preprocess_nv12_resize(dy.data_ptr(), duv.data_ptr(), out.data_ptr(), w, h, y_pitch, uv_pitch, dst[1], dst[0], norm, s) == 0
    torch.cuda.synchronize()
    want = twin.nv12_to_tensor(y[:, :w], uv[:, :2 * ((w + 1) // 2)], dst_hw=dst)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    # the pitch rules: preprocess_nv12's, and the whole last pair of an odd-width row
    assert L.unina_preprocess_nv12_resize(dy.data_ptr(), duv.data_ptr(), out.data_ptr(), w, h, w - 1, uv_pitch, dst[1], dst[0], norm, s) != 0
    assert L.unina_preprocess_nv12_resize(dy.data_ptr(), duv.data_ptr(), out.data_ptr(), w, h, y_pitch, 2 * ((w + 1) // 2) - 1, dst[1], dst[0], norm, s) != 0
    assert L.unina_preprocess_nv12_resize(dy.data_ptr(), None, out.data_ptr(), w, h, y_pitch, uv_pitch, dst[1], dst[0], norm, s) != 0


def test_preprocess_nv12_resize_at_the_source_size_is_preprocess_nv12(env):
    torch, engine, twin, _s, _x = env
    L = engine.load_library()
    h, w, pitch = 50, 70, 74
    y, uv = nv12_planes(72, h, w, pitch, pitch)
    dy, duv = upload(torch, y), upload(torch, uv)
    s = torch.cuda.current_stream().cuda_stream
    norm = L.create_norm_params_imagenet()
    a = torch.full((3, h, w), float("nan"), dtype=torch.float32, device="cuda")
    b = torch.full((3, h, w), float("nan"), dtype=torch.float32, device="cuda")
    assert L.unina_preprocess_nv12_resize(dy.data_ptr(), duv.data_ptr(), a.data_ptr(), w, h, pitch, pitch, w, h, norm, s) == 0
    assert L.preprocess_nv12(dy.data_ptr(), duv.data_ptr(), b.data_ptr(), w, h, pitch, pitch, norm, s) == 0
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert a.cpu().numpy().tobytes() == twin.nv12_to_tensor(y[:, :w], uv[:, :w]).tobytes()


# ------------------------------------------------------------------------------------ 2. / 3. whole frames in the stem

@pytest.mark.parametrize("name", list(CAMERAS))
def test_nv12_frame_in_the_stem_kernel_is_bit_identical(env, eng, name):
    """unina_infer_nv12 against the two-step form: same arithmetic, so the stem output and the detections agree bit for bit.
    The network's size with aligned planes (dword loads) and with odd pitches on planes one byte off (byte loads), 720p
    (down-scale) and 45 x 77 (up-scale, odd both ways)."""
    torch = env[0]
    c = camera(torch, name)
    check_in_stem_equals_two_step(env, eng, c)


@pytest.mark.parametrize("precision", ["FP32", "STRICT"])
def test_nv12_frame_in_the_other_stem_instantiations(env, sd7, precision):
    """The fp32 and the split-fp16 stem kernels on the network-sized camera (the fp16 one: the test above)."""
    torch, engine, _t, _s, export = env
    e = engine.Engine.from_state_dict(sd7, precision=getattr(export, precision))
    try:
        check_in_stem_equals_two_step(env, e, camera(torch, "640_wide"))
        check_in_stem_equals_two_step(env, e, camera(torch, "640_bytes"))
    finally:
        e.close()


def test_tensor_and_bgra_paths_are_unchanged_by_nv12_calls(env, eng):
    torch = env[0]
    rng = np.random.default_rng(73)
    images = torch.from_numpy(rng.standard_normal((1, 3, 640, 640)).astype(np.float32)).cuda()
    bgra = torch.from_numpy(rng.integers(0, 256, (480, 600 * 4 + 64), dtype=np.uint8)).cuda()
    before = eng.infer(images, CONF, IOU, Q)
    before_bgra = eng.infer_bgra(bgra, 600, 480, 600 * 4 + 64, None, CONF, IOU, Q)
    assert len(before) > 0 and len(before_bgra) > 0
    for name in ("720p_down", "640_bytes"):
        c = camera(torch, name)
        assert len(run_nv12(eng, c)) > 0
        assert eng.infer(images, CONF, IOU, Q).tobytes() == before.tobytes()
        assert eng.infer_bgra(bgra, 600, 480, 600 * 4 + 64, None, CONF, IOU, Q).tobytes() == before_bgra.tobytes()


# ------------------------------------------------------------------------------------ 4. the one-thread-per-pixel stem

def test_one_thread_per_pixel_stem_gives_the_same_bytes(env, eng, tmp_path):
    """UNINA_STEM_V1=1 is read once per process: one fresh child runs the 45 x 77 and a 640 x 640 camera through
    stem_conv_kernel; the parent's default (tiled) run must give the same records and the same stem buffer."""
    torch = env[0]
    out = str(tmp_path / "child.npz")
    child_env = dict(os.environ, UNINA_STEM_V1="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "nv12_child.py"), out], capture_output=True, text=True,
                       timeout=240, env=child_env)
    assert r.returncode == 0 and "NV12_CHILD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.load(out, allow_pickle=False)
    assert str(got["kernel"]).startswith("stem_conv_kernel")
    assert [o["kernel"] for o in eng.op_infos() if o["kernel"].startswith("stem_")][0].startswith("stem_tile_kernel")
    for k, name in enumerate(CHILD_CAMERAS):
        c = camera(torch, name)
        want = run_nv12(eng, c)
        assert len(want) > 0 and got[f"det{k}"].tobytes() == want.tobytes(), name
        assert np.array_equal(got[f"stem{k}"], eng.read_buffer("backbone.stem")), name


# ------------------------------------------------------------------------------------ 5. tiles

FRAME_H, FRAME_W = 1000, 1400
TILES = [(64, 32, 640, 640),                          # the network's size, even origin
         (33, 17, 640, 640),                          # the network's size, odd origin: the chroma pairs straddle the quads
         (701, 301, 320, 480),                        # resized, odd origin
         (FRAME_W - 640, FRAME_H - 640, 640, 640)]    # touches the bottom-right corner


def tiled_camera(torch, seed, h, w):
    """Low-contrast luma (as tests/test_gpu_tiled.py's camera()) so that a tile's records fit its slot."""
    y_pitch, uv_pitch = w + 8, w + 4
    y, uv = nv12_planes(seed, h, w, y_pitch, uv_pitch, lo=104, hi=152)
    return dict(h=h, w=w, y_pitch=y_pitch, uv_pitch=uv_pitch, y=y, uv=uv, d_y=upload(torch, y), d_uv=upload(torch, uv))


def run_tiled(e, c, tiles, out=None):
    return e.infer_tiled_nv12(c["d_y"], c["d_uv"], c["w"], c["h"], c["y_pitch"], c["uv_pitch"], tiles, None, CONF, IOU, Q, MERGE, out=out)


def test_tiled_nv12_equals_twin_per_tile_then_merge(env, eng):
    torch, engine, twin, slicing, _x = env
    c = tiled_camera(torch, 61, FRAME_H, FRAME_W)
    y, uv = visible(c)
    slots = np.zeros((len(TILES), MAXD), dtype=slicing.DET_DTYPE)
    counts = []
    buf = torch.zeros((MAXD * 8 + 8,), dtype=torch.int32, device="cuda")
    for t, (x0, y0, w, h) in enumerate(TILES):
        x = twin.nv12_to_tensor(y, uv, dst_hw=(640, 640), origin=(x0, y0), region=(w, h))
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
    print("per-tile counts", counts, "merged", len(want))
    assert min(counts) >= 1 and len(want) > 0
    got = run_tiled(eng, c, TILES)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() == slicing.merge_numpy(slots, counts, TILES, MERGE).tobytes()
    # the async form + a device -> host copy
    out2 = torch.full((MAXD * 8 + 8,), -1, dtype=torch.int32, device="cuda")
    run_tiled(eng, c, TILES, out=out2)
    torch.cuda.synchronize()
    assert engine.Engine.unpack(out2).tobytes() == want.tobytes()
    assert run_tiled(eng, c, TILES).tobytes() == want.tobytes()


def test_tiled_nv12_default_tiles_are_the_reference_slicing(env, eng):
    torch, engine, _t, _s, _x = env
    c = tiled_camera(torch, 62, 1080, 1920)
    n, tiles = engine.slice_tiles(1920, 1080)
    assert n == 8
    a = run_tiled(eng, c, tiles)
    b = run_tiled(eng, c, None)
    assert len(a) > 0 and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------ 6. rejections

def test_bad_arguments_are_rejected_and_leave_the_handle_intact(env, eng):
    torch, engine, _t, _s, _x = env
    images = torch.from_numpy(np.random.default_rng(74).standard_normal((1, 3, 640, 640)).astype(np.float32)).cuda()
    before = eng.infer(images, CONF, IOU, Q)
    assert len(before) > 0
    c = camera(torch, "45x77_up")          # width 77: the pair rule asks uv_pitch >= 78
    h, w, yp, uvp = c["h"], c["w"], c["y_pitch"], c["uv_pitch"]
    whole = [(0, 0, w, h)]
    cases = [
        lambda: eng.infer_nv12(c["d_y"], None, w, h, yp, uvp),                                     # null chroma plane
        lambda: eng.infer_nv12(c["d_y"], c["d_uv"], w, h, yp, uvp - 1),                            # uv_pitch 77 >= width, < 78
        lambda: eng.infer_tiled_nv12(c["d_y"], None, w, h, yp, uvp, whole),
        lambda: eng.infer_tiled_nv12(c["d_y"], c["d_uv"], w, h, yp, uvp - 1, whole),
        lambda: eng.infer_tiled_nv12(c["d_y"], c["d_uv"], w, h, yp, uvp, [(1, 0, w, h)]),          # one pixel outside
        lambda: eng.infer_tiled_nv12(c["d_y"], c["d_uv"], w, h, yp, uvp, [(0, 1, w, h)]),
        lambda: eng.infer_tiled_nv12(c["d_y"], c["d_uv"], w, h, yp, uvp, []),                      # 0 tiles
        lambda: eng.infer_tiled_nv12(c["d_y"], c["d_uv"], w, h, yp, uvp, whole * 65),              # 65 tiles
    ]
    out = torch.zeros((MAXD * 8 + 8,), dtype=torch.int32, device="cuda")
    cases.append(lambda: eng.infer_tiled_nv12(c["d_y"], c["d_uv"], w, h, yp, uvp, [(1, 0, w, h)], out=out))   # the async form
    for i, call in enumerate(cases):
        with pytest.raises(engine.EngineError, match=r"\[ARG\] unina_infer(_tiled)?_nv12: \S") as err:
            call()
        assert eng.L.unina_last_error(eng.h), i
        assert eng.infer(images, CONF, IOU, Q).tobytes() == before.tobytes(), (i, str(err.value))
    # the return code itself
    n = C.c_int()
    norm = eng.L.create_norm_params_imagenet()
    host = np.zeros(MAXD, dtype=engine.DET_DTYPE)
    assert eng.L.unina_infer_nv12(eng.h, c["d_y"].data_ptr(), None, w, h, yp, uvp, C.byref(norm), CONF, IOU, Q, host.ctypes.data, C.byref(n), None) == 4
    # the good call still works afterwards
    assert len(run_nv12(eng, c)) > 0
    assert eng.infer(images, CONF, IOU, Q).tobytes() == before.tobytes()
