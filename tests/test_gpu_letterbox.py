"""Letterboxed camera frames inside the stem, boxes back in camera pixels (unina_infer_letterbox_bgra / _nv12 and their _async
forms, unina_preprocess_letterbox_bgra / _nv12). Every comparison is byte-exact, on the 64 x 64 seed-7 engine: the two-step
tensor against the numpy twins (pinned to the oracle by tests/test_letterbox_cpu.py), the in-stem form against two-step +
unina_infer, the mapped records against camera.unmap_boxes of the unmapped ones. Every compared detection list is checked to
hold at least one record (the threshold comes from the CPU oracle: tests/letterbox_child.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from letterbox_child import CAMERAS, CONF, IOU, NET, PAD, Q, ROOT, device_camera, run_letterbox, visible

pytestmark = pytest.mark.gpu

MAXD = 1024
FORMATS = ("bgra", "nv12")


@pytest.fixture(scope="module")
def env(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unina_yolo_dla_amd import camera as twin, engine, export
    return torch, engine, twin, export


def make_engine(env, pkg, sd7, precision="FP16"):
    return env[1].Engine.from_state_dict(sd7, pkg.graph.Graph(in_h=NET, in_w=NET), precision=getattr(env[3], precision))


@pytest.fixture(scope="module")
def eng(env, pkg, sd7):
    e = make_engine(env, pkg, sd7)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cams(env):
    return {name: device_camera(env[0], name) for name in CAMERAS}


def two_step_tensor(env, e, c, fmt):
    """unina_preprocess_letterbox_* into an fp32 tensor (NaN first: every element must be written)."""
    torch, L = env[0], e.L
    images = torch.full((1, 3, e.height, e.width), float("nan"), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    norm = L.create_norm_params_imagenet()
    if fmt == "bgra":
        rc = L.unina_preprocess_letterbox_bgra(c["d_bgra"].data_ptr(), images.data_ptr(), c["w"], c["h"], c["pitch"], e.width, e.height,
                                               PAD, norm, s)
    else:
        rc = L.unina_preprocess_letterbox_nv12(c["d_y"].data_ptr(), c["d_uv"].data_ptr(), images.data_ptr(), c["w"], c["h"],
                                               c["y_pitch"], c["uv_pitch"], e.width, e.height, PAD, norm, s)
    assert rc == 0
    torch.cuda.synchronize()
    return images


def twin_tensor(env, c, fmt):
    img, y, uv = visible(c)
    if fmt == "bgra":
        return env[2].letterbox_bgra_to_tensor(img, (NET, NET), PAD)
    return env[2].letterbox_nv12_to_tensor(y, uv, (NET, NET), PAD)


def check_in_stem_equals_two_step(env, e, c, fmt):
    images = two_step_tensor(env, e, c, fmt)
    want = e.infer(images, CONF, IOU, Q)
    e.set_fusion(False)
    e.forward(images)
    stem_want = e.read_buffer("backbone.stem")
    e.set_fusion(True)
    got = run_letterbox(e, c, fmt)
    stem_got = e.read_buffer("backbone.stem")
    print(c["name"], fmt, "detections", len(want), "stem mismatches", int(np.count_nonzero(stem_got != stem_want)))
    assert np.array_equal(stem_got, stem_want)
    assert len(want) > 0 and got.tobytes() == want.tobytes()
    assert run_letterbox(e, c, fmt).tobytes() == want.tobytes()      # twice: the stem node is re-pointed per call
    return want


# ------------------------------------------------------------------------------------ 1. the two-step form

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(CAMERAS))
def test_two_step_tensor_equals_the_twin(env, eng, cams, name, fmt):
    c = cams[name]
    got = two_step_tensor(env, eng, c, fmt).cpu().numpy()[0]
    want = twin_tensor(env, c, fmt)
    print(name, fmt, "mismatches", int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))))
    assert got.tobytes() == want.tobytes()


def test_two_step_refuses_bad_geometry(env, eng, cams):
    torch, L = env[0], eng.L
    c = cams["40x30_up"]
    out = torch.zeros((3, NET, NET), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    norm = L.create_norm_params_imagenet()
    b, y, uv = c["d_bgra"].data_ptr(), c["d_y"].data_ptr(), c["d_uv"].data_ptr()
    w, h = c["w"], c["h"]
    assert L.unina_preprocess_letterbox_bgra(b, out.data_ptr(), w, h, 4 * w - 4, NET, NET, PAD, norm, s) != 0     # pitch too small
    assert L.unina_preprocess_letterbox_bgra(b, out.data_ptr(), w, h, c["pitch"], 0, NET, PAD, norm, s) != 0
    assert L.unina_preprocess_letterbox_bgra(b, out.data_ptr(), 0, h, c["pitch"], NET, NET, PAD, norm, s) != 0
    assert L.unina_preprocess_letterbox_bgra(None, out.data_ptr(), w, h, c["pitch"], NET, NET, PAD, norm, s) != 0
    assert L.unina_preprocess_letterbox_nv12(y, None, out.data_ptr(), w, h, c["y_pitch"], c["uv_pitch"], NET, NET, PAD, norm, s) != 0
    assert L.unina_preprocess_letterbox_nv12(y, uv, out.data_ptr(), w, h, w - 1, c["uv_pitch"], NET, NET, PAD, norm, s) != 0
    assert L.unina_preprocess_letterbox_nv12(y, uv, out.data_ptr(), w, h, c["y_pitch"], c["uv_pitch"], NET, -1, PAD, norm, s) != 0
    torch.cuda.synchronize()
    assert not out.any()                                                                  # nothing was enqueued


# ------------------------------------------------------------------------------------ 2. the in-stem form

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(CAMERAS))
def test_letterbox_in_the_stem_kernel_is_bit_identical(env, eng, cams, name, fmt):
    check_in_stem_equals_two_step(env, eng, cams[name], fmt)


@pytest.mark.parametrize("precision", ["FP32", "STRICT"])
def test_letterbox_in_the_other_stem_instantiations(env, pkg, sd7, cams, precision):
    e = make_engine(env, pkg, sd7, precision)
    try:
        for name in CAMERAS:
            for fmt in FORMATS:
                check_in_stem_equals_two_step(env, e, cams[name], fmt)
    finally:
        e.close()


def test_identity_frame_equals_the_plain_camera_calls(env, eng, cams):
    c = cams["64x64_identity"]
    a = eng.infer_bgra(c["d_bgra"], c["w"], c["h"], c["pitch"], None, CONF, IOU, Q)
    b = eng.infer_nv12(c["d_y"], c["d_uv"], c["w"], c["h"], c["y_pitch"], c["uv_pitch"], None, CONF, IOU, Q)
    assert len(a) > 0 and len(b) > 0
    for m in (False, True):
        assert run_letterbox(eng, c, "bgra", m).tobytes() == a.tobytes()
        assert run_letterbox(eng, c, "nv12", m).tobytes() == b.tobytes()


def test_one_thread_per_pixel_stem_gives_the_same_bytes(env, eng, cams, tmp_path):
    """UNINA_STEM_V1=1 is read once per process: one fresh child runs every camera through stem_conv_kernel."""
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "letterbox_child.py"), out], capture_output=True, text=True,
                       timeout=240, env=dict(os.environ, UNINA_STEM_V1="1"))
    assert r.returncode == 0 and "LETTERBOX_CHILD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.load(out, allow_pickle=False)
    assert str(got["kernel"]).startswith("stem_conv_kernel")
    assert [o["kernel"] for o in eng.op_infos() if o["kernel"].startswith("stem_")][0].startswith("stem_tile_kernel")
    for k, name in enumerate(CAMERAS):
        for fmt in FORMATS:
            want = run_letterbox(eng, cams[name], fmt)
            assert len(want) > 0 and got[f"det_{fmt}{k}"].tobytes() == want.tobytes(), (name, fmt)
            assert np.array_equal(got[f"stem_{fmt}{k}"], eng.read_buffer("backbone.stem")), (name, fmt)


# ------------------------------------------------------------------------------------ 3. the box map

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(CAMERAS))
def test_mapped_boxes_equal_the_twin_of_the_unmapped_ones(env, eng, cams, name, fmt):
    torch, engine, twin, _x = env
    c = cams[name]
    raw = run_letterbox(eng, c, fmt, map_boxes=False)
    want = twin.unmap_boxes(raw, c["w"], c["h"], NET, NET)
    got = run_letterbox(eng, c, fmt, map_boxes=True)
    print(name, fmt, "records", len(raw))
    assert len(raw) > 0 and len(got) == len(raw)
    assert got.tobytes() == want.tobytes()                         # counts, order and every byte
    if name != "64x64_identity":
        assert got.tobytes() != raw.tobytes()
    # the async form, mapped and unmapped, + a device -> host copy
    for m, ref in ((True, want), (False, raw)):
        buf = torch.full((MAXD * 8 + 8,), -1, dtype=torch.int32, device="cuda")
        run_letterbox(eng, c, fmt, map_boxes=m, out=buf)
        torch.cuda.synchronize()
        assert engine.Engine.unpack(buf).tobytes() == ref.tobytes()


def test_mapped_boxes_of_the_one_launch_post_process(env, pkg, sd7, cams, tmp_path):
    """UNINA_POST_SPLIT=0 (everything in one launch) writes its records elsewhere in the code: the same map there. The switch is
    read at load, so it is set around the construction of a second engine."""
    twin = env[2]
    old = os.environ.get("UNINA_POST_SPLIT")
    os.environ["UNINA_POST_SPLIT"] = "0"
    try:
        e = make_engine(env, pkg, sd7)
    finally:
        if old is None:
            del os.environ["UNINA_POST_SPLIT"]
        else:
            os.environ["UNINA_POST_SPLIT"] = old
    try:
        c = cams["128x72_down"]
        raw = run_letterbox(e, c, "bgra", map_boxes=False)
        got = run_letterbox(e, c, "bgra", map_boxes=True)
        assert len(raw) > 0 and got.tobytes() == twin.unmap_boxes(raw, c["w"], c["h"], NET, NET).tobytes()
    finally:
        e.close()


# ------------------------------------------------------------------------------------ 4. the other calls are untouched

def test_other_paths_return_the_same_bytes_after_letterbox_calls(env, eng, cams):
    torch = env[0]
    rng = np.random.default_rng(91)
    images = torch.from_numpy(rng.standard_normal((1, 3, NET, NET)).astype(np.float32)).cuda()
    c = cams["128x72_down"]
    tiles = [(0, 0, 64, 64), (64, 8, 64, 64), (30, 4, 80, 60)]

    def others():
        return [eng.infer(images, CONF, IOU, Q),
                eng.infer_bgra(c["d_bgra"], c["w"], c["h"], c["pitch"], None, CONF, IOU, Q),
                eng.infer_nv12(c["d_y"], c["d_uv"], c["w"], c["h"], c["y_pitch"], c["uv_pitch"], None, CONF, IOU, Q),
                eng.infer_tiled_bgra(c["d_bgra"], c["w"], c["h"], c["pitch"], tiles, None, CONF, IOU, Q, 0.45)]

    before = others()
    assert all(len(d) > 0 for d in before)
    buf = torch.zeros((MAXD * 8 + 8,), dtype=torch.int32, device="cuda")
    for name in ("40x30_up", "64x37_r1"):
        for fmt in FORMATS:
            assert len(run_letterbox(eng, cams[name], fmt, map_boxes=True)) > 0
            run_letterbox(eng, cams[name], fmt, map_boxes=True, out=buf)       # the async form leaves the flag off as well
            torch.cuda.synchronize()
            after = others()
            for a, b in zip(before, after):
                assert a.tobytes() == b.tobytes(), (name, fmt)


# ------------------------------------------------------------------------------------ 5. rejections

def test_bad_arguments_are_rejected_and_leave_the_handle_intact(env, eng, cams):
    torch, engine, _t, _x = env
    images = torch.from_numpy(np.random.default_rng(92).standard_normal((1, 3, NET, NET)).astype(np.float32)).cuda()
    before = eng.infer(images, CONF, IOU, Q)
    assert len(before) > 0
    c = cams["5x128_even"]                    # width 5: the pair rule asks uv_pitch >= 6
    w, h, p, yp, uvp = c["w"], c["h"], c["pitch"], c["y_pitch"], c["uv_pitch"]
    buf = torch.zeros((MAXD * 8 + 8,), dtype=torch.int32, device="cuda")
    B, N = eng.infer_letterbox_bgra, eng.infer_letterbox_nv12
    cases = [
        lambda: B(None, w, h, p),                                               # null frame
        lambda: B(c["d_bgra"], w, h, 4 * w - 4),                                # pitch too small
        lambda: B(c["d_bgra"], w, h, p + 2),                                    # pitch not a multiple of 4
        lambda: B(c["d_bgra"], 0, h, p),
        lambda: B(c["d_bgra"], w, -1, p),
        lambda: B(c["d_bgra"], w, h, p, map_boxes=2),
        lambda: B(c["d_bgra"], w, h, p + 2, out=buf),                           # the async form
        lambda: N(c["d_y"], None, w, h, yp, uvp),                               # null chroma plane
        lambda: N(c["d_y"], c["d_uv"], w, h, yp, uvp - 1),                      # uv_pitch 5 >= width, < 6
        lambda: N(c["d_y"], c["d_uv"], w, h, w - 1, uvp),
        lambda: N(c["d_y"], c["d_uv"], w, 0, yp, uvp),
        lambda: N(c["d_y"], c["d_uv"], w, h, yp, uvp, map_boxes=-1),
        lambda: N(None, c["d_uv"], w, h, yp, uvp, out=buf),
    ]
    for i, call in enumerate(cases):
        with pytest.raises(engine.EngineError, match=r"\[ARG\] unina_infer_letterbox_(bgra|nv12)(_async)?: \S") as err:
            call()
        assert eng.L.unina_last_error(eng.h), i
        assert eng.infer(images, CONF, IOU, Q).tobytes() == before.tobytes(), (i, str(err.value))
    torch.cuda.synchronize()
    assert not buf.any()                                                       # a refused call enqueues nothing
    # the return code itself
    n = C.c_int()
    norm = eng.L.create_norm_params_imagenet()
    host = np.zeros(MAXD, dtype=engine.DET_DTYPE)
    assert eng.L.unina_infer_letterbox_bgra(eng.h, c["d_bgra"].data_ptr(), w, h, p, C.byref(norm), CONF, IOU, Q, PAD, 3,
                                            host.ctypes.data, C.byref(n), None) == 4
    assert eng.L.unina_infer_letterbox_nv12(eng.h, c["d_y"].data_ptr(), None, w, h, yp, uvp, C.byref(norm), CONF, IOU, Q, PAD, 1,
                                            host.ctypes.data, C.byref(n), None) == 4
    # the good call still works afterwards
    assert len(run_letterbox(eng, c, "bgra", True)) > 0 and len(run_letterbox(eng, c, "nv12", True)) > 0
    assert eng.infer(images, CONF, IOU, Q).tobytes() == before.tobytes()
