"""csrc/camera_source.h -- the one definition of a network-input pixel computed from a camera frame, which both the stem kernels
and the pre-process kernels call -- compiled for the host (tests/camera_pixel_host.cpp: g++ -ffp-contract=off, no HIP) and compared
BYTE for byte with the scalar oracle and the numpy twins. Every case also runs in a second build of the driver with
-fsanitize=address,undefined as the stand-alone program it is. No GPU."""
import struct

import numpy as np
import pytest

import hostprog

TENSOR, BGRA_TAP, BGRA_RESIZE, NV12_TAP, NV12_RESIZE, BGRA_LETTERBOX, NV12_LETTERBOX = range(7)   # camera_source.h: CameraKind
NORM = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)
PAD = 114.0                                                                                        # (the letterbox cases: not 0)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("camera_pixel_host")
    return hostprog.build_pair(d, "camera_pixel_host.cpp"), d


def run(drivers, kind, plane, uv, w, h, pitch, uv_pitch, dst_hw, origin=(0, 0), inner=(0, 0, 0, 0), mode=0, skew=(0, 0),
        wide=(1, 1), x_even=0):
    """Both builds of the driver on one case; returns (float32 [3, dh, dw], what the driver printed). The sanitised build must give
    the same bytes."""
    dh, dw = dst_hw
    plane = np.ascontiguousarray(plane, dtype=np.uint8).tobytes()
    uv = b"" if uv is None else np.ascontiguousarray(uv, dtype=np.uint8).tobytes()
    head = struct.pack("<24i7f", 0x43414d31, mode, kind, w, h, pitch, uv_pitch, origin[0], origin[1], dw, dh, *inner, len(plane), len(uv),
                       skew[0], skew[1], wide[0], wide[1], x_even, 0, 0, PAD, *NORM)
    got, said = hostprog.run_pair(*drivers, head + plane + uv, dtype=np.float32, stdout=True)
    return got.reshape(3, dh, dw), said


def bgra_frame(seed, h, w, pitch):
    buf = np.random.default_rng(seed).integers(0, 256, (h, pitch), dtype=np.uint8)
    return buf, np.ascontiguousarray(buf[:, :4 * w]).reshape(h, w, 4)


def nv12_frame(seed, h, w, y_pitch, uv_pitch):
    """Pitched planes and their unpadded views: y [h, w], uv [(h + 1) // 2, 2 * ((w + 1) // 2)]."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 256, (h, y_pitch), dtype=np.uint8)
    uv = rng.integers(0, 256, ((h + 1) // 2, uv_pitch), dtype=np.uint8)
    return y, uv, np.ascontiguousarray(y[:, :w]), np.ascontiguousarray(uv[:, :2 * ((w + 1) // 2)])


def test_bgra_plain_equals_oracle(drivers, oracle_mod):
    h, w, pitch = 50, 70, 4 * 70 + 12
    buf, img = bgra_frame(41, h, w, pitch)
    got, _ = run(drivers, BGRA_TAP, buf, None, w, h, pitch, 0, (h, w))
    assert got.tobytes() == oracle_mod.preprocess_bgra(img).tobytes()


@pytest.mark.parametrize("src,dst", [((50, 70), (64, 64)), ((7, 9), (16, 16))])
def test_bgra_resize_equals_oracle(drivers, oracle_mod, src, dst):
    h, w = src
    buf, img = bgra_frame(42, h, w, 4 * w)
    got, _ = run(drivers, BGRA_RESIZE, buf, None, w, h, 4 * w, 0, dst)
    assert got.tobytes() == oracle_mod.preprocess_bgra(img, dst_hw=dst).tobytes()


@pytest.mark.parametrize("h,w,y_pitch,uv_pitch", [(50, 70, 74, 74), (7, 9, 9, 10)])
def test_nv12_plain_equals_oracle(drivers, oracle_mod, h, w, y_pitch, uv_pitch):
    y, uv, yv, uvv = nv12_frame(43, h, w, y_pitch, uv_pitch)
    got, _ = run(drivers, NV12_TAP, y, uv, w, h, y_pitch, uv_pitch, (h, w))
    assert got.tobytes() == oracle_mod.preprocess_nv12(yv, uvv).tobytes()


@pytest.mark.parametrize("dst", [(13, 21), (16, 20)])                         # the region's own size (tap) | resized
def test_nv12_region_at_odd_origin_equals_twin(drivers, pkg, dst):
    y, uv, yv, uvv = nv12_frame(44, 120, 160, 160, 160)
    x0, y0, w, h = 33, 17, 21, 13
    kind = NV12_TAP if dst == (h, w) else NV12_RESIZE
    got, _ = run(drivers, kind, y, uv, w, h, 160, 160, dst, origin=(x0, y0))
    want = pkg.camera.nv12_to_tensor(yv, uvv, dst_hw=dst, origin=(x0, y0), region=(w, h))
    assert got.tobytes() == want.tobytes()


# 5 x 128: half-to-even gives new_w = 2 | bars above and below | the rectangle has the frame's size: the tap path | identity
@pytest.mark.parametrize("w,h", [(5, 128), (128, 72), (64, 40), (64, 64)])
def test_letterboxes_equal_twins(drivers, pkg, w, h):
    dst = (64, 64)
    from unina_yolo_dla_amd.mine import letterbox_geometry
    new_w, new_h, left, top = letterbox_geometry(w, h, dst[1], dst[0])
    if (w, h) == (5, 128):
        assert new_w == 2
    if (w, h) in ((64, 40), (64, 64)):
        assert (new_w, new_h) == (w, h)
    inner = (left, top, new_w, new_h)
    buf, img = bgra_frame(45, h, w, 4 * w)
    got, _ = run(drivers, BGRA_LETTERBOX, buf, None, w, h, 4 * w, 0, dst, inner=inner)
    want = pkg.camera.letterbox_bgra_to_tensor(img, dst, pad_value=PAD, norm=NORM)
    assert got.tobytes() == want.tobytes()
    uv_pitch = 2 * ((w + 1) // 2)
    y, uv, yv, uvv = nv12_frame(46, h, w, w, uv_pitch)
    got, _ = run(drivers, NV12_LETTERBOX, y, uv, w, h, w, uv_pitch, dst, inner=inner)
    want = pkg.camera.letterbox_nv12_to_tensor(yv, uvv, dst, pad_value=PAD, norm=NORM)
    assert got.tobytes() == want.tobytes()
    assert len(np.unique(got)) > 50                                            # (not a constant picture)


# (y_pitch, uv_pitch, plane skew, chroma skew, origin) -> what nv12_quad_alignment must answer
QUAD_CASES = {
    "aligned": ((96, 96, 0, 0, (0, 0)), "1 1"),
    "luma_pitch": ((94, 96, 0, 0, (0, 0)), "0 1"),
    "chroma_base": ((96, 96, 0, 2, (0, 0)), "1 0"),
    "odd_origin": ((96, 96, 0, 0, (33, 17)), "0 0"),
    "even_origin": ((96, 96, 0, 0, (36, 18)), "1 1"),
}


@pytest.mark.parametrize("case", sorted(QUAD_CASES))
def test_quad_helper_equals_per_pixel_function(drivers, case):
    """nv12_quad against camera_pixel(kSrcNv12Tap) on the same frame: with the dword loads the alignment allows and with byte loads,
    and where the column is even also with each pair read once (x_even). Width 50: a row tail of two pixels."""
    (y_pitch, uv_pitch, skew_y, skew_c, origin), allowed = QUAD_CASES[case]
    fh, fw = 40, 90
    y, uv, _, _ = nv12_frame(47, fh, fw, y_pitch, uv_pitch)
    w, h = 50, 21
    kw = dict(origin=origin, skew=(skew_y, skew_c))
    want, _ = run(drivers, NV12_TAP, y, uv, w, h, y_pitch, uv_pitch, (h, w), **kw)
    assert len(np.unique(want)) > 100
    for wide in ((1, 1), (0, 0)):
        for x_even in ((0, 1) if origin[0] % 2 == 0 else (0,)):
            got, said = run(drivers, NV12_TAP, y, uv, w, h, y_pitch, uv_pitch, (h, w), mode=1, wide=wide, x_even=x_even, **kw)
            assert said.strip() == allowed
            assert got.tobytes() == want.tobytes(), (case, wide, x_even)
