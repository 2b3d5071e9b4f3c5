"""The frame descriptor's formats (RGB, RGBA, YUYV, UYVY, Bayer) without a GPU: csrc/camera_source.h compiled for the host
(tests/frame_formats_host.cpp: g++ -ffp-contract=off, no HIP) against the oracle, the NV12 twin (itself pinned to the oracle) and
the numpy twins of camera.py, BYTE for byte. Every case also runs in a second build of the driver with
-fsanitize=address,undefined as the stand-alone program it is; the plane it reads ends where its buffer ends."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hostprog

ROOT = hostprog.ROOT
BGRA, NV12, RGB, RGBA, YUYV, UYVY, RGGB, BGGR, GRBG, GBRG = range(10)      # include/unina_mi355.h: unina_pixel_format
BAYER = (RGGB, BGGR, GRBG, GBRG)
NORM = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)
PAD = 114.0


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_formats_host")
    return hostprog.build_pair(d, "frame_formats_host.cpp"), d


def run(drivers, fmt, plane, fw, fh, pitch, dst_hw=None, region=None, inner=None, mode=0, skew=0, wide=1):
    """Both builds of the driver on one case; returns (float32 [3, dh, dw] or None, what the driver printed). The sanitised build
    must give the same bytes. region = (x, y, w, h), default the whole frame; inner = (left, top, new_w, new_h): letterboxed."""
    x, y, w, h = region or (0, 0, fw, fh)
    dh, dw = dst_hw or (h, w)
    plane = b"" if plane is None else np.ascontiguousarray(plane, dtype=np.uint8).tobytes()
    boxed, inner = (0, (0, 0, 0, 0)) if inner is None else (1, inner)
    head = struct.pack("<24i7f", 0x43414d32, mode, fmt, fw, fh, pitch, x, y, w, h, dw, dh, boxed, *inner, len(plane), skew, wide, 0, 0, 0, 0,
                       PAD, *NORM)
    got, said = hostprog.run_pair(*drivers, head + plane, dtype=None if mode == 2 else np.float32, stdout=True)
    return (None if mode == 2 else got.reshape(3, dh, dw)), said


def pitched(rows: np.ndarray, pitch: int, seed: int = 99) -> np.ndarray:
    """[h, n] rows -> the bytes of a frame of `pitch` bytes per row, noise in the padding, cut after the last row's last byte."""
    h, n = rows.shape
    assert pitch >= n
    buf = np.random.default_rng(seed).integers(0, 256, (h, pitch), dtype=np.uint8)
    buf[:, :n] = rows
    return buf.reshape(-1)[:(h - 1) * pitch + n]


def bgra_image(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def nv12_frame(seed, h, w):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, ((h + 1) // 2, 2 * ((w + 1) // 2)), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- RGB / RGBA against the reference
@pytest.mark.parametrize("src,dst", [((50, 70), None), ((50, 70), (64, 64)), ((7, 9), (16, 16))])
def test_rgb_and_rgba_equal_oracle(drivers, oracle_mod, pkg, src, dst):
    h, w = src
    img = bgra_image(61, h, w)
    want = oracle_mod.preprocess_bgra(img) if dst is None else oracle_mod.preprocess_bgra(img, dst_hw=dst)
    cam = pkg.camera
    for fmt, pix in ((RGB, cam.bgra_to_rgb(img)), (RGBA, cam.bgra_to_rgba(img))):
        bpp = pix.shape[2]
        got, _ = run(drivers, fmt, pix.reshape(h, w * bpp), w, h, w * bpp, dst)
        assert got.tobytes() == want.tobytes(), (fmt, src, dst)
        assert cam.frame_to_tensor(fmt, pix, dst_hw=dst, norm=NORM).tobytes() == want.tobytes()


@pytest.mark.parametrize("dst", [None, (64, 64)])
def test_rgb_odd_pitch_and_skewed_base(drivers, oracle_mod, pkg, dst):
    h, w = 50, 70
    img = bgra_image(62, h, w)
    want = oracle_mod.preprocess_bgra(img) if dst is None else oracle_mod.preprocess_bgra(img, dst_hw=dst)
    rgb = pkg.camera.bgra_to_rgb(img).reshape(h, 3 * w)
    got, _ = run(drivers, RGB, pitched(rgb, 3 * w + 5), w, h, 3 * w + 5, dst, skew=1)
    assert got.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------- 4:2:2 against the NV12 twin
@pytest.mark.parametrize("fmt,order", [(YUYV, "yuyv"), (UYVY, "uyvy")])
@pytest.mark.parametrize("src,dst", [((50, 70), None), ((7, 9), (16, 16))])
def test_yuv422_equals_nv12_twin(drivers, pkg, fmt, order, src, dst):
    h, w = src
    y, uv = nv12_frame(63, h, w)
    want = pkg.camera.nv12_to_tensor(y, uv, dst_hw=dst, norm=NORM)
    packed = pkg.camera.nv12_to_yuv422(y, uv, order)
    assert packed.shape == (h, 4 * ((w + 1) // 2))
    got, _ = run(drivers, fmt, packed, w, h, packed.shape[1], dst)
    assert got.tobytes() == want.tobytes()
    assert pkg.camera.frame_to_tensor(fmt, packed, dst_hw=dst, norm=NORM, region=(w, h)).tobytes() == want.tobytes()
    assert len(np.unique(got)) > 50


@pytest.mark.parametrize("fmt,order", [(YUYV, "yuyv"), (UYVY, "uyvy")])
@pytest.mark.parametrize("dst", [(13, 21), (16, 20)])                         # the region's own size (tap) | resized
def test_yuv422_region_at_odd_origin(drivers, pkg, fmt, order, dst):
    y, uv = nv12_frame(64, 120, 160)
    x0, y0, w, h = 33, 17, 21, 13
    want = pkg.camera.nv12_to_tensor(y, uv, dst_hw=dst, norm=NORM, origin=(x0, y0), region=(w, h))
    packed = pkg.camera.nv12_to_yuv422(y, uv, order)
    got, _ = run(drivers, fmt, packed, 160, 120, 320, dst, region=(x0, y0, w, h))
    assert got.tobytes() == want.tobytes()
    assert pkg.camera.frame_to_tensor(fmt, packed, dst_hw=dst, norm=NORM, origin=(x0, y0), region=(w, h)).tobytes() == want.tobytes()


# the four letterboxes of test_camera_pixel_cpu.test_letterboxes_equal_twins
@pytest.mark.parametrize("w,h", [(5, 128), (128, 72), (64, 40), (64, 64)])
def test_yuv422_letterboxes_equal_nv12_twin(drivers, pkg, w, h):
    dst = (64, 64)
    from unina_yolo_dla_amd.mine import letterbox_geometry
    new_w, new_h, left, top = letterbox_geometry(w, h, dst[1], dst[0])
    y, uv = nv12_frame(65, h, w)
    want = pkg.camera.letterbox_nv12_to_tensor(y, uv, dst, pad_value=PAD, norm=NORM)
    for fmt, order in ((YUYV, "yuyv"), (UYVY, "uyvy")):
        packed = pkg.camera.nv12_to_yuv422(y, uv, order)
        got, _ = run(drivers, fmt, packed, w, h, packed.shape[1], dst, inner=(left, top, new_w, new_h))
        assert got.tobytes() == want.tobytes(), (fmt, w, h)
        assert pkg.camera.letterbox_frame_to_tensor(fmt, packed, dst, PAD, NORM, size=(w, h)).tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------- Bayer
def scalar_demosaic(raw, fmt):
    """The definition in include/unina_mi355.h at unina_pixel_format, one pixel at a time."""
    h, w = raw.shape
    colours = {RGGB: "RGGB", BGGR: "BGGR", GRBG: "GRBG", GBRG: "GBRG"}[fmt]          # of (X & 1, Y & 1) = (0,0), (1,0), (0,1), (1,1)
    f = np.float32

    def at(X, Y):
        X = 1 if X == -1 else (w - 2 if X == w else X)
        Y = 1 if Y == -1 else (h - 2 if Y == h else Y)
        return f(raw[Y, X])

    out = np.zeros((3, h, w), dtype=np.float32)
    for Y in range(h):
        for X in range(w):
            c = colours[(Y & 1) * 2 + (X & 1)]
            v = {}
            if c in "RB":
                v[c] = at(X, Y)
                v["G"] = (at(X, Y - 1) + at(X - 1, Y) + at(X + 1, Y) + at(X, Y + 1)) * f(0.25)
                v["B" if c == "R" else "R"] = (at(X - 1, Y - 1) + at(X + 1, Y - 1) + at(X - 1, Y + 1) + at(X + 1, Y + 1)) * f(0.25)
            else:
                v["G"] = at(X, Y)
                row_colour = colours[(Y & 1) * 2 + ((X + 1) & 1)]
                v[row_colour] = (at(X - 1, Y) + at(X + 1, Y)) * f(0.5)
                v["B" if row_colour == "R" else "R"] = (at(X, Y - 1) + at(X, Y + 1)) * f(0.5)
            out[:, Y, X] = v["R"], v["G"], v["B"]
    return out


def normalise(rgb):
    n = [np.float32(v) for v in NORM]
    return np.stack([((rgb[c] / np.float32(255.0)) - n[c]) / n[3 + c] for c in range(3)]).astype(np.float32)


@pytest.mark.parametrize("fmt", BAYER)
def test_bayer_constant_colour_equals_oracle(drivers, oracle_mod, pkg, fmt):
    h, w = 10, 12
    img = np.empty((h, w, 4), dtype=np.uint8)
    img[...] = (200, 90, 31, 255)                                             # B, G, R, A
    raw = pkg.camera.mosaic(pkg.camera.bgra_to_rgb(img), fmt)
    got, _ = run(drivers, fmt, raw, w, h, w)
    assert got.tobytes() == oracle_mod.preprocess_bgra(img).tobytes()


@pytest.mark.parametrize("fmt", BAYER)
def test_bayer_affine_image_equals_oracle_inside(drivers, oracle_mod, pkg, fmt):
    """Bilinear interpolation reproduces a channel that is affine in x and y wherever no neighbour is reflected."""
    h, w = 48, 64
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([200 - xx - 2 * yy, 5 + 3 * xx + yy, 10 + 2 * xx + yy, np.full((h, w), 255)], axis=-1)      # B, G, R, A
    assert img.min() >= 0 and img.max() <= 255
    img = img.astype(np.uint8)
    raw = pkg.camera.mosaic(pkg.camera.bgra_to_rgb(img), fmt)
    got, _ = run(drivers, fmt, raw, w, h, w)
    want = oracle_mod.preprocess_bgra(img)
    assert got[:, 1:-1, 1:-1].tobytes() == want[:, 1:-1, 1:-1].tobytes()
    assert got.tobytes() != want.tobytes()                                    # (the border is the reflection's, not the image's)


@pytest.mark.parametrize("fmt", BAYER)
@pytest.mark.parametrize("h,w", [(2, 2), (5, 6)])                             # reflection acts on both sides
def test_bayer_twin_equals_scalar_definition(drivers, pkg, fmt, h, w):
    raw = np.random.default_rng(66).integers(0, 256, (h, w), dtype=np.uint8)
    want = scalar_demosaic(raw, fmt)
    twin = np.stack(pkg.camera.bayer_to_rgb(raw, fmt))
    assert twin.dtype == np.float32 and twin.tobytes() == want.tobytes()
    got, _ = run(drivers, fmt, raw, w, h, w)
    assert got.tobytes() == normalise(want).tobytes()
    assert pkg.camera.frame_to_tensor(fmt, raw, norm=NORM).tobytes() == normalise(want).tobytes()


@pytest.mark.parametrize("fmt", BAYER)
def test_bayer_region_at_odd_origin_is_the_crop(drivers, pkg, fmt):
    fh, fw = 40, 90
    raw = np.random.default_rng(67).integers(0, 256, (fh, fw), dtype=np.uint8)
    full, _ = run(drivers, fmt, raw, fw, fh, fw)
    x0, y0, w, h = 33, 17, 21, 13
    got, _ = run(drivers, fmt, raw, fw, fh, fw, region=(x0, y0, w, h))
    assert got.tobytes() == np.ascontiguousarray(full[:, y0:y0 + h, x0:x0 + w]).tobytes()
    assert pkg.camera.frame_to_tensor(fmt, raw, norm=NORM, origin=(x0, y0), region=(w, h)).tobytes() == got.tobytes()
    # the region that touches the frame's far corner reflects at the FRAME's border
    got, _ = run(drivers, fmt, raw, fw, fh, fw, region=(fw - 5, fh - 3, 5, 3))
    assert got.tobytes() == np.ascontiguousarray(full[:, fh - 3:, fw - 5:]).tobytes()


@pytest.mark.parametrize("one,other", [(RGGB, BGGR), (GRBG, GBRG)])
def test_exchanged_pattern_exchanges_red_and_blue(drivers, pkg, one, other):
    """BGGR on the same bytes is RGGB with the r and b planes exchanged (and GBRG is GRBG likewise). The driver's planes are
    normalised per channel, so they are compared through the twin's un-normalised planes."""
    raw = np.random.default_rng(68).integers(0, 256, (9, 14), dtype=np.uint8)
    ra, ga, ba = pkg.camera.bayer_to_rgb(raw, one)
    rb, gb, bb = pkg.camera.bayer_to_rgb(raw, other)
    assert ra.tobytes() == bb.tobytes() and ba.tobytes() == rb.tobytes() and ga.tobytes() == gb.tobytes()
    assert ra.tobytes() != ba.tobytes()
    a, _ = run(drivers, one, raw, 14, 9, 14)
    b, _ = run(drivers, other, raw, 14, 9, 14)
    assert a.tobytes() == normalise(np.stack([ra, ga, ba])).tobytes() and b.tobytes() == normalise(np.stack([rb, gb, bb])).tobytes()


@pytest.mark.parametrize("fmt", BAYER)
def test_bayer_resize_and_letterbox_equal_twin(drivers, pkg, fmt):
    from unina_yolo_dla_amd.mine import letterbox_geometry
    raw = np.random.default_rng(69).integers(0, 256, (50, 70), dtype=np.uint8)
    for region, dst in (((0, 0, 70, 50), (64, 64)), ((33, 17, 21, 13), (16, 20)), ((0, 0, 9, 7), (16, 16))):
        got, _ = run(drivers, fmt, raw, 70, 50, 70, dst, region=region)
        want = pkg.camera.frame_to_tensor(fmt, raw, dst_hw=dst, norm=NORM, origin=region[:2], region=region[2:])
        assert got.tobytes() == want.tobytes(), (fmt, region, dst)
    for w, h in ((5, 128), (128, 72), (64, 40), (64, 64)):
        raw = np.random.default_rng(70).integers(0, 256, (h, w), dtype=np.uint8)
        new_w, new_h, left, top = letterbox_geometry(w, h, 64, 64)
        got, _ = run(drivers, fmt, raw, w, h, w, (64, 64), inner=(left, top, new_w, new_h))
        assert got.tobytes() == pkg.camera.letterbox_frame_to_tensor(fmt, raw, (64, 64), PAD, NORM).tobytes(), (fmt, w, h)


# ---------------------------------------------------------------------------------------------- quad helpers
# (pitch, base skew, origin) -> what the alignment predicate must answer, for a 4:2:2 frame 90 wide (180 bytes per row at least)
# and a Bayer frame 90 wide. Region 50 x 21: a row tail of two pixels.
YUV_QUADS = {
    "aligned": ((184, 0, (0, 0)), "1"),
    "odd_pitch": ((181, 0, (0, 0)), "0"),
    "pitch_4_not_8": ((188, 0, (0, 0)), "0"),
    "skewed_base": ((184, 4, (0, 0)), "0"),
    "odd_origin": ((184, 0, (33, 17)), "0"),
    "even_origin": ((184, 0, (36, 18)), "1"),
    "origin_2": ((184, 0, (2, 1)), "0"),            # even, but 2 * x0 = 4 is no multiple of 8
}
BAYER_QUADS = {
    "aligned": ((92, 0, (0, 0)), "1"),
    "odd_pitch": ((91, 0, (0, 0)), "0"),
    "skewed_base": ((92, 1, (0, 0)), "0"),
    "odd_origin": ((92, 0, (33, 17)), "0"),
    "skew_cancels_origin": ((92, 3, (33, 17)), "1"),
    "even_origin": ((92, 0, (36, 18)), "1"),
    "frame_edges": ((92, 0, (40, 19)), "1"),          # the region ends at the frame's right and bottom borders: 90 - 50, 40 - 21
}


def quad_check(drivers, fmt, rows, fw, fh, case, size=(50, 21)):
    (pitch, skew, origin), allowed = case
    plane = pitched(rows, pitch)
    region = (origin[0], origin[1], *size)
    want, _ = run(drivers, fmt, plane, fw, fh, pitch, region=region, skew=skew)
    assert len(np.unique(want)) > min(100, size[0] * size[1] // 2)
    for wide in (1, 0):
        got, said = run(drivers, fmt, plane, fw, fh, pitch, region=region, skew=skew, mode=1, wide=wide)
        assert said.strip() == allowed
        assert got.tobytes() == want.tobytes(), (fmt, case, wide)


@pytest.mark.parametrize("fmt", [YUYV, UYVY])
@pytest.mark.parametrize("case", sorted(YUV_QUADS))
def test_yuv422_quad_equals_per_pixel_function(drivers, fmt, case):
    fh, fw = 40, 90
    rows = np.random.default_rng(71).integers(0, 256, (fh, 2 * fw), dtype=np.uint8)
    quad_check(drivers, fmt, rows, fw, fh, YUV_QUADS[case])


@pytest.mark.parametrize("fmt", BAYER)
@pytest.mark.parametrize("case", sorted(BAYER_QUADS))
def test_bayer_quad_equals_per_pixel_function(drivers, fmt, case):
    fh, fw = 40, 90
    rows = np.random.default_rng(72).integers(0, 256, (fh, fw), dtype=np.uint8)
    quad_check(drivers, fmt, rows, fw, fh, BAYER_QUADS[case])


@pytest.mark.parametrize("fmt", BAYER)
def test_bayer_quad_whole_frame_reflects_under_wide_loads(drivers, fmt):
    """8 x 6, every quad wide: the first quad's left column and the last quad's right column are reflected, as are rows -1 and 6."""
    rows = np.random.default_rng(76).integers(0, 256, (6, 8), dtype=np.uint8)
    quad_check(drivers, fmt, rows, 8, 6, ((8, 0, (0, 0)), "1"), size=(8, 6))


# ---------------------------------------------------------------------------------------------- argument checks, header, packers
FRAME_CHECKS = [
    # format, w, h, pitch, plane bytes -> accepted
    ((RGB, 10, 4, 30, 120), True), ((RGB, 10, 4, 29, 120), False), ((RGB, 10, 4, 35, 140), True),
    ((RGBA, 10, 4, 40, 160), True), ((RGBA, 10, 4, 42, 168), False), ((RGBA, 10, 4, 36, 160), False),
    ((YUYV, 9, 4, 20, 80), True), ((YUYV, 9, 4, 18, 80), False), ((UYVY, 10, 4, 20, 80), True), ((UYVY, 10, 4, 19, 80), False),
    ((RGGB, 10, 4, 10, 40), True), ((RGGB, 10, 4, 9, 40), False), ((GBRG, 1, 4, 4, 16), False), ((BGGR, 4, 1, 4, 4), False),
    ((GRBG, 2, 2, 2, 4), True),
    ((-1, 10, 4, 40, 160), False), ((10, 10, 4, 40, 160), False), ((RGB, 0, 4, 30, 120), False), ((RGB, 10, 4, 30, 0), False),
]


@pytest.mark.parametrize("case,ok", FRAME_CHECKS)
def test_frame_geometry_checks(drivers, case, ok):
    fmt, w, h, pitch, nbytes = case
    _, said = run(drivers, fmt, np.zeros(nbytes, dtype=np.uint8) if nbytes else None, w, h, pitch, mode=2)
    assert (said.strip() == "ok") == ok, (case, said)


def test_misaligned_rgba_base_is_refused(drivers):
    _, said = run(drivers, RGBA, np.zeros(164, dtype=np.uint8), 10, 4, 40, mode=2, skew=2)
    assert said.strip() != "ok"
    _, said = run(drivers, RGB, np.zeros(124, dtype=np.uint8), 10, 4, 30, mode=2, skew=1)
    assert said.strip() == "ok"


def test_library_refuses_bad_frames_before_touching_a_device(pkg):
    """unina_preprocess_frame checks the frame first: no device is needed to be told UNINA_ERR_ARG."""
    from unina_yolo_dla_amd import build, engine
    build.build_native()
    L = engine.load_library()
    norm = L.create_norm_params_imagenet()
    fake = 0x1000                                                              # never dereferenced: every call below is refused
    for fmt, w, h, pitch in ((10, 8, 8, 32), (-1, 8, 8, 32), (RGB, 8, 8, 23), (YUYV, 9, 8, 18), (GBRG, 1, 8, 8), (RGBA, 8, 8, 34)):
        fr = engine.Frame.from_tensors(fmt, w, h, fake, pitch)
        assert L.unina_preprocess_frame(C.byref(fr), None, fake, 8, 8, C.byref(norm), None) == 4, (fmt, w, h, pitch)
        assert L.unina_preprocess_letterbox_frame(C.byref(fr), fake, 8, 8, 114.0, C.byref(norm), None) == 4
    fr = engine.Frame.from_tensors(RGB, 8, 8, None, 24)
    assert L.unina_preprocess_frame(C.byref(fr), None, fake, 8, 8, C.byref(norm), None) == 4         # null plane
    fr = engine.Frame.from_tensors(RGB, 8, 8, fake, 24)
    assert L.unina_preprocess_frame(C.byref(fr), C.byref(engine.Tile(4, 4, 5, 4)), fake, 8, 8, C.byref(norm), None) == 4   # region outside
    assert L.unina_preprocess_frame(C.byref(fr), None, None, 8, 8, C.byref(norm), None) == 4
    assert L.unina_infer_frame(None, C.byref(fr), C.byref(norm), 0.3, 0.45, 0.0, None, None, None) == 4
    assert C.sizeof(engine.Frame) == 40                                        # 3 ints, pad, 2 pointers, 2 ints


def test_header_compiles_as_plain_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc
    src = tmp_path / "use.c"
    src.write_text('#define UNINA_NO_HIP_HEADERS\n#include "unina_mi355.h"\n'
                   "int main(void) { unina_frame f = {UNINA_FMT_BAYER_GBRG, 2, 2, {0, 0}, {2, 0}}; unina_pixel_format p = UNINA_FMT_UYVY;\n"
                   "  return (f.format == 9 && p == 5 && UNINA_FMT_RGB == 2 && UNINA_FMT_RGBA == 3) ? 0 : 1; }\n")
    exe = tmp_path / "use"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_packers(pkg):
    cam = pkg.camera
    rgb = np.random.default_rng(73).integers(0, 256, (4, 6, 3), dtype=np.uint8)
    m = cam.mosaic(rgb, "grbg")                                                # G R / B G
    assert m[0, 0] == rgb[0, 0, 1] and m[0, 1] == rgb[0, 1, 0] and m[1, 0] == rgb[1, 0, 2] and m[1, 1] == rgb[1, 1, 1]
    m = cam.mosaic(rgb, cam.FMT_BAYER_RGGB)
    assert m[0, 0] == rgb[0, 0, 0] and m[0, 1] == rgb[0, 1, 1] and m[1, 0] == rgb[1, 0, 1] and m[1, 1] == rgb[1, 1, 2]
    y, uv = nv12_frame(74, 5, 7)
    p = cam.nv12_to_yuv422(y, uv, "uyvy")
    assert p.shape == (5, 16)
    assert p[3, 4 * 1 + 1] == y[3, 2] and p[3, 4 * 1 + 3] == y[3, 3] and p[3, 4] == uv[1, 2] and p[3, 6] == uv[1, 3]
    assert p[4, 4 * 3 + 1] == y[4, 6] and p[4, 4 * 3 + 3] == 0 and p[4, 12] == uv[2, 6]
    img = bgra_image(75, 3, 3)
    assert cam.bgra_to_rgb(img)[1, 2].tolist() == img[1, 2, [2, 1, 0]].tolist()
    assert cam.bgra_to_rgba(img)[1, 2].tolist() == img[1, 2, [2, 1, 0, 3]].tolist()
