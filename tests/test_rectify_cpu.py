"""unina_rectify_async without a GPU: rectify.rectify_numpy (the definition) against what rectification must do -- identity,
shifts whose answer is known, the direction of R, a float64 evaluation of the same camera model and its inverse, float64
bilinear sampling; csrc/rectify_map.h compiled for the host (tests/rectify_map_host.cpp, also under -fsanitize=undefined,address
as the stand-alone program it is) against the twin on whole images; the argument checks of the entry point; the layouts in C."""
import ctypes as C
import os

import numpy as np
import pytest

import hostprog
import rectify_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = (1, 3, 4)

# |fp32 coordinate - float64 coordinate| of rectify_source_numpy, in raw-image pixels. The chain from (u, v) to us is about 20
# fp32 operations, each rounded once: a relative error of at most 2^-24 of a value that, expressed in pixels (a normalised
# coordinate times the focal length, or the pixel coordinate itself), stays under 128. Were every rounding to reach the result
# undamped that is 20 * 128 * 2^-24 = 1.5e-4 px. The factor 2 on top covers what the chain does to an early error: the divide by
# W (0.96 .. 1.04 at 2 degrees) and the lens polynomial, whose gain |d(xd)/d(xn)| stays below 1.1 for DIST inside this image.
COORD_TOL = 2 * 20 * 128 * 2.0 ** -24       # 3.05e-4 px
# Back through the inverse model the same error is divided by the polynomial's least radial gain, asserted >= 0.5 below, and
# multiplied by dst.fx / src.fx < 1: twice the bound.
ROUND_TRIP_TOL = 2 * COORD_TOL


def twin(c):
    return rc.twin(c)


def channels_of(img):
    return img.reshape(img.shape[0], img.shape[1], -1)


# ---------------------------------------------------------------- what rectification must do
@pytest.mark.parametrize("channels", CHANNELS)
def test_identity_returns_the_input(pkg, channels):
    c = rc.named_cases(channels)[0]
    assert c["name"].startswith("identity")
    out = twin(c)
    assert out.shape == c["img"].shape and out.tobytes() == c["img"].tobytes()
    from unina_yolo_dla_amd import rectify
    _, _, inside, qx, qy = rectify.rectify_source_numpy(c["cam"], c["dst_hw"], c["img"].shape[:2])
    h, w = c["dst_hw"]
    assert inside.all() and (qx == 32 * np.arange(w)[None, :]).all() and (qy == 32 * np.arange(h)[:, None]).all()


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("border", (0, 114))
def test_integer_shift_moves_the_image(pkg, channels, border):
    """dst.cx = src.cx + 3, dst.cy = src.cy - 2: out[v, u] = in[v + 2, u - 3], `border` in the band nothing maps to."""
    c = next(x for x in rc.named_cases(channels) if x["name"].startswith(f"shift_b{border}"))
    assert c["border"] == border
    out, img = channels_of(twin(c)), channels_of(c["img"])
    h, w = c["dst_hw"]
    want = np.full_like(img, border)
    want[:h - 2, 3:] = img[2:, :w - 3]
    assert out.tobytes() == want.tobytes()
    assert (out[h - 2:] == border).all() and (out[:, :3] == border).all()


@pytest.mark.parametrize("channels", CHANNELS)
def test_half_pixel_shift_averages_two_neighbours(pkg, channels):
    """dst.cx = src.cx + 0.5: out[v, u] = (in[v, u - 1] + in[v, u] + 1) >> 1 for u >= 1; at u = 0 the left tap is the border."""
    c = next(x for x in rc.named_cases(channels) if x["name"].startswith("half_left"))
    out, img = channels_of(twin(c)).astype(np.int32), channels_of(c["img"]).astype(np.int32)
    assert (out[:, 1:] == (img[:, :-1] + img[:, 1:] + 1) >> 1).all()
    assert (out[:, 0] == (c["border"] + img[:, 0] + 1) >> 1).all() and c["border"] == 114


def test_direction_of_r(pkg):
    """p_rect = R * p_raw: the raw principal point, seen along (0, 0, 1), lands where the third column of R projects."""
    from unina_yolo_dla_amd import rectify
    h, w = rc.SMALL_HW
    fx, fy, cx, cy = rc.SMALL_PIN
    R = rc.rotation((0, 1, 0), 3.0)
    cam = rectify.make_rectify_cam(rc.SMALL_PIN, r=R)
    img = np.zeros((h, w), dtype=np.uint8)
    img[int(cy), int(cx)] = 255                                       # SMALL_PIN's principal point is a pixel centre
    assert (int(cx), int(cy)) == (cx, cy)
    out = rectify.rectify_numpy(img, cam, (h, w))
    want = (cx + fx * R[0, 2] / R[2, 2], cy + fy * R[1, 2] / R[2, 2])
    assert abs(want[0] - cx) > 1.5 and abs(want[0] - round(want[0])) < 0.3        # a real move, and not a tie between two pixels
    v, u = np.unravel_index(np.argmax(out), out.shape)
    assert (u, v) == (round(want[0]), round(want[1])) and out[v, u] > 128
    assert cam.r[2] == np.float32(R[0, 2]) and cam.r[6] == np.float32(R[2, 0]) and R[0, 2] > 0          # row-major


def model64(cam, u, v):
    """The header's model in float64, on the struct's (fp32) fields."""
    s, d, r = cam.src, cam.dst, np.array(list(cam.r), dtype=np.float64)
    x, y = (u - d.cx) / d.fx, (v - d.cy) / d.fy
    X, Y, W = r[0] * x + r[3] * y + r[6], r[1] * x + r[4] * y + r[7], r[2] * x + r[5] * y + r[8]
    xn, yn = X / W, Y / W
    r2 = xn * xn + yn * yn
    rad = ((cam.k3 * r2 + cam.k2) * r2 + cam.k1) * r2 + 1.0
    xd = xn * rad + cam.p1 * 2 * xn * yn + cam.p2 * (r2 + 2 * xn * xn)
    yd = yn * rad + cam.p1 * (r2 + 2 * yn * yn) + cam.p2 * 2 * xn * yn
    gain = 1.0 + 3 * cam.k1 * r2 + 5 * cam.k2 * r2 * r2 + 7 * cam.k3 * r2 ** 3       # d(r * rad) / dr
    return s.fx * xd + s.cx, s.fy * yd + s.cy, gain


def test_coordinates_against_float64_and_back(pkg):
    """97 x 61 -> 83 x 59 with DIST and a 2-degree rotation about a skew axis: us, vs agree with float64; undistorting (us, vs) by
    fixed-point iteration, rotating by R and projecting through dst returns (u, v)."""
    from unina_yolo_dla_amd import rectify
    cam = rc.distorted_cam()
    dh, dw = rc.DST_HW
    us, vs, inside, _, _ = rectify.rectify_source_numpy(cam, rc.DST_HW, rc.SRC_HW)
    v, u = np.mgrid[0:dh, 0:dw].astype(np.float64)
    us64, vs64, gain = model64(cam, u, v)
    assert np.abs(us64).max() < 128 and np.abs(vs64).max() < 128 and gain.min() >= 0.5
    err = max(np.abs(us - us64).max(), np.abs(vs - vs64).max())
    # the inverse: normalised distorted point -> undistorted by x <- (xd - tangential(x)) / rad(x), 60 times
    s, d = cam.src, cam.dst
    xd, yd = (us.astype(np.float64) - s.cx) / s.fx, (vs.astype(np.float64) - s.cy) / s.fy
    xn, yn = xd.copy(), yd.copy()
    for _ in range(60):
        r2 = xn * xn + yn * yn
        rad = ((cam.k3 * r2 + cam.k2) * r2 + cam.k1) * r2 + 1.0
        dx = cam.p1 * 2 * xn * yn + cam.p2 * (r2 + 2 * xn * xn)
        dy = cam.p1 * (r2 + 2 * yn * yn) + cam.p2 * 2 * xn * yn
        xn, yn = (xd - dx) / rad, (yd - dy) / rad
    R = np.array(list(cam.r), dtype=np.float64).reshape(3, 3)
    p = np.einsum("ij,jhw->ihw", R, np.stack([xn, yn, np.ones_like(xn)]))
    back_u, back_v = d.fx * p[0] / p[2] + d.cx, d.fy * p[1] / p[2] + d.cy
    back = max(np.abs(back_u - u).max(), np.abs(back_v - v).max())
    print(f"rectify coordinates: max |fp32 - float64| = {err:.3e} px (bound {COORD_TOL:.3e}), round trip {back:.3e} px (bound {ROUND_TRIP_TOL:.3e})")
    assert err <= COORD_TOL and back <= ROUND_TRIP_TOL
    assert inside.mean() > 0.9 and not inside.all()                   # the case shows image and border both


@pytest.mark.parametrize("channels", CHANNELS)
def test_integer_bilinear_against_float64(pkg, channels):
    """Every output within one grey level of float64 bilinear sampling at (qx / 32, qy / 32) with a constant border."""
    from unina_yolo_dla_amd import rectify
    c = next(x for x in rc.named_cases(channels) if x["name"].startswith("distorted"))
    out = channels_of(twin(c)).astype(np.float64)
    img = channels_of(c["img"]).astype(np.float64)
    sh, sw = img.shape[:2]
    _, _, inside, qx, qy = rectify.rectify_source_numpy(c["cam"], c["dst_hw"], (sh, sw))
    pad = np.full((sh + 2, sw + 2, img.shape[2]), float(c["border"]))
    pad[1:-1, 1:-1] = img
    x, y = qx / 32.0, qy / 32.0
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    want = ((1 - fx) * (1 - fy) * pad[y0 + 1, x0 + 1] + fx * (1 - fy) * pad[y0 + 1, x0 + 2] + (1 - fx) * fy * pad[y0 + 2, x0 + 1]
            + fx * fy * pad[y0 + 2, x0 + 2])
    want[~inside] = c["border"]
    assert np.abs(out - want).max() < 1.0
    assert (x0 == -1).any() or (y0 == -1).any() or (x0 == sw - 1).any() or (y0 == sh - 1).any()      # border taps took part


def test_pixels_behind_the_raw_camera_are_border(pkg):
    from unina_yolo_dla_amd import rectify
    c = next(x for x in rc.named_cases(1) if x["name"].startswith("behind"))
    cam, (dh, dw) = c["cam"], c["dst_hw"]
    _, _, inside, _, _ = rectify.rectify_source_numpy(cam, c["dst_hw"], c["img"].shape[:2])
    r = np.array(list(cam.r), dtype=np.float32)
    x = ((np.arange(dw, dtype=np.float32) - np.float32(cam.dst.cx)) / np.float32(cam.dst.fx))[None, :]
    y = ((np.arange(dh, dtype=np.float32) - np.float32(cam.dst.cy)) / np.float32(cam.dst.fy))[:, None]
    W = (r[2] * x + r[5] * y) + r[8]
    out = twin(c)
    assert (W <= 0).any() and inside.any() and not (inside & (W <= 0)).any()
    assert (out[W <= 0] == c["border"]).all() and (out[inside] != c["border"]).any()


def test_case_list_contains_what_the_gpu_tests_rely_on(pkg):
    """x0 = -1 and x0 = src_w - 1 with weight on the outside tap; ax = 0 at x0 = src_w - 1; a calibration with nothing inside."""
    from unina_yolo_dla_amd import rectify
    got = {}
    for c in rc.named_cases(1):
        sh, sw = c["img"].shape[:2]
        _, _, inside, qx, qy = rectify.rectify_source_numpy(c["cam"], c["dst_hw"], (sh, sw))
        got[c["name"][:-3]] = (inside, qx >> 5, qx & 31, qy >> 5, qy & 31, sw, sh)
    inside, x0, ax, y0, ay, sw, sh = got["half_left"]
    assert (x0[:, 0] == -1).all() and (ax[:, 0] == 16).all() and inside[:, 0].all()
    inside, x0, ax, y0, ay, sw, sh = got["half_right"]
    assert (x0[:, -1] == sw - 1).all() and (ax[:, -1] == 16).all() and (y0[-1] == sh - 1).all() and (ay[-1] == 16).all() and inside.all()
    inside, x0, ax, y0, ay, sw, sh = got["identity"]
    assert (x0[:, -1] == sw - 1).all() and (ax[:, -1] == 0).all() and (y0[-1] == sh - 1).all() and (ay[-1] == 0).all() and inside.all()
    assert not got["all_outside"][0].any()
    assert (twin(next(c for c in rc.named_cases(3) if c["name"].startswith("all_outside"))) == 201).all()


# ---------------------------------------------------------------- csrc/rectify_map.h on the host
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("rectify_map_host")
    return hostprog.build_pair(d, "rectify_map_host.cpp"), d


@pytest.mark.parametrize("channels", CHANNELS)
def test_host_program_returns_the_twins_bytes(pkg, drivers, channels):
    """Whole images through csrc/rectify_map.h in exactly sized heap buffers, plain and sanitised: every case at most 128 pixels
    wide, the structural sizes included."""
    cases = [c for c in rc.named_cases(channels) + rc.structural_cases(channels) if max(c["img"].shape[1], c["dst_hw"][1]) <= 128]
    got = hostprog.run_pair(*drivers, b"".join(rc.to_payload(c) for c in cases), dtype=np.uint8)      # one run: the cases back to back
    at, n = 0, 0
    for c in cases:
        want = twin(c).reshape(-1)
        mine = got[at:at + want.size]
        assert mine.size == want.size, c["name"]
        bad = np.flatnonzero(mine != want)
        assert bad.size == 0, (c["name"], bad.size, int(bad[0]))
        at, n = at + want.size, n + 1
    assert at == got.size
    assert n >= 60


# ---------------------------------------------------------------- the ABI
def test_header_is_c99_and_layouts_match_the_ctypes_mirror(pkg, tmp_path):
    from unina_yolo_dla_amd import engine
    hostprog.assert_header_is_c99()
    J, I, K = engine.RectifyJob, engine.Image, engine.RectifyCam
    assert (C.sizeof(K), C.sizeof(I), C.sizeof(J)) == (88, 24, 144)
    assert (K.k1.offset, K.r.offset, K.dst.offset, I.channels.offset, I.data.offset) == (16, 36, 72, 12, 16)
    assert (J.cam.offset, J.src.offset, J.dst.offset, J.border.offset) == (0, 88, 112, 136)
    assert (engine.RECTIFY_MAX_IMAGES, engine.RECTIFY_MAX_DIM) == (4, 16384)
    hostprog.compile_c99(tmp_path, 'typedef char cam88[(sizeof(unina_rectify_cam) == 88) ? 1 : -1];\n'
                                   'typedef char k16[(offsetof(unina_rectify_cam, k1) == 16 && offsetof(unina_rectify_cam, r) == 36) ? 1 : -1];\n'
                                   'typedef char dst72[(offsetof(unina_rectify_cam, dst) == 72) ? 1 : -1];\n'
                                   'typedef char img24[(sizeof(unina_image) == 24 && offsetof(unina_image, data) == 16) ? 1 : -1];\n'
                                   'typedef char ch12[(offsetof(unina_image, channels) == 12) ? 1 : -1];\n'
                                   'typedef char job144[(sizeof(unina_rectify_job) == 144) ? 1 : -1];\n'
                                   'typedef char src88[(offsetof(unina_rectify_job, src) == 88 && offsetof(unina_rectify_job, dst) == 112) ? 1 : -1];\n'
                                   'typedef char b136[(offsetof(unina_rectify_job, cam) == 0 && offsetof(unina_rectify_job, border) == 136) ? 1 : -1];\n'
                                   'typedef char lim[(UNINA_RECTIFY_MAX_IMAGES == 4 && UNINA_RECTIFY_MAX_DIM == 16384) ? 1 : -1];\n'
                                   'int use(const uint8_t *raw, uint8_t *out) {\n'
                                   '  unina_rectify_job j = {{{700.0f, 700.0f, 639.5f, 359.5f}, -0.3f, 0.1f, 0.0f, 0.0f, 0.0f,\n'
                                   '                         {1, 0, 0, 0, 1, 0, 0, 0, 1}, {650.0f, 650.0f, 639.5f, 359.5f}},\n'
                                   '                        {1280, 720, 1280, 1, 0}, {1280, 720, 1280, 1, 0}, 0};\n'
                                   '  j.src.data = raw; j.dst.data = out;\n'
                                   '  return unina_rectify_async(&j, 1, 0);\n}\n')


def test_every_bad_argument_is_refused_before_any_hip_call(pkg):
    """UNINA_ERR_ARG (4) for each refusal the header lists, in a process that has no device: a HIP call in front of the checks
    would answer 3 (UNINA_ERR_HIP) instead. The pointers are never dereferenced by a refused call."""
    from unina_yolo_dla_amd import build, engine, rectify
    build.build_native()
    L = engine.load_library()
    nan, inf = float("nan"), float("inf")
    SRC, DST = 0x30001, 0x50003

    def job(**kw):
        cam = dict(src=[100.0, 101.0, 48.3, 29.8], dist=list(rc.DIST), r=list(np.eye(3).reshape(-1)), dst=[88.0, 87.0, 41.2, 29.4])
        src = dict(width=97, height=61, pitch=97 * 3, channels=3, data=SRC)
        dst = dict(width=83, height=59, pitch=83 * 3 + 2, channels=3, data=DST)
        border = kw.pop("border", 7)
        for k, v in kw.items():
            group, field = k.split("_", 1)
            target = {"src": src, "dst": dst, "cam": cam}[group]
            if group == "cam":
                name, index = field.rsplit("_", 1)
                target[name][int(index)] = v
            else:
                target[field] = v
        j = engine.RectifyJob()
        j.cam = rectify.make_rectify_cam(cam["src"], cam["dist"], cam["r"], cam["dst"])
        j.src, j.dst, j.border = engine.Image(**src), engine.Image(**dst), border
        return j

    def call(jobs, n=None):
        arr = (engine.RectifyJob * len(jobs))(*jobs)
        return L.unina_rectify_async(arr, len(jobs) if n is None else n, None)

    good = job()
    assert L.unina_rectify_async(None, 1, None) == 4
    for n in (0, -1, 5, 1 << 20):
        assert call([good] * 4, n) == 4, n
    bad = [dict(src_data=None), dict(dst_data=None), dict(dst_data=SRC),
           *[{f"{g}_{f}": v} for g in ("src", "dst") for f in ("width", "height") for v in (0, -3, 16385)],
           *[{f"{g}_channels": v} for g in ("src", "dst") for v in (0, 2, 5, -1, 1, 4)],          # 1 and 4 differ from the other image's 3
           dict(src_channels=2, dst_channels=2), dict(src_pitch=97 * 3 - 1), dict(dst_pitch=83 * 3 - 1), dict(src_pitch=0), dict(dst_pitch=-400),
           dict(border=-1), dict(border=256),
           *[{f"cam_{name}_{i}": v} for name, n in (("src", 4), ("dist", 5), ("r", 9), ("dst", 4)) for i in range(n) for v in (nan, inf, -inf)],
           *[{f"cam_{name}_{i}": v} for name in ("src", "dst") for i in (0, 1) for v in (0.0, -1.0)]]
    for kw in bad:
        assert call([job(**kw)]) == 4, kw
        assert call([good, good, job(**kw)]) == 4, kw                      # wherever it stands in the call
    assert len(bad) > 100
    import torch
    if not torch.cuda.is_available():
        # good calls reach HIP, which has no device here: the checks above sit in front of it
        assert call([good]) == 3 and call([good] * 4) == 3
        assert call([job(src_width=16384, src_pitch=16384 * 3, dst_height=16384, border=255)]) == 3
        assert call([job(src_channels=1, dst_channels=1, src_pitch=97, dst_pitch=83, border=0)]) == 3
        assert call([job(cam_src_2=-5.0, cam_dst_3=-7.5, cam_r_0=-1.0)]) == 3                      # a principal point may be anywhere


def test_twin_refuses_what_the_entry_point_refuses(pkg):
    from unina_yolo_dla_amd import rectify
    img = np.zeros((4, 5, 2), dtype=np.uint8)
    cam = rectify.make_rectify_cam(rc.SMALL_PIN)
    for bad in (lambda: rectify.rectify_numpy(img, cam, (4, 5)), lambda: rectify.rectify_numpy(img[..., 0], cam, (4, 5), border=256),
                lambda: rectify.rectify_numpy(img[..., 0], cam, (0, 5)), lambda: rectify.rectify_numpy(img[..., 0].astype(np.float32), cam, (4, 5)),
                lambda: rectify.rectify_source_numpy(cam, (4, 16385), (4, 5)), lambda: rectify.make_rectify_cam(rc.SMALL_PIN, dist=(0.1, 0.2))):
        with pytest.raises(ValueError):
            bad()
