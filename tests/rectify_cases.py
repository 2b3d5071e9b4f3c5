"""Inputs shared by tests/test_rectify_cpu.py and tests/test_gpu_rectify.py: raw images, calibrations and the named cases of
unina_rectify_async (include/unina_mi355.h "Rectification"). Pure numpy; nothing here touches the device.

A case is a dict: name, img ([H, W] uint8 for one channel, [H, W, C] otherwise), cam (engine.RectifyCam), dst_hw, border."""
import numpy as np

from unina_yolo_dla_amd import rectify

DIST = (-0.30, 0.10, 1e-3, -5e-4, 0.01)          # k1, k2, p1, p2, k3: a strong barrel with some tangential part
SKEW_AXIS = (0.3, -0.8, 0.52)
SRC_HW, DST_HW = (61, 97), (59, 83)              # 97 x 61 -> 83 x 59
SRC_PIN, DST_PIN = (100.0, 101.0, 48.3, 29.8), (88.0, 87.0, 41.2, 29.4)
SMALL_HW = (23, 31)
SMALL_PIN = (40.0, 41.0, 15.0, 11.0)

# the kernel's tiles (csrc/rectify.hip): 4 rows; 256 pixels of a 1-channel row in groups of 4, 64 pixels of a 3- or 4-channel row
TILE_ROWS, GROUP, TILE_W1, TILE_WN = 4, 4, 256, 64
WIDTHS = (1, 3, 4, 5, 63, 64, 65, 257) + (2, 7, 8, 9, 127, 128, 129, 255, 256, 259, 260, 261)
HEIGHTS = (1, 15, 16, 17) + (3, 4, 5)


rotation = rectify.rotation


def image(hw, channels, seed):
    """Noise with smooth large-scale structure, so that both a one-pixel and a one-level error show."""
    h, w = hw
    r = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    planes = []
    for c in range(channels):
        wave = 90.0 + 60.0 * np.sin(0.37 * xx + 0.9 * c) * np.cos(0.23 * yy - 0.4 * c)
        planes.append(np.clip(wave + r.randint(-70, 71, (h, w)), 0, 255).astype(np.uint8))
    return planes[0] if channels == 1 else np.stack(planes, axis=2)


def case(name, channels, src_hw, cam, dst_hw, border=0, seed=3, img=None):
    return {"name": f"{name}_c{channels}", "img": image(src_hw, channels, seed) if img is None else img, "cam": cam,
            "dst_hw": tuple(dst_hw), "border": border}


def distorted_cam(src_hw=SRC_HW, dst_hw=DST_HW):
    """The distorted, rotated calibration (DIST, 2 degrees about SKEW_AXIS), rescaled to the two sizes."""
    (sh, sw), (dh, dw) = src_hw, dst_hw
    if (src_hw, dst_hw) == (SRC_HW, DST_HW):
        src, dst = SRC_PIN, DST_PIN
    else:
        f = 1.03 * max(sw, sh, 8)
        g = 0.9 * f * max(dw, dh, 8) / max(sw, sh, 8)
        src, dst = (f, 1.01 * f, (sw - 1) / 2 + 0.3, (sh - 1) / 2 - 0.2), (g, 0.99 * g, (dw - 1) / 2 - 0.3, (dh - 1) / 2 + 0.4)
    return rectify.make_rectify_cam(src, DIST, rotation(SKEW_AXIS, 2.0), dst)


def shifted_cam(dx, dy, pin=SMALL_PIN):
    """No distortion, no rotation, dst.cx = src.cx + dx, dst.cy = src.cy + dy: the image moved by (dx, dy)."""
    return rectify.make_rectify_cam(pin, dst=(pin[0], pin[1], pin[2] + dx, pin[3] + dy))


def named_cases(channels):
    """The cases the CPU tests pin on the twin, for one channel count."""
    h, w = SMALL_HW
    fx, fy, cx, cy = SMALL_PIN
    out = [
        case("identity", channels, SMALL_HW, shifted_cam(0, 0), SMALL_HW, border=77),       # ax = 0 at x0 = src_w - 1, ay = 0 at y0 = src_h - 1
        case("shift_b0", channels, SMALL_HW, shifted_cam(3, -2), SMALL_HW, border=0),
        case("shift_b114", channels, SMALL_HW, shifted_cam(3, -2), SMALL_HW, border=114),
        case("half_left", channels, SMALL_HW, shifted_cam(0.5, 0), SMALL_HW, border=114),    # u = 0: x0 = -1 with weight 16
        case("half_right", channels, SMALL_HW, shifted_cam(-0.5, -0.5), SMALL_HW, border=200),   # last column and row: x0 = src_w - 1, ax = 16
        case("rot_y3", channels, SMALL_HW, rectify.make_rectify_cam(SMALL_PIN, r=rotation((0, 1, 0), 3.0)), SMALL_HW, border=9),
        case("distorted", channels, SRC_HW, distorted_cam(), DST_HW, border=114),
        case("behind", channels, SRC_HW, behind_cam(), DST_HW, border=33),
        case("all_outside", channels, SMALL_HW, shifted_cam(1e5, 0), SMALL_HW, border=201),
        case("scale_up", channels, SMALL_HW, rectify.make_rectify_cam(SMALL_PIN, DIST, None, (2 * fx, 2 * fy, 2 * cx + 0.5, 2 * cy + 0.5)),
             (2 * h, 2 * w), border=5),
        case("scale_down", channels, SRC_HW, rectify.make_rectify_cam(SRC_PIN, DIST, None, (SRC_PIN[0] / 2, SRC_PIN[1] / 2, 23.9, 14.7)),
             (SRC_HW[0] // 2, SRC_HW[1] // 2), border=250),
    ]
    return out


def behind_cam():
    """120 degrees about y: the rectified camera looks mostly away from the raw one. W <= 0 left of x = tan(30 deg); the raw focal
    length is short enough for some of the rest to land on the raw image."""
    return rectify.make_rectify_cam((12.0, 12.0, 48.0, 30.0), r=rotation((0, 1, 0), 120.0), dst=(40.0, 40.0, 41.0, 29.0))


def structural_cases(channels):
    """Destination widths x heights on and beside every edge of the kernel's tiling: the 4-row tile, the 4-pixel group and the
    256-pixel tile of a 1-channel row, the 64-pixel tile of the others; the raw image is 3 columns and 2 rows larger."""
    out = []
    for w in WIDTHS:
        for h in HEIGHTS:
            src_hw = (h + 2, w + 3)
            out.append(case(f"size_{w}x{h}", channels, src_hw, distorted_cam(src_hw, (h, w)), (h, w), border=(w * 7 + h) % 256, seed=w + h))
    return out


def to_payload(c):
    """The case file of tests/rectify_map_host.cpp."""
    img = c["img"]
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    head = np.array([0x52454331, w, h, ch, c["dst_hw"][1], c["dst_hw"][0], c["border"]], dtype=np.int32)
    return head.tobytes() + bytes(c["cam"]) + np.ascontiguousarray(img).tobytes()


def twin(c):
    return rectify.rectify_numpy(c["img"], c["cam"], c["dst_hw"], c["border"])
