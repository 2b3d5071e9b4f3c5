"""Shared by tests/test_stem_sources_cpu.py, tests/test_gpu_stem_sources.py and the latter's child process
(tests/stem_sources_child.py): camera frames of every unina_pixel_format into the stem at network sizes where the stem's tiles are
partial and the network is not square. Pure numpy: what the engine is given (`device_frame` / `call`, GPU side only) and what the
numpy twins say the network then sees (`reference_tensors`).

The tiled stem kernel owns 2 output rows x 64 output columns per workgroup (a footprint of 5 x 132 input pixels from column
2 * tx0 - 4). SIZES, graph (A), seed-7 weights:

  16 x 16     stem output  8 x 8     every map smaller than every tile; the footprint is mostly padding on all four sides
  80 x 112                40 x 56    one partial tile column
  96 x 160                48 x 80    one whole tile, then a 16-column one whose footprint covers input columns 124..255 of 160
  32 x 272                16 x 136   two whole tiles and an 8-column third

in_h is a multiple of 16 (the graph asks for it), so the stem's output height is even and the 2-row tile is never partial in y:
there is no case for that.

Per size, cameras named by the CameraKind that frame_kind (csrc/camera_source.h) must choose for them:
  tap        a frame of the network's size: `wide` (everything 16-byte aligned: the quad loaders' wide loads) and `bytes` (an odd
             pitch, the plane one byte off: their byte loads)
  resize     `down` ((H + 40) x (W + 72): the x and y ratios differ) and `up` (odd both ways, not of the network's aspect)
  letterbox  `wide` (bars above and below), `tall` (bars left and right), `r1` (the network's width, r == 1, an odd remainder:
             top != bottom)
  tiled      one frame, odd both ways, of three tiles: the network's size at an odd origin; one resized with w / W != h / H; the
             network's size ending at the frame's bottom-right corner (Bayer reflects at the FRAME's border there)
"""
from collections import namedtuple

from frame_child import BGGR, BGRA, GBRG, GRBG, NAMES, NV12, RGB, RGBA, RGGB, UYVY, YUYV, frame_rows, make_frame
from nv12_child import nv12_planes

SIZES = ((16, 16), (80, 112), (96, 160), (32, 272))                      # (H, W) of the network
SIZE_ID = lambda s: f"{s[0]}x{s[1]}"
ALL_FORMATS = (BGRA, NV12, YUYV, UYVY, RGB, RGBA, RGGB, BGGR, GRBG, GBRG)
BOX_FORMATS = (BGRA, NV12, YUYV, GRBG)                                  # letterboxed
TILED_FORMATS = (BGRA, NV12, UYVY, RGGB)
# The 64-channel stem (stem_*_kernel<., 64>): Graph(base_channels=64) at 32 x 80 (one partial tile column), the tap and resize
# cameras of one 4:2:2 and one Bayer format. The seed-7 weights of that graph give the CPU oracle confidences of ~0.04 on every
# cell: there is no sensible threshold, so these cases compare buffers, not record lists.
B64_SIZE, B64_FORMATS = (32, 80), (UYVY, BGGR)
GEOMETRIES = ("tap", "resize", "letterbox", "tiled")
PAD = 114.0
IOU, Q, MERGE = 0.45, 0.1, 0.45
MAXD = 1024
TILE_W, TILE_H = 64, 2                                                   # the stem tile, output pixels (csrc/stem_pool.hip)

# camera_source.h: CameraKind
TENSOR, BGRA_TAP, BGRA_RESIZE, NV12_TAP, NV12_RESIZE, BGRA_LETTERBOX, NV12_LETTERBOX, FRAME_TAP, FRAME_RESIZE, FRAME_LETTERBOX = range(10)

# The confidence threshold per network size comes from the CPU oracle, not from an engine: tests/test_stem_sources_cpu.py runs
# oracle.forward + oracle.postprocess (fp32) on every reference tensor below and requires, at CONF[size], between 1 and 1024
# records on each and a strongest record at least 0.03 above the threshold (ten times what an fp16 engine's scores differ from the
# oracle's by). At 0.3 the oracle keeps 19 to 126 records per tensor of the three larger sizes, the strongest of the weakest tensor
# at 0.73. The 16 x 16 network has 21 cells in all and no record above 0.43; its weakest tensor's strongest record has 0.136, so
# its lists are compared at 0.05: 5 to 9 records each, short but not empty.
CONF = {(16, 16): 0.05, (80, 112): 0.3, (96, 160): 0.3, (32, 272): 0.3, B64_SIZE: 0.3}

Case = namedtuple("Case", "size geometry camera fmt seed h w misaligned tiles")


def cameras(size):
    """{geometry: [(camera name, frame height, frame width, misaligned)]} of one network size."""
    H, W = size
    up = {(16, 16): (7, 9), (80, 112): (45, 77), (96, 160): (53, 77), (32, 272): (17, 101), B64_SIZE: (17, 29)}[size]
    return {
        "tap": [("wide", H, W, False), ("bytes", H, W, True)],
        "resize": [("down", H + 40, W + 72, False), ("up", up[0], up[1], False)],
        "letterbox": [("wide", H + 10, 2 * W + 10, False), ("tall", 2 * H + 5, W // 2 + 3, True), ("r1", H - (5 if H < 32 else 13), W, False)],
        "tiled": [("odd", H + 7, W + 9, False)],
    }


def tiles_of(size):
    """The three tiles (x, y, w, h) of the (H + 7) x (W + 9) frame; the last one ends at the frame's corner."""
    H, W = size
    return ((3, 1, W, H), (2, 0, W + 6, H // 2 + 3), (9, 7, W, H))


def cases(size, geometry=None, formats=None):
    out = []
    si = (SIZES + (B64_SIZE,)).index(size)
    for gi, g in enumerate(GEOMETRIES):
        if geometry is not None and g != geometry:
            continue
        fmts = {"tap": ALL_FORMATS, "resize": ALL_FORMATS, "letterbox": BOX_FORMATS, "tiled": TILED_FORMATS}[g]
        for ci, (name, h, w, mis) in enumerate(cameras(size)[g]):
            for fmt in fmts:
                if formats is None or fmt in formats:
                    out.append(Case(size, g, name, fmt, 300 + 40 * si + 4 * gi + ci, h, w, mis, tiles_of(size) if g == "tiled" else None))
    return out


def case_id(c):
    return f"{SIZE_ID(c.size)}-{c.geometry}-{c.camera}-{NAMES[c.fmt]}"


def expected_kinds(c):
    """The CameraKind of each launch of the case (one per tile of a tiled call)."""
    tap = BGRA_TAP if c.fmt == BGRA else NV12_TAP if c.fmt == NV12 else FRAME_TAP
    if c.geometry == "tap":
        return [tap]
    if c.geometry == "resize":
        return [tap + 1]
    if c.geometry == "letterbox":
        return [BGRA_LETTERBOX if c.fmt == BGRA else NV12_LETTERBOX if c.fmt == NV12 else FRAME_LETTERBOX]
    return [tap, tap + 1, tap]


def planes(twin, c):
    """What the numpy twin takes as `planes` for the case's frame: the bytes frame_child.make_frame puts on the device (an NV12
    frame's padding bytes come from the same generator as its pixels, so the pitches are make_frame's)."""
    if c.fmt == NV12:
        yp, uvp = (c.w + 1, 2 * ((c.w + 1) // 2) + 1) if c.misaligned else (c.w, 2 * ((c.w + 1) // 2))
        y, uv = nv12_planes(c.seed, c.h, c.w, yp, uvp)
        return y[:, :c.w], uv[:, :2 * ((c.w + 1) // 2)]
    return frame_rows(twin, c.fmt, c.seed, c.h, c.w)[1]


def reference_tensors(twin, c, p=None):
    """The fp32 [3, H, W] tensors the network must see in the case's call: one, or one per tile."""
    p = planes(twin, c) if p is None else p
    if c.geometry == "letterbox":
        return [twin.letterbox_frame_to_tensor(c.fmt, p, c.size, PAD, size=(c.w, c.h))]
    if c.geometry == "tiled":
        return [twin.frame_to_tensor(c.fmt, p, c.size, origin=(x, y), region=(w, h)) for x, y, w, h in c.tiles]
    return [twin.frame_to_tensor(c.fmt, p, c.size, region=(c.w, c.h))]


def partial_tile(size):
    """(stem output columns in the last tile column, input columns of its footprint that lie beyond W)."""
    H, W = size
    wo = W // 2
    tx0 = (wo - 1) // TILE_W * TILE_W
    return wo - tx0, max(0, 2 * tx0 - 4 + 2 * TILE_W + 4 - W)


# ---------------------------------------------------------------------------------------------- GPU side

def device_frame(torch, engine, twin, c):
    """frame_child.make_frame of the case: dict(fmt, w, h, pitch, planes, d, frame, ...)."""
    return make_frame(torch, engine, twin, c.fmt, c.seed, c.h, c.w, c.misaligned)


def call(e, c, f, out=None, map_boxes=False, tiles=None, conf=None):
    """The case's camera call through the frame-descriptor methods (tests/test_gpu_frame_formats.py holds them equal to the
    format-named ones). f: device_frame(c). out: asynchronous into that tensor."""
    conf = CONF[c.size] if conf is None else conf
    if c.geometry == "letterbox":
        return e.infer_letterbox_frame(f["frame"], None, conf, IOU, Q, PAD, map_boxes, out=out)
    if c.geometry == "tiled":
        return e.infer_tiled_frame(f["frame"], list(c.tiles if tiles is None else tiles), None, conf, IOU, Q, MERGE, out=out)
    return e.infer_frame(f["frame"], None, conf, IOU, Q, out=out)


def child_cases():
    """A third of the cases, every size, geometry and format among them: what the one-thread-per-pixel child repeats."""
    out = []
    for size in SIZES:
        cs = cases(size)
        out += [c for i, c in enumerate(cs) if i % 3 == SIZES.index(size) % 3]
    return out


def b64_cases():
    return [c for c in cases(B64_SIZE, formats=B64_FORMATS) if c.geometry in ("tap", "resize")]


SEQUENCE_SIZE = (96, 160)


def sequence_cases():
    """The camera calls of `one engine, many sources`, in call order: an NV12 tap, a Bayer resize, a YUYV letterbox (bars left and
    right: the box map has an offset), a BGRA tiled call."""
    pick = lambda g, cam, fmt: [c for c in cases(SEQUENCE_SIZE, g, (fmt,)) if c.camera == cam][0]
    return [pick("tap", "wide", NV12), pick("resize", "down", RGGB), pick("letterbox", "tall", YUYV), pick("tiled", "odd", BGRA)]
