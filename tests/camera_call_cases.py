"""Shared by tests/test_camera_calls_cpu.py and tests/test_gpu_camera_calls.py: the camera calls both run -- plain, letterboxed and
tiled, on a BGRA, an NV12 and a YUYV frame (a format only the unina_frame calls take) of the cameras of tests/letterbox_child.py --
as the engine is called (`call`) and as the numpy twins describe what the network then sees (`reference_tensors`).

The thresholds are letterbox_child's. Its CONF was chosen for the letterboxed BGRA / NV12 frames; test_camera_calls_cpu.py repeats
that choice for the calls here: the CPU oracle alone keeps at least one record at CONF on every tensor below."""
from letterbox_child import CONF, IOU, NET, PAD, Q, visible
from nv12_child import upload

BGRA, NV12, YUYV = 0, 1, 4                      # include/unina_mi355.h: unina_pixel_format
FORMATS = ("bgra", "nv12", "yuyv")
# two tiles of 128x72_down: one that is resized, one of the network's size (the tap path) at an odd origin (NV12 and YUYV send
# the origin to the kernel: it enters the chroma index)
TILES = ((0, 0, 80, 72), (63, 5, 64, 64))
# (geometry, camera): 128x72_down takes the resize and the letterbox kinds, 64x64_identity the tap kind
CASES = (("plain", "128x72_down"), ("plain", "64x64_identity"), ("letterbox", "128x72_down"), ("tiled", "128x72_down"))


def twin_planes(twin, c, fmt):
    """(unina_pixel_format, what camera.frame_to_tensor takes as `planes`) of host camera `c` (letterbox_child.host_camera)."""
    bgra, y, uv = visible(c)
    if fmt == "bgra":
        return BGRA, bgra
    if fmt == "nv12":
        return NV12, (y, uv)
    return YUYV, twin.nv12_to_yuv422(y, uv, "yuyv")


def reference_tensors(twin, c, fmt, geometry):
    """The fp32 [3, NET, NET] tensors the network sees in the call: one, or one per tile."""
    f, planes = twin_planes(twin, c, fmt)
    if geometry == "plain":
        return [twin.frame_to_tensor(f, planes, (NET, NET))]
    if geometry == "letterbox":
        return [twin.letterbox_frame_to_tensor(f, planes, (NET, NET), PAD)]
    return [twin.frame_to_tensor(f, planes, (NET, NET), origin=(x, y), region=(w, h)) for x, y, w, h in TILES]


def add_frames(torch, engine, twin, c):
    """Adds to device camera `c` (letterbox_child.device_camera) its YUYV twin and an engine.Frame per format: c["frame_<fmt>"]."""
    rows = twin_planes(twin, c, "yuyv")[1]
    c["d_yuyv"] = upload(torch, rows)
    c["frame_bgra"] = engine.Frame.from_tensors(BGRA, c["w"], c["h"], c["d_bgra"], c["pitch"])
    c["frame_nv12"] = engine.Frame.from_tensors(NV12, c["w"], c["h"], c["d_y"], c["y_pitch"], c["d_uv"], c["uv_pitch"])
    c["frame_yuyv"] = engine.Frame.from_tensors(YUYV, c["w"], c["h"], c["d_yuyv"], rows.shape[1])
    return c


def call(e, c, fmt, geometry, out=None, map_boxes=True, conf=CONF):
    """The call through the Engine method of its format: BGRA and NV12 through the format-named symbols, YUYV through the
    unina_frame ones. out: asynchronous into that tensor (infer_bgra / infer_nv12 have no such form: infer_frame then)."""
    bgra = (c["d_bgra"], c["w"], c["h"], c["pitch"])
    nv12 = (c["d_y"], c["d_uv"], c["w"], c["h"], c["y_pitch"], c["uv_pitch"])
    if geometry == "plain":
        if fmt == "bgra" and out is None:
            return e.infer_bgra(*bgra, None, conf, IOU, Q)
        if fmt == "nv12" and out is None:
            return e.infer_nv12(*nv12, None, conf, IOU, Q)
        return e.infer_frame(c["frame_" + fmt], None, conf, IOU, Q, out=out)
    if geometry == "letterbox":
        if fmt == "bgra":
            return e.infer_letterbox_bgra(*bgra, None, conf, IOU, Q, PAD, map_boxes, out=out)
        if fmt == "nv12":
            return e.infer_letterbox_nv12(*nv12, None, conf, IOU, Q, PAD, map_boxes, out=out)
        return e.infer_letterbox_frame(c["frame_yuyv"], None, conf, IOU, Q, PAD, map_boxes, out=out)
    if fmt == "bgra":
        return e.infer_tiled_bgra(*bgra, TILES, None, conf, IOU, Q, out=out)
    if fmt == "nv12":
        return e.infer_tiled_nv12(*nv12, TILES, None, conf, IOU, Q, out=out)
    return e.infer_tiled_frame(c["frame_yuyv"], TILES, None, conf, IOU, Q, out=out)
