"""Host-side mirror of the reference's engine interface, over the C ABI (include/unina_mi355.h).

``Engine`` plays the role of the C++ ``TensorRTEngine`` wrapper (perception_node.cpp:223-351: load / bind
tensor addresses / enqueueV3 / getInputDimensions) plus the fused per-frame path (perception_node.cpp:612-656).
All compute happens inside libunina_mi355.so (hand-written HIP); torch is used only to own device memory and
streams. There is NO fallback: if the shared library is missing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
import tempfile
from typing import Dict, List, Optional

import numpy as np

from . import export as _export
from .graph import Graph, OUTPUT_NAMES

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UNINA_LIB") or os.path.join(_PKG, "libunina_mi355.so")   # (UNINA_LIB: another build of the library, for same-box A/B runs)
MAX_DETECTIONS = 1024

DET_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("confidence", "<f4"),
                      ("class_id", "<i4"), ("valid", "<i4"), ("_pad", "<i4")])
assert DET_DTYPE.itemsize == 32

ERRORS = {1: "IO", 2: "FORMAT", 3: "HIP", 4: "ARG", 5: "STATE", 6: "UNSUPPORTED"}


class OpInfo(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("kernel", C.c_char * 64), ("kind", C.c_int), ("m", C.c_int), ("n", C.c_int),
                ("k", C.c_int), ("flops", C.c_double), ("bytes", C.c_double), ("grid", C.c_int), ("block", C.c_int)]


class NormParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("mean_r", "mean_g", "mean_b", "std_r", "std_g", "std_b")]


class Tile(C.Structure):
    """unina_tile: a region of the camera frame, pixels."""
    _fields_ = [(n, C.c_int) for n in ("x", "y", "w", "h")]


class Letterbox(C.Structure):
    """unina_letterbox: the inner rectangle of a letterboxed frame in the network input."""
    _fields_ = [(n, C.c_int) for n in ("new_w", "new_h", "left", "top")]


# unina_pixel_format (include/unina_mi355.h): 0..3 are GpuBufferPtr.msg's codes
FMT_BGRA, FMT_NV12, FMT_RGB, FMT_RGBA, FMT_YUYV, FMT_UYVY, FMT_BAYER_RGGB, FMT_BAYER_BGGR, FMT_BAYER_GRBG, FMT_BAYER_GBRG = range(10)


class Frame(C.Structure):
    """unina_frame: a camera frame of any unina_pixel_format on the device. plane[1] / pitch[1]: the NV12 chroma plane."""
    _fields_ = [("format", C.c_int), ("width", C.c_int), ("height", C.c_int), ("plane", C.c_void_p * 2), ("pitch", C.c_int * 2)]

    @classmethod
    def from_tensors(cls, fmt: int, width: int, height: int, plane, pitch: int, uv=None, uv_pitch: int = 0) -> "Frame":
        """From uint8 CUDA tensors (or raw device addresses). The tensors must outlive the calls the frame is handed to."""
        f = cls(int(fmt), int(width), int(height))
        f.plane[0], f.plane[1] = _addr(plane), _addr(uv)
        f.pitch[0], f.pitch[1] = int(pitch), int(uv_pitch)
        return f


EVAL_SMALL, EVAL_CONFORMAL, EVAL_AP = 1, 2, 4   # include/unina_mi355.h UNINA_EVAL_*
EVAL_MAX_LABELS = 256
EVAL_MAX_CLASSES = 256
EVAL_ROW_DTYPE = np.dtype([("confidence", "<f4"), ("class_id", "<i4"), ("tp_mask", "<u4")])   # unina_eval_row


class EvalParams(C.Structure):
    """unina_eval_params."""
    _fields_ = [("sx", C.c_float), ("sy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("width", C.c_int), ("height", C.c_int),
                ("imgsz", C.c_int), ("size_threshold", C.c_double), ("iou_threshold", C.c_double)]


class EvalResult(C.Structure):
    """unina_eval_result."""
    _fields_ = [("tp", C.c_longlong), ("fp", C.c_longlong), ("fn", C.c_longlong), ("n_scores", C.c_ulonglong),
                ("n_rows", C.c_ulonglong), ("overflow", C.c_int), ("guard_intact", C.c_int),
                ("label_counts", C.c_longlong * EVAL_MAX_CLASSES)]


DEPTH_F32, DEPTH_U16 = 0, 1   # include/unina_mi355.h UNINA_DEPTH_*
CONE3D_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("u", "<f4"), ("v", "<f4"), ("n_valid", "<i4"),
                         ("n_samples", "<i4"), ("valid", "<i4")])   # unina_cone3d
assert CONE3D_DTYPE.itemsize == 32


class Depth(C.Structure):
    """unina_depth: a depth plane on the device; pitch in bytes, unit: raw -> metres."""
    _fields_ = [("format", C.c_int), ("width", C.c_int), ("height", C.c_int), ("pitch", C.c_int), ("plane", C.c_void_p),
                ("unit", C.c_float)]


class Pinhole(C.Structure):
    """unina_pinhole: intrinsics of the rectified image, in depth-map pixels."""
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy")]


class LocateParams(C.Structure):
    """unina_locate_params."""
    _fields_ = [("sx", C.c_float), ("sy", C.c_float), ("shrink", C.c_float), ("min_depth", C.c_float), ("max_depth", C.c_float),
                ("max_side", C.c_int), ("min_valid", C.c_int)]


STEREO_MAX_DISPARITIES, STEREO_MAX_SIDE = 1024, 64   # include/unina_mi355.h UNINA_STEREO_*
STEREO_MATCH_DTYPE = np.dtype([("disparity", "<f4"), ("d_best", "<i4"), ("cost_best", "<u4"), ("cost_second", "<u4")])   # unina_stereo_match
assert STEREO_MATCH_DTYPE.itemsize == 16


class StereoPair(C.Structure):
    """unina_stereo_pair: two rectified 8-bit luma planes of one size and pitch (bytes per row) on the device."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("pitch", C.c_int), ("left", C.c_void_p), ("right", C.c_void_p)]


class StereoParams(C.Structure):
    """unina_stereo_params."""
    _fields_ = [("sx", C.c_float), ("sy", C.c_float), ("shrink", C.c_float), ("min_depth", C.c_float), ("max_depth", C.c_float),
                ("max_side", C.c_int), ("max_mean_sad", C.c_int), ("uniqueness", C.c_int)]


RECTIFY_MAX_IMAGES, RECTIFY_MAX_DIM = 4, 16384   # include/unina_mi355.h UNINA_RECTIFY_*


class RectifyCam(C.Structure):
    """unina_rectify_cam: raw camera matrix, OpenCV's five distortion coefficients, row-major R (p_rect = R * p_raw), rectified pinhole."""
    _fields_ = [("src", Pinhole), ("k1", C.c_float), ("k2", C.c_float), ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float),
                ("r", C.c_float * 9), ("dst", Pinhole)]


class Image(C.Structure):
    """unina_image: an interleaved 8-bit image of 1, 3 or 4 channels on the device; pitch in bytes."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("pitch", C.c_int), ("channels", C.c_int), ("data", C.c_void_p)]


class RectifyJob(C.Structure):
    """unina_rectify_job."""
    _fields_ = [("cam", RectifyCam), ("src", Image), ("dst", Image), ("border", C.c_int)]


LIDAR_MAX_DIM, LIDAR_MAX_POINTS = 16384, 1 << 22   # include/unina_mi355.h UNINA_LIDAR_*
LIDAR_PIXEL_DTYPE = np.dtype([("u", "<i4"), ("v", "<i4"), ("key", "<u4"), ("projectable", "<i4")])   # unina_lidar_pixel
assert LIDAR_PIXEL_DTYPE.itemsize == 16


class Cloud(C.Structure):
    """unina_cloud: n_points points of `stride` bytes on the device, float32 x, y, z first in each."""
    _fields_ = [("n_points", C.c_int), ("stride", C.c_int), ("points", C.c_void_p)]


class LidarParams(C.Structure):
    """unina_lidar_params."""
    _fields_ = [("sx", C.c_float), ("sy", C.c_float), ("shrink", C.c_float), ("min_depth", C.c_float), ("max_depth", C.c_float),
                ("min_valid", C.c_int)]


DESKEW_MAX_KEYS, TIME_F32_S, TIME_U32_NS = 64, 0, 1   # include/unina_mi355.h UNINA_DESKEW_MAX_KEYS, UNINA_TIME_*
DESKEW_POSE_DTYPE = np.dtype([("t", "<f8"), ("q", "<f8", (4,)), ("p", "<f8", (3,))])                                    # unina_deskew_pose
DESKEW_KEY_DTYPE = np.dtype([(n, "<f4") for n in ("qw", "qx", "qy", "qz", "px", "py", "pz", "t")])                      # unina_deskew_key
DESKEW_HEADER_DTYPE = np.dtype([(n, "<i4") for n in ("n_points", "n_moved", "n_invalid", "n_before", "n_after")] +
                               [("max_shift2_bits", "<u4"), ("reserved", "<i4", (2,))])                                 # unina_deskew_header
assert DESKEW_POSE_DTYPE.itemsize == 64 and DESKEW_KEY_DTYPE.itemsize == 32 and DESKEW_HEADER_DTYPE.itemsize == 32


class PointTimes(C.Structure):
    """unina_point_times: a time per point on the device, `stride` bytes apart, TIME_F32_S or TIME_U32_NS."""
    _fields_ = [("t", C.c_void_p), ("stride", C.c_int), ("format", C.c_int)]


GROUND_MAX_SIDE, GROUND_MAX_REACH = 1024, 4   # include/unina_mi355.h UNINA_GROUND_*
GROUND_HEADER_DTYPE = np.dtype([("n_points", "<i4"), ("n_kept", "<i4"), ("n_label", "<i4", (5,)), ("n_cells_seeded", "<i4")])   # unina_ground_header
assert GROUND_HEADER_DTYPE.itemsize == 32


class GroundParams(C.Structure):
    """unina_ground_params: the grid (metres, level frame), the seed band, the envelope and the label thresholds."""
    _fields_ = [("x_min", C.c_float), ("y_min", C.c_float), ("cell", C.c_float), ("nx", C.c_int), ("ny", C.c_int), ("z_lo", C.c_float),
                ("z_hi", C.c_float), ("rise", C.c_float), ("band", C.c_float), ("max_height", C.c_float), ("reach", C.c_int),
                ("keep_unknown", C.c_int)]


CLUSTER_DTYPE = np.dtype([(n, "<f4") for n in ("x", "y", "z_lo", "z_hi", "x_lo", "x_hi", "y_lo", "y_hi")] +
                         [(n, "<i4") for n in ("n_points", "n_cells", "root", "cone")])             # unina_cluster
CLUSTER_HEADER_DTYPE = np.dtype([(n, "<i4") for n in ("n_points", "n_in_grid", "n_cells", "n_components", "n_cones", "n_written", "n_dropped",
                                                      "reserved")])                                   # unina_cluster_header
assert CLUSTER_DTYPE.itemsize == 48 and CLUSTER_HEADER_DTYPE.itemsize == 32


class ClusterParams(C.Structure):
    """unina_cluster_params: the grid (metres, level frame), the gate, and what the records of a CONE component carry."""
    _fields_ = [("x_min", C.c_float), ("y_min", C.c_float), ("cell", C.c_float), ("nx", C.c_int), ("ny", C.c_int), ("min_points", C.c_int),
                ("max_points", C.c_int), ("min_height", C.c_float), ("max_height", C.c_float), ("max_width", C.c_float),
                ("confidence", C.c_float), ("class_id", C.c_int)]


FUSE_BOTH, FUSE_CAMERA, FUSE_LIDAR = 1, 2, 3   # include/unina_mi355.h UNINA_FUSE_*
FUSE_LINK_DTYPE = np.dtype([("camera", "<i4"), ("lidar", "<i4"), ("d2", "<f4"), ("kind", "<i4")])                       # unina_fuse_link
FUSE_HEADER_DTYPE = np.dtype([(n, "<i4") for n in ("n_camera", "n_lidar", "n_projected", "n_matched", "n_camera_only", "n_lidar_only",
                                                   "n_written", "n_dropped")])                                          # unina_fuse_header
assert FUSE_LINK_DTYPE.itemsize == 16 and FUSE_HEADER_DTYPE.itemsize == 32


class FuseParams(C.Structure):
    """unina_fuse_params: level_to_cam = row-major 3 x 4 [R|t], level frame -> camera optical frame."""
    _fields_ = [("level_to_cam", C.c_float * 12), ("cam", Pinhole), ("sx", C.c_float), ("sy", C.c_float), ("lift", C.c_float),
                ("min_depth", C.c_float), ("max_depth", C.c_float), ("grow", C.c_float), ("pad", C.c_float), ("range_abs", C.c_float),
                ("range_rel", C.c_float)]


COLOUR_BGR, COLOUR_RGB = 0, 1                                                       # include/unina_mi355.h UNINA_COLOUR_*: pixel orders
COLOUR_YELLOW, COLOUR_BLUE, COLOUR_ORANGE, COLOUR_LARGE_ORANGE = 0, 1, 2, 3         # colour indices
COLOUR_WINDOW, COLOUR_SELECTED, COLOUR_DECIDED, COLOUR_LARGE, COLOUR_SIZE_WINDOW = 1, 2, 4, 8, 16   # status bits; best in bits 8..9
COLOUR_MAX_SIDE = 64
COLOUR_DTYPE = np.dtype([("votes", "<i4", (3,))] + [(n, "<i4") for n in ("n_white", "n_black", "n_mask", "n_stripes", "status")])   # unina_colour
COLOUR_HEADER_DTYPE = np.dtype([(n, "<i4") for n in ("n_records", "n_selected", "n_window", "n_decided")] + [("n_class", "<i4", (4,))])   # unina_colour_header
assert COLOUR_DTYPE.itemsize == 32 and COLOUR_HEADER_DTYPE.itemsize == 32


class ColourParams(C.Structure):
    """unina_colour_params: the window, the pixel thresholds, the hue ranges (yellow, blue, orange), the silhouette and the decision."""
    _fields_ = [(n, C.c_float) for n in ("sx", "sy", "shrink", "half_width", "above", "below")] + \
               [("max_side", C.c_int), ("order", C.c_int), ("only_class", C.c_int), ("class_of", C.c_int * 4), ("black_max", C.c_int),
                ("sat_min", C.c_int), ("val_min", C.c_int), ("white_min", C.c_int), ("hue_lo", C.c_int * 3), ("hue_hi", C.c_int * 3),
                ("taper", C.c_int), ("min_pixels", C.c_int), ("min_share", C.c_int), ("max_rival", C.c_int), ("require_stripe", C.c_int)]


POSE_OK, POSE_TOO_FEW, POSE_DEGENERATE = 0, 1, 2                                    # include/unina_mi355.h UNINA_POSE_*: status
POSE_MAX_ITERATIONS = 8
POSE_RESULT_DTYPE = np.dtype([("pose", "<f4", (12,))] + [(n, "<f4") for n in ("c", "s", "tx", "ty")])                     # unina_pose_result
POSE_HEADER_DTYPE = np.dtype([(n, "<i4") for n in ("n_records", "n_usable", "n_landmarks", "n_pairs", "iterations", "status")] +
                             [("max_d2_bits", "<u4"), ("reserved", "<i4")])                                                # unina_pose_header
assert POSE_RESULT_DTYPE.itemsize == 64 and POSE_HEADER_DTYPE.itemsize == 32


class PoseParams(C.Structure):
    """unina_pose_params: inc = row-major 3 x 4 [R|t], the prior pose or the odometry increment in front of d_prev's pose."""
    _fields_ = [("inc", C.c_float * 12), ("gate", C.c_float), ("class_aware", C.c_int), ("min_hits", C.c_int), ("iterations", C.c_int),
                ("min_pairs", C.c_int)]


BOUNDARY_NO_FIRST, BOUNDARY_NO_NEXT, BOUNDARY_FULL, BOUNDARY_NO_HEADING = 0, 1, 2, 3   # include/unina_mi355.h UNINA_BOUNDARY_*: end
BOUNDARY_MAX_CHAIN = 64
BOUNDARY_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("ref", "<i4")])                              # unina_boundary_point
BOUNDARY_HEADER_DTYPE = np.dtype([("n_candidates", "<i4", (2,)), ("n_chain", "<i4", (2,)), ("end", "<i4", (2,)), ("n_centre", "<i4"),
                                  ("n_wide", "<i4")])                                                                      # unina_boundary_header
assert BOUNDARY_POINT_DTYPE.itemsize == 16 and BOUNDARY_HEADER_DTYPE.itemsize == 32


class BoundaryParams(C.Structure):
    """unina_boundary_params: pose = row-major 3 x 4 [R|t], camera -> tracking frame, read only without a device pose."""
    _fields_ = [("pose", C.c_float * 12), ("forward", C.c_float * 3), ("first_gate", C.c_float), ("step_gate", C.c_float),
                ("cos_turn", C.c_float), ("width_gate", C.c_float), ("class_left", C.c_int), ("class_right", C.c_int), ("min_hits", C.c_int),
                ("max_chain", C.c_int)]


class TrackParams(C.Structure):
    """unina_track_params: pose = row-major 3 x 4 [R|t], camera frame -> tracking frame."""
    _fields_ = [("pose", C.c_float * 12), ("gate", C.c_float), ("alpha", C.c_float), ("birth_confidence", C.c_float),
                ("class_aware", C.c_int), ("confirm_hits", C.c_int), ("max_missed", C.c_int)]


def _tile_array(tiles):
    return (Tile * len(tiles))(*[Tile(*map(int, t)) for t in tiles])


class EngineError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None

# every symbol include/unina_mi355.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "unina_load_engine", "unina_unload_engine", "unina_engine_input_dims", "unina_set_tensor_address",
    "unina_tensor_address", "unina_enqueue", "unina_infer", "unina_infer_bgra", "unina_infer_nv12", "unina_infer_async", "unina_postprocess_async",
    "unina_last_error", "unina_op_count", "unina_get_op_info", "unina_profile_ops", "unina_profile_post", "unina_debug_read_buffer",
    "unina_version", "unina_conv_config_count", "unina_conv_config_name", "unina_set_op_config", "unina_autotune", "unina_debug_post_stamps", "unina_debug_conv_stamps", "unina_debug_dual_stamps", "unina_debug_dual_timeline", "unina_debug_block_stamps", "unina_debug_folded_heads", "unina_serial_latency",
    "unina_debug_owned_streams", "unina_debug_streams_overlap",
    "unina_set_fusion", "unina_fusion_groups", "unina_debug_fusable_groups",
    "unina_slice_tiles", "unina_infer_tiled_bgra", "unina_infer_tiled_bgra_async", "unina_merge_tiles_async",
    "unina_infer_tiled_nv12", "unina_infer_tiled_nv12_async", "unina_preprocess_nv12_resize",
    "unina_letterbox_geometry", "unina_infer_letterbox_bgra", "unina_infer_letterbox_nv12", "unina_infer_letterbox_bgra_async",
    "unina_infer_letterbox_nv12_async", "unina_preprocess_letterbox_bgra", "unina_preprocess_letterbox_nv12",
    "unina_infer_frame", "unina_infer_frame_async", "unina_infer_letterbox_frame", "unina_infer_letterbox_frame_async",
    "unina_infer_tiled_frame", "unina_infer_tiled_frame_async", "unina_preprocess_frame", "unina_preprocess_letterbox_frame",
    "unina_embedding_dim", "unina_mine_async", "unina_mine", "unina_mine_heads_async", "unina_kcenter",
    "unina_kmeans_workspace_bytes", "unina_kmeans", "unina_nearest_rows",
    "unina_abs_histogram_f16", "unina_calib_buffer_count", "unina_calib_buffer_name", "unina_calib_buffers_async", "unina_calib_async",
    "unina_eval_create", "unina_eval_destroy", "unina_eval_reset_async", "unina_eval_update_async", "unina_eval_read",
    "unina_locate_async", "unina_locate_stereo_async", "unina_rectify_async",
    "unina_lidar_create", "unina_lidar_destroy", "unina_locate_lidar_async", "unina_lidar_buffers",
    "unina_deskew_table", "unina_deskew_async",
    "unina_ground_create", "unina_ground_destroy", "unina_ground_filter_async", "unina_ground_buffers",
    "unina_cluster_create", "unina_cluster_destroy", "unina_cluster_async", "unina_cluster_buffers",
    "unina_fuse_async", "unina_colour_async",
    "unina_track_create", "unina_track_destroy", "unina_track_reset_async", "unina_track_update_async", "unina_track_buffers",
    "unina_track_read",
    "unina_pose_async", "unina_boundary_async",
    "unina_comm_unique_id", "unina_comm_init", "unina_comm_all_gather", "unina_comm_rank", "unina_comm_world", "unina_comm_destroy",
    "unina_comm_last_error",
    "create_norm_params_imagenet", "create_norm_params", "preprocess_bgra_resize", "preprocess_bgra", "preprocess_nv12",
    "allocate_preprocess_buffer", "free_preprocess_buffer", "create_preprocess_stream", "destroy_preprocess_stream",
    "init_postprocess_resources", "cleanup_postprocess_resources", "reset_detection_counter", "get_detection_count",
    "decode_yolo_head", "run_gpu_nms", "copy_valid_detections_to_host",
]


def load_library() -> C.CDLL:
    """Loads libunina_mi355.so; raises if it has not been built (``python unina-yolo-dla_amd/build.py``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                          f"(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.unina_load_engine.argtypes = [C.c_char_p, ci, C.POINTER(vp)]
    L.unina_unload_engine.argtypes = [vp]
    L.unina_unload_engine.restype = None
    L.unina_engine_input_dims.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.unina_set_tensor_address.argtypes = [vp, C.c_char_p, vp]
    L.unina_tensor_address.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.unina_enqueue.argtypes = [vp, vp]
    L.unina_infer.argtypes = [vp, vp, cf, cf, cf, vp, C.POINTER(ci), vp]
    L.unina_infer_async.argtypes = [vp, vp, cf, cf, cf, vp, vp, vp]
    L.unina_infer_bgra.argtypes = [vp, vp, ci, ci, ci, C.POINTER(NormParams), cf, cf, cf, vp, C.POINTER(ci), vp]
    L.unina_infer_nv12.argtypes = [vp, vp, vp, ci, ci, ci, ci, C.POINTER(NormParams), cf, cf, cf, vp, C.POINTER(ci), vp]
    L.unina_postprocess_async.argtypes = [vp, cf, cf, cf, vp, vp, vp]
    L.unina_last_error.argtypes = [vp]
    L.unina_last_error.restype = C.c_char_p
    L.unina_op_count.argtypes = [vp]
    L.unina_get_op_info.argtypes = [vp, ci, C.POINTER(OpInfo)]
    L.unina_profile_ops.argtypes = [vp, ci, C.POINTER(cf), vp]
    L.unina_profile_post.argtypes = [vp, ci, cf, cf, cf, C.POINTER(cf), vp]
    L.unina_debug_read_buffer.argtypes = [vp, C.c_char_p, vp, C.c_size_t, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.unina_version.restype = C.c_char_p
    L.unina_conv_config_name.restype = C.c_char_p
    L.unina_conv_config_name.argtypes = [ci]
    L.unina_set_op_config.argtypes = [vp, ci, ci]
    L.unina_autotune.argtypes = [vp, ci, vp]
    L.unina_set_fusion.argtypes = [vp, ci]
    L.unina_fusion_groups.argtypes = [vp]
    L.unina_debug_fusable_groups.argtypes = [C.c_char_p]
    L.unina_debug_post_stamps.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.unina_debug_conv_stamps.argtypes = [vp, ci, C.POINTER(C.c_longlong), vp]
    L.unina_debug_dual_stamps.argtypes = [vp, ci, C.POINTER(C.c_longlong), vp]
    L.unina_debug_dual_timeline.argtypes = [vp, ci, C.POINTER(C.c_longlong), ci, vp]
    L.unina_debug_block_stamps.argtypes = [vp, ci, C.POINTER(C.c_longlong), vp]
    L.unina_debug_folded_heads.argtypes = [vp]
    L.unina_debug_owned_streams.argtypes = []
    L.unina_debug_streams_overlap.argtypes = [ci, vp, vp, ci, C.POINTER(C.c_longlong), C.POINTER(ci)]
    L.unina_serial_latency.argtypes = [vp, C.POINTER(vp), ci, ci, cf, cf, cf, C.POINTER(C.c_double), vp]
    # sliced inference (csrc/postprocess.hip: tile_gather_kernel)
    L.unina_slice_tiles.argtypes = [ci, ci, ci, ci, cf, cf, C.POINTER(Tile), ci]
    L.unina_infer_tiled_bgra.argtypes = [vp, vp, ci, ci, ci, C.POINTER(Tile), ci, C.POINTER(NormParams), cf, cf, cf, cf, vp,
                                         C.POINTER(ci), vp]
    L.unina_infer_tiled_bgra_async.argtypes = [vp, vp, ci, ci, ci, C.POINTER(Tile), ci, C.POINTER(NormParams), cf, cf, cf, cf, vp,
                                               vp, vp]
    L.unina_infer_tiled_nv12.argtypes = [vp, vp, vp, ci, ci, ci, ci, C.POINTER(Tile), ci, C.POINTER(NormParams), cf, cf, cf, cf, vp,
                                         C.POINTER(ci), vp]
    L.unina_infer_tiled_nv12_async.argtypes = [vp, vp, vp, ci, ci, ci, ci, C.POINTER(Tile), ci, C.POINTER(NormParams), cf, cf, cf, cf,
                                               vp, vp, vp]
    L.unina_merge_tiles_async.argtypes = [vp, vp, vp, C.POINTER(Tile), ci, cf, vp, vp, vp]
    # letterboxed camera frames (csrc/stem_pool.hip: src_kind 5 / 6; csrc/postprocess.hip: map_box)
    L.unina_letterbox_geometry.argtypes = [ci, ci, ci, ci, C.POINTER(Letterbox)]
    L.unina_infer_letterbox_bgra.argtypes = [vp, vp, ci, ci, ci, C.POINTER(NormParams), cf, cf, cf, cf, ci, vp, C.POINTER(ci), vp]
    L.unina_infer_letterbox_bgra_async.argtypes = [vp, vp, ci, ci, ci, C.POINTER(NormParams), cf, cf, cf, cf, ci, vp, vp, vp]
    L.unina_infer_letterbox_nv12.argtypes = [vp, vp, vp, ci, ci, ci, ci, C.POINTER(NormParams), cf, cf, cf, cf, ci, vp,
                                             C.POINTER(ci), vp]
    L.unina_infer_letterbox_nv12_async.argtypes = [vp, vp, vp, ci, ci, ci, ci, C.POINTER(NormParams), cf, cf, cf, cf, ci, vp, vp, vp]
    L.unina_preprocess_letterbox_bgra.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, NormParams, vp]
    L.unina_preprocess_letterbox_nv12.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, NormParams, vp]
    # the frame descriptor: one family of calls for every unina_pixel_format
    fp, npp = C.POINTER(Frame), C.POINTER(NormParams)
    L.unina_infer_frame.argtypes = [vp, fp, npp, cf, cf, cf, vp, C.POINTER(ci), vp]
    L.unina_infer_frame_async.argtypes = [vp, fp, npp, cf, cf, cf, vp, vp, vp]
    L.unina_infer_letterbox_frame.argtypes = [vp, fp, npp, cf, cf, cf, cf, ci, vp, C.POINTER(ci), vp]
    L.unina_infer_letterbox_frame_async.argtypes = [vp, fp, npp, cf, cf, cf, cf, ci, vp, vp, vp]
    L.unina_infer_tiled_frame.argtypes = [vp, fp, C.POINTER(Tile), ci, npp, cf, cf, cf, cf, vp, C.POINTER(ci), vp]
    L.unina_infer_tiled_frame_async.argtypes = [vp, fp, C.POINTER(Tile), ci, npp, cf, cf, cf, cf, vp, vp, vp]
    L.unina_preprocess_frame.argtypes = [fp, C.POINTER(Tile), vp, ci, ci, npp, vp]
    L.unina_preprocess_letterbox_frame.argtypes = [fp, vp, ci, ci, cf, npp, vp]
    # data mining (csrc/mining.hip)
    L.unina_embedding_dim.argtypes = [vp]
    L.unina_mine_async.argtypes = [vp, vp, vp, vp, vp]
    L.unina_mine.argtypes = [vp, vp, vp, vp, vp]
    L.unina_mine_heads_async.argtypes = [vp, vp, vp]
    L.unina_kcenter.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp]
    # k-means coreset (csrc/kmeans.hip)
    L.unina_kmeans_workspace_bytes.restype = C.c_size_t
    L.unina_kmeans_workspace_bytes.argtypes = [ci, ci, ci]
    L.unina_kmeans.argtypes = [vp, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp]
    L.unina_nearest_rows.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp]
    # INT8 calibration (csrc/calib.hip)
    L.unina_abs_histogram_f16.argtypes = [vp, C.c_size_t, vp, vp]
    L.unina_calib_buffer_count.argtypes = [vp]
    L.unina_calib_buffer_name.argtypes = [vp, ci, C.c_char_p, C.c_size_t]
    L.unina_calib_buffers_async.argtypes = [vp, vp, vp]
    L.unina_calib_async.argtypes = [vp, vp, vp, vp]
    # evaluation (csrc/evalmatch.hip)
    L.unina_eval_create.argtypes = [ci, ci, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.unina_eval_destroy.argtypes = [vp]
    L.unina_eval_destroy.restype = None
    L.unina_eval_reset_async.argtypes = [vp, vp]
    L.unina_eval_update_async.argtypes = [vp, vp, vp, vp, ci, C.POINTER(EvalParams), C.c_uint, vp]
    L.unina_eval_read.argtypes = [vp, C.POINTER(EvalResult), vp, C.c_size_t, vp, C.c_size_t, vp]
    # 3-D localisation (csrc/locate.hip)
    L.unina_locate_async.argtypes = [vp, vp, C.POINTER(Depth), C.POINTER(Pinhole), C.POINTER(LocateParams), vp, vp]
    # 3-D localisation from a stereo pair (csrc/stereo.hip)
    L.unina_locate_stereo_async.argtypes = [vp, vp, C.POINTER(StereoPair), C.POINTER(Pinhole), cf, C.POINTER(StereoParams), vp, vp, vp]
    # rectification of raw camera images (csrc/rectify.hip)
    L.unina_rectify_async.argtypes = [C.POINTER(RectifyJob), ci, vp]
    # 3-D localisation from a LiDAR sweep (csrc/lidar.hip)
    L.unina_lidar_create.argtypes = [ci, ci, ci, ci, C.POINTER(vp)]
    L.unina_lidar_destroy.argtypes = [vp]
    L.unina_lidar_destroy.restype = None
    L.unina_locate_lidar_async.argtypes = [vp, vp, vp, C.POINTER(Cloud), C.POINTER(cf * 12), C.POINTER(Pinhole), ci, ci, C.POINTER(LidarParams),
                                           vp, vp]
    L.unina_lidar_buffers.argtypes = [vp, C.POINTER(vp)]
    # ground removal from a LiDAR sweep (csrc/ground.hip)
    L.unina_ground_create.argtypes = [ci, ci, C.POINTER(vp)]
    L.unina_ground_destroy.argtypes = [vp]
    L.unina_ground_destroy.restype = None
    L.unina_ground_filter_async.argtypes = [vp, C.POINTER(Cloud), C.POINTER(cf * 12), C.POINTER(GroundParams), vp, vp]
    L.unina_ground_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    # cone candidates from a ground-free LiDAR sweep (csrc/cluster.hip)
    L.unina_cluster_create.argtypes = [ci, ci, C.POINTER(vp)]
    L.unina_cluster_destroy.argtypes = [vp]
    L.unina_cluster_destroy.restype = None
    L.unina_cluster_async.argtypes = [vp, C.POINTER(Cloud), C.POINTER(cf * 12), C.POINTER(ClusterParams), vp, vp, vp, vp]
    L.unina_cluster_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    # motion de-skew of a LiDAR sweep (csrc/deskew.hip)
    L.unina_deskew_table.argtypes = [vp, ci, C.c_double, C.c_double, vp]
    L.unina_deskew_async.argtypes = [C.POINTER(Cloud), C.POINTER(PointTimes), ci, vp, ci, C.c_double, C.c_double, vp, vp, vp]
    # fusion of LiDAR cone candidates with camera records (csrc/fuse.hip)
    L.unina_fuse_async.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(FuseParams), vp, vp, vp, vp, vp, vp, vp]
    # class from pixels for records without one (csrc/colour.hip)
    L.unina_colour_async.argtypes = [vp, vp, vp, C.POINTER(Image), C.POINTER(Pinhole), C.POINTER(ColourParams), vp, vp, vp, vp]
    # the camera pose from the tracked cones (csrc/pose.hip)
    L.unina_pose_async.argtypes = [vp, vp, vp, vp, vp, C.POINTER(PoseParams), vp, vp, vp, vp]
    # track limits and centre line from the tracked cones (csrc/boundary.hip)
    L.unina_boundary_async.argtypes = [vp, vp, C.POINTER(BoundaryParams), vp, vp, vp]
    # tracking (csrc/track.hip)
    L.unina_track_create.argtypes = [ci, C.POINTER(vp)]
    L.unina_track_destroy.argtypes = [vp]
    L.unina_track_destroy.restype = None
    L.unina_track_reset_async.argtypes = [vp, vp]
    L.unina_track_update_async.argtypes = [vp, vp, vp, vp, C.POINTER(TrackParams), vp, vp]
    L.unina_track_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.unina_track_read.argtypes = [vp, vp, vp, C.c_size_t, vp]
    # multi-GPU: RCCL gather of detection slots behind the C ABI (csrc/comm.hip)
    L.unina_comm_unique_id.argtypes = [vp]
    L.unina_comm_init.argtypes = [C.POINTER(vp), vp, ci, ci, ci]
    L.unina_comm_all_gather.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.unina_comm_rank.argtypes = [vp]
    L.unina_comm_world.argtypes = [vp]
    L.unina_comm_destroy.argtypes = [vp]
    L.unina_comm_destroy.restype = None
    L.unina_comm_last_error.restype = C.c_char_p
    # cuda_preprocess.h drop-in symbols
    L.create_norm_params_imagenet.restype = NormParams
    L.create_norm_params.restype = NormParams
    L.create_norm_params.argtypes = [cf] * 6
    L.preprocess_bgra_resize.argtypes = [vp, vp, ci, ci, ci, ci, ci, NormParams, vp]
    L.preprocess_bgra.argtypes = [vp, vp, ci, ci, ci, NormParams, vp]
    L.preprocess_nv12.argtypes = [vp, vp, vp, ci, ci, ci, ci, NormParams, vp]
    L.unina_preprocess_nv12_resize.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, NormParams, vp]   # (ours: the reference's NV12 path cannot resize)
    L.allocate_preprocess_buffer.restype = vp
    L.allocate_preprocess_buffer.argtypes = [ci, ci]
    L.free_preprocess_buffer.argtypes = [vp]
    L.create_preprocess_stream.restype = vp
    L.destroy_preprocess_stream.argtypes = [vp]
    # gpu_postprocess.h drop-in symbols
    L.reset_detection_counter.argtypes = [vp]
    L.get_detection_count.argtypes = [C.POINTER(ci), vp]
    L.decode_yolo_head.argtypes = [vp, vp, vp, ci, ci, ci, ci, cf, cf, vp]
    L.run_gpu_nms.argtypes = [vp, ci, cf, vp]
    L.copy_valid_detections_to_host.argtypes = [vp, vp, ci, C.POINTER(ci), vp]
    _lib = L
    return L


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise EngineError("no MI355X visible to this process (torch.cuda.is_available() is False)")
    return torch


def _stream_ptr(stream) -> int:
    if stream is None:
        stream = _torch().cuda.current_stream()
    return stream if isinstance(stream, int) else stream.cuda_stream


def _ptr(t):
    """Device address of a CUDA tensor; None stays None (the ABI answers a null plane with UNINA_ERR_ARG)."""
    return None if t is None else t.data_ptr()


def _addr(t):
    """_ptr for an argument that may also be a raw device address already."""
    return t if isinstance(t, int) else _ptr(t)


def as_struct(cls, make, params):
    """`params` as a `cls`: the struct itself, a dict of `make`'s arguments, or a tuple in the struct's order."""
    if isinstance(params, cls):
        return params
    return make(**params) if isinstance(params, dict) else make(*params)


def device_view(address: int, count: int, typestr: str = "|u1", device: int = 0):
    """A CUDA tensor over `count` elements of `typestr` ("|u1" bytes, "<i4" words) at a device address: torch wraps the address,
    nothing is copied."""
    class View:
        __cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (address, False), "version": 2}
    return _torch().as_tensor(View(), device=f"cuda:{device}")


def _raise_on(rc: int, what: str) -> None:
    if rc:
        raise EngineError(f"{what} failed [{ERRORS.get(rc, rc)}]")


def det_buffer_ptrs(det_buf):
    """(records, count): the device addresses inside Engine.infer_async's int32 buffer (word 0 = count, records from word 8)."""
    base = det_buf.data_ptr()
    return base + 32, base


def read_records(stream, *pairs):
    """Synchronises `stream`; each (uint8 CUDA tensor, dtype) pair comes back as a host array of records."""
    torch = _torch()
    s = torch.cuda.current_stream() if stream is None else stream
    if not isinstance(s, int):
        with torch.cuda.stream(s):
            hosts = [t.cpu() for t, _ in pairs]
    else:
        torch.cuda.synchronize()
        hosts = [t.cpu() for t, _ in pairs]
    return tuple(h.numpy().view(dtype).copy() for h, (_, dtype) in zip(hosts, pairs))


def clamp_count(count, *arrays) -> int:
    """The device count word as the kernels read it, for the numpy twins: 0 .. MAX_DETECTIONS, and no more than the arrays hold."""
    return min(max(int(count), 0), MAX_DETECTIONS, *(len(a) for a in arrays))


def owned_streams() -> int:
    """Streams the library itself holds in this process (unina_debug_owned_streams): 0 whenever no call is running."""
    return load_library().unina_debug_owned_streams()


def streams_overlap(a, b, reps: int = 3, device: int = 0):
    """Do streams `a` and `b` (torch streams, raw handles, or None / 0 for the null stream) run on the chip at the same time
    (unina_debug_streams_overlap)? Returns (repetitions that overlapped, stamps [reps, 4] int64: start / end on `a`, start /
    end on `b`, 100 MHz ticks). Two streams that share a hardware queue give 0, as does a == b."""
    _torch()
    raw = [0 if s is None else (s if isinstance(s, int) else s.cuda_stream) for s in (a, b)]
    stamps = (C.c_longlong * (4 * reps))()
    n = C.c_int()
    _raise_on(load_library().unina_debug_streams_overlap(device, raw[0], raw[1], reps, stamps, C.byref(n)), "unina_debug_streams_overlap")
    return n.value, np.array(stamps[:], dtype=np.int64).reshape(reps, 4)


class Engine:
    """One engine handle on one GPU. Use two handles to keep two frames in flight."""

    def __init__(self, path: str, device: int = 0):
        self.L = load_library()
        torch = _torch()
        self.device = device
        self.h = C.c_void_p()
        rc = self.L.unina_load_engine(path.encode(), device, C.byref(self.h))
        if rc:
            raise EngineError(f"unina_load_engine({path}) failed [{ERRORS.get(rc, rc)}]: "
                              f"{self.L.unina_last_error(None).decode()}")
        w, h, nc = C.c_int(), C.c_int(), C.c_int()
        self._check(self.L.unina_engine_input_dims(self.h, C.byref(w), C.byref(h), C.byref(nc)))
        self.width, self.height, self.num_classes = w.value, h.value, nc.value
        dev = torch.device("cuda", device)
        # the caller (this wrapper) owns the I/O buffers, as the node does (perception_node.cpp:696-707).
        # self.outputs holds the six raw head tensors as enqueue() / forward() write them. infer() / infer_async() do NOT
        # update them (the heads' output convs run inside the decode launch, include/unina_mi355.h at unina_infer): after
        # an infer call they still hold the previous forward()'s values.
        self.outputs: Dict[str, "torch.Tensor"] = {}
        for name, s in zip(OUTPUT_NAMES, (4, 4, 8, 8, 16, 16)):
            c = nc.value if name.endswith("cls") else 4
            t = torch.zeros((1, c, h.value // s, w.value // s), dtype=torch.float32, device=dev)
            self.outputs[name] = t
            self._check(self.L.unina_set_tensor_address(self.h, name.encode(), t.data_ptr()))
        self._images = None
        self._det_buf = torch.zeros((MAX_DETECTIONS * 8 + 8,), dtype=torch.int32, device=dev)

    # -- construction helpers -------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd: Dict[str, np.ndarray], graph: Optional[Graph] = None, device: int = 0,
                        path: Optional[str] = None, precision: int = _export.FP16,
                        amax: Optional[Dict[str, float]] = None,
                        weight_amax: Optional[Dict[str, float]] = None) -> "Engine":
        """export_trt.py's role + load: folds/fuses `sd` into an engine file (temporary unless `path`) and loads it.
        INT8 needs `amax` (calibrate_amax below)."""
        if path is None:
            fd, tmp = tempfile.mkstemp(suffix=".une")
            os.close(fd)
            try:
                _export.export_engine(sd, tmp, graph, precision, amax, weight_amax)
                return cls(tmp, device)
            finally:
                os.unlink(tmp)
        _export.export_engine(sd, path, graph, precision, amax, weight_amax)
        return cls(path, device)

    def _check(self, rc: int):
        if rc:
            raise EngineError(f"[{ERRORS.get(rc, rc)}] {self.L.unina_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            _torch().cuda.synchronize(self.device)
            self.L.unina_unload_engine(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- TensorRTEngine-shaped path --------------------------------------------------------------------
    def bind_images(self, images) -> None:
        """images: torch cuda fp32 [1,3,H,W] contiguous (setInputTensorAddress("images", ...))."""
        assert images.is_cuda and images.dtype == _torch().float32 and images.is_contiguous()
        assert tuple(images.shape) == (1, 3, self.height, self.width), images.shape
        self._images = images
        self._check(self.L.unina_set_tensor_address(self.h, b"images", images.data_ptr()))

    def enqueue(self, stream=None) -> None:
        """enqueueV3: raw heads into self.outputs (asynchronous)."""
        self._check(self.L.unina_enqueue(self.h, _stream_ptr(stream)))

    def forward(self, images) -> Dict[str, np.ndarray]:
        """Raw-head forward, synchronous; returns {name: [C,H,W] fp32 ndarray}."""
        self.bind_images(images)
        self.enqueue()
        _torch().cuda.synchronize(self.device)
        return {k: v[0].cpu().numpy() for k, v in self.outputs.items()}

    # -- fused path ----------------------------------------------------------------------------------------
    def infer(self, images, conf_thr: float = 0.5, iou_thr: float = 0.45, conformal_q: float = 0.1, stream=None):
        """Forward + decode + NMS; returns a structured ndarray of kept detections (DET_DTYPE).
        The per-call Python work is kept minimal (the call is ~0.23 ms end to end): a tensor object is validated once,
        its address goes straight into unina_infer, and the host-side record buffer / count are reused."""
        ptr = None
        if images is not None:
            if images is not getattr(self, "_images", None):
                assert images.is_cuda and images.dtype == _torch().float32 and images.is_contiguous()
                assert tuple(images.shape) == (1, 3, self.height, self.width), images.shape
                self._images = images
            ptr = images.data_ptr()
        if getattr(self, "_host_out", None) is None:
            self._host_out = np.zeros(MAX_DETECTIONS, dtype=DET_DTYPE)
            self._host_out_ptr = self._host_out.ctypes.data
            self._host_n = C.c_int()
            self._host_n_ref = C.byref(self._host_n)
        self._check(self.L.unina_infer(self.h, ptr, conf_thr, iou_thr, conformal_q, self._host_out_ptr, self._host_n_ref,
                                       _stream_ptr(stream)))
        return self._host_out[:self._host_n.value].copy()

    def serial_latency(self, frames, n_calls: int, conf_thr: float = 0.5, iou_thr: float = 0.45, conformal_q: float = 0.1, stream=None):
        """`n_calls` serial unina_infer calls over the ring `frames` (CUDA tensors), timed INSIDE the C ABI: latencies in ms."""
        ptrs = (C.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
        lat = (C.c_double * n_calls)()
        self._check(self.L.unina_serial_latency(self.h, ptrs, len(frames), n_calls, conf_thr, iou_thr, conformal_q, lat, _stream_ptr(stream)))
        return np.array(lat[:], dtype=np.float64) * 1e-3

    def _camera_call(self, symbol: str, lead, norm, tail, out, stream):
        """One camera call of the ABI: `symbol`(handle, *lead, norm, *tail, records, count, stream). `out=None`: synchronous into a
        host buffer, returns the kept detections; `out` = an int32 CUDA tensor as infer_async's: `symbol`_async, returns it."""
        if norm is None:
            norm = self.L.create_norm_params_imagenet()
        if out is not None:
            self._check(getattr(self.L, symbol + "_async")(self.h, *lead, C.byref(norm), *tail, *det_buffer_ptrs(out), _stream_ptr(stream)))
            return out
        host = np.zeros(MAX_DETECTIONS, dtype=DET_DTYPE)
        n = C.c_int()
        self._check(getattr(self.L, symbol)(self.h, *lead, C.byref(norm), *tail, host.ctypes.data, C.byref(n), _stream_ptr(stream)))
        return host[:n.value].copy()

    def infer_bgra(self, frame, width: int, height: int, pitch: int, norm: Optional[NormParams] = None,
                   conf_thr: float = 0.5, iou_thr: float = 0.45, conformal_q: float = 0.1, stream=None):
        """Camera frame (uint8 CUDA tensor, pitched BGRA) -> detections: the pre-process runs inside the stem kernel
        (perception_node.cpp:601-656 as one launch sequence, no fp32 tensor in between)."""
        return self._camera_call("unina_infer_bgra", (_ptr(frame), width, height, pitch), norm, (conf_thr, iou_thr, conformal_q), None, stream)

    def infer_nv12(self, y, uv, width: int, height: int, y_pitch: int, uv_pitch: int, norm: Optional[NormParams] = None,
                   conf_thr: float = 0.5, iou_thr: float = 0.45, conformal_q: float = 0.1, stream=None):
        """NV12 camera frame (uint8 CUDA tensors: luma plane `y`, interleaved chroma plane `uv` of (height + 1) // 2 rows)
        -> detections, the pre-process inside the stem kernel (unina_infer_nv12; camera.nv12_to_tensor is its numpy twin)."""
        return self._camera_call("unina_infer_nv12", (_ptr(y), _ptr(uv), width, height, y_pitch, uv_pitch), norm,
                                 (conf_thr, iou_thr, conformal_q), None, stream)

    def infer_letterbox_bgra(self, frame, width: int, height: int, pitch: int, norm: Optional[NormParams] = None,
                             conf_thr: float = 0.5, iou_thr: float = 0.45, conformal_q: float = 0.1, pad_value: float = 114.0,
                             map_boxes: bool = True, out=None, stream=None):
        """infer_bgra without the stretch: the frame keeps its aspect ratio inside the network input (letterbox_geometry),
        `pad_value` around it, all computed in the stem kernel. map_boxes: boxes back in CAMERA pixels (mapped where the
        post-process writes them; camera.unmap_boxes is the numpy twin), False: network pixels. `out=None`: synchronous,
        returns the kept detections; `out` = an int32 CUDA tensor as infer_async's: asynchronous, returns it."""
        return self._camera_call("unina_infer_letterbox_bgra", (_ptr(frame), width, height, pitch), norm,
                                 (conf_thr, iou_thr, conformal_q, pad_value, int(map_boxes)), out, stream)

    def infer_letterbox_nv12(self, y, uv, width: int, height: int, y_pitch: int, uv_pitch: int, norm: Optional[NormParams] = None,
                             conf_thr: float = 0.5, iou_thr: float = 0.45, conformal_q: float = 0.1, pad_value: float = 114.0,
                             map_boxes: bool = True, out=None, stream=None):
        """infer_letterbox_bgra for an NV12 frame (planes and pitches as infer_nv12)."""
        return self._camera_call("unina_infer_letterbox_nv12", (_ptr(y), _ptr(uv), width, height, y_pitch, uv_pitch), norm,
                                 (conf_thr, iou_thr, conformal_q, pad_value, int(map_boxes)), out, stream)

    def infer_tiled_nv12(self, y, uv, width: int, height: int, y_pitch: int, uv_pitch: int, tiles=None,
                         norm: Optional[NormParams] = None, conf_thr: float = 0.5, iou_thr: float = 0.45, conformal_q: float = 0.1,
                         merge_iou: float = 0.45, out=None, stream=None):
        """infer_tiled_bgra on an NV12 frame: the tile's origin goes to the stem kernel (it enters the chroma index, so it may
        be odd). `tiles`, `out` and the result as there."""
        if tiles is None:
            tiles = self.default_tiles(width, height)
        return self._camera_call("unina_infer_tiled_nv12", (_ptr(y), _ptr(uv), width, height, y_pitch, uv_pitch, _tile_array(tiles), len(tiles)),
                                 norm, (conf_thr, iou_thr, conformal_q, merge_iou), out, stream)

    def infer_frame(self, frame: Frame, norm: Optional[NormParams] = None, conf_thr: float = 0.5, iou_thr: float = 0.45,
                    conformal_q: float = 0.1, out=None, stream=None):
        """A camera frame of any unina_pixel_format (Frame) -> detections, the pre-process inside the stem kernel
        (unina_infer_frame; camera.frame_to_tensor is its numpy twin). `out=None`: synchronous, returns the kept detections;
        `out` = an int32 CUDA tensor as infer_async's: asynchronous, returns it."""
        return self._camera_call("unina_infer_frame", (C.byref(frame),), norm, (conf_thr, iou_thr, conformal_q), out, stream)

    def infer_letterbox_frame(self, frame: Frame, norm: Optional[NormParams] = None, conf_thr: float = 0.5, iou_thr: float = 0.45,
                              conformal_q: float = 0.1, pad_value: float = 114.0, map_boxes: bool = True, out=None, stream=None):
        """infer_letterbox_bgra for a Frame of any format."""
        return self._camera_call("unina_infer_letterbox_frame", (C.byref(frame),), norm,
                                 (conf_thr, iou_thr, conformal_q, pad_value, int(map_boxes)), out, stream)

    def infer_tiled_frame(self, frame: Frame, tiles=None, norm: Optional[NormParams] = None, conf_thr: float = 0.5,
                          iou_thr: float = 0.45, conformal_q: float = 0.1, merge_iou: float = 0.45, out=None, stream=None):
        """infer_tiled_bgra for a Frame of any format (BGRA / RGB / RGBA tiles are pointer offsets, the other formats send the
        tile's origin to the stem kernel)."""
        if tiles is None:
            tiles = self.default_tiles(frame.width, frame.height)
        return self._camera_call("unina_infer_tiled_frame", (C.byref(frame), _tile_array(tiles), len(tiles)), norm,
                                 (conf_thr, iou_thr, conformal_q, merge_iou), out, stream)

    def default_tiles(self, width: int, height: int):
        """The reference's default slicing (20 % overlap) at the engine's input size, exact repeats dropped."""
        from . import slicing
        return slicing.get_slices(height, width, self.height, self.width)

    def infer_tiled_bgra(self, frame, width: int, height: int, pitch: int, tiles=None, norm: Optional[NormParams] = None,
                         conf_thr: float = 0.5, iou_thr: float = 0.45, conformal_q: float = 0.1, merge_iou: float = 0.45,
                         out=None, stream=None):
        """Sliced inference (auto_labeler.py:124-199): the detector on every tile (x, y, w, h) of the camera frame -- a tile is
        a pointer offset, nothing is copied -- and one merge on the GPU; boxes in CAMERA-FRAME pixels. `tiles=None` slices
        with the reference's defaults for the engine's input size. `out=None`: synchronous, returns the kept detections
        (DET_DTYPE); `out` = an int32 CUDA tensor as infer_async's: asynchronous, returns it."""
        if tiles is None:
            tiles = self.default_tiles(width, height)
        return self._camera_call("unina_infer_tiled_bgra", (_ptr(frame), width, height, pitch, _tile_array(tiles), len(tiles)), norm,
                                 (conf_thr, iou_thr, conformal_q, merge_iou), out, stream)

    def merge_tiles(self, slots, counts, tiles, merge_iou: float = 0.45, out=None, stream=None):
        """The merge alone (unina_merge_tiles_async): `slots` int32 CUDA tensor [T, 8 * MAX_DETECTIONS] (records), `counts`
        int32 CUDA tensor [T], `tiles` [(x, y, w, h)]. Asynchronous; returns `out` (int32 result tensor as infer_async's;
        Engine.unpack reads it)."""
        torch = _torch()
        for t in (slots, counts):
            assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()
        assert slots.numel() >= len(tiles) * 8 * MAX_DETECTIONS and counts.numel() >= len(tiles)
        out = self._det_buf if out is None else out
        self._check(self.L.unina_merge_tiles_async(self.h, slots.data_ptr(), counts.data_ptr(), _tile_array(tiles), len(tiles),
                                                   merge_iou, *det_buffer_ptrs(out), _stream_ptr(stream)))
        return out

    def infer_async(self, images, conf_thr: float = 0.5, iou_thr: float = 0.45, conformal_q: float = 0.1,
                    out=None, stream=None):
        """Asynchronous: results stay on the GPU in `out` (int32 tensor of 8 + 8*MAX_DETECTIONS words:
        word 0 = count, records from word 8). Returns `out`."""
        if images is not None:
            self.bind_images(images)
        out = self._det_buf if out is None else out
        self._check(self.L.unina_infer_async(self.h, None, conf_thr, iou_thr, conformal_q, *det_buffer_ptrs(out), _stream_ptr(stream)))
        return out

    def postprocess(self, conf_thr: float = 0.5, iou_thr: float = 0.45, conformal_q: float = 0.1, stream=None):
        """Decode + NMS on whatever the six output tensors currently hold (synchronous)."""
        self._check(self.L.unina_postprocess_async(self.h, conf_thr, iou_thr, conformal_q, *det_buffer_ptrs(self._det_buf),
                                                   _stream_ptr(stream)))
        return self.unpack(self._det_buf)

    # -- data mining (active_learning.py: difficulty scores + P4 embedding) ------------------------------------
    @property
    def embedding_dim(self) -> int:
        """Length of the embedding (channels of the backbone's P4 map); raises for an engine without one (graph (B))."""
        d = self.L.unina_embedding_dim(self.h)
        if d < 0:
            raise EngineError(f"[{ERRORS.get(-d, -d)}] this engine has no embedding (graph (B) models have no .backbone)")
        return d

    def _checked_images_ptr(self, images):
        if images is None:
            return None
        if images is not getattr(self, "_images", None):
            assert images.is_cuda and images.dtype == _torch().float32 and images.is_contiguous()
            assert tuple(images.shape) == (1, 3, self.height, self.width), images.shape
            self._images = images
        return images.data_ptr()

    def mine(self, images, embed: bool = True, stream=None):
        """Forward + difficulty scores + pooled embedding of one frame, synchronous: (scores[8], embed[D] or None).
        scores: [0..2] entropy score per level, [3..5] loc_var score per level, [6] / [7] the image's score in mode
        "entropy" / "loc_var" (include/unina_mi355.h at UNINA_MINE_SCORES)."""
        scores = np.empty(8, dtype=np.float32)
        emb = np.empty(self.embedding_dim, dtype=np.float32) if embed else None
        self._check(self.L.unina_mine(self.h, self._checked_images_ptr(images), scores.ctypes.data,
                                      emb.ctypes.data if embed else None, _stream_ptr(stream)))
        return scores, emb

    def mine_async(self, images, scores_out, embed_out=None, stream=None) -> None:
        """Asynchronous: results go to the CUDA fp32 tensors `scores_out` (8 values) and `embed_out` (D values or None),
        e.g. rows of [N,8] / [N,D] matrices that stay on the device for kcenter()."""
        assert scores_out.is_cuda and scores_out.dtype == _torch().float32 and scores_out.is_contiguous() and scores_out.numel() >= 8
        if embed_out is not None:
            assert embed_out.is_cuda and embed_out.dtype == _torch().float32 and embed_out.is_contiguous()
            assert embed_out.numel() >= self.embedding_dim
        self._check(self.L.unina_mine_async(self.h, self._checked_images_ptr(images), scores_out.data_ptr(),
                                            None if embed_out is None else embed_out.data_ptr(), _stream_ptr(stream)))

    def mine_heads(self, stream=None) -> np.ndarray:
        """The 8 scores of whatever the six output tensors currently hold (synchronous)."""
        torch = _torch()
        out = torch.zeros(8, dtype=torch.float32, device=torch.device("cuda", self.device))
        self._check(self.L.unina_mine_heads_async(self.h, out.data_ptr(), _stream_ptr(stream)))
        return out.cpu().numpy()

    # -- INT8 calibration (csrc/calib.hip: |x| value-count tables of the fp16 activation buffers) ----------------
    def calib_buffer_names(self) -> List[str]:
        """The buffers a calibration covers (every fp16 activation buffer of the engine file, in file order): the row
        order of calib_counts()."""
        if getattr(self, "_calib_names", None) is None:
            n = self.L.unina_calib_buffer_count(self.h)
            if n < 0:
                raise EngineError(f"[{ERRORS.get(-n, -n)}] unina_calib_buffer_count")
            names = []
            for i in range(n):
                buf = C.create_string_buffer(64)
                self._check(self.L.unina_calib_buffer_name(self.h, i, buf, len(buf)))
                names.append(buf.value.decode())
            self._calib_names = names
        return list(self._calib_names)

    def calib_counts_async(self, images, out, stream=None) -> None:
        """Asynchronous: forward of `images` (None: no forward, the buffers as they stand) + the value-count tables into
        the CUDA int32 tensor `out` ([n_buf, 32768], the bits are uint32 counts). Fusion must be off (set_fusion(False))."""
        torch = _torch()
        n = len(self.calib_buffer_names())
        assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= n * _export.CALIB_BINS
        if images is None:
            self._check(self.L.unina_calib_buffers_async(self.h, out.data_ptr(), _stream_ptr(stream)))
        else:
            self._check(self.L.unina_calib_async(self.h, self._checked_images_ptr(images), out.data_ptr(), _stream_ptr(stream)))

    def calib_counts(self, images=None) -> np.ndarray:
        """Value-count tables of every calibration buffer, synchronous: uint32 [n_buf, 32768], row i = how many elements of
        buffer calib_buffer_names()[i] carry each 15-bit fp16 pattern (bits & 0x7fff). `images`: a frame to run first
        (raw-head forward); None = the buffers as they stand."""
        torch = _torch()
        n = len(self.calib_buffer_names())
        out = torch.empty((max(n, 1), _export.CALIB_BINS), dtype=torch.int32, device=torch.device("cuda", self.device))
        self.calib_counts_async(images, out)
        torch.cuda.synchronize(self.device)
        return out[:n].cpu().numpy().view(np.uint32)

    @staticmethod
    def unpack(buf) -> np.ndarray:
        """int32 result tensor (see infer_async) -> structured ndarray of the kept detections."""
        host = buf.cpu().numpy()
        n = int(host[0])
        return host[8:8 + 8 * n].view(DET_DTYPE).copy()

    # -- introspection ---------------------------------------------------------------------------------------
    def op_infos(self) -> List[dict]:
        out = []
        for i in range(self.L.unina_op_count(self.h)):
            info = OpInfo()
            self._check(self.L.unina_get_op_info(self.h, i, C.byref(info)))
            out.append(dict(name=info.name.decode(), kernel=info.kernel.decode(), kind=info.kind, m=info.m, n=info.n,
                            k=info.k, flops=info.flops, bytes=info.bytes, grid=info.grid, block=info.block))
        return out

    def profile_ops(self, iters: int = 20, stream=None) -> List[dict]:
        n = self.L.unina_op_count(self.h)
        ms = (C.c_float * n)()
        self._check(self.L.unina_profile_ops(self.h, iters, ms, _stream_ptr(stream)))
        infos = self.op_infos()
        for i, d in enumerate(infos):
            d["ms"] = float(ms[i])
        return infos

    def profile_post(self, iters: int = 20, conf_thr: float = 0.5, iou_thr: float = 0.45, conformal_q: float = 0.1, stream=None):
        """(ms of the decode launch, ms of the pair-tile / scan / output launch) inside the frame sequence."""
        ms = (C.c_float * 2)()
        self._check(self.L.unina_profile_post(self.h, iters, conf_thr, iou_thr, conformal_q, ms, _stream_ptr(stream)))
        return float(ms[0]), float(ms[1])

    def autotune(self, images=None, iters: int = 10, stream=None, cache: Optional[str] = None) -> None:
        """Pick the fastest tile configuration per conv op by timing on this GPU (results are unchanged).
        `cache`: JSON tactic cache (the role of TensorRT's timing cache): reused when it matches this engine."""
        import json
        names = self.conv_configs()
        key = f"{self.width}x{self.height}:{self.op_infos()[1]['kernel'][:13]}:" + "|".join(f"{o['m']},{o['n']},{o['k']}" for o in self.op_infos())
        if cache and os.path.exists(cache):
            try:
                with open(cache) as f:
                    blob = json.load(f)
                if blob.get("key") == key and blob.get("configs") == names:
                    for i, c in enumerate(blob["choice"]):
                        if c >= 0:
                            self.set_op_config(i, c)
                    return
            except (ValueError, KeyError):
                pass
        if images is None and self._images is None:
            images = _torch().zeros((1, 3, self.height, self.width), dtype=_torch().float32,
                                    device=_torch().device("cuda", self.device))
        if images is not None:
            self.bind_images(images)
        self._check(self.L.unina_autotune(self.h, iters, _stream_ptr(stream)))
        _torch().cuda.synchronize(self.device)
        if cache:
            norm = [o["kernel"].replace("<f32,", "<f16,") for o in self.op_infos()]
            choice = [names.index(k) if k in names else -1 for k in norm]
            with open(cache, "w") as f:
                json.dump({"key": key, "configs": names, "choice": choice}, f)

    def debug_stamps(self):
        """Phase time stamps (100 MHz ticks) of the last unina_infer's post-process (needs UNINA_POST_STAMPS=1)."""
        buf = (C.c_longlong * 16)()
        self._check(self.L.unina_debug_post_stamps(self.h, buf))
        return [int(v) for v in buf]

    def conv_stamps(self, op_index: int, stream=None) -> List[int]:
        """In-kernel phase stamps (shader-clock ticks) of one launch of conv op `op_index` (debug)."""
        buf = (C.c_longlong * 8)()
        self._check(self.L.unina_debug_conv_stamps(self.h, op_index, buf, _stream_ptr(stream)))
        return [int(v) for v in buf]

    def dual_stamps(self, op_index: int, stream=None) -> List[int]:
        """In-kernel phase stamps of the dual conv launch led by op `op_index`: 8 values per conv (debug)."""
        buf = (C.c_longlong * 16)()
        self._check(self.L.unina_debug_dual_stamps(self.h, op_index, buf, _stream_ptr(stream)))
        return [int(v) for v in buf]

    def block_stamps(self, op_index: int, stream=None) -> List[int]:
        """Per-step shader-clock stamps of the fused C3k2 block led by op `op_index` (debug twin; the 40x40-level blocks)."""
        buf = (C.c_longlong * 16)()
        self._check(self.L.unina_debug_block_stamps(self.h, op_index, buf, _stream_ptr(stream)))
        return [int(v) for v in buf]

    def dual_timeline(self, op_index: int, stream=None):
        """Start / end (100 MHz wall clock) of every workgroup of the dual conv launch led by op `op_index`: array [grid + 1, 2];
        the last row = a marker kernel enqueued right before the launch, one right after it."""
        cap = 2 * 4096 + 2
        buf = (C.c_longlong * cap)()
        n = self.L.unina_debug_dual_timeline(self.h, op_index, buf, cap, _stream_ptr(stream))
        if n <= 0:
            raise RuntimeError(f"unina_debug_dual_timeline: error {-n}")
        return np.array(buf[:2 * n + 2], dtype=np.int64).reshape(n + 1, 2)

    def folded_heads(self) -> List[bool]:
        """Per head (P2, P3, P4): does the decode launch of infer() compute its output convs itself (unina_debug_folded_heads)?"""
        m = self.L.unina_debug_folded_heads(self.h)
        if m < 0:
            raise EngineError(f"[{ERRORS.get(-m, -m)}] unina_debug_folded_heads")
        return [bool(m >> h & 1) for h in range(3)]

    def conv_configs(self) -> List[str]:
        return [self.L.unina_conv_config_name(i).decode() for i in range(self.L.unina_conv_config_count())]

    def set_op_config(self, op_index: int, cfg: int) -> bool:
        """Force a tile configuration for one conv op (-1 = heuristic). Returns False if it does not fit."""
        rc = self.L.unina_set_op_config(self.h, op_index, cfg)
        if rc == 6:
            return False
        self._check(rc)
        return True

    def set_fusion(self, enable: bool) -> int:
        """C3k2 block fusion on/off (bit-identical results; off = every internal buffer is written, for per-layer
        checks and calibration). Returns the number of blocks now running as one launch."""
        self._check(self.L.unina_set_fusion(self.h, int(bool(enable))))
        return self.L.unina_fusion_groups(self.h)

    def read_buffer(self, name: str) -> np.ndarray:
        """Internal activation buffer -> [C,H,W] fp32 (parity tests)."""
        c, h, w = C.c_int(-1), C.c_int(), C.c_int()
        self.L.unina_debug_read_buffer(self.h, name.encode(), None, 0, C.byref(c), C.byref(h), C.byref(w))  # dims only
        if c.value < 0:
            raise EngineError(f"unknown buffer {name!r}")
        out = np.empty(c.value * h.value * w.value, dtype=np.float32)
        self._check(self.L.unina_debug_read_buffer(self.h, name.encode(), out.ctypes.data, out.size, C.byref(c),
                                                   C.byref(h), C.byref(w)))
        return out.reshape(c.value, h.value, w.value)


def _behind_current(torch, stream, device):
    """For the selection wrappers, which create and initialise their tensors on the CURRENT stream and launch on `stream`:
    the torch stream of `stream` (a torch stream or a raw handle), made to wait for everything enqueued on the current
    stream of `device` so far, so the kernels run behind those fills, clones and uploads; None when the launch goes to the
    current stream anyway. The caller synchronises the returned stream before it reads results back on the current one."""
    if stream is None:
        return None
    current = torch.cuda.current_stream(device)
    side = torch.cuda.ExternalStream(stream, device=device) if isinstance(stream, int) else stream
    if side.cuda_stream == current.cuda_stream:
        return None
    side.wait_stream(current)
    return side


def kcenter(embeddings, k: int, first_index: int, stream=None) -> np.ndarray:
    """K-center greedy on the GPU (coreset_selection_kcenter's loop, active_learning.py:139-161): the `k` selected row
    indices in selection order. `embeddings`: [N,D] fp32, a CUDA tensor (used in place) or an ndarray (uploaded). `stream`:
    the launches go there, behind whatever the current stream holds at the call; the call returns when they are done."""
    L = load_library()
    torch = _torch()
    if not isinstance(embeddings, torch.Tensor):
        embeddings = torch.from_numpy(np.ascontiguousarray(embeddings, dtype=np.float32)).cuda()
    assert embeddings.is_cuda and embeddings.dtype == torch.float32 and embeddings.is_contiguous() and embeddings.dim() == 2
    n, d = embeddings.shape
    with torch.cuda.device(embeddings.device):
        sel = torch.zeros(max(k, 1), dtype=torch.int32, device=embeddings.device)
        ws = torch.empty(n, dtype=torch.float32, device=embeddings.device)
        side = _behind_current(torch, stream, embeddings.device)
        rc = L.unina_kcenter(embeddings.data_ptr(), n, d, k, first_index, sel.data_ptr(), ws.data_ptr(), _stream_ptr(stream))
        if rc:
            raise EngineError(f"unina_kcenter failed [{ERRORS.get(rc, rc)}] (n={n}, dim={d}, k={k}, first_index={first_index})")
        if side is not None:
            side.synchronize()   # (the copy below runs on the current stream, the selection on `stream`)
        return sel.cpu().numpy()[:k].astype(np.int64)


KMEANS_CONVERGED = 1 << 30   # include/unina_mi355.h UNINA_KMEANS_CONVERGED


def _device_matrix(torch, x, device=None):
    """[rows, cols] fp32 contiguous CUDA tensor: a tensor is used in place, an ndarray is uploaded."""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        x = x.cuda() if device is None else x.to(device)
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
    return x


def kmeans(embeddings, k: int, init_rows=None, centroids=None, max_iter: int = 100, stream=None):
    """Full-batch Lloyd k-means on the GPU (unina_kmeans, csrc/kmeans.hip): all `max_iter` iterations are enqueued by one
    call and a device flag ends the loop once an assignment changes no label. Start centroids: the rows `init_rows` (k
    indices) or the [k, D] matrix `centroids` (exactly one of the two). `embeddings`: [N,D] fp32, a CUDA tensor (used in
    place) or an ndarray (uploaded). Returns (centroids [k,D] fp32, labels [N] int64, inertia_history [iters] float64, iters,
    converged), all on the host."""
    L = load_library()
    torch = _torch()
    if (init_rows is None) == (centroids is None):
        raise ValueError("give the start as init_rows or as centroids, not both")
    embeddings = _device_matrix(torch, embeddings)
    n, d = embeddings.shape
    dev = embeddings.device
    with torch.cuda.device(dev):
        if centroids is None:
            init = torch.from_numpy(np.ascontiguousarray(init_rows, dtype=np.int32).reshape(-1)).to(dev)
            if init.numel() != k:
                raise ValueError(f"init_rows holds {init.numel()} indices, k = {k}")
            cen = torch.zeros((k, d), dtype=torch.float32, device=dev)
        else:
            init = None
            cen = _device_matrix(torch, centroids, dev).clone()
            if tuple(cen.shape) != (k, d):
                raise ValueError(f"centroids of shape {tuple(cen.shape)}, expected {(k, d)}")
        labels = torch.zeros(n, dtype=torch.int32, device=dev)
        hist = torch.zeros(max(max_iter, 1), dtype=torch.float64, device=dev)
        iters = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(max(int(L.unina_kmeans_workspace_bytes(n, d, k)), 16), dtype=torch.uint8, device=dev)
        side = _behind_current(torch, stream, dev)
        rc = L.unina_kmeans(embeddings.data_ptr(), n, d, k, init.data_ptr() if init is not None else None, max_iter, cen.data_ptr(),
                            labels.data_ptr(), hist.data_ptr(), iters.data_ptr(), ws.data_ptr(), _stream_ptr(stream))
        if rc:
            raise EngineError(f"unina_kmeans failed [{ERRORS.get(rc, rc)}] (n={n}, dim={d}, k={k}, max_iter={max_iter})")
        if side is not None:
            side.synchronize()   # (the copies below run on the current stream, the loop on `stream`)
        it = int(iters.cpu()[0])
        if it < 0:
            raise EngineError(f"unina_kmeans: an init row lies outside [0, {n})")
        done = it & (KMEANS_CONVERGED - 1)
        return (cen.cpu().numpy(), labels.cpu().numpy().astype(np.int64), hist.cpu().numpy()[:done].copy(), done,
                bool(it & KMEANS_CONVERGED))


def nearest_rows(embeddings, centroids, stream=None) -> np.ndarray:
    """For each centroid in order, the index of the nearest row not chosen by an earlier centroid (unina_nearest_rows: the
    selection loop of coreset_selection_kmeans, active_learning.py:203-209). Tensors or ndarrays, as kmeans()."""
    L = load_library()
    torch = _torch()
    embeddings = _device_matrix(torch, embeddings)
    centroids = _device_matrix(torch, centroids, embeddings.device)
    n, d = embeddings.shape
    k = centroids.shape[0]
    if centroids.shape[1] != d:
        raise ValueError(f"centroids of shape {tuple(centroids.shape)} for embeddings of dimension {d}")
    with torch.cuda.device(embeddings.device):
        sel = torch.zeros(max(k, 1), dtype=torch.int32, device=embeddings.device)
        ws = torch.empty(n, dtype=torch.float32, device=embeddings.device)
        side = _behind_current(torch, stream, embeddings.device)
        rc = L.unina_nearest_rows(embeddings.data_ptr(), n, d, centroids.data_ptr(), k, sel.data_ptr(), ws.data_ptr(), _stream_ptr(stream))
        if rc:
            raise EngineError(f"unina_nearest_rows failed [{ERRORS.get(rc, rc)}] (n={n}, dim={d}, centroids {tuple(centroids.shape)})")
        if side is not None:
            side.synchronize()
        return sel.cpu().numpy()[:k].astype(np.int64)


def abs_histogram_f16(tensor, stream=None) -> np.ndarray:
    """unina_abs_histogram_f16: the |x| value-count table (uint32 [32768]) of a contiguous CUDA fp16 tensor, synchronous."""
    L = load_library()
    torch = _torch()
    assert tensor.is_cuda and tensor.dtype == torch.float16 and tensor.is_contiguous()
    with torch.cuda.device(tensor.device):
        out = torch.empty(_export.CALIB_BINS, dtype=torch.int32, device=tensor.device)
        rc = L.unina_abs_histogram_f16(tensor.data_ptr(), tensor.numel(), out.data_ptr(), _stream_ptr(stream))
        if rc:
            raise EngineError(f"unina_abs_histogram_f16 failed [{ERRORS.get(rc, rc)}] (n={tensor.numel()}, address {tensor.data_ptr():#x})")
        torch.cuda.synchronize(tensor.device)
        return out.cpu().numpy().view(np.uint32)


def calibrate_amax_device(sd: Dict[str, np.ndarray], graph: Optional[Graph], frames, device: int = 0,
                          percentile: Optional[float] = None, method: Optional[str] = None, specs=None):
    """calibrate_amax with the collection on the GPU: same arguments, same dict, float for float. Per frame the engine
    counts, for every fp16 activation buffer, how many elements carry each of the 32 768 |x| patterns (csrc/calib.hip, one
    launch behind the forward); only those tables cross to the host, where export.calibrate_counts folds them exactly as
    export.calibrate folds the tensors. method None / "max" WITH a percentile is not offered (ValueError; np.percentile
    needs the raw tensor: calibrate_amax)."""
    torch = _torch()
    if specs is None and method in (None, "max") and percentile is not None:
        raise ValueError('method "max" with a per-frame percentile needs the raw tensors: use calibrate_amax')
    eng = Engine.from_state_dict(sd, graph, device)
    eng.set_fusion(False)          # every internal buffer must be written: the tables cover them all
    try:
        names = eng.calib_buffer_names()

        def per_frame():
            for x in frames:
                yield eng.calib_counts(torch.from_numpy(np.ascontiguousarray(x)).cuda(device))
        if specs is not None:
            return _export.calibrate_counts_all(per_frame(), names, specs)
        return _export.calibrate_counts(per_frame(), names, percentile, method)
    finally:
        eng.close()


def calibrate_amax(sd: Dict[str, np.ndarray], graph: Optional[Graph], frames, device: int = 0,
                   percentile: Optional[float] = None, method: Optional[str] = None, specs=None):
    """INT8 calibration on the GPU (the role of qat.py:171-220 `calibrate_model`, 30 batches in train.py:809): runs the
    fp16 engine over `frames` (iterable of [1,3,H,W] fp32 ndarrays) and records, per activation buffer, the
    (percentile of the) absolute maximum, or -- `method` = "entropy" | "mse" | "percentile" -- the range a |x| histogram over
    all frames selects (export.HistogramCalibrator: the reference's QuantDescriptor(calib_method="histogram"), qat.py:91-126).
    calibrate_amax_device above returns the same dict with the per-buffer collection on the GPU instead of read_buffer.
    Feed the result to from_state_dict(..., precision=INT8, amax=...)."""
    torch = _torch()
    b = _export.EngineBuilder(sd, graph)
    names = [n for (n, _h, _w, _c, dtype, _f, _s) in b.buffers if dtype == _export.BUF_F16]
    eng = Engine.from_state_dict(sd, graph, device)
    eng.set_fusion(False)          # every internal buffer must be written: the calibrator reads them all
    try:
        def per_frame():
            for x in frames:
                eng.forward(torch.from_numpy(np.ascontiguousarray(x)).cuda(device))
                yield {n: eng.read_buffer(n) for n in names}
        if specs is not None:                      # several range selections from one pass (tools/int8_drift.py)
            return _export.calibrate_all(per_frame(), specs)
        return _export.calibrate(per_frame(), percentile, method)
    finally:
        eng.close()


class DeviceEval:
    """unina_eval_*: detections scored against labels on the GPU (csrc/evalmatch.hip), one launch per image behind the frame
    that produced the records. `max_scores` / `max_rows`: capacity of the conformal-score and AP-row lists."""

    def __init__(self, num_classes: int, max_scores: int, max_rows: int, device: int = 0):
        self.L = load_library()
        self.device, self.num_classes, self.max_scores, self.max_rows = device, num_classes, max_scores, max_rows
        self.h = C.c_void_p()
        rc = self.L.unina_eval_create(device, num_classes, max_scores, max_rows, C.byref(self.h))
        if rc:
            raise EngineError(f"unina_eval_create failed [{ERRORS.get(rc, rc)}] (num_classes={num_classes})")
        self._labels = []      # label tensors of the updates in flight (kept until the next read / reset)

    def reset(self, stream=None) -> None:
        _raise_on(self.L.unina_eval_reset_async(self.h, _stream_ptr(stream)), "unina_eval_reset_async")

    def update(self, det_buf, labels, params: EvalParams, what: int, stream=None) -> None:
        """One image, asynchronous. det_buf: int32 CUDA tensor as infer_async's (word 0 = count, records from word 8);
        labels: [M,5] rows cls, xc, yc, w, h (ndarray: uploaded as float64; or a float64 CUDA tensor)."""
        torch = _torch()
        if not isinstance(labels, torch.Tensor):
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float64).reshape(-1, 5)).to(det_buf.device)
        assert labels.is_cuda and labels.dtype == torch.float64 and labels.is_contiguous()
        self._labels.append(labels)
        n = labels.shape[0]
        _raise_on(self.L.unina_eval_update_async(self.h, *det_buffer_ptrs(det_buf), labels.data_ptr() if n else None, n, C.byref(params),
                                                 what, _stream_ptr(stream)), f"unina_eval_update_async ({n} labels)")

    def read(self, stream=None):
        """Synchronises; returns (EvalResult, scores float64 [n], rows EVAL_ROW_DTYPE [m]) -- the lists as far as they fit."""
        res = EvalResult()
        scores = np.empty(self.max_scores, dtype=np.float64)
        rows = np.zeros(self.max_rows, dtype=EVAL_ROW_DTYPE)
        _raise_on(self.L.unina_eval_read(self.h, C.byref(res), scores.ctypes.data, scores.size, rows.ctypes.data, rows.size,
                                         _stream_ptr(stream)), "unina_eval_read")
        self._labels.clear()
        return res, scores[:min(res.n_scores, self.max_scores)].copy(), rows[:min(res.n_rows, self.max_rows)].copy()

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.unina_eval_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def preprocess_frame(frame: Frame, out, region=None, norm: Optional[NormParams] = None, stream=None):
    """unina_preprocess_frame: `region` (x, y, w, h; None: the whole frame) of a Frame -> the float32 CUDA tensor `out`
    [..., 3, H, W], tapped where the region has the output's size, resized otherwise. Asynchronous; returns `out`."""
    L = load_library()
    torch = _torch()
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape[-3] == 3
    if norm is None:
        norm = L.create_norm_params_imagenet()
    tile = None if region is None else C.byref(Tile(*map(int, region)))
    rc = L.unina_preprocess_frame(C.byref(frame), tile, out.data_ptr(), int(out.shape[-1]), int(out.shape[-2]), C.byref(norm),
                                  _stream_ptr(stream))
    if rc:
        raise EngineError(f"unina_preprocess_frame failed [{ERRORS.get(rc, rc)}]")
    return out


def preprocess_letterbox_frame(frame: Frame, out, pad_value: float = 114.0, norm: Optional[NormParams] = None, stream=None):
    """unina_preprocess_letterbox_frame: the whole Frame letterboxed into the float32 CUDA tensor `out` [..., 3, H, W]."""
    L = load_library()
    torch = _torch()
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape[-3] == 3
    if norm is None:
        norm = L.create_norm_params_imagenet()
    rc = L.unina_preprocess_letterbox_frame(C.byref(frame), out.data_ptr(), int(out.shape[-1]), int(out.shape[-2]), pad_value,
                                            C.byref(norm), _stream_ptr(stream))
    if rc:
        raise EngineError(f"unina_preprocess_letterbox_frame failed [{ERRORS.get(rc, rc)}]")
    return out


def letterbox_geometry(src_w: int, src_h: int, dst_w: int, dst_h: int):
    """unina_letterbox_geometry through the C ABI (host only, no device): (new_w, new_h, left, top)."""
    L = load_library()
    box = Letterbox()
    rc = L.unina_letterbox_geometry(src_w, src_h, dst_w, dst_h, C.byref(box))
    if rc:
        raise EngineError(f"unina_letterbox_geometry failed [{ERRORS.get(-rc, -rc)}] ({src_w} x {src_h} into {dst_w} x {dst_h})")
    return box.new_w, box.new_h, box.left, box.top


def slice_tiles(frame_w: int, frame_h: int, slice_w: int = 640, slice_h: int = 640, overlap_w: float = 0.2,
                overlap_h: float = 0.2, cap: Optional[int] = None):
    """unina_slice_tiles through the C ABI (host only, no device): (count, [(x, y, w, h)] -- at most `cap` of them)."""
    L = load_library()
    n = L.unina_slice_tiles(frame_w, frame_h, slice_w, slice_h, overlap_w, overlap_h, None, 0)
    if n < 0:
        raise EngineError(f"unina_slice_tiles failed [{ERRORS.get(-n, -n)}]")
    cap = n if cap is None else cap
    arr = (Tile * max(cap, 1))()
    n = L.unina_slice_tiles(frame_w, frame_h, slice_w, slice_h, overlap_w, overlap_h, arr, cap)
    return n, [(t.x, t.y, t.w, t.h) for t in arr[:min(n, cap)]]
