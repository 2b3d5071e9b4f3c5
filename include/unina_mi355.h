/*
 * unina_mi355.h -- C ABI of libunina_mi355.so, the MI355X (gfx950) engine for the
 * UNINA-YOLO-DLA detector hot path: forward graph + decode/NMS.
 *
 * This is the drop-in boundary. Every entry point names the reference interface it
 * replaces (paths relative to /root/reference/unina_yolo_dla/):
 *
 *   engine object ......... class TensorRTEngine          ros2_ws/src/perception/src/perception_node.cpp:223-351
 *   post-process C API .... extern "C" block              ros2_ws/src/perception/include/gpu_postprocess.h:36-84
 *   detection record ...... struct GpuDetection           ros2_ws/src/perception/include/gpu_postprocess.h:27-33
 *   tensor names .......... "images", "p2_cls".."p4_reg"  perception_node.cpp:612-618, model.py:382-383
 *
 * Conventions: plain C, no exceptions cross the boundary, 0 == success everywhere.
 * Device pointers are ordinary HIP device pointers; streams are hipStream_t.
 * A handle may be used by one thread at a time; distinct handles (e.g. one per GPU,
 * or two on one GPU to keep two frames in flight) are fully independent.
 */
#ifndef UNINA_MI355_H
#define UNINA_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef UNINA_NO_HIP_HEADERS /* for pure-C consumers / ctypes documentation builds */
typedef struct ihipStream_t *hipStream_t;
typedef int hipError_t;
#else
#include <hip/hip_runtime_api.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MAX_DETECTIONS 1024 /* gpu_postprocess.h:24 */

/* 32-byte record, identical layout to the reference (gpu_postprocess.h:27-33).
 * Coordinates are xyxy in input-tensor pixels. */
#if defined(__cplusplus)
struct alignas(32) GpuDetection {
#else
struct GpuDetection {
#endif
  float x1, y1, x2, y2;
  float confidence;
  int class_id;
  int valid; /* 1 = kept */
  int _pad;
};
typedef struct GpuDetection GpuDetection;

/* ------------------------------------------------------------------ error codes */
enum {
  UNINA_OK = 0,
  UNINA_ERR_IO = 1,          /* engine file unreadable                    */
  UNINA_ERR_FORMAT = 2,      /* bad magic / version / table               */
  UNINA_ERR_HIP = 3,         /* a HIP call failed (see unina_last_error)  */
  UNINA_ERR_ARG = 4,         /* null / misaligned / unknown tensor name   */
  UNINA_ERR_STATE = 5,       /* e.g. "images" not bound before enqueue    */
  UNINA_ERR_UNSUPPORTED = 6  /* layer shape the kernels do not cover      */
};

typedef struct unina_engine unina_engine_t;

/* ------------------------------------------------------------------ engine (TensorRTEngine role) */

/* Replaces TensorRTEngine::load(engine_path, logger, dla_core) (perception_node.cpp:228-259).
 * `path` is an engine file written by unina-yolo-dla_amd/export.py (folded weights + op table);
 * `device_id` plays the role of dla_core: which accelerator the handle lives on. */
int unina_load_engine(const char *path, int device_id, unina_engine_t **out);

/* Replaces TensorRTEngine::unload() / the destructor (perception_node.cpp:226,261-266). NULL is a no-op. */
void unina_unload_engine(unina_engine_t *e);

/* Replaces TensorRTEngine::getInputDimensions(w,h) (perception_node.cpp:297-325); also reports num_classes,
 * which the node hard-codes to 4 (perception_node.cpp:630-639). Any out pointer may be NULL. */
int unina_engine_input_dims(const unina_engine_t *e, int *width, int *height, int *num_classes);

/* Replaces setInputTensorAddress / setOutputTensorAddress (perception_node.cpp:268-276).
 * Names: "images" fp32 [1,3,H,W]; "p2_cls","p2_reg","p3_cls","p3_reg","p4_cls","p4_reg" fp32 planar
 * [1,C,H/s,W/s], s = 4/8/16. Pointers must be 16-byte aligned device pointers owned by the caller.
 * Outputs left unbound are written to engine-owned buffers (see unina_tensor_address). */
int unina_set_tensor_address(unina_engine_t *e, const char *name, void *device_ptr);

/* Current device address + element count of a named tensor (engine-owned default or the bound one). */
int unina_tensor_address(const unina_engine_t *e, const char *name, void **device_ptr, size_t *num_floats);

/* Replaces TensorRTEngine::enqueueV3(stream) (perception_node.cpp:278-282, call site :621):
 * runs the forward graph asynchronously on `stream`, producing the six raw head tensors. */
int unina_enqueue(unina_engine_t *e, hipStream_t stream);

/* The fused path the north star names: forward + sigmoid/argmax/threshold + TLBR decode + conformal dilation
 * + sort + class-aware NMS + compaction, all on the GPU, no host round-trip in between. It replaces
 * perception_node.cpp:612-656 (bind, enqueueV3, reset_detection_counter, 3 x decode_yolo_head,
 * get_detection_count, run_gpu_nms, copy_valid_detections_to_host).
 *
 *   d_images_nchw : device, fp32 [1,3,H,W] (same as binding "images"); NULL = keep the current binding
 *   out           : HOST buffer for up to MAX_DETECTIONS records (sorted by confidence, valid=1)
 *   out_count     : HOST int
 * Synchronous: returns after the records are in `out`. The post-process writes the count and the kept records straight
 * into a pinned host block and then a completion word (system-scope release); the call spins on that word, so the
 * latency path has neither a D2H copy command nor a stream synchronisation. `stream` may still hold the tail of the
 * frame's launch for a few microseconds after the call returns (work submitted to it later is ordered as usual).
 * UNINA_HOST_RESULT=0 / UNINA_HOST_POLL=0 restore the device buffer + copy / hipStreamSynchronize.
 *
 * NOTE on the six head tensors ("p2_cls" ... "p4_reg"): unina_infer / unina_infer_async / unina_infer_bgra compute the heads'
 * output convs INSIDE the decode launch and do NOT write the fp32 planes of those heads (P3 / P4 always; P2 too unless its
 * head runs as one fused kernel). After these calls unina_tensor_address / unina_debug_read_buffer of such a plane return
 * whatever an earlier unina_enqueue left there (or zeros). A caller that wants the raw heads (the TensorRT-shaped path of
 * perception_node.cpp:612-640) calls unina_enqueue, which always writes all six; UNINA_POST_FOLD=0 makes the frame path
 * write them too. */
int unina_infer(unina_engine_t *e, const float *d_images_nchw, float conf_threshold, float iou_threshold,
                float conformal_q, GpuDetection *out, int *out_count, hipStream_t stream);

/* Normalisation constants of the pre-process (pre-process C API below; also taken by unina_infer_bgra). */
typedef struct {
  float mean_r, mean_g, mean_b;
  float std_r, std_g, std_b;
} NormParams; /* cuda_preprocess.h:38-45 */

/* `n_calls` serial unina_infer calls over a ring of `n_ring` device frames, each timed on the host's steady clock from entry to
 * return (records copied out): the latency a C / C++ caller sees, free of a binding layer's per-call cost. lat_us[n_calls]. */
int unina_serial_latency(unina_engine_t *e, const float *const *d_frames, int n_ring, int n_calls, float conf_threshold,
                         float iou_threshold, float conformal_q, double *lat_us, hipStream_t stream);

/* Camera frame -> detections in one call: unina_infer with the pre-process of cuda_preprocess.h:50-112
 * (preprocess_bgra when the frame has the network's size, preprocess_bgra_resize otherwise) computed inside the
 * stem kernel, i.e. perception_node.cpp:601-656 (preprocess_bgra_resize ... copy_valid_detections_to_host) as ONE
 * graph launch without the fp32 tensor in between. Identical results to the two-step form.
 *   d_bgra : device, pitched BGRA8 (src_pitch bytes per row, multiple of 4, >= 4 * src_width) */
int unina_infer_bgra(unina_engine_t *e, const uint8_t *d_bgra, int src_width, int src_height, int src_pitch,
                     const NormParams *norm, float conf_threshold, float iou_threshold, float conformal_q,
                     GpuDetection *out, int *out_count, hipStream_t stream);

/* The same for an NV12 camera frame (GpuBufferHandle::format 1; 1.5 B/px in): d_y the luma plane (y_pitch bytes per row), d_uv the
 * interleaved U,V plane ((src_height + 1) / 2 rows of uv_pitch bytes). The arithmetic, all fp32, each operation rounded once:
 *   tap at camera pixel (X, Y), cuda_preprocess.cu:224-241:
 *     Yv = y[Y * y_pitch + X];  U = uv[(Y / 2) * uv_pitch + (X / 2) * 2] - 128.0f;  V = uv[... + 1] - 128.0f
 *     r = Yv + 1.402f * V;  g = Yv - 0.344136f * U - 0.714136f * V;  b = Yv + 1.772f * U
 *     each clamped with fmaxf(0, fminf(255, .)); the clamped values stay floats, they are never rounded to u8
 *   a frame (or tile) of the network's size: the tap, then ((v / 255.0f) - mean) / std -- preprocess_nv12
 *   any other size: the REFERENCE HAS NO NV12 RESIZE; this one is defined here. Coordinates, clamps and weights are those of
 *     preprocess_bgra_resize (cuda_preprocess.cu:155-178) unchanged, the four taps are the clamped float r, g, b above instead of
 *     u8 channels, blended per channel as w00 * t00 + w01 * t01 + w10 * t10 + w11 * t11 left to right, then normalised --
 *     unina_preprocess_nv12_resize below. On a grey frame (every chroma byte 128) it equals the BGRA resize of B = G = R = Y.
 * Identical results to the two-step form (preprocess_nv12 / unina_preprocess_nv12_resize, then unina_infer). Nothing is asked
 * of the alignment of the planes or pitches (aligned ones are read with wider loads). UNINA_ERR_ARG: a null plane, a
 * non-positive size, y_pitch < src_width, uv_pitch < src_width or < 2 * ((src_width + 1) / 2) (the last chroma pair of an
 * odd-width row is read whole). */
int unina_infer_nv12(unina_engine_t *e, const uint8_t *d_y, const uint8_t *d_uv, int src_width, int src_height, int y_pitch,
                     int uv_pitch, const NormParams *norm, float conf_threshold, float iou_threshold, float conformal_q,
                     GpuDetection *out, int *out_count, hipStream_t stream);

/* ------------------------------------------------------------------ letterboxed camera frames
 * unina_infer_bgra / unina_infer_nv12 STRETCH the frame to the network input: 1920 x 1080 into 640 x 640 squeezes every object
 * 1.78 x narrower than the model was trained on. These calls keep the aspect ratio instead: the frame is resized into an inner
 * rectangle of the network input, the rest is padded, and the boxes can come back in the camera's own pixels -- all inside the
 * frame graph (the stem kernel computes the letterboxed pixel, the post-process maps the kept records where it writes them).
 * Everything below is THIS PROJECT'S definition. Parity with Ultralytics' LetterBox / cv2.resize is unpinned: cv2 blends u8 in
 * fixed point and rounds to u8, here the blended values stay floats.
 *
 * Geometry (unina_letterbox_geometry; host only, no engine, no device -- unina_slice_tiles' role), all in double:
 *   r = min((double)dst_h / src_h, (double)dst_w / src_w)
 *   new_w = round(src_w * r), new_h = round(src_h * r), each at least 1
 *   left = round((dst_w - new_w) / 2.0 - 0.1), top = round((dst_h - new_h) / 2.0 - 0.1); right / bottom padding: what remains
 *   round = round-half-to-even (Python's round, nearbyint in the default rounding mode): 5 x 128 into 64 x 64 has r = 0.5 and
 *   new_w = round(2.5) = 2. 1920 x 1080 into 640 x 640: 640 x 360 at (0, 140). Returns 0, or -UNINA_ERR_ARG (non-positive size, NULL).
 * Network-input pixel (x, y):
 *   inside the inner rectangle (left <= x < left + new_w, top <= y < top + new_h):
 *     (new_w, new_h) == (src_w, src_h): the plain tap at (x - left, y - top), as preprocess_bgra / preprocess_nv12;
 *     otherwise preprocess_bgra_resize / unina_preprocess_nv12_resize evaluated for a destination of new_w x new_h at
 *     (x - left, y - top): scale_x = (float)src_w / (float)new_w, coordinates, clamps, weights and the left-to-right blend unchanged
 *   outside: r = g = b = (float)pad_value (Ultralytics pads with 114)
 *   both then ((v / 255.0f) - mean) / std. So the inner rectangle of a letterboxed tensor equals the resize of the frame to
 *   new_w x new_h bit for bit, and the conv's zero padding outside the network input stays zero.
 * Box map, map_boxes: 0 = records in network pixels, as unina_infer; 1 = camera pixels. Decode, conformal dilation and NMS always
 * run in network pixels; only the KEPT records are mapped, both corners, fp32, each step rounded separately:
 *   X = (x - (float)left) * ((float)src_w / (float)new_w)      Y = (y - (float)top) * ((float)src_h / (float)new_h)
 * NOTHING IS CLAMPED to the frame (the engine clamps nowhere): a box over the padding maps to coordinates outside the camera. */
typedef struct { int new_w, new_h, left, top; } unina_letterbox;
int unina_letterbox_geometry(int src_w, int src_h, int dst_w, int dst_h, unina_letterbox *out);

/* unina_infer_bgra / unina_infer_nv12 with the letterbox above in place of the stretch: same arguments and argument checks, plus
 * pad_value and map_boxes (0 / 1, anything else UNINA_ERR_ARG). Synchronous, delivered as unina_infer delivers (pinned block +
 * completion word: no D2H copy, no stream synchronisation, no extra launch for the map). A refused call enqueues nothing, and
 * no call leaves anything behind in the handle: the frame, the letterbox and the map flag travel with the call. With map_boxes = 0 the results equal
 * unina_preprocess_letterbox_* + unina_infer bit for bit; a frame of the network's size is unina_infer_bgra / unina_infer_nv12. */
int unina_infer_letterbox_bgra(unina_engine_t *e, const uint8_t *d_bgra, int src_width, int src_height, int src_pitch,
                               const NormParams *norm, float conf_threshold, float iou_threshold, float conformal_q,
                               float pad_value, int map_boxes, GpuDetection *out, int *out_count, hipStream_t stream);
int unina_infer_letterbox_nv12(unina_engine_t *e, const uint8_t *d_y, const uint8_t *d_uv, int src_width, int src_height,
                               int y_pitch, int uv_pitch, const NormParams *norm, float conf_threshold, float iou_threshold,
                               float conformal_q, float pad_value, int map_boxes, GpuDetection *out, int *out_count,
                               hipStream_t stream);
/* The same, results on the device (d_out: MAX_DETECTIONS records, 16-byte aligned; d_out_count: one int), nothing synchronised. */
int unina_infer_letterbox_bgra_async(unina_engine_t *e, const uint8_t *d_bgra, int src_width, int src_height, int src_pitch,
                                     const NormParams *norm, float conf_threshold, float iou_threshold, float conformal_q,
                                     float pad_value, int map_boxes, GpuDetection *d_out, int *d_out_count, hipStream_t stream);
int unina_infer_letterbox_nv12_async(unina_engine_t *e, const uint8_t *d_y, const uint8_t *d_uv, int src_width, int src_height,
                                     int y_pitch, int uv_pitch, const NormParams *norm, float conf_threshold, float iou_threshold,
                                     float conformal_q, float pad_value, int map_boxes, GpuDetection *d_out, int *d_out_count,
                                     hipStream_t stream);

/* Asynchronous variant: results stay on the device (d_out: MAX_DETECTIONS records, d_out_count: one int);
 * nothing is synchronised. Used to pipeline frames and to feed the RCCL gather without touching the host. */
int unina_infer_async(unina_engine_t *e, const float *d_images_nchw, float conf_threshold, float iou_threshold,
                      float conformal_q, GpuDetection *d_out, int *d_out_count, hipStream_t stream);

/* Decode + NMS only, on head tensors already on the device (the six bound/owned outputs). */
int unina_postprocess_async(unina_engine_t *e, float conf_threshold, float iou_threshold, float conformal_q,
                            GpuDetection *d_out, int *d_out_count, hipStream_t stream);

/* ------------------------------------------------------------------ sliced inference (auto_labeler.py:124-199, 255-271)
 * A high-resolution camera frame resized whole to the network input loses its small objects (1920 px -> 640 px: a 12 px cone
 * arrives as 4 px). The reference's answer is SAHI_Wrapper: network-sized tiles with 20 % overlap, the detector on each, the
 * boxes shifted back (map_boxes_to_global) and one global per-class NMS at 0.45. Here: one frame graph per tile, enqueued back
 * to back into engine-owned device slots -- a tile is a pointer offset into the camera frame, nothing is copied -- and one merge
 * on the GPU, all on one stream with no host round-trip in between. Boxes come back in CAMERA-FRAME pixels.
 *
 * Merge semantics: the engine's own on the union of the tiles' records mapped to the frame -- stable sort
 * by confidence descending, ties by enumeration index t * MAX_DETECTIONS + i (tile-major), the MAX_DETECTIONS best kept,
 * sequential greedy class-aware NMS at IoU > merge_iou (+1e-6f denominator), only a strictly lower confidence is suppressed;
 * output compact and sorted, valid = 1, _pad = 0. Mapping, fp32, each step rounded: X = x * ((float)w / (float)net_w) + (float)x0
 * (for a network-sized tile the scale is 1.0f and the map is the reference's offset add). Confidences must lie in [0, 1]. */
#define UNINA_MAX_TILES 64
typedef struct { int x, y, w, h; } unina_tile;   /* region of the camera frame, pixels */

/* Host only, no engine, no device: the slices of SAHI_Wrapper.get_slices (auto_labeler.py:132-154), in its order, with exact
 * repeats dropped (first occurrence kept): the reference yields the last row / column twice where the stride does not divide
 * the frame (h = 1080, slice 640, stride 512: y = 0, 440, 440), and since equal confidences never suppress each other a repeated
 * tile would double every one of its detections. stride = (int)(slice * (1 - overlap)) in double, as the reference computes it.
 * A frame no larger than the slice in both dimensions is one tile, the whole frame; one smaller in one dimension gives
 * non-square tiles. Returns the number of tiles and writes at most `cap` of them (out may be NULL when cap is 0);
 * < 0: -error code (non-positive sizes, a stride below 1). */
int unina_slice_tiles(int frame_w, int frame_h, int slice_w, int slice_h, float overlap_w, float overlap_h,
                      unina_tile *out, int cap);

/* Camera frame -> merged detections in frame pixels. Synchronous; host `out` / `out_count` as unina_infer (delivered through the
 * same pinned block and completion word). Per tile: unina_infer_bgra's frame on d_bgra + y * pitch + 4 * x with the tile's
 * width and height (a tile of any size is resized to the network input), thresholds conf / iou / conformal_q as there; then the
 * merge at merge_iou. d_bgra / src_pitch: as unina_infer_bgra. UNINA_ERR_ARG: null pointer, n_tiles outside
 * 1..UNINA_MAX_TILES, a tile that is empty or not inside the frame, bad pitch. */
int unina_infer_tiled_bgra(unina_engine_t *e, const uint8_t *d_bgra, int src_width, int src_height, int src_pitch,
                           const unina_tile *tiles, int n_tiles, const NormParams *norm, float conf_threshold,
                           float iou_threshold, float conformal_q, float merge_iou, GpuDetection *out, int *out_count,
                           hipStream_t stream);
/* The same, results on the device (d_out: MAX_DETECTIONS records, d_out_count: one int), nothing synchronised
 * (unina_infer_async's role). */
int unina_infer_tiled_bgra_async(unina_engine_t *e, const uint8_t *d_bgra, int src_width, int src_height, int src_pitch,
                                 const unina_tile *tiles, int n_tiles, const NormParams *norm, float conf_threshold,
                                 float iou_threshold, float conformal_q, float merge_iou, GpuDetection *d_out,
                                 int *d_out_count, hipStream_t stream);
/* The NV12 pair: the same tiles, slots and merge on an NV12 frame (planes and pitches as unina_infer_nv12). A tile (x, y, w, h)
 * is pre-processed as a frame of w x h whose tap (xs, ys) is read at camera pixel (x + xs, y + ys): source coordinates are
 * tile-local, and the tile's origin enters the chroma index ((y + ys) / 2, (x + xs) / 2) -- so an NV12 tile is not a pointer
 * offset, the origin travels to the kernel, and it may be odd. UNINA_ERR_ARG as the BGRA pair and unina_infer_nv12. */
int unina_infer_tiled_nv12(unina_engine_t *e, const uint8_t *d_y, const uint8_t *d_uv, int src_width, int src_height,
                           int y_pitch, int uv_pitch, const unina_tile *tiles, int n_tiles, const NormParams *norm,
                           float conf_threshold, float iou_threshold, float conformal_q, float merge_iou, GpuDetection *out,
                           int *out_count, hipStream_t stream);
int unina_infer_tiled_nv12_async(unina_engine_t *e, const uint8_t *d_y, const uint8_t *d_uv, int src_width, int src_height,
                                 int y_pitch, int uv_pitch, const unina_tile *tiles, int n_tiles, const NormParams *norm,
                                 float conf_threshold, float iou_threshold, float conformal_q, float merge_iou,
                                 GpuDetection *d_out, int *d_out_count, hipStream_t stream);
/* The merge alone, on slots already on the device: d_slots[n_tiles][MAX_DETECTIONS] (16-byte aligned), d_counts[n_tiles]
 * (what unina_postprocess_async is to unina_infer_async). Only a tile's x, y, w, h enter (offset and scale). It uses the
 * handle's post-process workspace, so it is ordered like any other call on the handle: behind the previous one on `stream`. */
int unina_merge_tiles_async(unina_engine_t *e, const GpuDetection *d_slots, const int *d_counts, const unina_tile *tiles,
                            int n_tiles, float merge_iou, GpuDetection *d_out, int *d_out_count, hipStream_t stream);

/* ------------------------------------------------------------------ frame descriptor: every camera format through one call
 * The transport message declares four formats (GpuBufferPtr.msg:24-27: 0 BGRA, 1 NV12, 2 RGB, 3 RGBA) and the node copies the
 * code into GpuBufferHandle::format (perception_node.cpp:362, 558) -- then calls preprocess_bgra_resize whatever it says
 * (:601-604). Here the code travels with the frame: one descriptor, one family of calls, and the formats cameras deliver where no
 * converter sits in front of the node (packed 4:2:2 from GMSL / USB cameras, raw 8-bit Bayer from machine-vision cameras).
 * Formats 0 and 1 through these calls ARE unina_infer_bgra / unina_infer_nv12 and their relatives: the same kernel paths, the
 * same bytes. All arithmetic below is fp32, each operation rounded once, never contracted; tap values stay floats, they are never
 * rounded to u8. Frame pixel (X, Y) is pixel (xs, ys) of a region (the whole frame, or a tile) whose origin is (x0, y0).
 *   RGB / RGBA   r, g, b = bytes 0, 1, 2 of the 3- / 4-byte pixel at plane[0] + Y * pitch + 3 X (4 X), converted to float;
 *                everything else as BGRA. A tile is a pointer offset (3 * x for RGB, hence nothing is asked of its alignment).
 *   YUYV / UYVY  pair = plane[0] + Y * pitch + 4 * (X / 2)
 *                YUYV: Yv = pair[2 * (X & 1)],     U = pair[1] - 128.0f, V = pair[3] - 128.0f
 *                UYVY: Yv = pair[1 + 2 * (X & 1)], U = pair[0] - 128.0f, V = pair[2] - 128.0f
 *                then the BT.601 conversion and clamp of unina_infer_nv12 above, unchanged (cuda_preprocess.cu:229-241). The
 *                origin enters the pair index and may be odd: as for NV12 a tile is not a pointer offset.
 *   Bayer        8-bit mosaic, BILINEAR demosaic. THIS PROJECT'S definition, as the letterbox is: parity with cv2.cvtColor's
 *                demosaic is unpinned (cv2 rounds to u8, here the interpolated values stay floats). The pattern names the colours
 *                of (X & 1, Y & 1) = (0,0), (1,0), (0,1), (1,1): RGGB is R G / G B. raw(X, Y) reads the FRAME with reflect-101 at
 *                the frame's borders (-1 -> 1, W -> W - 2), which keeps the colour phase; a tile reads its neighbours from the
 *                frame, not from a crop, so its pixels are the full-frame demosaic's pixels. At a site its own colour is raw(X, Y).
 *                R or B site: G = (raw(X,Y-1) + raw(X-1,Y) + raw(X+1,Y) + raw(X,Y+1)) * 0.25f
 *                             opposite colour = (raw(X-1,Y-1) + raw(X+1,Y-1) + raw(X-1,Y+1) + raw(X+1,Y+1)) * 0.25f
 *                G site:      the colour on its row = (raw(X-1,Y) + raw(X+1,Y)) * 0.5f
 *                             the colour on its column = (raw(X,Y-1) + raw(X,Y+1)) * 0.5f
 *                Every sum is an integer of at most 1020 and every factor a power of two: the values are exact.
 *   geometry     a region of the destination's size: the tap above, then ((v / 255.0f) - mean) / std. Any other size: the
 *                coordinates, clamps, weights and left-to-right blend of preprocess_bgra_resize on four float taps, as the NV12
 *                resize. Letterbox: exactly as for BGRA / NV12 (unina_letterbox_geometry above).
 * Frame geometry, UNINA_ERR_ARG otherwise (pitch = pitch[0]; sizes positive; plane[0] not NULL):
 *   BGRA / RGBA  pitch >= 4 * width, pitch and plane[0] multiples of 4        NV12   as unina_infer_nv12 (plane[1], pitch[1]: chroma)
 *   RGB          pitch >= 3 * width                                           Bayer  pitch >= width, width >= 2, height >= 2,
 *                                                                                    pitch * height < 4 GiB
 *   YUYV / UYVY  pitch >= 4 * ((width + 1) / 2) (the last pair of an odd-width row is read whole)
 * Nothing else is asked of the alignment (aligned 4:2:2 and Bayer frames are read with wider loads). A format code outside 0..9
 * is UNINA_ERR_ARG. */
typedef enum { UNINA_FMT_BGRA = 0, UNINA_FMT_NV12 = 1, UNINA_FMT_RGB = 2, UNINA_FMT_RGBA = 3,   /* GpuBufferPtr.msg:24-27 */
               UNINA_FMT_YUYV = 4, UNINA_FMT_UYVY = 5,
               UNINA_FMT_BAYER_RGGB = 6, UNINA_FMT_BAYER_BGGR = 7, UNINA_FMT_BAYER_GRBG = 8, UNINA_FMT_BAYER_GBRG = 9 } unina_pixel_format;
typedef struct { int format, width, height; const uint8_t *plane[2]; int pitch[2]; } unina_frame;   /* plane[1] / pitch[1]: NV12 chroma, else NULL / 0 */

/* unina_infer_bgra / unina_infer_nv12 for any format: semantics, delivery and the rest of the argument checks are theirs. A
 * refused call enqueues nothing and leaves the handle intact. Identical results to unina_preprocess_frame + unina_infer. */
int unina_infer_frame(unina_engine_t *e, const unina_frame *frame, const NormParams *norm, float conf_threshold,
                      float iou_threshold, float conformal_q, GpuDetection *out, int *out_count, hipStream_t stream);
int unina_infer_frame_async(unina_engine_t *e, const unina_frame *frame, const NormParams *norm, float conf_threshold,
                            float iou_threshold, float conformal_q, GpuDetection *d_out, int *d_out_count, hipStream_t stream);
/* unina_infer_letterbox_bgra / _nv12 [_async] for any format (pad_value, map_boxes as there). */
int unina_infer_letterbox_frame(unina_engine_t *e, const unina_frame *frame, const NormParams *norm, float conf_threshold,
                                float iou_threshold, float conformal_q, float pad_value, int map_boxes, GpuDetection *out,
                                int *out_count, hipStream_t stream);
int unina_infer_letterbox_frame_async(unina_engine_t *e, const unina_frame *frame, const NormParams *norm, float conf_threshold,
                                      float iou_threshold, float conformal_q, float pad_value, int map_boxes,
                                      GpuDetection *d_out, int *d_out_count, hipStream_t stream);
/* unina_infer_tiled_bgra / _nv12 [_async] for any format: the same tiles, slots and merge. BGRA, RGB and RGBA tiles are pointer
 * offsets; for the other formats the tile's origin travels to the kernel (and may be odd). */
int unina_infer_tiled_frame(unina_engine_t *e, const unina_frame *frame, const unina_tile *tiles, int n_tiles,
                            const NormParams *norm, float conf_threshold, float iou_threshold, float conformal_q,
                            float merge_iou, GpuDetection *out, int *out_count, hipStream_t stream);
int unina_infer_tiled_frame_async(unina_engine_t *e, const unina_frame *frame, const unina_tile *tiles, int n_tiles,
                                  const NormParams *norm, float conf_threshold, float iou_threshold, float conformal_q,
                                  float merge_iou, GpuDetection *d_out, int *d_out_count, hipStream_t stream);

/* ------------------------------------------------------------------ data mining (active_learning.py, mine_data.py)
 * The reference's third consumer of the forward graph: the active-learning loop pushes an unlabeled image set through the
 * detector and keeps, per image, a difficulty score and an embedding, then picks a diverse subset. These calls run BEHIND the
 * raw-head forward (unina_enqueue's launch sequence); the frame path (unina_infer*) is untouched by them.
 *
 * scores8 (UNINA_MINE_SCORES floats), p = 1/(1+exp(-logit)) over the three cls planes:
 *   [0..2] per level P2,P3,P4: max over classes and cells of -(p*log(p+1e-10) + (1-p)*log(1-p+1e-10))   active_learning.py:292-294
 *   [3..5] per level: max over cells of 1 - |max_c p_c - 0.5| * 2                                        active_learning.py:298-301
 *   [6] = max of [0..2]: the image's score in mode "entropy"; [7] = max of [3..5]: mode "loc_var"        active_learning.py:303
 * Every max is numpy's / torch's: it keeps a NaN. A level that holds a NaN logit reports NaN in both of its scores, and so do
 * [6] and [7]; the other levels are untouched. +-inf and saturating logits give finite scores (p = 0 or 1: entropy and loc_var 0).
 * embedding: mean over H, W of the backbone's P4 map before SPPF (features[2], the output of backbone.stage3_c3k2;
 * adaptive_avg_pool2d, active_learning.py:57-60,90-91), fp32 accumulation in a fixed order: two runs give identical bits.
 * Graph (B) engines (qat.py models: no .backbone) score but do not embed: UNINA_ERR_UNSUPPORTED. */
#define UNINA_MINE_SCORES 8

/* Length of the embedding (channels of the pooled map: 8 * base_channels of the model); < 0: -error code. */
int unina_embedding_dim(const unina_engine_t *e);

/* One iteration of the loops at active_learning.py:52-94 and :255-303 for one image: forward (all six head planes written,
 * as unina_enqueue) + scores + pooled embedding, enqueued on `stream`; nothing is synchronised.
 *   d_images_nchw : as unina_infer; NULL = keep the current binding
 *   d_scores8     : device, UNINA_MINE_SCORES floats      d_embed : device, unina_embedding_dim floats, or NULL (scores only)
 * Both may be rows of caller-owned [N,8] / [N,D] matrices, so the embeddings stay on the device for unina_kcenter. */
int unina_mine_async(unina_engine_t *e, const float *d_images_nchw, float *d_scores8, float *d_embed, hipStream_t stream);

/* The same with the results in HOST memory; synchronous (`.item()` / `.cpu().numpy()`, active_learning.py:93,294,301). */
int unina_mine(unina_engine_t *e, const float *d_images_nchw, float *scores8, float *embed, hipStream_t stream);

/* Scores only, from the six head tensors currently bound / owned (active_learning.py:276-303 on given outputs): what
 * unina_postprocess_async is to unina_infer_async. */
int unina_mine_heads_async(unina_engine_t *e, float *d_scores8, hipStream_t stream);

/* K-center greedy (coreset_selection_kcenter, active_learning.py:139-161) on device data; no engine handle.
 *   d_embeddings : device, fp32 [n, dim] row-major, 16-byte aligned      d_selected : device, k ints (selection order)
 *   first_index  : the reference's random start (np.random.randint(n), :140)
 *   d_min_dist   : device, n floats of workspace, or NULL: the call allocates it and then returns only after the selection
 *                  has finished (it frees the workspace). With a workspace nothing is synchronised.
 * Every step measures sqrt(sum (a-b)^2) to the row chosen last, keeps the running minimum, forces chosen rows to -1 and takes
 * the arg-max with the lowest index winning ties (numpy's argmax); the next step reads the chosen index from device memory,
 * so the k-1 steps run without a host round-trip. UNINA_ERR_ARG: null / misaligned pointer, k > n, first_index outside [0, n). */
int unina_kcenter(const float *d_embeddings, int n, int dim, int k, int first_index, int *d_selected, float *d_min_dist,
                  hipStream_t stream);

/* K-means coreset (coreset_selection_kmeans, active_learning.py:166-211) on device data; no engine handle. The reference
 * fits scikit-learn's MiniBatchKMeans, whose trajectory and RNG stream cannot be reproduced; the clustering here is FULL-BATCH
 * LLOYD by this build's own specification, the selection (unina_nearest_rows) is the reference's loop line for line.
 * One iteration = |c_j|^2 -> assign -> update -> inertia:
 *   assign  : label[i] = argmin_j |c_j|^2 - 2 <x_i, c_j>, the dot products on the f32-input MFMA (a d-ordered fp32 fma
 *             chain); the LOWEST index wins exact ties.
 *   update  : c_j = (sum of its member rows in ascending row index, fp32) / count_j; a cluster WITHOUT members keeps its
 *             previous centroid.
 *   inertia : sum_i sum_d (x_id - c_{label_i,d})^2 with the updated centroids, in double, fixed order -> history[iteration].
 * All max_iter iterations are enqueued by the call, no host round-trip: an iteration whose assignment changes no label is
 * completed and sets a device flag that makes every kernel behind it return at once (labels are compared from the call's
 * second iteration on, so a call executes at least two iterations before it can report convergence, max_iter permitting).
 * Fixed reduction orders, no float atomics: two runs give identical bytes, and one call of max_iter = T gives the bytes of T
 * chained calls of max_iter = 1.
 *   d_embeddings : device, fp32 [n, dim] row-major, 16-byte aligned, dim % 4 == 0
 *   d_init_rows  : device, k row indices: the start centroids are those rows; NULL: d_centroids holds the start
 *   d_centroids  : device, fp32 [k, dim], 16-byte aligned, in/out        d_labels : device, n ints, out
 *   d_inertia_history : device, max_iter doubles or NULL; entries of iterations that were not executed are NaN
 *   d_iters      : device, one int: iterations executed, bit 30 (UNINA_KMEANS_CONVERGED) set when converged
 *   d_workspace  : device, unina_kmeans_workspace_bytes(n, dim, k) bytes, 16-byte aligned; or NULL: the call allocates it and
 *                  then returns only when the loop has finished. With a workspace nothing is synchronised.
 * UNINA_ERR_ARG: null / misaligned pointer, dim % 4 != 0, k < 1, k > n, max_iter < 1 (unina_kmeans_workspace_bytes: 0).
 * An init row outside [0, n) is found ON THE DEVICE (the indices live there): the call returns UNINA_OK, *d_iters becomes -1
 * and centroids, labels and history are left untouched.
 * NON-FINITE VALUES are not validated; they follow IEEE arithmetic and one rule. The arg-min is a running minimum that
 * starts at (+inf, index 0) and that only a strictly smaller score replaces, so a NaN score never wins, and a row all of
 * whose scores are NaN or +inf takes label 0. (A row with a NaN channel therefore joins cluster 0 in the first iteration and
 * makes that centroid NaN; from the second iteration on no other row can choose it. The inertia of such a run is NaN.)
 * mining.kmeans_numpy follows the same rule. */
#define UNINA_KMEANS_CONVERGED (1 << 30)
size_t unina_kmeans_workspace_bytes(int n, int dim, int k);
int unina_kmeans(const float *d_embeddings, int n, int dim, int k, const int *d_init_rows, int max_iter, float *d_centroids,
                 int *d_labels, double *d_inertia_history, int *d_iters, void *d_workspace, hipStream_t stream);
/* The selection loop (active_learning.py:203-209): for each of the k centroids IN ORDER the row with the smallest
 * sqrt(sum (a-b)^2) (unina_kcenter's direct form) among the rows not chosen by an earlier centroid, the lowest index winning
 * ties (numpy's argmin); the next step reads the chosen index from device memory, so the k steps run without a host
 * round-trip.
 *   d_selected  : device, k ints (one row per centroid, in centroid order)
 *   d_workspace : device, n floats, or NULL: allocated by the call, which then returns only when finished
 * UNINA_ERR_ARG: null / misaligned pointer (16 bytes for the two matrices), dim % 4 != 0, k < 1, k > n. */
int unina_nearest_rows(const float *d_embeddings, int n, int dim, const float *d_centroids, int k, int *d_selected,
                       float *d_workspace, hipStream_t stream);

/* ------------------------------------------------------------------ INT8 calibration (qat.py:171-220, train.py:809)
 * The collection half of the reference's calibrate_model, on the device. An fp16 tensor has at most 32 768 distinct |x| (the
 * sign bit drops out, 15 bits remain), so a table "how many elements carry each 15-bit pattern" is a LOSSLESS summary of it for
 * everything a calibrator does with |x|: export.HistogramCalibrator.collect_counts folds a frame's table into bit-identical
 * histograms, edges and ranges to folding the tensor. counts[bits & 0x7fff] += 1 per element: +0 and -0 share bin 0, Inf / NaN
 * patterns are counted like any other (values are not interpreted). Counts are exact integers: two runs give the same bytes and
 * a table sums to its element count (below 2^32 per buffer per frame). These calls run BEHIND the raw-head forward
 * (unina_enqueue's launch sequence); the frame path (unina_infer*) is untouched by them. */
#define UNINA_CALIB_BINS 32768
/* No engine handle (unina_kcenter's role): value-count table of n fp16 elements on the device. d_half and d_counts 16-byte
 * aligned (UNINA_ERR_ARG otherwise, and for NULL / n == 0); the call zeroes d_counts itself; nothing is synchronised. */
int unina_abs_histogram_f16(const void *d_half, size_t n, uint32_t *d_counts, hipStream_t stream);
/* The buffers a calibration covers: every kBufF16Nhwc buffer of the engine file, in file order. */
int unina_calib_buffer_count(const unina_engine_t *e);                    /* < 0: -error code */
int unina_calib_buffer_name(const unina_engine_t *e, int i, char *name, size_t cap);
/* Tables of the buffers as they stand now: d_counts[count][UNINA_CALIB_BINS], 16-byte aligned, zeroed by the call; every
 * buffer in ONE launch (what unina_mine_heads_async is to unina_mine_async). UNINA_ERR_UNSUPPORTED: the engine's precision is
 * not fp16 (calibration runs on the fp16 engine). UNINA_ERR_STATE: unina_fusion_groups(e) > 0 -- fused launches do not write
 * their internal buffers, call unina_set_fusion(e, 0) first. A refused call enqueues nothing. */
int unina_calib_buffers_async(unina_engine_t *e, uint32_t *d_counts, hipStream_t stream);
/* Forward (unina_enqueue's launch sequence) + the tables, enqueued on `stream`; d_images_nchw as unina_infer (NULL = current
 * binding). Nothing is synchronised. */
int unina_calib_async(unina_engine_t *e, const float *d_images_nchw, uint32_t *d_counts, hipStream_t stream);

/* ------------------------------------------------------------------ evaluation (eval.py:18-138, train.py:299-520)
 * Scoring detections against labels where the records already are: one small launch per image (csrc/evalmatch.hip: one
 * workgroup of 11 waves), enqueued behind the frame that produced the records (unina_infer_async and the camera / letterbox /
 * tiled _async calls); no engine handle. Only counters, conformal scores and per-detection true-positive masks cross to the
 * host, once per data set (unina_eval_read). The HOST code is the definition, decision for decision and bit for bit:
 *   UNINA_EVAL_SMALL     metrics.SmallObjectMetric.update on the rows evaluate() builds from the records: x * sx / y * sy in fp32,
 *                        x2 - x1 in fp32 (detections_to_coco), then double: centre format normalised by width / height, small =
 *                        w * imgsz < size_threshold and h * imgsz < size_threshold (both strict), TP at best IoU >= iou_threshold,
 *                        FP only for a small prediction, FN = small labels left unmatched; an image without a small label
 *                        counts nothing
 *   UNINA_EVAL_CONFORMAL metrics.conformal_quantile's matcher on the records scaled by cx / cy in fp32 (to imgsz pixels) and the
 *                        labels converted with the ONE size imgsz: a pair is a candidate if iou > best and iou >= 0.5; every match
 *                        appends the score 1 - best_iou (double), in the host's order
 *   UNINA_EVAL_AP        the same matcher at the ten thresholds t_j = (10 + j) / 20.0, j = 0..9 (metrics.ap_rows_numpy): one row
 *                        per record, in matching order, bit j of tp_mask = matched at t_j; and the labels counted per class
 * Matching order: greater confidence first, equal confidences by record index (np.argsort(-confidence, kind="stable")); the
 * records need not arrive sorted. Among labels of equal IoU the lowest index wins. Every launch handles one image: at most
 * UNINA_EVAL_MAX_LABELS labels, at most MAX_DETECTIONS records, the count read from device memory. Integer counters, fixed
 * append order (one workgroup per launch, launches stream-ordered): two runs give identical bytes. */
#define UNINA_EVAL_SMALL 1u
#define UNINA_EVAL_CONFORMAL 2u
#define UNINA_EVAL_AP 4u
#define UNINA_EVAL_MAX_LABELS 256
#define UNINA_EVAL_MAX_CLASSES 256
typedef struct unina_eval unina_eval_t;
typedef struct {
  float sx, sy;            /* SMALL: record -> pixels of the image itself (evaluate(): w / net_w, h / net_h)                */
  float cx, cy;            /* CONFORMAL / AP: record -> imgsz pixels (evaluate(): imgsz / net_w, imgsz / net_h)              */
  int width, height;       /* the image's own size: what the labels are normalised to (eval.py:96-108)                       */
  int imgsz;               /* SmallObjectMetric.image_size and conformal_quantile's imgsz                                     */
  double size_threshold;   /* SmallObjectMetric.size_threshold (15)                                                           */
  double iou_threshold;    /* SmallObjectMetric.iou_threshold (0.5), > 0                                                      */
} unina_eval_params;
typedef struct {
  float confidence;
  int class_id;
  unsigned tp_mask;
} unina_eval_row;
typedef struct {
  long long tp, fp, fn;                /* SmallObjectMetric's accumulators                                                    */
  unsigned long long n_scores, n_rows; /* TRUE totals since the last reset, also where a list ran past its capacity           */
  int overflow;                        /* bit 0: scores past max_scores, bit 1: rows past max_rows (the excess is dropped)    */
  int guard_intact;                    /* 1: the canary words the handle keeps behind both lists still hold their pattern     */
  long long label_counts[UNINA_EVAL_MAX_CLASSES]; /* AP: labels per class id in [0, num_classes)                              */
} unina_eval_result;

/* Host only: no HIP call; the device memory (counters, max_scores doubles, max_rows rows) is allocated -- and zeroed -- by the
 * first reset / update / read, on that call's stream, which then fails with UNINA_ERR_HIP where there is no device.
 * UNINA_ERR_ARG: NULL out, negative device_id, num_classes outside 1..UNINA_EVAL_MAX_CLASSES. */
int unina_eval_create(int device_id, int num_classes, size_t max_scores, size_t max_rows, unina_eval_t **out);
/* Waits for the device, frees. NULL is a no-op. */
void unina_eval_destroy(unina_eval_t *ev);
/* Zeroes counters and list lengths, enqueued on `stream`. */
int unina_eval_reset_async(unina_eval_t *ev, hipStream_t stream);
/* One image, enqueued on `stream`; nothing is synchronised.
 *   d_dets / d_count : device, MAX_DETECTIONS records / one int, as unina_infer_async writes them (*d_count is clamped to
 *                      0..MAX_DETECTIONS on the device)
 *   d_labels         : device, double [n_labels, 5] rows cls, xc, yc, w, h (normalised); may be NULL when n_labels == 0
 *   what             : mask of UNINA_EVAL_*; all parts of one call see the same records
 * UNINA_ERR_ARG, before any HIP call: NULL ev / d_dets / d_count / p, n_labels outside 0..UNINA_EVAL_MAX_LABELS, d_labels NULL
 * with labels, `what` zero or with unknown bits, a non-positive size, iou_threshold <= 0, a misaligned pointer. */
int unina_eval_update_async(unina_eval_t *ev, const GpuDetection *d_dets, const int *d_count, const double *d_labels,
                            int n_labels, const unina_eval_params *p, unsigned what, hipStream_t stream);
/* Synchronises `stream`, then copies out the counters and min(n_scores, max_scores, score_cap) scores /
 * min(n_rows, max_rows, row_cap) rows (scores / rows may be NULL when their cap is 0). */
int unina_eval_read(unina_eval_t *ev, unina_eval_result *res, double *scores, size_t score_cap, unina_eval_row *rows,
                    size_t row_cap, hipStream_t stream);

/* ------------------------------------------------------------------ 3-D localisation (perception_node.cpp:545-550: the camera
 * delivers a depth map on the GPU beside every colour frame)
 * Kept records + a depth plane + pinhole intrinsics -> one 3-D point per record, in the camera frame (x right, y down, z
 * forward, metres): one launch (csrc/locate.hip) enqueued behind whichever _async call produced the records; no engine handle,
 * nothing is synchronised, the depth map never crosses to the host. localize.locate_numpy is the definition, decision for
 * decision and bit for bit. Everything is fp32, each operation rounded once, never contracted; the divide is correctly rounded.
 *   window   X1 = x1 * sx, X2 = x2 * sx, Y1 = y1 * sy, Y2 = y2 * sy (record -> depth-map pixels; pixel i covers [i, i + 1))
 *            uc = 0.5f * (X1 + X2), vc = 0.5f * (Y1 + Y2); hw = (0.5f * shrink) * (X2 - X1), hh = (0.5f * shrink) * (Y2 - Y1)
 *            columns floorf(uc - hw) .. floorf(uc + hw) clipped to 0 .. width - 1, rows floorf(vc - hh) .. floorf(vc + hh) clipped
 *            to 0 .. height - 1. Emptiness is decided in float, integers are formed after the clip. EMPTY: a non-finite X1, X2,
 *            Y1, Y2 or window bound, X2 < X1, Y2 < Y1, or a window wholly off the map (last bound < 0 or first bound > size - 1).
 *            A degenerate box (X2 == X1) still covers the one column under its centre.
 *            An empty window writes an ALL-ZERO record (n_samples = 0, valid = 0, u = v = 0).
 *   grid     integers: nx = u1 - u0 + 1, stride = (nx + max_side - 1) / max_side, sampled columns u0 + i * stride <= u1; rows
 *            likewise, each axis with its own stride. n_samples = columns * rows <= max_side * max_side <= 65 536.
 *   sample   UNINA_DEPTH_F32: valid if the raw float is finite; UNINA_DEPTH_U16: valid if raw != 0. In both z = (float)raw * unit
 *            must satisfy min_depth <= z <= max_depth. So NaN, +-inf, negatives, -0.0 and 0 are holes, and since min_depth > 0
 *            every valid float is positive: its bit pattern orders as an unsigned integer.
 *   depth    the LOWER MEDIAN: the valid sample of rank (n_valid - 1) / 2 in ascending raw order (np.sort(raw)[(n - 1) // 2]); an
 *            actual sample, nothing is averaged. Found by counting (radix select on the raw bits), so exact and run-to-run
 *            identical. Z = (float)raw_median * unit.
 *   point    x = ((uc - cx) * Z) / fx, y = ((vc - cy) * Z) / fy, z = Z; u = uc, v = vc (depth-map pixels)
 *   valid    1 iff n_valid >= max(1, min_valid); otherwise x = y = z = 0 (u, v, n_valid, n_samples stay)
 * Records 0 .. count - 1 are processed whatever their `valid` field says (the _async calls write them compact, valid = 1);
 * *d_count is clamped to 0..MAX_DETECTIONS on the device; the slots at and beyond it are written as all-zero bytes, so all
 * MAX_DETECTIONS outputs are defined after every launch. */
#define UNINA_DEPTH_F32 0   /* float32, e.g. ZED MEASURE::DEPTH; NaN / +-inf = hole */
#define UNINA_DEPTH_U16 1   /* uint16, e.g. ROS 16UC1 millimetres; 0 = hole         */
typedef struct { int format, width, height, pitch; const void *plane; float unit; } unina_depth;  /* pitch: bytes per row; unit: raw -> metres */
typedef struct { float fx, fy, cx, cy; } unina_pinhole;   /* rectified image, depth-map pixels */
typedef struct { float sx, sy, shrink, min_depth, max_depth; int max_side, min_valid; } unina_locate_params;
typedef struct { float x, y, z, u, v; int n_valid, n_samples, valid; } unina_cone3d;   /* 32 bytes, index-aligned with the records */
/*   d_dets / d_count : device, MAX_DETECTIONS records (16-byte aligned) / one int, as the _async calls write them
 *   depth->plane     : device; d_out : device, MAX_DETECTIONS unina_cone3d, 16-byte aligned
 * UNINA_ERR_ARG, before any HIP call: a NULL pointer (plane included); an unknown format; a size that is not positive (or above
 * 16 777 216); a pitch below width * element size or not a multiple of the element size; plane not aligned to its element; d_out
 * or d_dets not 16-byte aligned; fx, fy, unit, sx or sy not finite and positive; cx or cy not finite; shrink outside (0, 1];
 * max_side outside 1..256; min_valid < 0; not 0 < min_depth < max_depth < inf. */
int unina_locate_async(const GpuDetection *d_dets, const int *d_count, const unina_depth *depth, const unina_pinhole *cam,
                       const unina_locate_params *p, unina_cone3d *d_out, hipStream_t stream);

/* ------------------------------------------------------------------ 3-D localisation from a stereo pair (for a camera whose
 * depth map is not on this GPU: two rectified luma planes are all it needs)
 * Kept records + a rectified pair + the left camera's intrinsics + the baseline -> the same unina_cone3d records as
 * unina_locate_async writes, so unina_track_update_async goes behind it unchanged. One launch (csrc/stereo.hip) enqueued behind
 * whichever _async call produced the records; no engine handle, nothing is synchronised, neither plane crosses to the host. Only
 * each record's window is matched, along its own rows of the right image: sum of absolute differences over the window's
 * sampling grid, one cost per integer disparity. localize.locate_stereo_numpy is the definition, decision for decision and bit
 * for bit. Every comparison of costs is on integers; the floats are fp32, each operation rounded once, never contracted; the
 * divide is correctly rounded.
 *   count    as unina_locate_async: *d_count clamped to 0..MAX_DETECTIONS on the device; the slots at and beyond it are all-zero
 *            bytes in d_out and in d_match
 *   window   and grid: exactly unina_locate_async's (above), on the LEFT plane, with max_side limited to 1..UNINA_STEREO_MAX_SIDE:
 *            n_samples <= 4096, every cost <= 4096 * 255 = 1 044 480 < 2^20, and every integer converted to float below is under
 *            2^24, so the conversion is exact. An empty window writes all-zero records (d_out and d_match)
 *   range    once per call, on the host, in fp32: fxB = fx * baseline; d_lo = max(1, ceilf(fxB / max_depth)); d_hi_all =
 *            min(floorf(fxB / min_depth), width - 1); both clipped in float before they become ints (d_lo also to `width`, which
 *            changes no result). d_hi_all < d_lo is legal: no record can then be valid. Per record d_hi = min(d_hi_all, u0), so
 *            every right column u - d >= 0; nd = max(0, d_hi - d_lo + 1) disparities are searched
 *   cost     for d in d_lo..d_hi: cost(d) = sum over the grid's sampled (u, v) of |L[v, u] - R[v, u - d]|, a uint32
 *   best     the minimum of (cost, d) in ascending order: the smaller disparity wins a tie. cost_second = the least cost over the
 *            d with |d - d_best| > 1, 0xFFFFFFFF where there is none
 *   accepted iff nd >= 1, and cost_best <= (uint64)max_mean_sad * n_samples, and (cost_second == 0xFFFFFFFF or
 *            (uint64)cost_second * 100 > (uint64)cost_best * (100 + uniqueness)). The inequality is strict: an exact tie between
 *            two separated disparities is ambiguous and fails, so a flat patch (all costs equal) fails whatever `uniqueness` is
 *   subpixel only when d_lo < d_best < d_hi, with cm = cost(d_best - 1), cp = cost(d_best + 1): den = cm - 2 * cost_best + cp (an
 *            integer, never negative); delta = den == 0 ? 0 : (float)(cm - cp) / (float)(2 * den); |delta| <= 0.5 always, because
 *            |cm - cp| <= den. At either end of the range delta = 0: a parabola needs both neighbours, and half of one is a bias.
 *            disparity = (float)d_best + delta
 *   point    Z = fxB / disparity; x = ((uc - cx) * Z) / fx, y = ((vc - cy) * Z) / fy, z = Z; u = uc, v = vc: the expressions of
 *            unina_locate_async. Z is NOT checked against [min_depth, max_depth] again: the sub-pixel step can carry it a hair
 *            outside
 *   record   n_samples = the grid's count; n_valid = nd, the disparities searched; valid = accepted. Not accepted: x = y = z = 0
 *            (u, v, n_valid, n_samples stay). d_match[i] = {disparity, d_best, cost_best, cost_second} for every non-empty
 *            window, accepted or not, with disparity = 0 where it is not; nd == 0 gives {0, 0, 0xFFFFFFFF, 0xFFFFFFFF}
 * Integer costs and minima of packed integers (cost << 10 | d - d_lo): two runs give identical bytes.
 * The planes must be row-aligned: unina_rectify_async (below, "Rectification") makes them so from the raw images.
 * NOT covered: zero-mean or census costs (two cameras with different exposure or gain), a left-right consistency check (an
 * occluded window can be accepted at a wrong disparity). */
#define UNINA_STEREO_MAX_DISPARITIES 1024
#define UNINA_STEREO_MAX_SIDE 64
typedef struct { int width, height, pitch; const uint8_t *left, *right; } unina_stereo_pair;
      /* rectified 8-bit luma planes of one size and pitch (bytes per row); an NV12 Y plane is one. Row v of left is row v of
         right; a point at column u of left is at column u - d of right, d >= 0. No alignment is required of either pointer or
         of the pitch. The planes may be the halves of one side-by-side buffer (right = left + width, shared pitch). */
typedef struct { float sx, sy, shrink, min_depth, max_depth; int max_side, max_mean_sad, uniqueness; } unina_stereo_params;
      /* sx, sy: record -> plane pixels; max_mean_sad: grey levels per sample, 0..255; uniqueness: per cent, 0..1000 */
typedef struct { float disparity; int d_best; uint32_t cost_best, cost_second; } unina_stereo_match;   /* 16 bytes */
/*   d_dets / d_count : device, MAX_DETECTIONS records (16-byte aligned) / one int, as the _async calls write them
 *   pair->left/right : device; d_out : device, MAX_DETECTIONS unina_cone3d, 16-byte aligned
 *   d_match          : device, MAX_DETECTIONS unina_stereo_match, 16-byte aligned, or NULL
 * UNINA_ERR_ARG, before any HIP call: a NULL pointer other than d_match (left and right included); d_out, d_dets or d_match not
 * 16-byte aligned, or d_count not 4-byte aligned; a width or height outside 1..16 777 216, or pitch < width; fx, fy, baseline, sx
 * or sy not finite and positive; cx or cy not finite; fxB or fxB / min_depth not finite; shrink outside (0, 1]; max_side outside
 * 1..UNINA_STEREO_MAX_SIDE; max_mean_sad outside 0..255; uniqueness outside 0..1000; not 0 < min_depth < max_depth < inf;
 * d_hi_all - d_lo + 1 > UNINA_STEREO_MAX_DISPARITIES (raise min_depth). */
int unina_locate_stereo_async(const GpuDetection *d_dets, const int *d_count, const unina_stereo_pair *pair,
                              const unina_pinhole *cam /* left rectified image, plane pixels */, float baseline /* metres */,
                              const unina_stereo_params *p, unina_cone3d *d_out,
                              unina_stereo_match *d_match /* MAX_DETECTIONS, 16-byte aligned, or NULL */, hipStream_t stream);

/* ------------------------------------------------------------------ Rectification (a camera delivers raw, distorted images and
 * a calibration; every locator above takes the rectified image's pinhole)
 * 1 to UNINA_RECTIFY_MAX_IMAGES raw 8-bit images + one calibration each -> the undistorted, rotated images, in ONE launch
 * (csrc/rectify.hip) on the caller's stream: the left and right luma planes of a stereo head and the colour frame the detector
 * takes, say. No engine handle, nothing is synchronised, nothing is allocated, no image crosses to the host. The calibration is
 * OpenCV's: camera matrix K and five distortion coefficients of the raw image, R1 / R2 and P1 / P2 of stereoRectify (or K, D, R, P
 * of a ROS camera_info). Coordinates index PIXEL CENTRES, as initUndistortRectifyMap does, so such calibrations apply unchanged
 * (the "pixel i covers [i, i + 1)" of the locators is a statement about binning, a different one). rectify.rectify_numpy is the
 * definition, byte for byte (rectify.rectify_source_numpy for the coordinates). The coordinates are fp32, each operation rounded
 * once in the order written, never contracted, the divides correctly rounded; everything behind the inside test is integer.
 * For the integer output pixel (u, v) of job->dst:
 *   ray      x = ((float)u - dst.cx) / dst.fx, y = ((float)v - dst.cy) / dst.fy
 *            X = (r[0] * x + r[3] * y) + r[6], Y = (r[1] * x + r[4] * y) + r[7], W = (r[2] * x + r[5] * y) + r[8]   (R^T * (x, y, 1))
 *            xn = X / W, yn = Y / W
 *   lens     r2 = xn * xn + yn * yn; rad = ((k3 * r2 + k2) * r2 + k1) * r2 + 1.0f; xy2 = (2.0f * xn) * yn
 *            xd = (xn * rad + p1 * xy2) + p2 * (r2 + 2.0f * (xn * xn)); yd = (yn * rad + p1 * (r2 + 2.0f * (yn * yn))) + p2 * xy2
 *   source   us = src.fx * xd + src.cx, vs = src.fy * yd + src.cy (raw-image pixels); tx = us * 32.0f + 0.5f, ty = vs * 32.0f + 0.5f
 *   inside   iff W > 0 and -32.0f <= tx < (float)(32 * src.width) and -32.0f <= ty < (float)(32 * src.height); a NaN fails. Sizes
 *            are at most UNINA_RECTIFY_MAX_DIM, so the float bounds are exact. A pixel that is not inside is `border` in every
 *            channel
 *   taps     qx = (int)floorf(tx), x0 = qx >> 5 (arithmetic: -1 .. src.width - 1), ax = qx & 31; y0, ay likewise. The taps are
 *            (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1); a tap outside the raw image has the value `border` and its
 *            address is never formed, a tap of weight 0 included
 *   blend    per channel, integers, 5 fractional bits as in OpenCV's fixed-point remap:
 *            out = ((32 - ax) * (32 - ay) * t00 + ax * (32 - ay) * t10 + (32 - ax) * ay * t01 + ax * ay * t11 + 512) >> 10
 * Source and destination sizes are independent: a crop or a scale goes through `dst` (the pinhole the locators then take).
 * Images of different size and channel count may share a call. Every output byte is written by one thread from integers: two
 * runs give identical bytes. Bytes of a destination row beyond width * channels are not written.
 * NOT covered: rational, fisheye and thin-prism distortion models, precomputed maps, NV12 chroma and planar colour (an NV12 Y
 * plane is a 1-channel image), bicubic sampling. */
#define UNINA_RECTIFY_MAX_IMAGES 4
#define UNINA_RECTIFY_MAX_DIM 16384
typedef struct {
  unina_pinhole src;          /* raw camera matrix K, raw-image pixels */
  float k1, k2, p1, p2, k3;   /* OpenCV's 5-coefficient order */
  float r[9];                 /* row-major 3x3, OpenCV's R1/R2: p_rect = R * p_raw */
  unina_pinhole dst;          /* P[:, :3] of the rectified image; the pinhole the locators take */
} unina_rectify_cam;
typedef struct { int width, height, pitch, channels; const uint8_t *data; } unina_image;
      /* device; interleaved 8-bit, channels 1, 3 or 4; pitch: bytes per row. No alignment is required of data or pitch (a
         1-channel row is stored, and a 4-channel pixel loaded and stored, a dword at a time where the address allows) */
typedef struct { unina_rectify_cam cam; unina_image src; unina_image dst; int border; } unina_rectify_job;
      /* dst.data is written (the const is the shared type's) */
/* UNINA_ERR_ARG, before any HIP call: jobs NULL or a NULL data pointer; n_jobs outside 1..UNINA_RECTIFY_MAX_IMAGES; a width or
 * height outside 1..UNINA_RECTIFY_MAX_DIM; channels not 1, 3 or 4, or different between src and dst; pitch < width * channels;
 * border outside 0..255; a non-finite field of cam; fx or fy of either pinhole not positive; dst.data == src.data. Images that
 * overlap otherwise are the caller's to avoid. */
int unina_rectify_async(const unina_rectify_job *jobs, int n_jobs, hipStream_t stream);

/* ------------------------------------------------------------------ 3-D localisation from a LiDAR sweep (for a vehicle with one
 * camera and a LiDAR: no depth map, no second image)
 * Kept records + a point cloud on the device + the LiDAR -> camera extrinsic + the camera's intrinsics -> the same unina_cone3d
 * records as unina_locate_async writes, so unina_track_update_async goes behind it unchanged. One call enqueues everything
 * (csrc/lidar.hip: project and count, scan, scatter, select) on the caller's stream behind whichever _async call produced the
 * records; nothing is synchronised, neither the records nor the cloud cross to the host. localize.locate_lidar_numpy is the
 * definition, decision for decision and bit for bit (localize.project_lidar_numpy for the per-point half). Everything is fp32,
 * each operation rounded once in the order written, never contracted; the divide is correctly rounded; every decision after the
 * projection is on integers.
 *   point    (x, y, z) = the first three float32 of each `stride`-byte point; the rest of a point is never read.
 *            xc = ((r00 * x + r01 * y) + r02 * z) + t0, yc and zc from rows 1 and 2 of lidar_to_cam ([R|t], row-major 3 x 4,
 *            LiDAR frame -> camera frame: the pose convention of unina_track_params);
 *            u = (fx * xc) / zc + cx, v = (fy * yc) / zc + cy (image pixels; pixel i covers [i, i + 1))
 *            PROJECTABLE iff xc, yc, zc are finite, zc > 0, 0 <= u < (float)width and 0 <= v < (float)height (a NaN fails).
 *            pixel = ((int)u, (int)v); key = the bits of zc where min_depth <= zc <= max_depth, else 0. min_depth > 0, so a
 *            non-zero key orders as an unsigned integer exactly as its depth does. A point that is not projectable contributes
 *            nothing (its unina_lidar_pixel is all-zero)
 *   count    as unina_locate_async: *d_count clamped to 0..MAX_DETECTIONS on the device; the slots at and beyond it are all-zero
 *   window   exactly unina_locate_async's window on a width x height map, with max_side = UNINA_LIDAR_MAX_DIM: every covered
 *            pixel u0..u1 x v0..v1 counts (stride 1). An empty window writes the all-zero record
 *   members  the projectable points whose pixel lies in u0..u1 x v0..v1; a point may be a member of several records.
 *            n_samples = the number of members, n_valid = the number of members with key != 0
 *   depth    the LOWER MEDIAN of the valid keys (np.sort(keys)[(n_valid - 1) // 2]): an actual point's zc, found by counting, so
 *            it does not depend on the order of the cloud
 *   record   valid = n_valid >= max(1, min_valid); valid: x = ((uc - cx) * Z) / fx, y = ((vc - cy) * Z) / fy, z = Z (the
 *            expressions of unina_locate_async), otherwise x = y = z = 0; u = uc, v = vc always
 * Integer counters only (no float atomics): two runs, and any permutation of the cloud, give identical unina_cone3d bytes.
 * NOT covered: ground removal (unina_ground_filter_async below goes in front of this call and strips the road; without it a
 * ground point inside the window counts as any other), lens distortion (the pinhole is the rectified image's), clustering --
 * the median of what falls in the shrunk box is the whole model. Motion de-skew and the time alignment of sweep and frame are
 * unina_deskew_async below, which goes in front of this call. */
#define UNINA_LIDAR_MAX_DIM    16384       /* width, height */
#define UNINA_LIDAR_MAX_POINTS (1 << 22)
typedef struct { int n_points, stride; const void *points; } unina_cloud;   /* device; xyz float32 first in each point */
typedef struct { float sx, sy, shrink, min_depth, max_depth; int min_valid; } unina_lidar_params;   /* sx, sy: record -> image pixels */
typedef struct { int u, v; uint32_t key; int projectable; } unina_lidar_pixel;   /* 16 bytes, point order; not projectable = all zero */
typedef struct unina_lidar unina_lidar_t;

/* Host only: no HIP call. The device workspace (bounded by max_points and by the 32 x 32-pixel cells of max_width x max_height,
 * and by nothing else: no legal input can overflow a list) is allocated by the first unina_locate_lidar_async, on that call's
 * stream, which then fails with UNINA_ERR_HIP where there is no device. One handle serves any sequence of clouds and image sizes
 * within its limits; calls on one handle belong on one stream, or are ordered by the caller.
 * UNINA_ERR_ARG: NULL out, negative device_id, max_points outside 1..UNINA_LIDAR_MAX_POINTS, max_width or max_height outside
 * 1..UNINA_LIDAR_MAX_DIM. */
int unina_lidar_create(int device_id, int max_points, int max_width, int max_height, unina_lidar_t **out);
/* Waits for the device, frees. NULL is a no-op. */
void unina_lidar_destroy(unina_lidar_t *l);
/*   d_dets / d_count : device, MAX_DETECTIONS records (16-byte aligned) / one int, as the _async calls write them
 *   cloud->points    : device, n_points * stride bytes, 4-byte aligned (read 16 bytes at a time where the base and the stride
 *                      allow it); d_out : device, MAX_DETECTIONS unina_cone3d, 16-byte aligned
 * UNINA_ERR_ARG, before any HIP call: a NULL pointer (points may be NULL only when n_points == 0); d_dets or d_out not 16-byte
 * aligned, or d_count not 4-byte aligned; n_points outside 0..max_points; stride < 12 or not a multiple of 4, or points not
 * 4-byte aligned; width or height outside 1..max_width / 1..max_height; a non-finite element of lidar_to_cam; fx, fy, sx or sy
 * not finite and positive; cx or cy not finite; shrink outside (0, 1]; not 0 < min_depth < max_depth < inf; min_valid < 0.
 * n_points == 0 is legal: every non-empty window gets n_samples = 0 and valid = 0, with u and v set. */
int unina_locate_lidar_async(unina_lidar_t *l, const GpuDetection *d_dets, const int *d_count, const unina_cloud *cloud,
                             const float lidar_to_cam[12], const unina_pinhole *cam, int width, int height,
                             const unina_lidar_params *p, unina_cone3d *d_out, hipStream_t stream);
/* Device address of the per-point result of the last call (n_points unina_lidar_pixel, in point order), for a consumer that
 * stays on the GPU or a test; read it behind the call on its stream. UNINA_ERR_STATE before the first unina_locate_lidar_async. */
int unina_lidar_buffers(unina_lidar_t *l, const unina_lidar_pixel **d_pixels);

/* ------------------------------------------------------------------ motion de-skew of a LiDAR sweep (in front of
 * unina_ground_filter_async, unina_cluster_async or unina_locate_lidar_async: a rotating LiDAR takes about 100 ms per sweep, and
 * at 15 m/s and 1.5 rad/s of yaw a static cone is displaced by metres between the first and the last column)
 * A point cloud on the device + a time per point + the LiDAR's poses over the sweep (host memory) + a reference time -> a cloud of
 * the same length and order with 16-byte points, every point moved to where the LiDAR would have seen it at t_ref. The stages
 * behind it take {n_points, 16, d_out} unchanged; the caller's lidar_to_level / lidar_to_cam still apply and now describe the
 * LiDAR at t_ref. With t_ref = the camera frame's exposure time, sweep and frame are aligned as well. The call is stateless: no
 * handle, no workspace. It enqueues one memset of the header and one kernel (csrc/deskew.hip) on the caller's stream and the
 * current device; nothing is synchronised. deskew.table_numpy and deskew.deskew_numpy are the definition, decision for decision and
 * bit for bit.
 * HOST HALF (unina_deskew_table; float64 throughout, each operation rounded once in the order written; the absolute stamps and
 * the large odometry coordinates cancel here and never reach the device):
 *   1 normalise  q_k = q_k / sqrt(((w*w + x*x) + y*y) + z*z), component by component
 *   2 reference  r = (the number of keys with t_j <= t_ref) - 1, clamped to 0..K-2; s = (t_ref - t_r) / (t_{r+1} - t_r);
 *                b = q_{r+1}, negated when ((aw*bw + ax*bx) + ay*by) + az*bz < 0 for a = q_r; q_ref = a + s * (b - a) per
 *                component, normalised as in 1; p_ref = p_r + s * (p_{r+1} - p_r)
 *   3 relative   with c = conj(q_ref) = (w, -x, -y, -z): D_k = c (x) q_k (Hamilton product: w = ((cw*qw - cx*qx) - cy*qy) - cz*qz,
 *                x = ((cw*qx + cx*qw) + cy*qz) - cz*qy, y = ((cw*qy - cx*qz) + cy*qw) + cz*qx, z = ((cw*qz + cx*qy) - cy*qx) + cz*qw),
 *                normalised as in 1; d_k = R(c) (p_k - p_ref), row i as (Ri0 * vx + Ri1 * vy) + Ri2 * vz, with R(q):
 *                R00 = 1 - 2*(y*y + z*z)  R01 = 2*(x*y - w*z)      R02 = 2*(x*z + w*y)
 *                R10 = 2*(x*y + w*z)      R11 = 1 - 2*(x*x + z*z)  R12 = 2*(y*z - w*x)
 *                R20 = 2*(x*z - w*y)      R21 = 2*(y*z + w*x)      R22 = 1 - 2*(x*x + y*y)
 *   4 hemisphere D_0 is negated when its w < 0; for k >= 1 D_k is negated when dot(D_k, D_{k-1}) < 0 (so keys given as q or
 *                as -q make the same table)
 *   5 round      the float32 row {(float)(D_k.w + 0.0), .x, .y, .z, (float)(d_k.x + 0.0), .y, .z, t = (float)(t_k - t_sweep)}:
 *                the sum turns a -0.0 into +0.0 and changes nothing else
 * DEVICE HALF (fp32 throughout, each operation rounded once in the order written, never contracted; divide and square root are
 * correctly rounded), per point i:
 *   time      tau = the float32 at times.t + i * times.stride (UNINA_TIME_F32_S), or (float)ns * 1e-9f of the uint32 there
 *             (UNINA_TIME_U32_NS: one conversion, one multiply); seconds after t_sweep
 *   validity  INVALID iff any of x, y, z is not finite, or tau is not finite. An INVALID point writes four words 0x7fc00000: the
 *             ground filter's absent entry, which every later stage skips
 *   segment   k = (the number of keys with t_j <= tau) - 1, clamped to 0..K-2; s = (tau - t_k) / (t_{k+1} - t_k), clamped to
 *             [0, 1]: tau == t_j belongs to segment j, tau == t_{K-1} gives segment K-2 with s == 1 exactly. BEFORE iff
 *             tau < t_0, AFTER iff tau > t_{K-1}: such a point takes the first or the last key's pose and is counted
 *   pose      each of the seven values of the rows k and k+1 as a + s * (b - a); n = sqrt(((qw*qw + qx*qx) + qy*qy) + qz*qz),
 *             q = q / n per component; the nine elements of R(q) by the expressions of step 3
 *   point     x' = ((R00 * x + R01 * y) + R02 * z) + px, y' and z' from rows 1 and 2 (the expression of lidar_to_cam)
 *   output    entry i of d_out = (x', y', z', carry): carry = the 32-bit word at byte carry_offset of the point, verbatim, or
 *             0x7fc00000 for carry_offset == -1. A NaN result (coordinates so near the fp32 limit that the sums overflow both
 *             ways) is stored as the word 0x7fc00000
 *   header    n_points; n_moved = the points that are not INVALID; n_invalid; n_before; n_after; max_shift2_bits = the largest
 *             bit pattern, as an unsigned integer, of (dx*dx + dy*dy) + dz*dz with dx = x' - x over the moved points (never
 *             negative, so the patterns order as the values do; a NaN as 0x7fc00000); two reserved words, 0
 * Integer counters and one integer maximum only (no float atomics): two runs give identical bytes, and any permutation of the
 * cloud the same header and the permuted points.
 * The model between two keys is nlerp of the rotation and a linear translation: its error falls with the square of the key
 * spacing. NOT covered: estimating the poses (odometry / IMU integration is the caller's), per-point times derived
 * from the azimuth, slerp, more than UNINA_DESKEW_MAX_KEYS keys, rolling-shutter correction of the camera. */
#define UNINA_DESKEW_MAX_KEYS 64
#define UNINA_TIME_F32_S  0                /* float32 seconds after t_sweep */
#define UNINA_TIME_U32_NS 1                /* uint32 nanoseconds after t_sweep */
typedef struct { const void *t; int stride; int format; } unina_point_times;   /* device; a time inside the point: t = points + offset, stride = the cloud's; a plane: stride = 4 */
typedef struct { double t; double q[4]; double p[3]; } unina_deskew_pose;       /* 64 bytes, host; q = w, x, y, z; LiDAR frame -> a fixed (odometry) frame at time t */
typedef struct { float qw, qx, qy, qz, px, py, pz, t; } unina_deskew_key;       /* 32 bytes: the pose of key k relative to the pose at t_ref */
typedef struct { int n_points, n_moved, n_invalid, n_before, n_after; uint32_t max_shift2_bits; int reserved[2]; } unina_deskew_header;   /* 32 bytes */

/* The host half on its own: no HIP call, no device. out: n_keys rows, written only on UNINA_OK.
 * UNINA_ERR_ARG: a NULL pointer; n_keys outside 2..UNINA_DESKEW_MAX_KEYS; a non-finite field of a pose, t_sweep or t_ref; a
 * zero-norm quaternion; the float32 key times (float)(t_k - t_sweep) not finite or not strictly increasing; t_ref outside
 * [t_0, t_{K-1}]; after step 4 dot(D_k, D_{k-1}) < 0.5 (more than 120 degrees between two keys: nlerp would approach a zero
 * norm); a relative translation that is not finite as a float32. */
int unina_deskew_table(const unina_deskew_pose *poses, int n_keys, double t_sweep, double t_ref, unina_deskew_key *out);
/*   cloud->points : device, n_points * stride bytes, 4-byte aligned (read 16 bytes at a time where the base and the stride allow)
 *   times->t      : device, 4-byte aligned; times->stride a multiple of 4, at least 4; may be NULL only when n_points == 0
 *   carry_offset  : -1, or a multiple of 4 in 12 .. stride - 4
 *   poses         : host, n_keys of them; read before the call returns
 *   d_out         : device, n_points * 16 bytes, 16-byte aligned; every entry is written exactly once
 *   d_header      : device, one unina_deskew_header, 4-byte aligned
 * UNINA_ERR_ARG, before any HIP call: what unina_deskew_table refuses; a NULL cloud, times, d_out or d_header (points may be NULL
 * only when n_points == 0); n_points outside 0..UNINA_LIDAR_MAX_POINTS; stride < 12 or not a multiple of 4, or points not 4-byte
 * aligned; times->t not 4-byte aligned, times->stride < 4 or not a multiple of 4, an unknown format; a carry_offset that is not
 * -1 and not a multiple of 4 in 12 .. stride - 4; d_out not 16-byte or d_header not 4-byte aligned; the n_points * 16 bytes at
 * d_out overlapping the cloud, the time plane or the header.
 * n_points == 0 is legal: the header is all-zero and nothing is written to d_out. */
int unina_deskew_async(const unina_cloud *cloud, const unina_point_times *times, int carry_offset, const unina_deskew_pose *poses,
                       int n_keys, double t_sweep, double t_ref, void *d_out, unina_deskew_header *d_header, hipStream_t stream);

/* ------------------------------------------------------------------ ground removal from a LiDAR sweep (in front of
 * unina_locate_lidar_async: a road return inside a record's window would otherwise count as any other)
 * A point cloud on the device + the LiDAR -> level extrinsic + a grid -> a filtered cloud of the same length on the device: the
 * points that stand on the ground first, in cloud order, then entries of four NaN words, which unina_locate_lidar_async treats
 * as not projectable. So the locator takes {n_points, 16, d_out} as its cloud unchanged, with the caller's lidar_to_cam, and the
 * number of kept points never crosses to the host. One call enqueues everything (csrc/ground.hip: two memsets, then seed,
 * envelope, classify, scan, scatter) on the caller's stream; nothing is synchronised. ground.ground_numpy is the definition,
 * decision for decision and bit for bit. Everything is fp32, each operation rounded once in the order written, never
 * contracted; the divides are correctly rounded; every decision after the transform compares integers, or fp32 values of which
 * none is a NaN.
 *   point     (x, y, z) = the first three float32 of each `stride`-byte point; the rest of a point is never read.
 *             xl = ((r00 * x + r01 * y) + r02 * z) + t0, yl and zl from rows 1 and 2 of lidar_to_level ([R|t], row-major 3 x 4,
 *             LiDAR frame -> a gravity-levelled frame with z up: the pose convention and the expression of lidar_to_cam)
 *   grid      fx = (xl - x_min) / cell, fy = (yl - y_min) / cell. IN_GRID iff xl, yl, zl are finite, 0 <= fx < (float)nx and
 *             0 <= fy < (float)ny (a NaN fails); the point's cell is (int)fy * nx + (int)fx
 *   key       key(f) = bits(f) ^ (bits(f) >> 31 ? 0xffffffff : 0x80000000): keys order as unsigned integers exactly as finite
 *             floats do, -0.0 below +0.0. 0xffffffff is no finite float's key and means EMPTY
 *   seed      SEED iff IN_GRID and z_lo <= zl <= z_hi. cellmin[c] = the minimum key(zl) over the seeds of cell c, or EMPTY. The
 *             band keeps multipath returns far below the road, and cells that see only a wall, from founding a ground height
 *   envelope  g[c] = the minimum, over every non-EMPTY cell n of the grid at Chebyshev distance k = max(|di|, |dj|) <= reach of
 *             c (c itself is k = 0), of key(cellmin_value[n] + (float)k * rise): one multiply and one add, each rounded once,
 *             for every k (a -0.0 minimum therefore enters as +0.0); EMPTY where there is no such cell. rise, in metres per
 *             ring of cells, is the steepest ground the envelope follows; rise = 0 is a plain minimum filter, reach = 0 the
 *             cell's own minimum
 *   label     0 OUTSIDE: not IN_GRID.  1 UNKNOWN: IN_GRID and g[cell] EMPTY.  With G = the value of g[cell]:
 *             2 GROUND: zl <= G + band.  3 OBJECT: G + band < zl <= G + max_height.  4 ABOVE: otherwise. Each sum rounded once
 *   kept      label == OBJECT, or label == UNKNOWN and keep_unknown != 0
 *   output    entry r of d_out, for the r-th kept point in cloud order, is (x, y, z, h): the point's own three input words (the
 *             LiDAR frame: the caller's lidar_to_cam still applies) and h = zl - G, or the word 0x7fc00000 for a kept UNKNOWN
 *             point. Entries n_kept .. n_points - 1 are four words of 0x7fc00000 each
 *   header    n_points, n_kept, n_label[5] (points per label), n_cells_seeded (cells whose cellmin is not EMPTY)
 * Integer counters and integer minima only (no float atomics): two runs give identical bytes, and any permutation of the cloud
 * gives every point the same label and the same cellmin, g and header.
 * NOT covered: ground steeper than `rise` allows between neighbouring cells (a banked or sloped track beyond it is labelled
 * OBJECT or ABOVE), plane or line fitting, an estimate of lidar_to_level (the caller's calibration or IMU supplies it). Motion
 * de-skew is unina_deskew_async above, which goes in front of this call. Clustering of what is kept is unina_cluster_async below, which takes {n_points, 16, d_out} as its cloud. */
#define UNINA_GROUND_MAX_SIDE  1024        /* nx, ny */
#define UNINA_GROUND_MAX_REACH 4
typedef struct { float x_min, y_min, cell; int nx, ny;
                 float z_lo, z_hi, rise, band, max_height; int reach, keep_unknown; } unina_ground_params;   /* 48 bytes; metres, level frame */
typedef struct { int n_points, n_kept, n_label[5], n_cells_seeded; } unina_ground_header;   /* 32 bytes */
typedef struct unina_ground unina_ground_t;

/* Host only: no HIP call, as unina_lidar_create. The device workspace (bounded by max_points and by the UNINA_GROUND_MAX_SIDE^2
 * cells of the largest grid, and by nothing else: no legal input can overflow a list) is allocated by the first
 * unina_ground_filter_async, on that call's stream, which then fails with UNINA_ERR_HIP where there is no device. One handle
 * serves any sequence of clouds and grids within its limits; calls on one handle belong on one stream, or are ordered by the
 * caller. UNINA_ERR_ARG: NULL out, negative device_id, max_points outside 1..UNINA_LIDAR_MAX_POINTS. */
int unina_ground_create(int device_id, int max_points, unina_ground_t **out);
/* Waits for the device, frees. NULL is a no-op. */
void unina_ground_destroy(unina_ground_t *g);
/*   cloud->points : device, n_points * stride bytes, 4-byte aligned (read 16 bytes at a time where the base and the stride allow)
 *   d_out         : device, n_points * 16 bytes, 16-byte aligned; every entry is written exactly once
 * UNINA_ERR_ARG, before any HIP call: a NULL pointer (points may be NULL only when n_points == 0); d_out not 16-byte aligned;
 * n_points outside 0..max_points; stride < 12 or not a multiple of 4, or points not 4-byte aligned; a non-finite element of
 * lidar_to_level; x_min, y_min, z_lo, z_hi, rise, band or max_height not finite; cell not finite and positive; nx or ny outside
 * 1..UNINA_GROUND_MAX_SIDE; z_lo > z_hi; rise < 0, band < 0 or max_height < band; reach outside 0..UNINA_GROUND_MAX_REACH; the
 * n_points * 16 bytes at d_out overlapping the n_points * stride bytes of the cloud.
 * n_points == 0 is legal: the header is all-zero, cellmin and g are EMPTY and nothing is written to d_out. */
int unina_ground_filter_async(unina_ground_t *g, const unina_cloud *cloud, const float lidar_to_level[12],
                              const unina_ground_params *p, void *d_out, hipStream_t stream);
/* Device addresses of what the last call left in the workspace, for a consumer that stays on the GPU or a test; read them behind
 * the call on its stream: n_points label bytes in point order, the nx * ny words of cellmin and of g (row fy, column fx), and
 * the header. A NULL argument is skipped. UNINA_ERR_STATE before the first unina_ground_filter_async. */
int unina_ground_buffers(unina_ground_t *g, const uint8_t **d_labels, const uint32_t **d_cellmin, const uint32_t **d_ground,
                         const unina_ground_header **d_header);

/* ------------------------------------------------------------------ cone candidates from a ground-free LiDAR sweep (behind
 * unina_ground_filter_async, in front of unina_track_update_async: a cone the camera detector missed still becomes an object)
 * A point cloud on the device (normally {n_points, 16, d_out} of the ground filter, whose NaN entries fall out by themselves) +
 * the LiDAR -> level extrinsic + a grid + a gate -> the connected components of the occupied grid cells, their statistics, and
 * those that pass the gate as GpuDetection + unina_cone3d records with a count: exactly what unina_track_update_async takes. One
 * call enqueues everything (csrc/cluster.hip: two memsets, then mark, label, merge, flatten, scan, rank, cells, sums, finish,
 * scan, emit) on the caller's stream; nothing is synchronised, nothing crosses to the host. cluster.cluster_numpy is the
 * definition, decision for decision and bit for bit. Everything is fp32, each operation rounded once in the order written, never
 * contracted; the divides are correctly rounded; every decision compares integers, or fp32 values of which none is a NaN.
 *   point      xl, yl, zl, fx, fy, IN_GRID and the cell exactly as unina_ground_filter_async computes them (one expression in
 *              csrc/ground_cell.h serves both), with this call's x_min, y_min, cell, nx, ny
 *   occupied   a cell that holds at least one IN_GRID point
 *   component  occupied cells joined under 8-connectivity; root = the smallest cell index of the component
 *   statistics per component over its points: n_points; n_cells; x_lo / x_hi, y_lo / y_hi, z_lo / z_hi = the values of the
 *              minimum / maximum key (the ground stage's key) of xl, yl, zl; Sx = the sum of (int)(fx * 256.0f), Sy likewise, as
 *              64-bit integers (the product is exact, below 2^18 and not negative: the conversion truncates)
 *   position   x = x_min + ((float)(Sx / n_points) * 0.00390625f) * cell, y likewise (an integer division; the conversion and the
 *              first product are exact), z = z_lo
 *   gate       CONE iff min_points <= n_points <= max_points and x_hi - x_lo <= max_width and y_hi - y_lo <= max_width and
 *              min_height <= z_hi - z_lo <= max_height, each difference rounded once
 *   table      one unina_cluster per component in ascending root; cone = 1 for CONE, else 0
 *   records    the CONE components in ascending root go to slots 0, 1, ..; at most MAX_DETECTIONS are written (n_written), the
 *              others are counted in n_dropped. GpuDetection: (x1, y1, x2, y2) = (x_lo, y_lo, x_hi, y_hi), a bird's-eye box in
 *              metres of the level frame; confidence and class_id are the parameters'; valid = 1, _pad = 0. unina_cone3d:
 *              (x, y, z), u = v = 0, n_valid = n_samples = n_points, valid = 1. *d_count = n_written. Every slot at and beyond
 *              n_written is all-zero bytes in both arrays: all MAX_DETECTIONS entries are defined after every call
 *   per point  the position of the point's component in the table, -1 for a point that is not IN_GRID
 *   header     n_points, n_in_grid, n_cells (occupied), n_components, n_cones, n_written, n_dropped, 0
 * The coordinates are those of the LEVEL frame: the pose handed to unina_track_update_async behind this call is level frame ->
 * tracking frame. Integer counters, minima, maxima and sums only (no float atomics): two runs give identical bytes, and any
 * permutation of the cloud the same header, table, records and count, and every point its component.
 * NOT covered: bridging of gaps wider than a cell (a cone whose returns leave an empty cell between them is two components),
 * colour and class from the image (unina_fuse_async below associates the LiDAR cones with the camera records and hands a
 * matched cone the detector's class), 3-D (voxel) connectivity (a branch over a cone joins it). Motion de-skew is
 * unina_deskew_async, in front of the ground filter. */
typedef struct { float x_min, y_min, cell; int nx, ny; int min_points, max_points;
                 float min_height, max_height, max_width, confidence; int class_id; } unina_cluster_params;   /* 48 bytes; nx, ny in 1..UNINA_GROUND_MAX_SIDE */
typedef struct { float x, y, z_lo, z_hi, x_lo, x_hi, y_lo, y_hi; int n_points, n_cells, root, cone; } unina_cluster;   /* 48 bytes */
typedef struct { int n_points, n_in_grid, n_cells, n_components, n_cones, n_written, n_dropped, reserved; } unina_cluster_header;   /* 32 bytes */
typedef struct unina_clusterer unina_cluster_t;

/* Host only: no HIP call, as unina_ground_create. The device workspace (8 bytes per cell of the UNINA_GROUND_MAX_SIDE^2 cells of
 * the largest grid, about 100 bytes per point of max_points, and nothing else: there are never more components than IN_GRID
 * points, so the table has max_points entries and no legal input can overflow a list) is allocated by the first
 * unina_cluster_async, on that call's stream, which then fails with UNINA_ERR_HIP where there is no device. One handle serves any
 * sequence of clouds and grids within its limits; calls on one handle belong on one stream, or are ordered by the caller.
 * UNINA_ERR_ARG: NULL out, negative device_id, max_points outside 1..UNINA_LIDAR_MAX_POINTS. */
int unina_cluster_create(int device_id, int max_points, unina_cluster_t **out);
/* Waits for the device, frees. NULL is a no-op. */
void unina_cluster_destroy(unina_cluster_t *c);
/*   cloud->points   : device, n_points * stride bytes, 4-byte aligned (read 16 bytes at a time where the base and the stride allow)
 *   d_dets, d_cones : device, MAX_DETECTIONS records each, 16-byte aligned; d_count : device, one int, 4-byte aligned
 * UNINA_ERR_ARG, before any HIP call: a NULL pointer (points may be NULL only when n_points == 0); d_dets or d_cones not 16-byte
 * aligned, d_count not 4-byte aligned; n_points outside 0..max_points; stride < 12 or not a multiple of 4, or points not 4-byte
 * aligned; a non-finite element of lidar_to_level; x_min, y_min, min_height, max_height or max_width not finite; cell not finite
 * and positive; nx or ny outside 1..UNINA_GROUND_MAX_SIDE; min_points < 1 or max_points < min_points; min_height < 0 or
 * max_height < min_height; max_width < 0; a NaN confidence; d_dets, d_cones or d_count overlapping the n_points * stride bytes
 * of the cloud. n_points == 0 is legal: the header, the records and the count are all-zero. */
int unina_cluster_async(unina_cluster_t *c, const unina_cloud *cloud, const float lidar_to_level[12], const unina_cluster_params *p,
                        GpuDetection *d_dets, int *d_count, unina_cone3d *d_cones, hipStream_t stream);
/* Device addresses of what the last call left in the workspace, for a consumer that stays on the GPU or a test; read them behind
 * the call on its stream: the n_components entries of the table, the n_points component indices in point order, and the header.
 * A NULL argument is skipped. UNINA_ERR_STATE before the first unina_cluster_async. */
int unina_cluster_buffers(unina_cluster_t *c, const unina_cluster **d_components, const int **d_point_component,
                          const unina_cluster_header **d_header);

/* ------------------------------------------------------------------ fusion of LiDAR cone candidates with camera records (behind
 * unina_cluster_async and any of unina_locate_async / unina_locate_stereo_async / unina_locate_lidar_async, in front of ONE
 * unina_track_update_async)
 * The camera branch's records (class and box, camera frame) + the clusterer's records (accurate range, no class, level frame) ->
 * ONE record list in the camera frame and a link per record: a matched record carries the detector's class and box and the
 * LiDAR's position. One launch (csrc/fuse.hip: one workgroup of 1024 threads) on the caller's stream; nothing is synchronised,
 * nothing crosses to the host. The call is stateless: no handle, no workspace, everything it leaves is in the caller's buffers.
 * fusion.fuse_numpy is the definition, decision for decision and bit for bit. Everything is fp32, each operation rounded once in
 * the order written, never contracted; the divides are correctly rounded; every decision compares integers, or fp32 values where
 * a NaN fails.
 *   counts     nc = *d_count, nl = *d_lcount, each clamped to 0..MAX_DETECTIONS on the device
 *   LiDAR j    (xc, yc, zc) = level_to_cam applied to (x, y, z + lift) of lcones[j] (rows as ((r0 * x + r1 * y) + r2 * z) + t).
 *              USABLE iff lcones[j].valid != 0 and xc, yc, zc are finite. PROJECTED iff usable and min_depth <= zc <= max_depth;
 *              then u = (fx * xc) / zc + cx and v = (fy * yc) / zc + cy, kept as floats and not clipped to any image size
 *   camera i   X1 = x1 * sx, X2 = x2 * sx, Y1 = y1 * sy, Y2 = y2 * sy. BOXED iff the four are finite, X2 >= X1 and Y2 >= Y1; the
 *              record's own `valid` is ignored, as in every stage. uc = 0.5f * (X1 + X2), vc = 0.5f * (Y1 + Y2),
 *              hw = (0.5f * grow) * (X2 - X1) + pad, hh = (0.5f * grow) * (Y2 - Y1) + pad
 *   candidate  (i, j) with i boxed, j projected, du = u - uc, dv = v - vc, fabsf(du) <= hw and fabsf(dv) <= hh, and, where
 *              cones[i].valid != 0, fabsf(zc - cones[i].z) <= range_abs + range_rel * zc (a camera record without a depth has no
 *              depth gate). d2 = du * du + dv * dv is never negative, so its bits order as an unsigned integer
 *   match      greedy over all candidates in ascending (d2 bits, i, j); a pair is taken iff both its members are free
 *   slot i < nc  belongs to camera record i (the tracker's d_assign stays index-aligned with the camera records). Matched with
 *              j: the GpuDetection is the camera's, byte for byte; the cone is (xc, yc, zc, u, v, lcones[j].n_valid,
 *              lcones[j].n_samples, valid = 1); the link {i, j, d2, UNINA_FUSE_BOTH}. Unmatched: both records are the camera's,
 *              byte for byte (a cone with valid = 0 included); the link {i, -1, 0, UNINA_FUSE_CAMERA}
 *   slots nc.. the usable unmatched LiDAR cones in ascending j while a slot is left, the others are counted in n_dropped.
 *              GpuDetection: x1 = x2 = u / sx and y1 = y2 = v / sy where projected (a point box in record coordinates), else the
 *              four are 0; confidence and class_id are ldets[j]'s; valid = 1, _pad = 0. Cone: (xc, yc, zc, u, v -- or 0, 0 --,
 *              lcones[j].n_valid, lcones[j].n_samples, valid = 1). Link {-1, j, 0, UNINA_FUSE_LIDAR}
 *   the rest   *d_out_count = n_written; every slot at and beyond n_written is all-zero bytes in the three arrays: all
 *              MAX_DETECTIONS entries are defined after every call. d_lidar_slot[j] = the output slot LiDAR cone j went to (its
 *              match's, or its own appended one), -1 where it is unusable, dropped or j >= nl; all MAX_DETECTIONS words are written
 *   header     nc, nl, n_projected, n_matched, nc - n_matched, n_lidar_only (usable unmatched), n_written, n_dropped
 * Integer counters, 64-bit unsigned minima and a fixed order of every fp32 operation: two runs give identical bytes.
 * LiDAR-only records carry the clusterer's class_id: give it an id the detector does not use and put unina_colour_async (below)
 * behind this call with only_class = that id, which writes the class from the rectified image's pixels; a record it leaves
 * undecided keeps the unknown id, and such a track and a coloured one stay apart until the camera or the colour stage names it.
 * Time alignment of sweep and frame and motion de-skew are unina_deskew_async, in front of the LiDAR branch, with t_ref = the
 * frame's exposure time. NOT covered: a globally optimal (Hungarian) assignment, raising the
 * confidence of a matched record, lens distortion (the image is rectified). */
typedef struct {
  float level_to_cam[12];         /* row-major 3 x 4 [R|t]: level frame (the clusterer's) -> camera OPTICAL frame */
  unina_pinhole cam;              /* of the image the camera records live on */
  float sx, sy;                   /* record -> image pixels, as unina_lidar_params */
  float lift;                     /* metres above the component's lowest point at which a LiDAR cone is represented (e.g. 0.15) */
  float min_depth, max_depth;     /* zc range in which a LiDAR cone may be matched; min_depth > 0 */
  float grow, pad;                /* the box a LiDAR pixel must fall into: half extents (0.5*grow)*(X2-X1) + pad, pad in image pixels */
  float range_abs, range_rel;     /* depth gate where the camera cone has a depth: |zc - cones[i].z| <= range_abs + range_rel * zc */
} unina_fuse_params;              /* 100 bytes */
typedef struct { int camera, lidar; float d2; int kind; } unina_fuse_link;      /* 16 bytes, index-aligned with the OUTPUT records */
typedef struct { int n_camera, n_lidar, n_projected, n_matched, n_camera_only, n_lidar_only, n_written, n_dropped; } unina_fuse_header; /* 32 bytes */
#define UNINA_FUSE_BOTH 1
#define UNINA_FUSE_CAMERA 2
#define UNINA_FUSE_LIDAR 3

/* One launch, enqueued on `stream`; nothing is synchronised.
 *   d_dets / d_count / d_cones    : device, the camera branch: MAX_DETECTIONS records / one int / MAX_DETECTIONS unina_cone3d
 *   d_ldets / d_lcount / d_lcones : device, unina_cluster_async's outputs
 *   d_out_dets / d_out_count / d_out_cones : device, what unina_track_update_async takes
 *   d_links : device, MAX_DETECTIONS links; d_lidar_slot : device, MAX_DETECTIONS ints, or NULL; d_header : device, one header
 * Record arrays, d_links and d_header are 16-byte aligned; the counts and d_lidar_slot 4-byte aligned.
 * UNINA_ERR_ARG, before any HIP call: a NULL pointer (d_lidar_slot alone may be NULL); a misaligned pointer; a non-finite
 * level_to_cam element or pinhole value, fx or fy equal to 0; sx or sy not finite and positive; lift not finite; min_depth not
 * finite and positive, max_depth not finite or below min_depth; grow, pad, range_abs or range_rel not finite or negative; any
 * output array (its whole MAX_DETECTIONS extent) overlapping any input array or another output. */
int unina_fuse_async(const GpuDetection *d_dets,  const int *d_count,  const unina_cone3d *d_cones,
                     const GpuDetection *d_ldets, const int *d_lcount, const unina_cone3d *d_lcones,
                     const unina_fuse_params *p,
                     GpuDetection *d_out_dets, int *d_out_count, unina_cone3d *d_out_cones,
                     unina_fuse_link *d_links, int *d_lidar_slot, unina_fuse_header *d_header, hipStream_t stream);

/* ------------------------------------------------------------------ class from pixels (behind unina_fuse_async or any locator,
 * in front of unina_track_update_async)
 * A record without a class -- a LiDAR cone the detector missed -- + the rectified colour image (unina_rectify_async's output) ->
 * the record with the class its pixels show: blue, yellow, orange or large orange. A memset of the header and one launch
 * (csrc/colour.hip: one workgroup per record slot) on the caller's stream; nothing is synchronised, nothing crosses to the host.
 * The call is stateless: no handle, no workspace. colour.colour_numpy is the definition, bit for bit. Everything behind the
 * window is integer arithmetic (divisions are floor divisions of non-negative integers); the window's floats are fp32, each
 * operation rounded once in the order written, never contracted; the divides are correctly rounded.
 *   count      n = *d_count clamped to 0..MAX_DETECTIONS on the device. Slots at and beyond n are all-zero bytes in d_out_dets
 *              and d_colour: all MAX_DETECTIONS entries of both are defined after every call
 *   selected   record i < n is SELECTED iff only_class < 0 or dets[i].class_id == only_class; the record's own `valid` is
 *              ignored, as in every stage. A record that is not selected is copied byte for byte, its d_colour entry is zero
 *   window     BOX: where X1 = x1 * sx, X2 = x2 * sx, Y1 = y1 * sy, Y2 = y2 * sy are finite, X2 > X1 and Y2 > Y1, the window and
 *              its grid are those of unina_locate_async (csrc/locate_window.h: the covered pixels floorf(c - h) .. floorf(c + h)
 *              per axis with h = (0.5f * shrink) * (X2 - X1), clipped to the image; stride = ceil(span / max_side)) on
 *              (x1, y1, x2, y2, sx, sy, shrink, width, height, max_side).
 *              SIZE: where the BOX conditions fail (the fuser's point box x1 = x2), d_cones != NULL, cones[i].valid != 0 and u, v,
 *              z of cones[i] are finite with z > 0: hw = (fx * half_width) / z, up = (fy * above) / z, down = (fy * below) / z, and
 *              the same function on the box (u - hw, v - up, u + hw, v + down) with sx = sy = 1 and the same shrink and max_side.
 *              half_width, above and below are metres relative to the represented point (the fuser's `lift` above the base); the
 *              camera is taken to be level: optical y points down.
 *              Neither case, or a window that covers no pixel: the record is copied byte for byte, its d_colour entry is
 *              {0, .., status = SELECTED}
 *   grid       the sampled pixels (u0 + c * stride_x, v0 + k * stride_y), c < cols, k < rows; cols, rows <= max_side <= 64
 *   silhouette sample (c, k) is INSIDE iff |2c - (cols - 1)| * 256 * rows <= cols * (taper * rows + (256 - taper) * (k + 1)):
 *              a trapezoid centred on the grid whose top is taper / 256 of its base; taper = 256: every sample.
 *              mask_k = the inside samples of row k, n_mask their sum
 *   pixel      bytes 0..2 of the pixel are B, G, R (order == UNINA_COLOUR_BGR) or R, G, B (UNINA_COLOUR_RGB); a fourth channel
 *              is ignored. mx = max, mn = min, d = mx - mn. The first that holds: BLACK iff mx <= black_max; COLOURED iff
 *              d * 256 >= sat_min * mx and mx >= val_min (sat_min >= 1: d > 0); WHITE iff mx >= white_min; else OTHER
 *   hue        of a COLOURED pixel, 0..1535 (256 per sextant):
 *              mx == R: h = 256 * (G - B) / d where G >= B, else (1536 - 256 * (B - G) / d) % 1536
 *              else mx == G: h = 512 + 256 * (B - R) / d where B >= R, else 512 - 256 * (R - B) / d
 *              else: h = 1024 + 256 * (R - G) / d where R >= G, else 1024 - 256 * (G - R) / d
 *              The pixel votes for the first colour c in the order yellow (0), blue (1), orange (2) whose range holds h:
 *              hue_lo[c] <= h <= hue_hi[c] where lo <= hi, else h >= lo or h <= hi (a range across 0); no range: OTHER
 *   rows       per row k six counts over its inside samples: votes_k[3], white_k, black_k, mask_k
 *   body       votes[c] = the sum of votes_k[c]. best = the colour with the most votes, second = the one with the most of the
 *              other two; ties go to the earlier colour
 *   stripes    the stripe colour is BLACK where best is yellow, else WHITE. A row with mask_k > 0 is B iff
 *              2 * votes_k[best] >= mask_k, else S iff 2 * stripe_k >= mask_k, else it is dropped. n_stripes = the maximal runs
 *              of S in the string of the remaining rows (top to bottom) with a B somewhere before and a B somewhere after them
 *   class      the colour index is 3 (large orange) iff best is orange, n_stripes >= 2 and class_of[3] >= 0, else best.
 *              DECIDED iff n_mask >= min_pixels, votes[best] * 256 >= min_share * n_mask,
 *              votes[second] * 256 <= max_rival * votes[best], votes[best] > 0, n_stripes >= 1 where require_stripe != 0, and
 *              class_of[colour index] >= 0. The status bit LARGE: DECIDED with the colour index 3. class_of is a parameter
 *              because data sets disagree on the ids (yellow 0 and blue 1 in one, blue 0 and yellow 1 in another)
 *   output     d_out_dets[i] = d_dets[i] byte for byte, except class_id = class_of[colour index] where selected and DECIDED.
 *              d_colour[i], for a selected record with a window, decided or not: votes[3], n_white, n_black, n_mask, n_stripes,
 *              status = WINDOW | SELECTED | DECIDED? | LARGE? | SIZE_WINDOW? | best << 8
 *   header     n_records = n, n_selected, n_window, n_decided, n_class[colour index] over the decided: integer atomics
 * Every count is an integer: two runs give identical bytes.
 * NOT covered: cones cut by the image border (the silhouette is centred on the clipped grid), a camera that is not level, white
 * balance or exposure correction, NV12 or planar colour, raising a record's confidence, learning the thresholds from data. */
#define UNINA_COLOUR_BGR 0
#define UNINA_COLOUR_RGB 1
#define UNINA_COLOUR_YELLOW 0             /* colour indices: votes[], hue_lo[], hue_hi[], class_of[], n_class[] */
#define UNINA_COLOUR_BLUE 1
#define UNINA_COLOUR_ORANGE 2
#define UNINA_COLOUR_LARGE_ORANGE 3       /* class_of[] and n_class[] only */
#define UNINA_COLOUR_WINDOW 1             /* status bits */
#define UNINA_COLOUR_SELECTED 2
#define UNINA_COLOUR_DECIDED 4
#define UNINA_COLOUR_LARGE 8
#define UNINA_COLOUR_SIZE_WINDOW 16
#define UNINA_COLOUR_MAX_SIDE 64
typedef struct {
  float sx, sy, shrink;                   /* record -> image pixels; the share of the box (BOX or SIZE) that is sampled, (0, 1] */
  float half_width, above, below;         /* SIZE window, metres around the represented point (small cone: 0.114, 0.175, 0.15) */
  int max_side;                           /* 1..UNINA_COLOUR_MAX_SIDE samples per axis */
  int order;                              /* UNINA_COLOUR_BGR / UNINA_COLOUR_RGB */
  int only_class;                         /* < 0: every record; else the records with this class_id (the clusterer's unknown id) */
  int class_of[4];                        /* class_id written for yellow, blue, orange, large orange; < 0: never decided */
  int black_max, sat_min, val_min, white_min;   /* 0..255, 1..256 (saturation in 1/256), 0..255, 0..255 */
  int hue_lo[3], hue_hi[3];               /* 0..1535 per colour; lo > hi: a range across 0 */
  int taper;                              /* 0..256: the silhouette's top width in 1/256 of its base */
  int min_pixels, min_share, max_rival;   /* >= 1; 0..256: best's share of n_mask, second's share of best, in 1/256 */
  int require_stripe;                     /* != 0: an undecided record unless n_stripes >= 1 */
} unina_colour_params;                    /* 112 bytes */
typedef struct { int votes[3]; int n_white, n_black, n_mask, n_stripes, status; } unina_colour;                 /* 32 bytes, index-aligned with the records */
typedef struct { int n_records, n_selected, n_window, n_decided, n_class[4]; } unina_colour_header;             /* 32 bytes */

/* A memset of *d_header and one launch, enqueued on `stream`; nothing is synchronised.
 *   d_dets / d_count : device, MAX_DETECTIONS records / one int, as unina_fuse_async or the _async calls write them
 *   d_cones    : device, MAX_DETECTIONS unina_cone3d index-aligned with the records, or NULL (then no record has a SIZE window)
 *   image      : host struct; data on the device, 3 or 4 interleaved 8-bit channels, pitch in bytes. No alignment is required
 *                of data or of the pitch; no byte behind a pixel's last one is read
 *   cam        : of that image
 *   d_out_dets : device, MAX_DETECTIONS records; may be d_dets itself (in place: a workgroup reads and writes its own record only)
 *   d_colour   : device, MAX_DETECTIONS unina_colour; d_header : device, one header
 * Record arrays, d_colour and d_header are 16-byte aligned, d_count 4-byte aligned.
 * UNINA_ERR_ARG, before any HIP call: a NULL pointer other than d_cones, or a NULL image->data; a misaligned pointer; channels
 * not 3 or 4, width or height outside 1..16384, pitch < width * channels; a non-finite pinhole value, fx or fy not positive; sx
 * or sy not finite and positive, shrink outside (0, 1]; half_width, above or below not finite or negative; max_side outside
 * 1..64; order not one of the two; black_max, val_min or white_min outside 0..255, sat_min outside 1..256, a hue bound outside
 * 0..1535, taper, min_share or max_rival outside 0..256, min_pixels < 1; d_out_dets or d_colour overlapping d_dets or each other
 * over their MAX_DETECTIONS extent, except d_out_dets == d_dets exactly. */
int unina_colour_async(const GpuDetection *d_dets, const int *d_count, const unina_cone3d *d_cones, const unina_image *image,
                       const unina_pinhole *cam, const unina_colour_params *p, GpuDetection *d_out_dets, unina_colour *d_colour,
                       unina_colour_header *d_header, hipStream_t stream);

/* ------------------------------------------------------------------ tracking (cones are static landmarks: no motion model)
 * The frame's records, their unina_cone3d points and the camera's pose in a fixed frame -> a persistent table of tracks on the
 * device: stable ids, smoothed positions, hit and miss counts. One launch per frame (csrc/track.hip: one workgroup of 1024
 * threads) enqueued behind unina_locate_async on the same stream; nothing is synchronised and nothing crosses to the host until
 * unina_track_read. tracking.update_numpy is the definition, decision for decision and bit for bit. Everything is fp32, each
 * operation rounded once in the order written, never contracted.
 *   count     n = *d_count clamped to 0..MAX_DETECTIONS, on the device
 *   point     record j < n: px = ((r00 * x + r01 * y) + r02 * z) + t0, py and pz from rows 1 and 2 of the pose ([R|t], row-major
 *             3 x 4, camera frame -> tracking frame). USABLE iff cones[j].valid != 0 and px, py, pz are all finite; the record's
 *             own `valid` is ignored, as in unina_locate_async
 *   gate      (slot s with id != 0, usable j) is a CANDIDATE iff (class_aware == 0 or track.class_id == dets[j].class_id) and
 *             d2 <= gate * gate, with dx = px - track.x (dy, dz likewise) and d2 = (dx * dx + dy * dy) + dz * dz. A NaN d2 fails;
 *             d2 is never negative, so its bits order as an unsigned integer
 *   match     greedy over all candidates in ascending (d2 bits, s, j); a pair is taken iff its slot and its record are both free
 *   matched   x = x + alpha * dx with the dx of the gate (y, z likewise); confidence and class_id are the record's;
 *             hits = min(hits + 1, 1 000 000 000); missed = 0
 *   unmatched live slot: missed += 1 (it stays at INT_MAX); missed > max_missed: the slot becomes all-zero bytes (a death)
 *   births    usable unmatched records with confidence >= birth_confidence (a NaN confidence fails), in ascending j, go to the
 *             free slots in ascending s, the slots freed by this update's deaths included: (px, py, pz, confidence, id = next_id++,
 *             class_id, hits = 1, missed = 0). A birth is DROPPED when no slot is left or next_id has reached INT_MAX
 *   assign    assign[j] = id of the track record j matched or founded, else 0; all MAX_DETECTIONS words are written by every update
 *   header    frame += 1; n_matched, n_born, n_died, n_dropped are of this update; n_live and n_confirmed (hits >= confirm_hits)
 *             are of the table after it
 * Integer counters and a fixed order of every fp32 operation: two runs give identical bytes. */
#define UNINA_TRACK_MAX 1024
typedef struct { float x, y, z, confidence; int id, class_id, hits, missed; } unina_track;   /* 32 bytes; id 0 = free slot = all-zero bytes */
typedef struct { int frame, n_live, n_confirmed, next_id, n_matched, n_born, n_died, n_dropped; } unina_track_header;   /* 32 bytes */
typedef struct {
  float pose[12];                        /* row-major 3 x 4 [R|t]: camera frame -> tracking frame (odometry, or the identity) */
  float gate, alpha, birth_confidence;   /* metres; smoothing step in (0, 1]; lowest confidence that may found a track       */
  int class_aware, confirm_hits, max_missed;
} unina_track_params;
typedef struct unina_tracker unina_tracker_t;

/* Host only: no HIP call. The device memory (the header and UNINA_TRACK_MAX slots) is allocated -- and reset -- by the first
 * reset / update / read, on that call's stream, which then fails with UNINA_ERR_HIP where there is no device.
 * UNINA_ERR_ARG: NULL out, negative device_id. */
int unina_track_create(int device_id, unina_tracker_t **out);
/* Waits for the device, frees. NULL is a no-op. */
void unina_track_destroy(unina_tracker_t *t);
/* Empty table, frame = 0, next_id = 1; enqueued on `stream`. */
int unina_track_reset_async(unina_tracker_t *t, hipStream_t stream);
/* One frame, enqueued on `stream`; nothing is synchronised.
 *   d_dets / d_count : device, MAX_DETECTIONS records (16-byte aligned) / one int, as the _async calls write them
 *   d_cones          : device, MAX_DETECTIONS unina_cone3d (16-byte aligned), as unina_locate_async writes them
 *   d_assign         : device, MAX_DETECTIONS ints, or NULL (stored 16 bytes at a time where it is 16-byte aligned)
 * UNINA_ERR_ARG, before any HIP call: a NULL t, d_dets, d_count, d_cones or p; d_dets or d_cones not 16-byte aligned, d_count or
 * d_assign not 4-byte aligned; a non-finite pose element; gate not finite and positive, or gate * gate not finite (with a finite
 * gate * gate no update stores a NaN coordinate, whose sign would be the processor's); alpha outside (0, 1]; a NaN
 * birth_confidence; confirm_hits < 1; max_missed < 0. */
int unina_track_update_async(unina_tracker_t *t, const GpuDetection *d_dets, const int *d_count, const unina_cone3d *d_cones,
                             const unina_track_params *p, int *d_assign, hipStream_t stream);
/* Device addresses of the table and the header, for a consumer that stays on the GPU (read them behind the update on its
 * stream). Either out pointer may be NULL. UNINA_ERR_STATE before the first reset / update / read. */
int unina_track_buffers(unina_tracker_t *t, const unina_track **d_tracks, const unina_track_header **d_header);
/* Synchronises `stream`, then copies out the header and min(cap, UNINA_TRACK_MAX) slots (tracks may be NULL when cap is 0). */
int unina_track_read(unina_tracker_t *t, unina_track_header *hdr, unina_track *tracks, size_t cap, hipStream_t stream);

/* ------------------------------------------------------------------ pose from the tracked cones (behind any locator,
 * unina_fuse_async or unina_colour_async, in front of unina_track_update_async)
 * The tracker takes the camera's pose on trust, and odometry drifts. The tracker's confirmed tracks are static landmarks with
 * smoothed positions, resident on the device: this stage aligns the frame's located cones with them by a planar rigid correction
 * -- a yaw about the tracking frame's z axis (z is up) plus (tx, ty) -- and writes the corrected camera -> tracking pose and the
 * frame's unina_cone3d records moved into the tracking frame, in place if wanted. The tracker then runs behind it unchanged with
 * the IDENTITY pose. Stateless: one memset of the 32-byte header and ONE launch (csrc/pose.hip: one workgroup of 1024 threads) on
 * the caller's stream; nothing is synchronised. pose.pose_numpy is the definition, bit for bit. Every fp32 and float64 operation
 * is rounded once in the order written, never contracted.
 *   prior     d_prev == NULL: P = inc, the prior camera -> tracking pose. Else P = d_prev->pose o inc, and inc is this frame's
 *             camera -> the last frame's camera, which is what odometry gives: the estimate never returns to the host between
 *             frames. Row-major 3 x 4 [R|t], fp32: P[4r+k] = ((a[4r] * b[k] + a[4r+1] * b[4+k]) + a[4r+2] * b[8+k]), + a[4r+3]
 *             where k == 3, with a = d_prev->pose and b = inc
 *   count     n = *d_count clamped to 0..MAX_DETECTIONS, on the device
 *   point     record j < n: (px, py, pz) as unina_track_update_async's point with the pose P. USABLE iff cones[j].valid != 0, the
 *             point is finite and |px|, |py| <= 32768
 *   landmark  a slot with id != 0, hits >= min_hits and |x|, |y| <= 32768 (a NaN fails)
 *   loop      the correction starts as (c, s, tx, ty) = (1, 0, 0, 0); then `iterations` times:
 *     move      qx = (c * px - s * py) + tx, qy = (s * px + c * py) + ty, qz = pz
 *     candidate (landmark k, usable j) iff (class_aware == 0 or track.class_id == dets[j].class_id) and d2 <= gate * gate, d2 as
 *               the tracker's with q for the point. A NaN d2 fails
 *     pairs     record j picks the least (d2 bits, k) over its candidates, landmark k the least (d2 bits, j); a PAIR is a mutual
 *               choice. ONE round, not the tracker's chain of rounds: a record whose landmark prefers another record does not
 *               vote in this iteration. N = the number of pairs
 *     too few   N < min_pairs: status = UNINA_POSE_TOO_FEW and the loop ends; the correction of the earlier iterations stays
 *     sums      over the pairs, in 64-bit integers of 2^-10 m of the UNMOVED point and the landmark (ipx = rint(px * 1024); ipy,
 *               imx, imy likewise): N, Spx, Spy, Smx, Smy, Sdot = sum(ipx * imx + ipy * imy), Scross = sum(ipx * imy - ipy * imx).
 *               Exact and free of any order: a term is below 2^51 and 1024 of them below 2^61. Every iteration solves for the
 *               whole correction, so no error is composed
 *     rotation  float64: A = Sdot - (Spx * Smx + Spy * Smy) / N, B = Scross - (Spx * Smy - Spy * Smx) / N. fp32: Af = (float)A,
 *               Bf = (float)B, h = sqrtf(Af * Af + Bf * Bf). h finite and > 0: c = Af / h, s = Bf / h, status = UNINA_POSE_OK.
 *               Else c = 1, s = 0 and status = UNINA_POSE_DEGENERATE (all pairs at one point); the loop goes on
 *     translation  float64 with (double)c, (double)s: tx = (float)(((Smx - (c * Spx - s * Spy)) / N) / 1024),
 *               ty = (float)(((Smy - (s * Spx + c * Spy)) / N) / 1024)
 *   out cones record j < n: x, y, z = the move of its point under the final correction (for a record that is not usable: of
 *             whatever the point came out as; a NaN's sign and payload are the processor's), every other field copied. Records
 *             from n on are copied unchanged
 *   result    c, s, tx, ty and the corrected pose: pose[k] = (c * P[k] - s * P[4+k]), pose[4+k] = (s * P[k] + c * P[4+k]), + tx
 *             and + ty where k == 3; row 2 is P's
 *   header    n_records = n; n_usable; n_landmarks; n_pairs and max_d2_bits (the bits of the largest pair d2, 0 without a pair)
 *             are of the last pairing made, a too small one included; iterations = those that updated the correction; status =
 *             that of the last iteration run
 * Integer sums, integer minima and maxima and a fixed order of every floating operation: two runs give identical bytes, and any
 * order of the records gives the same result and header wherever no two candidate d2 tie.
 * NOT covered: roll, pitch and height correction; re-orthonormalising a long d_prev chain (re-seed with d_prev = NULL);
 * outlier-robust weights; loop closure; feeding the estimate to unina_deskew_table. */
typedef struct { float inc[12]; float gate; int class_aware, min_hits, iterations, min_pairs; } unina_pose_params;   /* 68 bytes */
typedef struct { float pose[12]; float c, s, tx, ty; } unina_pose_result;                                             /* 64 bytes, device */
typedef struct { int n_records, n_usable, n_landmarks, n_pairs, iterations, status; uint32_t max_d2_bits; int reserved; } unina_pose_header;   /* 32 bytes */
enum { UNINA_POSE_OK = 0, UNINA_POSE_TOO_FEW = 1, UNINA_POSE_DEGENERATE = 2 };
#define UNINA_POSE_MAX_ITERATIONS 8
/*   d_dets / d_count / d_cones : device, as unina_track_update_async takes them
 *   d_tracks    : device, UNINA_TRACK_MAX slots, 16-byte aligned (unina_track_buffers)
 *   d_prev      : device, 16-byte aligned, or NULL
 *   d_out_cones : device, MAX_DETECTIONS unina_cone3d, 16-byte aligned; may be d_cones
 *   d_result    : device, 16-byte aligned; may be d_prev
 *   d_header    : device, 16-byte aligned
 * UNINA_ERR_ARG, before any HIP call: a NULL pointer other than d_prev; a misaligned pointer (d_count: 4 bytes); d_out_cones
 * overlapping d_cones without being equal to it, d_result and d_prev likewise; a non-finite inc element; gate not finite and
 * positive, or gate * gate not finite; min_hits < 1; iterations outside 1..UNINA_POSE_MAX_ITERATIONS; min_pairs < 2. */
int unina_pose_async(const GpuDetection *d_dets, const int *d_count, const unina_cone3d *d_cones, const unina_track *d_tracks,
                     const unina_pose_result *d_prev, const unina_pose_params *p, unina_cone3d *d_out_cones,
                     unina_pose_result *d_result, unina_pose_header *d_header, hipStream_t stream);

/* ------------------------------------------------------------------ track limits and centre line from the tracked cones (behind
 * unina_track_update_async)
 * The tracker's table is an unordered set of points; a driverless car needs the left limit and the right limit as ORDERED
 * polylines and the line between them. This stage reads the table where it lies on the device (unina_track_buffers) and the
 * camera's pose (unina_pose_async's d_result, or the parameters'), chains the confirmed cones of each side from the vehicle
 * onwards and walks the two chains as a ladder. Stateless: one memset of the 32-byte header and ONE launch (csrc/boundary.hip:
 * one workgroup of 1024 threads) on the caller's stream; nothing is synchronised. boundary.boundary_numpy is the definition, bit
 * for bit. Everything is fp32, each operation rounded once in the order written, never contracted.
 *   origin    P = d_pose->pose, or p->pose where d_pose == NULL. o = (P[3], P[7]); the heading h: hx = (P[0] * f0 + P[1] * f1) +
 *             P[2] * f2 with f = forward, hy the same from row 1. Where o is not finite, or hx * hx + hy * hy is not finite and
 *             > 0: end[0] = end[1] = UNINA_BOUNDARY_NO_HEADING, every other word of the header and every point is zero
 *   candidate slot s of side k iff id != 0, hits >= min_hits, class_id == class_left (k = 0) or class_right (k = 1), and |x|, |y|
 *             <= 32768 (a NaN fails). z is carried and never tested. n_candidates[k] counts them
 *   chain     per side, links m = 0, 1, ...: the current point c is o for m = 0, else the chain's last point; the direction d is h
 *             for m = 0 and m = 1, else the last point minus the one before, per component. For a candidate not yet in the chain
 *             dx = x - cx, dy = y - cy, d2 = dx * dx + dy * dy, dot = dx * d.x + dy * d.y. ELIGIBLE for m = 0 iff d2 <= first_gate
 *             * first_gate and dot >= 0; for m >= 1 iff d2 <= step_gate * step_gate, dot > 0 and dot * dot >= cos2 * (d2 * (d.x *
 *             d.x + d.y * d.y)), cos2 = cos_turn * cos_turn computed once on the host. A NaN fails every test. The link takes the
 *             eligible candidate with the least (d2 bits, slot) and writes (x, y, z, ref = the track's id). Without one, end[k] =
 *             UNINA_BOUNDARY_NO_FIRST (m = 0) or UNINA_BOUNDARY_NO_NEXT; a chain of max_chain points ends UNINA_BOUNDARY_FULL
 *   centre    a ladder walk over the chains L and R; n_centre = 0 where either is empty. From i = j = 0: w2 = d2(L[i], R[j]) in the
 *             plane with dx = L.x - R.x; w2 <= width_gate * width_gate: the rung's point ((L.x + R.x) * 0.5f, y and z likewise,
 *             ref = i | j << 16) is written, else n_wide += 1. The walk stops when neither i + 1 < nL nor j + 1 < nR; it advances i
 *             if i + 1 < nL and either j + 1 >= nR or d2(L[i+1], R[j]) <= d2(L[i], R[j+1]), else j. At most 127 rungs. A track's z
 *             is copied as it is; the sign and payload of a NaN that a rung's z sum produces are the processor's
 *   points    d_points[0, 64) the left chain, [64, 128) the right chain, [128, 256) the centre line. Every call writes all 256
 *             points and the header; entries behind their count are all-zero bytes
 * Integer minima and a fixed order of every fp32 operation: two runs give identical bytes, and any order of the slots gives the
 * same points and header wherever no two eligible candidates tie in d2.
 * NOT covered: a track seen on one side only (offsetting one chain); orange start / finish cones; closing the loop; smoothing or
 * splines; curvature and speed; a Delaunay or graph search in place of the greedy chain. */
#define UNINA_BOUNDARY_MAX_CHAIN 64
typedef struct {
  float pose[12];      /* row-major 3 x 4 [R|t], camera -> tracking frame; read only when d_pose == NULL            */
  float forward[3];    /* the vehicle's forward axis in the camera frame: (0,0,1) pinhole camera, (1,0,0) level frame */
  float first_gate, step_gate, cos_turn, width_gate;   /* m; m; cosine of the widest turn between two links, [0, 1); m */
  int class_left, class_right, min_hits, max_chain;    /* class ids differ between data sets, as in unina_colour_params */
} unina_boundary_params;                                                                  /* 92 bytes */
typedef struct { float x, y, z; int ref; } unina_boundary_point;                          /* 16 bytes */
typedef struct { int n_candidates[2], n_chain[2], end[2], n_centre, n_wide; } unina_boundary_header;   /* 32 bytes; [0] left, [1] right */
enum { UNINA_BOUNDARY_NO_FIRST = 0, UNINA_BOUNDARY_NO_NEXT = 1, UNINA_BOUNDARY_FULL = 2, UNINA_BOUNDARY_NO_HEADING = 3 };
/*   d_tracks : device, UNINA_TRACK_MAX slots, 16-byte aligned (unina_track_buffers)
 *   d_pose   : device, 16-byte aligned (unina_pose_async's d_result), or NULL: p->pose is the pose
 *   d_points : device, 4 * UNINA_BOUNDARY_MAX_CHAIN points, 16-byte aligned
 *   d_header : device, 16-byte aligned
 * UNINA_ERR_ARG, before any HIP call: a NULL d_tracks, p, d_points or d_header; a pointer that is not 16-byte aligned, d_pose
 * included; a non-finite pose element while d_pose == NULL (with d_pose set, pose is not read); a non-finite forward element; a
 * gate that is not finite and positive, or whose square is not finite; cos_turn NaN or outside [0, 1); min_hits < 1; max_chain
 * outside 1..UNINA_BOUNDARY_MAX_CHAIN; a negative class id, or class_left == class_right; d_points overlapping d_header. */
int unina_boundary_async(const unina_track *d_tracks, const unina_pose_result *d_pose, const unina_boundary_params *p,
                         unina_boundary_point *d_points, unina_boundary_header *d_header, hipStream_t stream);

/* Error text of the last failing call on this handle (never NULL). With e == NULL: last load failure. */
const char *unina_last_error(const unina_engine_t *e);

/* ------------------------------------------------------------------ introspection / measurement */

typedef struct unina_op_info {
  char name[96];      /* reference module path(s), e.g. "head_p3.cls_branch.0+head_p3.reg_branch.0" */
  char kernel[64];    /* device kernel (template instantiation) that executes it */
  int kind;           /* 1 conv, 2 stem, 3 sppf pool, 4 upsample */
  int m, n, k;        /* implicit-GEMM shape (pixels, out channels, taps*in channels); 0 for non-conv */
  double flops;       /* 2*m*n*k */
  double bytes;       /* algorithmic bytes: inputs once + weights once + outputs once */
  int grid, block;    /* launch geometry */
} unina_op_info;

int unina_op_count(const unina_engine_t *e);
int unina_get_op_info(const unina_engine_t *e, int index, unina_op_info *info);

/* Times every op of the forward with HIP events on `stream`, INSIDE the frame sequence: each of the `iters`
 * repetitions replays ops 0..i-1 and then times op i alone, so the op meets the cache state of a real frame (weights
 * not L2-resident). Event-to-event time of a single launch: like rocprofv3's kernel duration it includes the
 * dispatch cost (the two agree within a few percent). ms_per_op[i] = mean milliseconds of op i (0 for ops that run
 * inside a fused block's launch). Used by bench.py's roofline leg. */
int unina_profile_ops(unina_engine_t *e, int iters, float *ms_per_op, hipStream_t stream);

/* The same for the post-process launches of a frame (each repetition replays the whole forward first): ms2[0] = decode
 * launch (including the head output convs folded into it; ops the frame leaves out because of that report 0 in
 * unina_profile_ops), ms2[1] = pair tiles + greedy scan + output launch (0 if the post-process is one launch). */
int unina_profile_post(unina_engine_t *e, int iters, float conf_threshold, float iou_threshold, float conformal_q, float *ms2,
                       hipStream_t stream);

/* Tile-configuration control of the implicit-GEMM conv kernel (autotuning, tests). cfg = -1 restores the heuristic.
 * Returns UNINA_ERR_UNSUPPORTED if the configuration does not fit the op's shape. */
int unina_conv_config_count(void);
const char *unina_conv_config_name(int cfg);
int unina_set_op_config(unina_engine_t *e, int op_index, int cfg);
/* Times every fitting configuration of every conv op (`iters` launches each, in the frame sequence like
 * unina_profile_ops, HIP events on `stream`) and keeps the
 * fastest -- the engine-build "tactic selection" the reference leaves to TensorRT (export_trt.py:459-468).
 * Needs "images" bound. Results are bit-identical under every configuration. */
int unina_autotune(unina_engine_t *e, int iters, hipStream_t stream);

/* Block fusion (fp16 engines). At load the engine recognises every C3k2 block of the op table (the reference's
 * model.py:76-110: cv1|cv2 -> n x Bottleneck -> cv3) and, while fusion is on (the default; UNINA_FUSE=0 in the
 * environment starts with it off), runs each as ONE launch that keeps the block's intermediates in LDS
 * (csrc/c3k2_fused.hip) -- the role of TensorRT's layer fusion in the reference's engine build. Results are
 * bit-identical either way; with fusion on the blocks' internal buffers are not written (unina_debug_read_buffer of
 * e.g. "neck.pan_c3k2_1.cat" then returns stale data), so per-layer checks and calibration switch it off.
 * unina_fusion_groups: number of blocks currently running fused (0 when off / none recognised). */
int unina_set_fusion(unina_engine_t *e, int enable);
int unina_fusion_groups(const unina_engine_t *e);
/* Load-time analysis alone, no device needed: runs exactly the host-side checks and fusion matchers of
 * unina_load_engine on the engine file and returns the number of fused groups it finds (C3k2 blocks, heads, conv
 * pairs), or -code where unina_load_engine would fail with that code before touching the device. */
int unina_debug_fusable_groups(const char *path);

/* Copies an internal activation buffer to the host as fp32 NCHW ([C,H,W]) -- parity tests only.
 * `name` is a buffer name from the engine file (e.g. "p3_fused"); returns UNINA_ERR_ARG if unknown. */
int unina_debug_read_buffer(unina_engine_t *e, const char *name, float *host_out, size_t capacity_floats,
                            int *c, int *h, int *w);

/* Debug: wall_clock64 stamps (100 MHz) of the phases of the last unina_infer's post-process launches; only written
 * when the environment has UNINA_POST_STAMPS=1. out16 (16 values): [7] launch 1 starts (workgroup 0), [0] its decode is
 * done, [1] last arriver found, [2] candidates gathered (launch 1 ends), [3] launch 2 starts, [4] its last arriver
 * found (all pair tiles done), [8] ranks / masks loaded, [9] per-class row lists built, [5] greedy scan done, [6] output
 * written, [10..13] scan wave v = 0..3: its number of rows in bits 0..19, the low clock bits at its end from bit 20 up.
 * (The one-launch form uses [0..6] as decode, hand-off, gather, sort, masks, scan, output.) Slots 14 and 15 are unused. */
int unina_debug_post_stamps(unina_engine_t *e, long long *out16);

/* Debug: one launch of conv op `op_index` with in-kernel s_memtime stamps of a mid-grid workgroup:
 * out5 = start, prologue issued, first operands usable, K loop done, stores drained (shader-clock ticks). */
int unina_debug_conv_stamps(unina_engine_t *e, int op_index, long long *out5, hipStream_t stream);

/* Debug: the same for the DUAL conv launch led by op `op_index` (two independent convs as one grid, e.g. the P3 | P4 head
 * layers): out16[0..7] = stamps of conv A's mid workgroup, out16[8..15] = conv B's (each: start, loads issued, patch
 * landed, K loop done, stores issued, 2 x 100 MHz reference). UNINA_ERR_ARG if the op does not lead such a launch. */
int unina_debug_dual_stamps(unina_engine_t *e, int op_index, long long *out16, hipStream_t stream);
/* Debug: the same launch with every workgroup's start / end on the 100 MHz wall clock (out[2*i], out[2*i+1]); returns the
   grid size or a negative error code. */
int unina_debug_dual_timeline(unina_engine_t* e, int op_index, long long* out, int cap, hipStream_t stream);
/* Debug: the fused C3k2 block led by op `op_index` run once as a stamped twin (after the ops in front of it): out16[k] =
 * shader-clock stamp of its mid workgroup after step k (0 entry, 1 patch landed, 2 pre-conv, 3 cv1|cv2, 4 b0.cv1, 5 b0.cv2,
 * 6 b1.cv1, 7 last bottleneck, 8 cv3, 9 output stored, 10 tail conv, 11 drained), [14] / [15] = 100 MHz clock at end / entry.
 * Only the 40x40-level blocks have twins (UNINA_ERR_HIP otherwise). */
int unina_debug_block_stamps(unina_engine_t *e, int op_index, long long *out16, hipStream_t stream);
/* Debug, read-only: which heads' output convs the decode launch of unina_infer computes itself (folded), as the frame stands
 * now: bit h (0 = P2, 1 = P3, 2 = P4) set = that head is not read from its planes. Negative error code for a null handle. */
int unina_debug_folded_heads(unina_engine_t *e);
/* Debug: the number of streams the library itself holds in this process, all handles together. The runtime maps streams onto
 * GPU_MAX_HW_QUEUES hardware queues per priority (default 4) as they are created, and two streams on one queue run one after
 * the other, so an idle stream of the library's could cost the caller the overlap of two frames in flight. The library makes
 * a stream only for the duration of a graph capture (the first call of a plan): the count is 0 whenever no call is running.
 * (create_preprocess_stream hands its stream to the caller and is not counted.) */
int unina_debug_owned_streams(void);
/* Debug: do streams `a` and `b` of device `device` run on the chip at the same time, or one after the other (one hardware
 * queue)? `reps` (1..64) times: one single-wave kernel on each stream that holds its compute unit for 300 us of the 100 MHz
 * wall clock and waits for nothing else, then both streams are synchronised. stamps (host, reps x 4): start and end of the
 * kernel on `a`, start and end of the one on `b`; *overlapped = the repetitions whose two intervals intersect. a == b is the
 * negative control: 0. Work already queued on the streams runs first. tools/stream_queues.py prints the matrix for the two
 * frame streams and the null stream. */
int unina_debug_streams_overlap(int device, hipStream_t a, hipStream_t b, int reps, long long *stamps, int *overlapped);

/* Library/build identification: "unina_mi355 <version> gfx950". */
const char *unina_version(void);

/* ------------------------------------------------------------------ multi-GPU: the gather of detection slots, over RCCL
 * SURVEY.md section 8e. The path shards by frame: one process per GPU, the engine file loaded by each, NO data-path collective;
 * the only exchange is an all-gather of fixed-size detection records (e.g. k slots of 8 + 8 * MAX_DETECTIONS int32 words, as
 * bench.py / gather.py use) so that one rank -- the node that publishes -- sees every GPU's detections. The reference has no
 * counterpart (one GPU, one stream: perception_node.cpp:472,802); these entry points are what its node would call with
 * several MI355X (INTEGRATION.md "Several GPUs"). RCCL is loaded on first use: single-GPU consumers never touch it, and
 * unina_comm_* return UNINA_ERR_UNSUPPORTED (message in unina_comm_last_error) where librccl is absent.
 * Issue the gather on a stream of its own behind an event of the frames it carries, as gather.SlotRing does: the call only
 * enqueues (RCCL semantics), inference streams need not wait for it. */
#define UNINA_COMM_ID_BYTES 128
typedef struct unina_comm unina_comm;
/* rank 0: 128 opaque bytes to hand to every rank out of band (file, socket, MPI, ROS parameter ...) */
int unina_comm_unique_id(void *id128);
/* every rank, collectively: joins the communicator `id128` as `rank` of `world` on HIP device `device_id` */
int unina_comm_init(unina_comm **out, const void *id128, int rank, int world, int device_id);
/* d_send: bytes_per_rank bytes on this rank's device; d_recv: world * bytes_per_rank bytes, rank-major. Enqueued on `stream`. */
int unina_comm_all_gather(unina_comm *c, const void *d_send, void *d_recv, size_t bytes_per_rank, hipStream_t stream);
int unina_comm_rank(const unina_comm *c);
int unina_comm_world(const unina_comm *c);
void unina_comm_destroy(unina_comm *c);
const char *unina_comm_last_error(void);

/* ------------------------------------------------------------------ post-process C API (gpu_postprocess.h:42-80)
 * Same seven symbols, same argument meaning, hipError_t/hipStream_t in place of cudaError_t/cudaStream_t
 * (ABI-identical: int + pointer), so perception_node.cpp:627-656 recompiles unchanged under HIP.
 * Semantics are the deterministic ones of SURVEY.md App. D (the reference kernel's atomic append order and
 * racy NMS are not reproducible by construction). One process-global workspace, like the reference
 * (gpu_postprocess.cu:56-57); the engine handles above each own a private one instead. */
hipError_t init_postprocess_resources(void);
hipError_t cleanup_postprocess_resources(void);
hipError_t reset_detection_counter(hipStream_t stream);
hipError_t get_detection_count(int *count, hipStream_t stream);
hipError_t decode_yolo_head(const float *d_cls, const float *d_reg, GpuDetection *d_detections, int grid_w,
                            int grid_h, int stride, int num_classes, float conf_threshold, float conformal_q,
                            hipStream_t stream);
hipError_t run_gpu_nms(GpuDetection *d_detections, int num_detections, float iou_threshold, hipStream_t stream);
hipError_t copy_valid_detections_to_host(const GpuDetection *d_detections, GpuDetection *h_detections,
                                         int num_detections, int *out_valid_count, hipStream_t stream);

/* ------------------------------------------------------------------ pre-process C API (cuda_preprocess.h:50-112)
 * The step right before the engine in processGpuBuffer (perception_node.cpp:601-604): camera buffer -> fp32 RGB
 * planar "images" tensor. Same names, argument order and error behaviour as the reference (allocators and the
 * stream factory return NULL on failure, cuda_preprocess.cu:395-428); arithmetic per cuda_preprocess.cu:99-253. */

NormParams create_norm_params_imagenet(void);
NormParams create_norm_params(float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b);
hipError_t preprocess_bgra_resize(const uint8_t *d_input, float *d_output, int src_width, int src_height,
                                  int src_pitch, int dst_width, int dst_height, NormParams params,
                                  hipStream_t stream);
hipError_t preprocess_bgra(const uint8_t *d_input, float *d_output, int width, int height, int pitch,
                           NormParams params, hipStream_t stream);
hipError_t preprocess_nv12(const uint8_t *d_y_plane, const uint8_t *d_uv_plane, float *d_output, int width,
                           int height, int y_pitch, int uv_pitch, NormParams params, hipStream_t stream);
/* Not in the reference (its NV12 path cannot resize): NV12 of any size -> the dst_width x dst_height tensor, by the definition
 * at unina_infer_nv12 above; with dst == src it is preprocess_nv12. Odd sizes are legal (chroma plane: (src_height + 1) / 2
 * rows); hipErrorInvalidValue for a null pointer, a non-positive size, y_pitch < src_width, uv_pitch < src_width or
 * < 2 * ((src_width + 1) / 2). */
hipError_t unina_preprocess_nv12_resize(const uint8_t *d_y_plane, const uint8_t *d_uv_plane, float *d_output, int src_width,
                                        int src_height, int y_pitch, int uv_pitch, int dst_width, int dst_height,
                                        NormParams params, hipStream_t stream);
/* The letterbox as a step of its own (the definition at unina_letterbox_geometry above): camera frame -> the dst_width x
 * dst_height tensor, resized into the inner rectangle, pad_value around it. Arguments as preprocess_bgra_resize /
 * unina_preprocess_nv12_resize plus pad_value; hipErrorInvalidValue for what those refuse, and for a BGRA pitch or address that
 * is not a multiple of 4. */
hipError_t unina_preprocess_letterbox_bgra(const uint8_t *d_input, float *d_output, int src_width, int src_height,
                                           int src_pitch, int dst_width, int dst_height, float pad_value, NormParams params,
                                           hipStream_t stream);
hipError_t unina_preprocess_letterbox_nv12(const uint8_t *d_y_plane, const uint8_t *d_uv_plane, float *d_output, int src_width,
                                           int src_height, int y_pitch, int uv_pitch, int dst_width, int dst_height,
                                           float pad_value, NormParams params, hipStream_t stream);
/* The pre-process of a unina_frame as a step of its own (the definitions at unina_pixel_format above): `region` (NULL: the whole
 * frame) of the frame -> the dst_w x dst_h tensor, tapped where the region has that size, resized otherwise; and the letterbox of
 * the whole frame. Formats 0 and 1 run the kernels of the calls above. 0, or UNINA_ERR_ARG (what the frame checks refuse, a NULL
 * pointer, a non-positive size, a region that is empty or not inside the frame), or UNINA_ERR_HIP. */
int unina_preprocess_frame(const unina_frame *frame, const unina_tile *region, float *d_output, int dst_width, int dst_height,
                           const NormParams *params, hipStream_t stream);
int unina_preprocess_letterbox_frame(const unina_frame *frame, float *d_output, int dst_width, int dst_height, float pad_value,
                                     const NormParams *params, hipStream_t stream);
float *allocate_preprocess_buffer(int width, int height);
void free_preprocess_buffer(float *d_buffer);
hipStream_t create_preprocess_stream(void);
void destroy_preprocess_stream(hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UNINA_MI355_H */
