// preprocess.hip -- camera-buffer pre-processing on the GPU (gfx950): the step right before the engine in the
// reference's processGpuBuffer (perception_node.cpp:601-604), behind the reference's C API names. The ARITHMETIC per
// pixel is defined once, in camera_source.h (plain BGRA, BGRA resize, NV12, NV12 resize, RGB / RGBA / 4:2:2 / Bayer, the letterbox of
// every format); the
// stem kernels call the same functions, so unina_infer_bgra / _nv12 / _letterbox_*'s in-stem form equals the two-step form, and
// both are compared bit for bit with oracle/preprocess_oracle.c and the numpy twins (camera.py).
// The DATA MOVEMENT is not the reference's one-thread-per-pixel form: all three are HBM-bound byte movers (4 B/px in,
// 12 B/px out), so ONE kernel template, thread = FOUR consecutive output pixels of a row: the no-resize paths read the
// quad with one 16-byte load (BGRA) or one dword of luma + one dword of chroma (NV12: 2 chroma pairs for 4 pixels), every
// path writes one 16-byte store per output plane (a wave: 1 KiB contiguous per plane per instruction instead of 256 B),
// and a flat grid-stride loop over the quads replaces the 2-D grid. Row tails (width % 4) and unaligned tensors fall back to
// scalar accesses inside the same kernel. Built with -ffp-contract=off so the expression trees round exactly as written.
#include <cmath>
#include <cstdio>
#include <hip/hip_runtime.h>

#include "../../include/unina_mi355.h"
#include "camera_source.h"

#pragma clang fp contract(off)

namespace {

using namespace unina;

// MODE of the kernel template: the CameraKind of the source (never kSrcTensor). kSrcBgraTap, kSrcNv12Tap and (for packed 4:2:2
// and Bayer frames) kSrcFrameTap have quad loads of their own; the others go through camera_pixel with the constant kind.
struct PreParams {
  CameraSource cam;       // the frame; cam.dst_w x cam.dst_h is the output size
  float* out;             // [3][dst_h][dst_w]
};

template <int MODE>
__global__ __launch_bounds__(256) void preprocess_quads_kernel(const PreParams p) {
  const CameraSource& q = p.cam;
  const int dw = q.dst_w, dh = q.dst_h;
  const int qpr = (dw + 3) >> 2;                           // quads per output row
  const long long nquads = (long long)qpr * dh;
  const size_t plane = (size_t)dw * dh;
  // wide accesses only where they are aligned: every row of the output starts 16-byte aligned iff dw % 4 == 0 and the
  // tensor does; every row of the source iff the pitch and the base allow it
  const bool wide_out = (dw & 3) == 0 && ((uintptr_t)p.out & 15) == 0;
  bool wide_in = false;                                    // (the camera_pixel modes read per tap)
  if constexpr (MODE == kSrcBgraTap) {
    wide_in = (q.pitch & 15) == 0 && ((uintptr_t)q.plane & 15) == 0;
  } else if constexpr (MODE == kSrcNv12Tap) {
    bool wide_y, wide_c;
    nv12_quad_alignment(q, wide_y, wide_c);
    wide_in = wide_y && wide_c;
  } else if constexpr (MODE == kSrcFrameTap) {
    wide_in = cam_is_yuv422(q.format) ? yuv422_quad_alignment(q) : (cam_is_bayer(q.format) && bayer_quad_alignment(q));
  }
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nquads; t += (long long)gridDim.x * blockDim.x) {
    const int y = (int)(t / qpr), x = (int)(t - (long long)y * qpr) * 4;
    const int n = dw - x < 4 ? dw - x : 4;                 // pixels of this quad inside the row
    float o[4][3];
    if constexpr (MODE == kSrcBgraTap) {
      BgraPixel px[4];
      if (wide_in && n == 4) {
        const uint4 v = *reinterpret_cast<const uint4*>(q.plane + (size_t)y * q.pitch + (size_t)x * 4);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) px[i] = BgraPixel{(uint8_t)w[i], (uint8_t)(w[i] >> 8), (uint8_t)(w[i] >> 16), (uint8_t)(w[i] >> 24)};
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) px[i] = i < n ? bgra_tap(q, x + i, y) : BgraPixel{0, 0, 0, 0};
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) cam_normalise(q.norm, (float)px[i].r, (float)px[i].g, (float)px[i].b, o[i]);
    } else if constexpr (MODE == kSrcNv12Tap) {
      // (the region's origin: 0 for the whole frame, where x is even by construction; a region of unina_preprocess_frame may start
      // at an odd column, and then the chroma pairs straddle the quad)
      nv12_quad(q, q.x0 + x, q.y0 + y, n, (q.x0 & 1) == 0, wide_in && n == 4, wide_in && n == 4, o);
    } else if constexpr (MODE == kSrcFrameTap) {
      // (the format is uniform over the grid; RGB / RGBA stay per pixel)
      if (cam_is_yuv422(q.format)) {
        yuv422_quad(q, q.format, q.x0 + x, q.y0 + y, n, wide_in && n == 4, o);
      } else if (cam_is_bayer(q.format)) {
        bayer_quad(q, q.format, q.x0 + x, q.y0 + y, n, wide_in && n == 4, o);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < n) camera_pixel(q, MODE, x + i, y, o[i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < n) camera_pixel(q, MODE, x + i, y, o[i]);
    }
    const size_t idx = (size_t)y * dw + x;
    if (wide_out) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(p.out + c * plane + idx) = make_float4(o[0][c], o[1][c], o[2][c], o[3][c]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < n) {
#pragma unroll
          for (int c = 0; c < 3; ++c) p.out[c * plane + idx + i] = o[i][c];
        }
    }
  }
}

template <int MODE>
hipError_t launch_quads(const PreParams& q, hipStream_t stream) {
  const long long nquads = (long long)((q.cam.dst_w + 3) / 4) * q.cam.dst_h;
  long long blocks = (nquads + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;                 // grid-stride beyond 16 workgroups per CU
  preprocess_quads_kernel<MODE><<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(q);
  return hipGetLastError();
}

// One launch of `region` into the dst_width x dst_height tensor as `kind` (frame_kind's answer, or the kind a reference-named entry
// point is defined as); lb: the inner rectangle of the letterbox kinds
hipError_t launch_frame(const CameraSource& region, int kind, float* d_output, int dst_width, int dst_height, hipStream_t stream,
                        const unina_letterbox* lb = nullptr, float pad_value = 0.f) {
  const PreParams q{launch_source(region, kind, dst_width, dst_height, lb, pad_value), d_output};
  switch (kind) {
    case kSrcBgraTap: return launch_quads<kSrcBgraTap>(q, stream);
    case kSrcBgraResize: return launch_quads<kSrcBgraResize>(q, stream);
    case kSrcNv12Tap: return launch_quads<kSrcNv12Tap>(q, stream);
    case kSrcNv12Resize: return launch_quads<kSrcNv12Resize>(q, stream);
    case kSrcBgraLetterbox: return launch_quads<kSrcBgraLetterbox>(q, stream);
    case kSrcNv12Letterbox: return launch_quads<kSrcNv12Letterbox>(q, stream);
    case kSrcFrameTap: return launch_quads<kSrcFrameTap>(q, stream);
    case kSrcFrameResize: return launch_quads<kSrcFrameResize>(q, stream);
    case kSrcFrameLetterbox: return launch_quads<kSrcFrameLetterbox>(q, stream);
  }
  return hipErrorInvalidValue;
}
int code_of(hipError_t err) { return err == hipSuccess ? UNINA_OK : UNINA_ERR_HIP; }

// The whole frame of a format-named entry point (BGRA: uv == nullptr)
CameraSource plane_source(const uint8_t* plane, const uint8_t* uv, int w, int h, int pitch, int uv_pitch, const NormParams& norm) {
  return frame_source(unina_frame{uv ? UNINA_FMT_NV12 : UNINA_FMT_BGRA, w, h, {plane, uv}, {pitch, uv_pitch}}, norm);
}

}  // namespace

extern "C" {

NormParams create_norm_params_imagenet(void) {  // cuda_preprocess.cu:262 (defaults :73-75)
  NormParams p = {0.485f, 0.456f, 0.406f, 0.229f, 0.224f, 0.225f};
  return p;
}

NormParams create_norm_params(float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b) {
  NormParams p = {mean_r, mean_g, mean_b, std_r, std_g, std_b};
  return p;
}

hipError_t preprocess_bgra_resize(const uint8_t* d_input, float* d_output, int src_width, int src_height, int src_pitch,
                                  int dst_width, int dst_height, NormParams params, hipStream_t stream) {
  if (!d_input || !d_output || src_width <= 0 || src_height <= 0 || dst_width <= 0 || dst_height <= 0 || src_pitch < 4 * src_width)
    return hipErrorInvalidValue;
  return launch_frame(plane_source(d_input, nullptr, src_width, src_height, src_pitch, 0, params), kSrcBgraResize, d_output, dst_width, dst_height, stream);
}

hipError_t preprocess_bgra(const uint8_t* d_input, float* d_output, int width, int height, int pitch, NormParams params,
                           hipStream_t stream) {
  if (!d_input || !d_output || width <= 0 || height <= 0 || pitch < 4 * width || (pitch & 3)) return hipErrorInvalidValue;
  return launch_frame(plane_source(d_input, nullptr, width, height, pitch, 0, params), kSrcBgraTap, d_output, width, height, stream);
}

hipError_t preprocess_nv12(const uint8_t* d_y_plane, const uint8_t* d_uv_plane, float* d_output, int width, int height,
                           int y_pitch, int uv_pitch, NormParams params, hipStream_t stream) {
  if (!d_y_plane || !d_uv_plane || !d_output || width <= 0 || height <= 0 || y_pitch < width || uv_pitch < width)
    return hipErrorInvalidValue;
  return launch_frame(plane_source(d_y_plane, d_uv_plane, width, height, y_pitch, uv_pitch, params), kSrcNv12Tap, d_output, width, height, stream);
}

// NV12 of any size -> the dst_width x dst_height tensor (camera_source.h defines the resize; the reference has none). At
// dst == src it is preprocess_nv12, launch included. Odd sizes are legal: the chroma plane then has (src_height + 1) / 2 rows,
// and the last pair of an odd-width row is read whole, hence uv_pitch >= 2 * ((src_width + 1) / 2).
hipError_t unina_preprocess_nv12_resize(const uint8_t* d_y_plane, const uint8_t* d_uv_plane, float* d_output, int src_width,
                                        int src_height, int y_pitch, int uv_pitch, int dst_width, int dst_height,
                                        NormParams params, hipStream_t stream) {
  if (!d_y_plane || !d_uv_plane || !d_output || src_width <= 0 || src_height <= 0 || dst_width <= 0 || dst_height <= 0 ||
      y_pitch < src_width || uv_pitch < src_width || uv_pitch < 2 * ((src_width + 1) / 2))
    return hipErrorInvalidValue;
  const bool same = dst_width == src_width && dst_height == src_height;
  return launch_frame(plane_source(d_y_plane, d_uv_plane, src_width, src_height, y_pitch, uv_pitch, params), same ? kSrcNv12Tap : kSrcNv12Resize,
                      d_output, dst_width, dst_height, stream);
}

// Host only. Python's round() is round-half-to-even: nearbyint in the default rounding mode (lround rounds halves away from zero:
// 5 x 128 into 64 x 64 has r = 0.5 and new_w = round(2.5) = 2, not 3).
int unina_letterbox_geometry(int src_w, int src_h, int dst_w, int dst_h, unina_letterbox* out) {
  if (!out || src_w <= 0 || src_h <= 0 || dst_w <= 0 || dst_h <= 0) return -UNINA_ERR_ARG;
  const double rh = (double)dst_h / src_h, rw = (double)dst_w / src_w;
  const double r = rh < rw ? rh : rw;
  int new_w = (int)nearbyint(src_w * r), new_h = (int)nearbyint(src_h * r);
  if (new_w < 1) new_w = 1;
  if (new_h < 1) new_h = 1;
  out->new_w = new_w;
  out->new_h = new_h;
  out->left = (int)nearbyint((dst_w - new_w) / 2.0 - 0.1);
  out->top = (int)nearbyint((dst_h - new_h) / 2.0 - 0.1);
  return UNINA_OK;
}

hipError_t unina_preprocess_letterbox_bgra(const uint8_t* d_input, float* d_output, int src_width, int src_height, int src_pitch,
                                           int dst_width, int dst_height, float pad_value, NormParams params, hipStream_t stream) {
  unina_letterbox lb;
  if (!d_input || !d_output || src_pitch < 4 * src_width || (src_pitch & 3) || ((uintptr_t)d_input & 3) ||
      unina_letterbox_geometry(src_width, src_height, dst_width, dst_height, &lb) != UNINA_OK)
    return hipErrorInvalidValue;
  return launch_frame(plane_source(d_input, nullptr, src_width, src_height, src_pitch, 0, params), kSrcBgraLetterbox, d_output, dst_width, dst_height, stream,
                      &lb, pad_value);
}

hipError_t unina_preprocess_letterbox_nv12(const uint8_t* d_y_plane, const uint8_t* d_uv_plane, float* d_output, int src_width,
                                           int src_height, int y_pitch, int uv_pitch, int dst_width, int dst_height,
                                           float pad_value, NormParams params, hipStream_t stream) {
  unina_letterbox lb;
  if (!d_y_plane || !d_uv_plane || !d_output || unina_letterbox_geometry(src_width, src_height, dst_width, dst_height, &lb) != UNINA_OK ||
      y_pitch < src_width || uv_pitch < src_width || uv_pitch < 2 * ((src_width + 1) / 2))
    return hipErrorInvalidValue;
  return launch_frame(plane_source(d_y_plane, d_uv_plane, src_width, src_height, y_pitch, uv_pitch, params), kSrcNv12Letterbox, d_output,
                      dst_width, dst_height, stream, &lb, pad_value);
}

// ---- a unina_frame of any format (include/unina_mi355.h at unina_pixel_format) ----
int unina_preprocess_frame(const unina_frame* frame, const unina_tile* region, float* d_output, int dst_width, int dst_height,
                           const NormParams* params, hipStream_t stream) {
  if (frame_defect(frame) || !d_output || !params || dst_width <= 0 || dst_height <= 0) return UNINA_ERR_ARG;
  const unina_tile whole = {0, 0, frame->width, frame->height};
  const unina_tile& r = region ? *region : whole;
  if (r.w <= 0 || r.h <= 0 || r.x < 0 || r.y < 0 || (long long)r.x + r.w > frame->width || (long long)r.y + r.h > frame->height) return UNINA_ERR_ARG;
  const int kind = frame_kind(frame->format, r.w, r.h, dst_width, dst_height, nullptr);
  return code_of(launch_frame(frame_region(frame_source(*frame, *params), r.x, r.y, r.w, r.h), kind, d_output, dst_width, dst_height, stream));
}

int unina_preprocess_letterbox_frame(const unina_frame* frame, float* d_output, int dst_width, int dst_height, float pad_value,
                                     const NormParams* params, hipStream_t stream) {
  unina_letterbox lb;
  if (frame_defect(frame) || !d_output || !params || unina_letterbox_geometry(frame->width, frame->height, dst_width, dst_height, &lb) != UNINA_OK)
    return UNINA_ERR_ARG;
  const int kind = frame_kind(frame->format, frame->width, frame->height, dst_width, dst_height, &lb);
  return code_of(launch_frame(frame_source(*frame, *params), kind, d_output, dst_width, dst_height, stream, &lb, pad_value));
}

float* allocate_preprocess_buffer(int width, int height) {  // nullptr on failure (cuda_preprocess.cu:395-405)
  float* d = nullptr;
  if (width <= 0 || height <= 0) return nullptr;
  hipError_t err = hipMalloc(&d, (size_t)3 * width * height * sizeof(float));
  if (err != hipSuccess) {
    fprintf(stderr, "Failed to allocate preprocess buffer: %s\n", hipGetErrorString(err));
    return nullptr;
  }
  return d;
}

void free_preprocess_buffer(float* d_buffer) {
  if (d_buffer) (void)hipFree(d_buffer);
}

hipStream_t create_preprocess_stream(void) {  // nullptr on failure (cuda_preprocess.cu:419-428)
  hipStream_t s = nullptr;
  hipError_t err = hipStreamCreate(&s);
  if (err != hipSuccess) {
    fprintf(stderr, "Failed to create HIP stream: %s\n", hipGetErrorString(err));
    return nullptr;
  }
  return s;
}

void destroy_preprocess_stream(hipStream_t stream) {
  if (stream) (void)hipStreamDestroy(stream);
}

}  // extern "C"
