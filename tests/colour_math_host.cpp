// colour_math_host.cpp -- stand-alone host driver of csrc/colour_math.h for tests/test_colour_cpu.py: one whole call of
// unina_colour_async restated as scalar loops over the functions csrc/colour.hip calls -- the window, the silhouette, the pixel
// fetch, the pixel's bin, the row letters, the stripe count and the decision -- built by a host compiler (no HIP, no GPU) and run
// on a case from a file. The image lies in a heap buffer of exactly its size, so under -fsanitize=address a fetch behind a
// pixel's last byte is reported.
//   colour_math_host IN OUT
// IN : 12 int32 -- magic, count, m (records in the file), has_cones, width, height, pitch, channels, offset, image bytes, 2 float32
//      bits fx, fy -- then the 112 bytes of unina_colour_params, m GpuDetection, m unina_cone3d (where has_cones), the image bytes
// OUT: the unina_colour_header, MAX_DETECTIONS GpuDetection, MAX_DETECTIONS unina_colour
#include "../unina-yolo-dla_amd/csrc/colour_math.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace unina;

static_assert(sizeof(unina_colour_params) == 112 && sizeof(unina_colour) == 32 && sizeof(unina_colour_header) == 32, "layouts");

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  union {
    int32_t i[12];
    float f[12];
  } h;
  if (fread(h.i, sizeof h.i, 1, f) != 1 || h.i[0] != 0x434f4c31) return 4;
  const int count = h.i[1], m = h.i[2], has_cones = h.i[3], width = h.i[4], height = h.i[5], pitch = h.i[6], channels = h.i[7], offset = h.i[8];
  const size_t bytes = (size_t)h.i[9];
  const float fx = h.f[10], fy = h.f[11];
  if (m < 0 || m > MAX_DETECTIONS || width < 1 || height < 1 || (channels != 3 && channels != 4) || pitch < width * channels || offset < 0 ||
      bytes != (size_t)offset + (size_t)(height - 1) * (size_t)pitch + (size_t)width * (size_t)channels)
    return 4;
  unina_colour_params p;
  std::vector<GpuDetection> dets((size_t)m);
  std::vector<unina_cone3d> cones((size_t)m);
  uint8_t* buf = (uint8_t*)malloc(bytes);   // exactly the image: the allocator's red zone starts behind the last pixel
  if (!buf || fread(&p, sizeof p, 1, f) != 1) return 4;
  if (m && fread(dets.data(), sizeof(GpuDetection), (size_t)m, f) != (size_t)m) return 4;
  if (m && has_cones && fread(cones.data(), sizeof(unina_cone3d), (size_t)m, f) != (size_t)m) return 4;
  if (fread(buf, 1, bytes, f) != bytes) return 4;
  fclose(f);
  if (p.max_side < 1 || p.max_side > UNINA_COLOUR_MAX_SIDE) return 4;
  const uint8_t* data = buf + offset;

  unina_colour_header head;
  memset(&head, 0, sizeof head);
  std::vector<GpuDetection> out(MAX_DETECTIONS);
  std::vector<unina_colour> colour(MAX_DETECTIONS);
  memset(out.data(), 0, sizeof(GpuDetection) * MAX_DETECTIONS);
  memset(colour.data(), 0, sizeof(unina_colour) * MAX_DETECTIONS);
  int n = count < 0 ? 0 : (count > MAX_DETECTIONS ? MAX_DETECTIONS : count);
  n = n > m ? m : n;
  head.n_records = n;
  for (int i = 0; i < n; ++i) {
    out[i] = dets[i];
    if (!(p.only_class < 0 || dets[i].class_id == p.only_class)) continue;
    head.n_selected += 1;
    colour[i].status = UNINA_COLOUR_SELECTED;
    const unina_cone3d& c3 = cones[i];
    const ColourWindow cw =
        colour_window(dets[i].x1, dets[i].y1, dets[i].x2, dets[i].y2, has_cones, c3.valid, c3.u, c3.v, c3.z, fx, fy, p, width, height);
    if (cw.w.empty) continue;
    head.n_window += 1;
    const LocateWindow& w = cw.w;
    if (w.rows > 64 || w.cols > 64 || w.u0 < 0 || w.v0 < 0 || w.u0 + (w.cols - 1) * w.stride_x >= width || w.v0 + (w.rows - 1) * w.stride_y >= height)
      return 6;   // the grid the kernel's LDS and loads rely on
    int rows[64][kColourBins];
    memset(rows, 0, sizeof rows);
    for (int k = 0; k < w.rows; ++k)
      for (int c = 0; c < w.cols; ++c) {
        if (!colour_inside(c, k, w.cols, w.rows, p.taper)) continue;
        const uint8_t* px = data + (size_t)(w.v0 + k * w.stride_y) * (size_t)pitch + (size_t)(w.u0 + c * w.stride_x) * (size_t)channels;
        const int bin = colour_pixel(colour_fetch(px, channels), p);
        if (bin >= 0) rows[k][bin] += 1;
        rows[k][kColourMask] += 1;
      }
    int tot[kColourBins] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < w.rows; ++k)
      for (int b = 0; b < kColourBins; ++b) tot[b] += rows[k][b];
    int best, second;
    colour_rank(tot, &best, &second);
    uint64_t body = 0, stripe = 0;
    for (int k = 0; k < w.rows; ++k) {
      const int letter = colour_row_letter(rows[k][kColourMask], colour_pick(rows[k], best), rows[k][best == UNINA_COLOUR_YELLOW ? kColourBlack : kColourWhite]);
      if (letter == 1) body |= 1ull << k;
      if (letter == 2) stripe |= 1ull << k;
    }
    const int n_stripes = colour_stripes(body, stripe);
    const ColourDecision d = colour_decide(tot, best, second, tot[kColourMask], n_stripes, p);
    colour[i].votes[0] = tot[0];
    colour[i].votes[1] = tot[1];
    colour[i].votes[2] = tot[2];
    colour[i].n_white = tot[kColourWhite];
    colour[i].n_black = tot[kColourBlack];
    colour[i].n_mask = tot[kColourMask];
    colour[i].n_stripes = n_stripes;
    colour[i].status = colour_status(cw.size, best, d);
    if (d.decided) {
      out[i].class_id = d.class_id;
      head.n_decided += 1;
      head.n_class[d.index] += 1;
    }
  }
  free(buf);
  f = fopen(argv[2], "wb");
  if (!f || fwrite(&head, sizeof head, 1, f) != 1 || fwrite(out.data(), sizeof(GpuDetection), MAX_DETECTIONS, f) != MAX_DETECTIONS ||
      fwrite(colour.data(), sizeof(unina_colour), MAX_DETECTIONS, f) != MAX_DETECTIONS || fclose(f))
    return 5;
  return 0;
}
