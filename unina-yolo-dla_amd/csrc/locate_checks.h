// locate_checks.h -- the argument checks unina_locate_async (csrc/locate.hip) and unina_locate_stereo_async (csrc/stereo.hip)
// share, as host functions: a plane's size, the pinhole, and the window's and the depth range's parameters. Each entry point
// adds the checks that are its own and touches HIP only after the last one has passed.
#ifndef UNINA_LOCATE_CHECKS_H
#define UNINA_LOCATE_CHECKS_H

#include "locate_window.h"
#include "record_io.h"

namespace unina {

inline bool plane_dims_ok(int width, int height) { return width >= 1 && height >= 1 && width <= kLocateMaxDim && height <= kLocateMaxDim; }

inline bool pinhole_ok(const unina_pinhole* cam) {
  return cam && finite_pos(cam->fx) && finite_pos(cam->fy) && finite(cam->cx) && finite(cam->cy);
}

inline bool window_params_ok(float sx, float sy, float shrink, float min_depth, float max_depth) {
  return finite_pos(sx) && finite_pos(sy) && shrink > 0.0f && shrink <= 1.0f && min_depth > 0.0f && min_depth < max_depth && finite(max_depth);
}

}  // namespace unina
#endif  // UNINA_LOCATE_CHECKS_H
