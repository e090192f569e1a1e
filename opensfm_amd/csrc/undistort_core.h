// undistort_core.h -- the per-pixel numerics of image undistortion (opensfm/undistort.py: pygeometry.compute_camera_mapping of
// geometry/src/camera.cc:319-342, cv2.remap, cv2.resize(INTER_NEAREST), render_perspective_view_of_a_panorama), for the device, the
// host emulation and the tests.  undistort.hip adds the lanes, the kernels and the C ABI.
//
// The camera models are NOT restated here: the bearing is osfm_rp::pixel_bearing_generic (relpose_core.h), the projection
// osfm_ba::project_generic (ba_math.h); the spherical projection, which the bundle adjustment never needed, is the only addition.
//
// OpenCV is not available to this project, so cv2.remap and cv2.resize are RESTATED from memory of OpenCV, unpinned:
//   remap INTER_LINEAR (uint8; INTER_AREA is treated as INTER_LINEAR, as cv2.remap does):  sx = round_half_even(x * 32), the integer part
//     sx >> 5 (arithmetic shift: floor), the fraction fx = sx & 31; the four taps get the int32 weights 32 (32 - fx)(32 - fy),
//     32 fx (32 - fy), 32 (32 - fx) fy, 32 fx fy (sum 32768); out = (sum tap * weight + 16384) >> 15, the same weights for every channel;
//   remap INTER_NEAREST:  the tap (round_half_even(x), round_half_even(y));
//   BORDER_CONSTANT: a tap outside the image reads 0;  BORDER_WRAP: a tap index is taken modulo the size, non-negative, in both axes;
//   resize INTER_NEAREST to (W', H'):  src_x = min(floor(X * (1.0 / ((double)W' / W))), W - 1), the same in y.
// Divergences (include/osfm_mi355.h lists them for callers):
//   - a map entry that is NaN or infinite, or whose rounded (fixed-point) value does not fit int32, gives 0 in either border mode
//     (OpenCV's cast is undefined there);
//   - sides above 32767 are refused (OpenCV's int16 maps cannot address them either);  only uint8 with 1, 3 or 4 channels.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ba_math.h"
#include "relpose_core.h"  // OSFM_HD, pixel_bearing_generic

namespace osfm_und {

constexpr int kMaxSide = 32767;
enum Interpolation { kNearest = 0, kLinear = 1, kArea = 3 };  // cv2.INTER_NEAREST, INTER_LINEAR, INTER_AREA
enum Border { kConstant = 0, kWrap = 3 };                      // cv2.BORDER_CONSTANT, BORDER_WRAP
enum MapKind { kCameraMapping = 0, kPanoramaView = 1 };

struct Camera {
  double par[16];  // native order, as osfm_pixel_bearings
  int model, pad;
};

// one map: destination pixels of a w x h image -> float source coordinates
struct MapJob {
  Camera from, to;  // kCameraMapping: the distorted and the undistorted camera;  kPanoramaView: the panorama's and the view's
  double R[9];      // kPanoramaView: R_pano R_view^T, row-major (a view bearing b goes to R b)
  int64_t off;      // und_map_kernel: first float of this map in map1 / map2
  int kind, w, h;
  int src_w, src_h;  // kPanoramaView: size of the panorama the coordinates address
  int pad;
};

// one remap: dst (out_w x out_h x channels) from src (src_w x src_h x channels) through a map of map_w x map_h
struct RemapJob {
  const uint8_t *src;
  const float *map1, *map2;  // null in the fused kernel
  uint8_t *dst;
  int src_w, src_h, map_w, map_h, out_w, out_h, channels, pad;
};

// SphericalProjection::Forward (camera_projections_functions.h:214-223)
__device__ inline void spherical_project(const double *X, double *out) {
  const double lon = atan2(X[0], X[2]);
  const double lat = atan2(-X[1], sqrt(X[0] * X[0] + X[2] * X[2]));
  const double inv_norm = 1.0 / (2.0 * M_PI);
  out[0] = lon * inv_norm;
  out[1] = -lat * inv_norm;
}

// Camera::Project for every model
__device__ inline void camera_project(const Camera &c, const double *X, double *out) {
  if (c.model == OSFM_CAMERA_SPHERICAL)
    spherical_project(X, out);
  else
    osfm_ba::project_generic<false, true>(c.model, c.par, X, out, nullptr);  // x / z, as the reference's Forward
}

// The map entry of destination pixel (u, v), narrowed to float as the reference stores it.
//   kCameraMapping  ComputeCameraMapping (camera.cc:319-342), literally, in double;
//   kPanoramaView   render_perspective_view_of_a_panorama (undistort.py:360-403): normalized_image_coordinates, the view's bearing,
//                   the rotation, the panorama's projection, denormalized_image_coordinates.
__device__ inline void map_pixel(const MapJob &J, int u, int v, float *x, float *y) {
  double b[3], p[2];
  if (J.kind == kCameraMapping) {
    const int normalizer_factor = J.w > J.h ? J.w : J.h;
    const double inv_normalizer_factor = 1.0 / normalizer_factor;
    const double half_width = J.w * 0.5, half_height = J.h * 0.5;
    const double uv0 = u - half_width, uv1 = v - half_height;
    osfm_rp::pixel_bearing_generic(J.to.model, J.to.par, inv_normalizer_factor * uv0, inv_normalizer_factor * uv1, b);
    camera_project(J.from, b, p);
    *x = (float)(normalizer_factor * p[0] + half_width);
    *y = (float)(normalizer_factor * p[1] + half_height);
    return;
  }
  // the destination pixels are a float32 array there, and numpy keeps float32 through "+ 0.5 - width / 2.0) / size"
  const float size = (float)(J.w > J.h ? J.w : J.h);
  const double src_size = J.src_w > J.src_h ? J.src_w : J.src_h;
  const float px = ((float)u + 0.5f - (float)(J.w / 2.0)) / size, py = ((float)v + 0.5f - (float)(J.h / 2.0)) / size;
  osfm_rp::pixel_bearing_generic(J.to.model, J.to.par, (double)px, (double)py, b);
  double rb[3];
  for (int i = 0; i < 3; i++) rb[i] = b[0] * J.R[3 * i] + b[1] * J.R[3 * i + 1] + b[2] * J.R[3 * i + 2];
  camera_project(J.from, rb, p);
  *x = (float)(p[0] * src_size - 0.5 + J.src_w / 2.0);
  *y = (float)(p[1] * src_size - 0.5 + J.src_h / 2.0);
}

// round_half_even(x * scale) as an int32; false when x is not finite or the value does not fit
OSFM_HD bool round_to_int(float x, double scale, int32_t *out) {
  const double s = rint((double)x * scale);  // x * 32 is exact in double; rint rounds half to even in the default mode
  if (!(s >= -2147483648.0 && s <= 2147483647.0)) return false;  // (NaN fails both)
  *out = (int32_t)s;
  return true;
}

// the fixed-point split of a coordinate: integer part (floor) and the 5-bit fraction
OSFM_HD bool split_coordinate(float x, int32_t *i, int32_t *f) {
  int32_t s;
  if (!round_to_int(x, 32.0, &s)) return false;
  *i = s >> 5;
  *f = s & 31;
  return true;
}

// the index a tap reads in an axis of n pixels, -1 for "outside" (BORDER_CONSTANT)
OSFM_HD int tap_index(int32_t i, int n, int border) {
  if (i >= 0 && i < n) return i;
  if (border != kWrap) return -1;
  const int32_t m = i % n;
  return m < 0 ? m + n : m;
}

// nearest resize: the source index of destination index X when n pixels become n_out
OSFM_HD int resize_index(int X, int n_out, int n) {
  const double inv_scale = 1.0 / ((double)n_out / n);
  const int s = (int)floor(X * inv_scale);
  return s < n - 1 ? s : n - 1;
}

// one output pixel of `channels` bytes sampled at (x, y)
template <int C>
OSFM_HD void sample_pixel(const uint8_t *src, int w, int h, float x, float y, int interpolation, int border, uint8_t *out) {
  for (int c = 0; c < C; c++) out[c] = 0;
  if (interpolation == kNearest) {
    int32_t ix, iy;
    if (!round_to_int(x, 1.0, &ix) || !round_to_int(y, 1.0, &iy)) return;
    const int tx = tap_index(ix, w, border), ty = tap_index(iy, h, border);
    if (tx < 0 || ty < 0) return;
    const uint8_t *p = src + ((size_t)ty * w + tx) * C;
    for (int c = 0; c < C; c++) out[c] = p[c];
    return;
  }
  int32_t ix, iy, fx, fy;
  if (!split_coordinate(x, &ix, &fx) || !split_coordinate(y, &iy, &fy)) return;
  const int tx0 = tap_index(ix, w, border), tx1 = tap_index(ix + 1, w, border);
  const int ty0 = tap_index(iy, h, border), ty1 = tap_index(iy + 1, h, border);
  const int32_t wgt[4] = {32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy), 32 * (32 - fx) * fy, 32 * fx * fy};
  const int txs[4] = {tx0, tx1, tx0, tx1}, tys[4] = {ty0, ty0, ty1, ty1};
  int32_t acc[C];
  for (int c = 0; c < C; c++) acc[c] = 16384;
  for (int t = 0; t < 4; t++) {
    if (txs[t] < 0 || tys[t] < 0) continue;
    const uint8_t *p = src + ((size_t)tys[t] * w + txs[t]) * C;
    for (int c = 0; c < C; c++) acc[c] += (int32_t)p[c] * wgt[t];
  }
  for (int c = 0; c < C; c++) out[c] = (uint8_t)(acc[c] >> 15);
}

}  // namespace osfm_und
