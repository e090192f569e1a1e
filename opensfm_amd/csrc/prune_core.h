// prune_core.h -- the per-pixel rule of dense::DepthmapPruner::Prune (opensfm/src/dense/src/depthmap.cc:565-625), for the device, the host
// and the host emulation of the tests.  prune.hip adds the lanes, the ordered compaction and the C ABI.
//
// Like depthmap_core.h this RESTATES depthmap.cc: float32 where it uses float, double where it uses double, its order of operations, no
// contraction.  The types are the pruner's, not the cleaner's: the reprojection stays a Vec3d, the pixel it lands on is found by
// truncation toward zero of x / z + 0.5 (a value in (-1, 0) lands on row or column 0), and the depth bound is a double.
// What the restatement takes from memory of OpenCV and has NOT compared with its source (besides what depthmap_core.h lists):
//   - cv::normalize(Vec3f): nv = sqrt of the squares summed in double, k = 0, 1, 2;  v * (nv ? 1. / nv : 0.), each product formed in
//     double and rounded to float;
//   - Matx33f * Vec3f: float products summed k = 0, 1, 2.
// Divergences from depthmap.cc, both in place of undefined or implementation-defined behaviour (include/osfm_mi355.h lists them):
//   1. x / z + 0.5 that is NaN, infinite or 2^31 or more in magnitude counts as outside the image (the reference casts it to int64);
//   2. the reference narrows that int64 to the int of IsInsideImage: the same values count as outside here.
#pragma once
#include "depthmap_core.h"

namespace osfm_dm {

struct PruneView {
  double K[9], R[9], t[3];
  const float *depth, *plane;  // (h, w) and (h, w, 3)
  int w, h;
};
struct PruneProblem {
  double Kinv[9];             // K_0^-1
  float Rinv[9];              // R_0 transposed, narrowed to a Matx33f
  int64_t view0, pix0, blk0;  // first view, first keep flag, first block count
  const uint8_t *color, *label;  // of view 0: (h, w, 3) and (h, w)
  int n_views, w, h, pad;
};

// cv::normalize(Vec3f)
OSFM_HD void normalize3_cv(const float *v, float *out) {
  double s = 0.0;
  for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
  const double nv = sqrt(s);
  const double scale = nv != 0.0 ? 1.0 / nv : 0.0;
  for (int k = 0; k < 3; k++) out[k] = (float)((double)v[k] * scale);
}

// the row or column static_cast<int64>(q + 0.5) names, or false where that cast is undefined or does not fit IsInsideImage's int
OSFM_HD bool landing(double q, int64_t *at) {
  const double r = q + 0.5;
  if (!(fabs(r) < 2147483648.0)) return false;
  *at = (int64_t)r;
  return true;
}

// what Prune computes of pixel (i, j) before it looks at the other views; false when depth <= 0 skips the pixel (a NaN does not)
OSFM_HD bool prune_point(const PruneView &v0, const PruneProblem &P, int i, int j, float *depth, float *normal, float *point) {
  *depth = v0.depth[(int64_t)i * P.w + j];
  if (*depth <= 0.0f) return false;
  normalize3_cv(v0.plane + 3 * ((int64_t)i * P.w + j), normal);
  double X[3];
  backproject((double)j, (double)i, (double)*depth, P.Kinv, v0.R, v0.t, X);
  for (int k = 0; k < 3; k++) point[k] = (float)X[k];
  return true;
}

// DepthmapPruner::Prune for one pixel: is it kept?  The reference's `break` does not change an AND over the views.
OSFM_HD bool prune_pixel(const PruneView *views, const PruneProblem &P, float same_depth_threshold, int i, int j) {
  const PruneView &v0 = views[P.view0];
  float depth, normal[3], pointf[3];
  if (!prune_point(v0, P, i, j, &depth, normal, pointf)) return false;
  const float area = (float)((double)(-normal[2] / depth) * v0.K[0]);
  const double point[3] = {(double)pointf[0], (double)pointf[1], (double)pointf[2]};
  const double bound = (double)(1.0f - same_depth_threshold);
  bool keep = true;
  for (int other = 1; other < P.n_views; ++other) {
    const PruneView &vo = views[P.view0 + other];
    double rp[3];
    project(point, vo.K, vo.R, vo.t, rp);
    if (rp[2] < 1e-8 || rp[2] != rp[2]) continue;
    int64_t iu, iv;
    if (!landing(rp[0] / rp[2], &iu) || !landing(rp[1] / rp[2], &iv)) continue;
    if (!(iv >= 0 && iv < vo.h && iu >= 0 && iu < vo.w)) continue;
    const float depth_at = vo.depth[iv * vo.w + iu];
    if ((double)depth_at > bound * rp[2]) {
      float normal_at[3];
      normalize3_cv(vo.plane + 3 * (iv * vo.w + iu), normal_at);
      if (depth_at == 0.0f || (double)(-normal_at[2] / depth_at) * vo.K[0] > (double)area) keep = false;
    }
  }
  return keep;
}

// what a kept pixel emits: the point, Rinv * normal, the colour and the label
OSFM_HD void prune_emit(const PruneView *views, const PruneProblem &P, int i, int j, float *point, float *normal, uint8_t *color, uint8_t *label) {
  float depth, n[3];
  prune_point(views[P.view0], P, i, j, &depth, n, point);
  for (int r = 0; r < 3; r++) normal[r] = (P.Rinv[3 * r] * n[0] + P.Rinv[3 * r + 1] * n[1]) + P.Rinv[3 * r + 2] * n[2];
  const int64_t pix = (int64_t)i * P.w + j;
  for (int k = 0; k < 3; k++) color[k] = P.color[3 * pix + k];
  *label = P.label[pix];
}

}  // namespace osfm_dm
