// depthmap_core.h -- the per-pixel numerics of dense::DepthmapEstimator and dense::DepthmapCleaner (opensfm/src/dense/src/depthmap.cc),
// for the device, the host and the host emulation of the tests.  depthmap.hip adds the lanes, the kernels and the C ABI.
//
// OpenCV is not available to this project, so depthmap.cc is RESTATED: float32 where it uses float, double where it uses double, its
// order of operations, no contraction.  What the restatement takes from memory of OpenCV and has NOT compared with its source:
//   - Matx33d::inv(): cofactors times the reciprocal of the determinant (inverse3_cv);
//   - Matx products: each entry summed k = 0, 1, 2;  Vec3f / float: a product with 1.f / alpha;  Vec3f::dot: a float sum in index order;
//   - cv::medianBlur(CV_32F, 5): the exact median of the 5 x 5 window with a replicated border.
// Divergences from depthmap.cc (include/osfm_mi355.h lists them for callers):
//   - a sample coordinate that is NaN reads as 0 (the reference casts it to int, which is undefined);
//   - the bilateral weight is read from a table of exp() evaluated in double on the host and rounded to float (the reference calls expf:
//     at most one ulp apart);
//   - every random variate is a pure function of (seed, sweep, pixel, draw) through splitmix64's finaliser and host-built tables;
//   - the other neighbour is drawn by an offset, not by redrawing;  with a single view no candidate is ever scored in a view: PatchMatch
//     keeps score -1 and nghbr 0 in both modes, brute force stays all-zero (the reference's sample mode scores view 0 against itself).
// Also unpinned: whether the unqualified exp() of lines 344 / 473 and fabs() of line 485 resolve to the float or the double overload.
#pragma once
#include <math.h>
#include <stdint.h>

#include "relpose_core.h"  // OSFM_HD

namespace osfm_dm {

constexpr int kMaxPatch = 15;                                      // largest patch_size
constexpr int kMaxViews = 32;                                      // views of one problem, view 0 included
constexpr int kR2 = 2 * (kMaxPatch / 2) * (kMaxPatch / 2) + 1;     // dx^2 + dy^2 of the weight table: 0 .. 98
constexpr int kQuantiles = 4096;                                   // entries of the standard normal table (12 draw bits)
constexpr int kPerturb = 6;                                        // random planes of PatchMatchUpdatePixel
constexpr int kDrawsPerSweep = 32;                                 // draw indices a pixel owns in one sweep (19 are used)
enum Method { kBruteForce = 0, kPatchMatch = 1, kPatchMatchSample = 2 };

struct View {
  double K[9], Q[9], a[3];  // K_o, Q_o = R_o R_0^T, a_o = Q_o t_0 - t_o (AddView)
  const uint8_t *image;
  int w, h;
};

struct Problem {
  double Kinv[9];           // K_0^-1
  double min_depth, max_depth;
  int64_t view0, pix0, scr0;  // first view, first output pixel, first scratch float
  const uint8_t *mask;      // of view 0
  const float *init_depth;  // kQuantiles initial depths of this problem's range (PatchMatch)
  int n_views, w, h, pad;
};

struct Tables {
  const float *normal;  // kQuantiles
  const float *factor;  // kPerturb x kQuantiles
  const float *weight;  // 256 x kR2
};

struct Params {
  uint64_t seed;
  int patch_size, iterations, num_planes, method;
  float min_patch_variance;
};

struct Out {
  float *depth, *plane, *score;
  int32_t *nghbr;
};

// ---- small matrices as cv::Matx does them ----
OSFM_HD void inverse3_cv(const double *a, double *b) {
  double d = a[0] * (a[4] * a[8] - a[7] * a[5]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
  d = 1.0 / d;
  b[0] = (a[4] * a[8] - a[5] * a[7]) * d;
  b[1] = (a[2] * a[7] - a[1] * a[8]) * d;
  b[2] = (a[1] * a[5] - a[2] * a[4]) * d;
  b[3] = (a[5] * a[6] - a[3] * a[8]) * d;
  b[4] = (a[0] * a[8] - a[2] * a[6]) * d;
  b[5] = (a[2] * a[3] - a[0] * a[5]) * d;
  b[6] = (a[3] * a[7] - a[4] * a[6]) * d;
  b[7] = (a[1] * a[6] - a[0] * a[7]) * d;
  b[8] = (a[0] * a[4] - a[1] * a[3]) * d;
}
OSFM_HD void mat33_mul(const double *a, const double *b, double *c) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}
OSFM_HD void mat33_vec(const double *a, const double *x, double *y) {
  for (int i = 0; i < 3; i++) y[i] = (a[3 * i] * x[0] + a[3 * i + 1] * x[1]) + a[3 * i + 2] * x[2];
}
OSFM_HD bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }

// AddView: Kinv of view 0, Q and a of view `o` from the poses of view 0 and view o
OSFM_HD void baked_view(const double *R0, const double *t0, const double *Ro, const double *to, double *Q, double *a) {
  const double R0t[9] = {R0[0], R0[3], R0[6], R0[1], R0[4], R0[7], R0[2], R0[5], R0[8]};
  mat33_mul(Ro, R0t, Q);
  double q[3];
  mat33_vec(Q, t0, q);
  for (int k = 0; k < 3; k++) a[k] = q[k] - to[k];
}

// PlaneFromDepthAndNormal (depthmap.cc:120-125)
OSFM_HD void plane_from_depth_normal(int x, int y, const double *Kinv, float depth, const float *normal, float *plane) {
  double S[9];
  for (int k = 0; k < 9; k++) S[k] = Kinv[k] * (double)depth;
  const double xy1[3] = {(double)x, (double)y, 1.0};
  double pd[3];
  mat33_vec(S, xy1, pd);
  const float p[3] = {(float)pd[0], (float)pd[1], (float)pd[2]};
  const float denom = -((normal[0] * p[0] + normal[1] * p[1]) + normal[2] * p[2]);
  const float inv = 1.f / (denom > 1e-6f ? denom : 1e-6f);
  for (int k = 0; k < 3; k++) plane[k] = normal[k] * inv;
}

// DepthOfPlaneBackprojection (depthmap.cc:114-118)
OSFM_HD float depth_of_plane(int x, int y, const double *Kinv, const float *plane) {
  const double v[3] = {(double)plane[0], (double)plane[1], (double)plane[2]};
  double r[3];
  for (int c = 0; c < 3; c++) r[c] = (v[0] * Kinv[c] + v[1] * Kinv[3 + c]) + v[2] * Kinv[6 + c];
  const float denom = (float)(-((r[0] * (double)x + r[1] * (double)y) + r[2] * 1.0));
  return 1.0f / (denom > 1e-6f ? denom : 1e-6f);
}

// PlaneInducedHomographyBaked (depthmap.cc:96-102), narrowed to float
OSFM_HD void homography(const View &vo, const double *Kinv, const float *plane, float *H) {
  double M[9], T[9], Hd[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) M[3 * r + c] = vo.Q[3 * r + c] + vo.a[r] * (double)plane[c];
  mat33_mul(vo.K, M, T);
  mat33_mul(T, Kinv, Hd);
  for (int k = 0; k < 9; k++) H[k] = (float)Hd[k];
}

// LinearInterpolation<T> (depthmap.cc:14-30); a coordinate that is NaN reads as 0
template <class T>
OSFM_HD float interpolate(const T *image, int cols, int rows, float y, float x) {
  if (!(x >= 0.0f && x < (float)(cols - 1) && y >= 0.0f && y < (float)(rows - 1))) return 0.0f;
  const int ix = (int)x, iy = (int)y;
  const float dx = x - (float)ix, dy = y - (float)iy;
  const float im00 = (float)image[(int64_t)iy * cols + ix], im01 = (float)image[(int64_t)iy * cols + ix + 1];
  const float im10 = (float)image[(int64_t)(iy + 1) * cols + ix], im11 = (float)image[(int64_t)(iy + 1) * cols + ix + 1];
  const float im0 = (1.f - dx) * im00 + dx * im01;
  const float im1 = (1.f - dx) * im10 + dx * im11;
  return (1.f - dy) * im0 + dy * im1;
}

// NCCEstimator (depthmap.cc:46-74)
struct Ncc {
  float sumx = 0.f, sumy = 0.f, sumxx = 0.f, sumyy = 0.f, sumxy = 0.f, sumw = 0.f;
  OSFM_HD void push(float x, float y, float w) {
    sumx += w * x;
    sumy += w * y;
    sumxx += (w * x) * x;
    sumyy += (w * y) * y;
    sumxy += (w * x) * y;
    sumw += w;
  }
  OSFM_HD float get() const {
    if (sumw == 0.0f) return -1.f;
    const float meanx = sumx / sumw, meany = sumy / sumw;
    const float meanxx = sumxx / sumw, meanyy = sumyy / sumw, meanxy = sumxy / sumw;
    const float varx = meanxx - meanx * meanx, vary = meanyy - meany * meany;
    if ((double)varx < 0.1 || (double)vary < 0.1) return -1.f;
    return (meanxy - meanx * meany) / sqrtf(varx * vary);
  }
};

// ComputePlaneImageScore (depthmap.cc:426-465); `weight` is the bilateral table
OSFM_HD float image_score(const View &v0, const View &vo, const double *Kinv, const float *weight, int hpz, int i, int j, const float *plane) {
  float H[9];
  homography(vo, Kinv, plane, H);
  const float fi = (float)i, fj = (float)j;
  const float u = (H[0] * fj + H[1] * fi) + H[2];
  const float v = (H[3] * fj + H[4] * fi) + H[5];
  const float w = (H[6] * fj + H[7] * fi) + H[8];
  if (w == 0.0f) return -1.0f;
  const float dfdx_x = (H[0] * w - H[6] * u) / (w * w);
  const float dfdx_y = (H[3] * w - H[6] * v) / (w * w);
  const float dfdy_x = (H[1] * w - H[7] * u) / (w * w);
  const float dfdy_y = (H[4] * w - H[7] * v) / (w * w);
  const float Hx0 = u / w, Hy0 = v / w;
  const uint8_t *im = v0.image;
  const int center = im[(int64_t)i * v0.w + j];
  Ncc ncc;
  for (int dy = -hpz; dy <= hpz; ++dy)
    for (int dx = -hpz; dx <= hpz; ++dx) {
      const int p = im[(int64_t)(i + dy) * v0.w + (j + dx)];
      const float x2 = (Hx0 + dfdx_x * (float)dx) + dfdy_x * (float)dy;
      const float y2 = (Hy0 + dfdx_y * (float)dx) + dfdy_y * (float)dy;
      const float im2 = interpolate<uint8_t>(vo.image, vo.w, vo.h, y2, x2);
      const int dc = p > center ? p - center : center - p;
      ncc.push((float)p, im2, weight[dc * kR2 + dx * dx + dy * dy]);
    }
  return ncc.get();
}

// ComputePlaneScore (depthmap.cc:413-424): the strict > keeps the lowest view on a tie
OSFM_HD void plane_score(const View *views, const Problem &P, const float *weight, int hpz, int i, int j, const float *plane, float *score, int *nghbr) {
  *score = -1.0f;
  *nghbr = 0;
  for (int other = 1; other < P.n_views; ++other) {
    const float s = image_score(views[P.view0], views[P.view0 + other], P.Kinv, weight, hpz, i, j, plane);
    if (s > *score) {
      *score = s;
      *nghbr = other;
    }
  }
}

OSFM_HD void assign_pixel(const Out &out, int64_t pix, float depth, const float *plane, float score, int nghbr) {
  out.depth[pix] = depth;
  for (int k = 0; k < 3; k++) out.plane[3 * pix + k] = plane[k];
  out.score[pix] = score;
  out.nghbr[pix] = nghbr;
}

// CheckPlaneCandidate / CheckPlaneImageCandidate once the candidate's score is known
OSFM_HD void check_candidate(const Out &out, const Problem &P, int i, int j, const float *plane, float score, int nghbr) {
  const int64_t pix = P.pix0 + (int64_t)i * P.w + j;
  if (score > out.score[pix]) assign_pixel(out, pix, depth_of_plane(j, i, P.Kinv, plane), plane, score, nghbr);
}

// the depth of plane d of ComputeBruteForce (depthmap.cc:193-198)
OSFM_HD float brute_force_depth(const Problem &P, int d, int num_planes) {
  if (num_planes <= 1) return (float)P.min_depth;
  return (float)(1.0 / (1.0 / P.min_depth + (double)d * (1.0 / P.max_depth - 1.0 / P.min_depth) / (double)(num_planes - 1)));
}

// ComputeBruteForce for one pixel
OSFM_HD void brute_force_pixel(const View *views, const Problem &P, const Tables &tab, const Params &prm, const Out &out, int i, int j) {
  const int hpz = (prm.patch_size - 1) / 2;
  const float normal[3] = {0.f, 0.f, -1.f};
  for (int d = 0; d < prm.num_planes; ++d) {
    float plane[3], score;
    int nghbr;
    plane_from_depth_normal(j, i, P.Kinv, brute_force_depth(P, d, prm.num_planes), normal, plane);
    plane_score(views, P, tab.weight, hpz, i, j, plane, &score, &nghbr);
    check_candidate(out, P, i, j, plane, score, nghbr);
  }
}

// ---- randomness ----
// draw k of pixel `pixel` (row * width + column) in sweep `sweep` (0 the initialisation, 1 + 2 it the forward and 2 + 2 it the backward
// pass of iteration it): splitmix64's finaliser over seed + 0x9E3779B97F4A7C15 (((sweep << 40) + pixel) * 32 + k + 1)
OSFM_HD uint64_t draw_bits(uint64_t seed, int sweep, int64_t pixel, int k) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (((((uint64_t)sweep) << 40) + (uint64_t)pixel) * (uint64_t)kDrawsPerSweep + (uint64_t)k + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
OSFM_HD int quantile_index(uint64_t z) { return (int)(z >> 52); }                              // 12 bits
OSFM_HD float uniform_pm1(uint64_t z) { return (float)(int)(z >> 40) * 0x1p-23f - 1.0f; }      // 24 bits: exact, in [-1, 1)
OSFM_HD int neighbour_draw(uint64_t z, int n_views) { return 1 + (int)((uint32_t)(z >> 32) % (uint32_t)(n_views - 1)); }
OSFM_HD int other_neighbour_draw(uint64_t z, int n_views, int current) {
  return 1 + (int)(((uint32_t)current + (uint32_t)(z >> 32) % (uint32_t)(n_views - 2)) % (uint32_t)(n_views - 1));
}
// depth_range and normal_range of perturbation k (depthmap.cc:339-364: float *= double)
OSFM_HD float depth_range(int k) {
  float r = 0.02f;
  for (int q = 0; q < k; q++) r = (float)((double)r * 0.3);
  return r;
}
OSFM_HD float normal_range(int k) {
  float r = 0.5f;
  for (int q = 0; q < k; q++) r = (float)((double)r * 0.8);
  return r;
}

OSFM_HD bool sample_mode(const Problem &P, const Params &prm) { return prm.method == kPatchMatchSample && P.n_views > 1; }

// RandomInitialization then ComputeIgnoreMask (depthmap.cc:241-286) for one pixel
OSFM_HD void init_pixel(const View *views, const Problem &P, const Tables &tab, const Params &prm, const Out &out, int i, int j) {
  const int hpz = (prm.patch_size - 1) / 2;
  const int64_t local = (int64_t)i * P.w + j, pix = P.pix0 + local;
  const View &v0 = views[P.view0];
  float sum = 0.f;
  const int n = prm.patch_size * prm.patch_size;
  for (int u = -hpz; u <= hpz; ++u)
    for (int v = -hpz; v <= hpz; ++v) sum += (float)v0.image[(int64_t)(i + u) * v0.w + (j + v)];
  const float mean = sum / (float)n;
  float sum2 = 0.f;
  for (int u = -hpz; u <= hpz; ++u)
    for (int v = -hpz; v <= hpz; ++v) {
      const float x = (float)v0.image[(int64_t)(i + u) * v0.w + (j + v)];
      sum2 += (x - mean) * (x - mean);
    }
  const bool low_variance = sum2 / (float)n < prm.min_patch_variance;
  if (P.mask[local] == 0 || low_variance) {
    const float zero[3] = {0.f, 0.f, 0.f};
    assign_pixel(out, pix, 0.f, zero, 0.f, 0);
    return;
  }
  const float depth = P.init_depth[quantile_index(draw_bits(prm.seed, 0, local, 0))];
  const float normal[3] = {uniform_pm1(draw_bits(prm.seed, 0, local, 1)), uniform_pm1(draw_bits(prm.seed, 0, local, 2)), -1.f};
  float plane[3], score;
  int nghbr;
  plane_from_depth_normal(j, i, P.Kinv, depth, normal, plane);
  if (sample_mode(P, prm)) {
    nghbr = neighbour_draw(draw_bits(prm.seed, 0, local, 3), P.n_views);
    score = image_score(v0, views[P.view0 + nghbr], P.Kinv, tab.weight, hpz, i, j, plane);
  } else {
    plane_score(views, P, tab.weight, hpz, i, j, plane, &score, &nghbr);
  }
  assign_pixel(out, pix, depth, plane, score, nghbr);
}

// Candidate c of PatchMatchUpdatePixel (depthmap.cc:310-379) for pixel (i, j) from the CURRENT values: 0 and 1 the planes of the two
// adjacent pixels (di, dj = the pass's adjacency), 2 .. 7 the six perturbations, 8 the current plane in another view (sample mode, more
// than two views).  False when the reference skips it.  *nghbr is the view a sample-mode candidate is scored in.
constexpr int kCandidates = 9;
OSFM_HD bool candidate(const Problem &P, const Tables &tab, const Params &prm, const Out &out, int sweep, bool backward, int i, int j, int c,
                       float *plane, int *nghbr) {
  const int64_t local = (int64_t)i * P.w + j, pix = P.pix0 + local;
  if (out.depth[pix] == 0.0f) return false;
  if (c < 2) {
    const int di = backward ? (c == 0 ? 0 : 1) : (c == 0 ? -1 : 0), dj = backward ? (c == 0 ? 1 : 0) : (c == 0 ? 0 : -1);
    const int64_t adj = P.pix0 + (int64_t)(i + di) * P.w + (j + dj);
    if (out.depth[adj] == 0.0f) return false;
    for (int k = 0; k < 3; k++) plane[k] = out.plane[3 * adj + k];
    *nghbr = out.nghbr[adj];
    return true;
  }
  *nghbr = out.nghbr[pix];
  const float cp[3] = {out.plane[3 * pix], out.plane[3 * pix + 1], out.plane[3 * pix + 2]};
  if (c == 8) {
    if (!sample_mode(P, prm) || P.n_views <= 2) return false;
    *nghbr = other_neighbour_draw(draw_bits(prm.seed, sweep, local, 3 * kPerturb), P.n_views, *nghbr);
    for (int k = 0; k < 3; k++) plane[k] = cp[k];
    return true;
  }
  const int k = c - 2;
  if (cp[2] == 0.0f) return false;
  const float depth = out.depth[pix] * tab.factor[k * kQuantiles + quantile_index(draw_bits(prm.seed, sweep, local, 3 * k))];
  const float nr = normal_range(k);
  const float normal[3] = {-cp[0] / cp[2] + nr * tab.normal[quantile_index(draw_bits(prm.seed, sweep, local, 3 * k + 1))],
                           -cp[1] / cp[2] + nr * tab.normal[quantile_index(draw_bits(prm.seed, sweep, local, 3 * k + 2))], -1.0f};
  plane_from_depth_normal(j, i, P.Kinv, depth, normal, plane);
  return true;
}

// PatchMatchUpdatePixel by one lane: sample mode (every candidate is scored in one view)
OSFM_HD void update_pixel_sample(const View *views, const Problem &P, const Tables &tab, const Params &prm, const Out &out, int sweep, bool backward,
                                 int i, int j) {
  const int hpz = (prm.patch_size - 1) / 2;
  for (int c = 0; c < kCandidates; c++) {
    float plane[3];
    int nghbr;
    if (!candidate(P, tab, prm, out, sweep, backward, i, j, c, plane, &nghbr)) continue;
    const float score = image_score(views[P.view0], views[P.view0 + nghbr], P.Kinv, tab.weight, hpz, i, j, plane);
    check_candidate(out, P, i, j, plane, score, nghbr);
  }
}

// cv::medianBlur(depth, 5) at (i, j): the median of the 5 x 5 window, border replicated
OSFM_HD float median5(const float *depth, int w, int h, int i, int j) {
  float v[25];
  int n = 0;
  for (int di = -2; di <= 2; di++)
    for (int dj = -2; dj <= 2; dj++) {
      int y = i + di, x = j + dj;
      y = y < 0 ? 0 : y >= h ? h - 1 : y;
      x = x < 0 ? 0 : x >= w ? w - 1 : x;
      const float a = depth[(int64_t)y * w + x];
      int q = n++;
      while (q > 0 && v[q - 1] > a) {
        v[q] = v[q - 1];
        q--;
      }
      v[q] = a;
    }
  return v[12];
}
// PostProcess (depthmap.cc:477-490) of one pixel given its median
OSFM_HD float post_process(float d, float m) { return (d == 0.0f || (double)(fabsf(d - m) / d) > 0.05) ? 0.f : d; }

// ---- DepthmapCleaner ----
struct CleanView {
  double K[9], R[9], t[3];
  const float *depth;
  int w, h;
};
struct CleanProblem {
  double Kinv[9];
  int64_t view0, pix0;
  int n_views, w, h, pad;
};

// Backproject (depthmap.cc:109-112): R^T (depth K^-1 (x, y, 1) - t)
OSFM_HD void backproject(double x, double y, double depth, const double *Kinv, const double *R, const double *t, double *X) {
  double S[9], q[3];
  for (int k = 0; k < 9; k++) S[k] = Kinv[k] * depth;
  const double xy1[3] = {x, y, 1.0};
  mat33_vec(S, xy1, q);
  for (int k = 0; k < 3; k++) q[k] = q[k] - t[k];
  for (int k = 0; k < 3; k++) X[k] = (R[k] * q[0] + R[3 + k] * q[1]) + R[6 + k] * q[2];
}
// Project (depthmap.cc:104-107): K (R x + t)
OSFM_HD void project(const double *x, const double *K, const double *R, const double *t, double *out) {
  double r[3];
  mat33_vec(R, x, r);
  for (int k = 0; k < 3; k++) r[k] = r[k] + t[k];
  mat33_vec(K, r, out);
}

// DepthmapCleaner::Clean (depthmap.cc:515-541) for one pixel
OSFM_HD float clean_pixel(const CleanView *views, const CleanProblem &P, float threshold, int min_consistent, int i, int j) {
  const CleanView &v0 = views[P.view0];
  const float depth = v0.depth[(int64_t)i * P.w + j];
  double X[3];
  backproject((double)j, (double)i, (double)depth, P.Kinv, v0.R, v0.t, X);
  const double point[3] = {(double)(float)X[0], (double)(float)X[1], (double)(float)X[2]};  // narrowed to a Vec3f
  int consistent = 1;
  for (int other = 1; other < P.n_views; ++other) {
    const CleanView &vo = views[P.view0 + other];
    double pr[3];
    project(point, vo.K, vo.R, vo.t, pr);
    const float rp[3] = {(float)pr[0], (float)pr[1], (float)pr[2]};
    if ((double)rp[2] < 1e-8 || rp[2] != rp[2]) continue;
    const float u = rp[0] / rp[2], v = rp[1] / rp[2];
    const float depth_of_point = rp[2];
    const float depth_at = interpolate<float>(vo.depth, vo.w, vo.h, v, u);
    if (fabsf(depth_at - depth_of_point) < depth_of_point * threshold) consistent++;
  }
  return consistent >= min_consistent ? depth : 0.f;
}

}  // namespace osfm_dm
