// plane_core.h -- the plane-based half of bootstrap_reconstruction's two-view step: a homography by LO-RANSAC, its decomposition into
// eight candidate motions (Faugeras & Lustman 1988) and the choice between them.
//
// reference: reconstruction.two_view_reconstruction_plane_based (opensfm/reconstruction.py:298-333): multiview.euclidean on both sides,
// cv2.findHomography(x1, x2, cv2.RANSAC, threshold), multiview.motion_from_plane_homography (opensfm/multiview.py:366-441), every motion
// scored by _two_view_reconstruction_inliers (compute_inliers_bearings with R^T, -R^T t), the best one returned through cv2.Rodrigues.
//
// Everything is host + device, with the discipline of abspose_core.h: tests/native/plane_host.cpp compiles this header with g++ and runs
// the same per-pair code with loops in place of lanes, plane.hip runs it with one wavefront per pair.  Contraction is off, every sum has
// a written-out order and the decision path uses + - * / sqrt only, so host and device give the same bits (the angle-axis of the picked
// rotation goes through atan2 and is the one exception).
//
// What is restated and what is not.
//  * motion_from_plane_homography is restated line by line.  Its 3 x 3 SVD is jacobi_svd3 (relrot_core.h, the two-sided Jacobi of
//    Eigen::JacobiSVD restated), not svd3 (relpose_core.h): the one-sided svd3 forms U as the scaled columns of A V and completes it by a
//    cross product when the third singular value vanishes, so its U is orthogonal only as far as the singular values are well separated
//    from zero; R = s U R' V^T needs both factors orthogonal to working precision whatever H is, which the two-sided method gives.
//    numpy's LAPACK leaves the sign of each singular-vector pair free and the order of the eight motions depends on those signs, so the
//    signs are fixed before the loop: the largest-magnitude entry of every column of u is made positive (the first one among equals), the
//    matching row of vh flipped with it.  The order of the motions is then a property of H alone.
//  * The choice (plane_pick) is the motion with the most inliers, the lowest index on ties.  That is the reference's intent, not its
//    behaviour: np.argmax(map(len, motion_inliers)) is the argmax of a 0-d object array, 0 under Python 3, so the reference always
//    returns motions[0], whichever LAPACK's signs put there.  This divergence is deliberate.
//  * cv2.findHomography is NOT restated.  The RANSAC here is this project's LO-RANSAC walk (loransac_walk.h) over a normalised DLT: no
//    checkSubset, draws from std::mt19937(42) instead of cv::RNG, the walk's stopping rule; the ten Levenberg-Marquardt iterations cv2
//    runs after its refit are left out; the points stay in double (cv2 converts to float32).  The inlier test is cv2's: the one-way
//    transfer error in the second image.  None of OpenCV can be pinned by this project's tests; what reaches the caller is (R, t, inliers),
//    which depends on H only through its accuracy.
//  * The scale of H: the middle singular value is 1 and the determinant positive, so t of a motion is the baseline over the distance of
//    the plane.  The reference inherits cv2's h33 = 1; the scale of a bootstrap is free (the 5-point branch returns a unit baseline).
#pragma once
#include "relrot_core.h"

namespace osfm_pl {

using osfm_lo::kLdsInliers;
using osfm_lo::RngTable;
using osfm_rp::det3;
using osfm_rp::inlier_bearing;
using osfm_rp::jacobi_eig9;
using osfm_rp::rotmat_to_aa;
using osfm_rr::jacobi_svd3;

constexpr int kMinimalSamples = 4;
constexpr int kMotions = 8;
constexpr int kMotionSize = 16;  // R (9, row-major), t (3), n (3), d
constexpr double kSqrt2 = 1.4142135623730951;
constexpr double kDblMax = 1.79769313486231570815e308;
enum { kPlaneOk = 0, kPlaneNoHomography = 1, kPlaneDegenerate = 2 };

OSFM_HD bool finite_d(double x) { return fabs(x) <= kDblMax; }  // false for NaN too

// multiview.euclidean on one correspondence: x = (b0 / b2, b1 / b2) per side.  A row with b2 <= 0 on either side keeps its place (the
// caller's numbering holds) with NaN coordinates on both sides: it is an inlier of no homography, and a sample that draws it has no model.
OSFM_HD void normalised_row(const double* b1, const double* b2, double* x1, double* x2) {
  if (b1[2] > 0.0 && b2[2] > 0.0) {
    x1[0] = b1[0] / b1[2];
    x1[1] = b1[1] / b1[2];
    x2[0] = b2[0] / b2[2];
    x2[1] = b2[1] / b2[2];
  } else {
    const double nan = __builtin_nan("");
    x1[0] = x1[1] = x2[0] = x2[1] = nan;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Normalised DLT.  Per side the centroid c is subtracted and the points scaled by s so that their mean distance to it is sqrt(2).
// With p = (u0, u1, 1) of side 1 and (v0, v1) of side 2 the two DLT rows of a correspondence are (-p, 0, v0 p) and (0, -p, v1 p); the
// 9 x 9 normal matrix of all rows is, in 3 x 3 blocks of P = sum p p^T,
//     [   P     0   -P0 ]        P0 = sum v0 p p^T,  P1 = sum v1 p p^T,  PQ = sum (v0^2 + v1^2) p p^T,
//     [   0     P   -P1 ]
//     [ -P0   -P1    PQ ]
// so 24 sums (the six distinct entries of each) are all that is accumulated: kDltSums.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kDltSums = 24;

struct DltFrame {  // the normalisation of both sides
  double c1[2], s1, c2[2], s2;
};

// what row i adds to the four coordinate sums / the two distance sums / the 24 sums of the normal matrix
OSFM_HD void dlt_add_coords(const double* x1, const double* x2, int i, double* acc) {
  acc[0] = acc[0] + x1[2 * i];
  acc[1] = acc[1] + x1[2 * i + 1];
  acc[2] = acc[2] + x2[2 * i];
  acc[3] = acc[3] + x2[2 * i + 1];
}
OSFM_HD void dlt_add_dists(const double* x1, const double* x2, int i, const double* c, double* acc) {
  const double a0 = x1[2 * i] - c[0], a1 = x1[2 * i + 1] - c[1], b0 = x2[2 * i] - c[2], b1 = x2[2 * i + 1] - c[3];
  acc[0] = acc[0] + sqrt(a0 * a0 + a1 * a1);
  acc[1] = acc[1] + sqrt(b0 * b0 + b1 * b1);
}
OSFM_HD void dlt_add_normal(const double* x1, const double* x2, int i, const DltFrame& f, double* acc) {
  const double u0 = (x1[2 * i] - f.c1[0]) * f.s1, u1 = (x1[2 * i + 1] - f.c1[1]) * f.s1;
  const double v0 = (x2[2 * i] - f.c2[0]) * f.s2, v1 = (x2[2 * i + 1] - f.c2[1]) * f.s2;
  const double P[6] = {u0 * u0, u0 * u1, u0, u1 * u1, u1, 1.0};
  const double q = v0 * v0 + v1 * v1;
  OSFM_UNROLL for (int k = 0; k < 6; k++) {
    acc[k] = acc[k] + P[k];
    acc[6 + k] = acc[6 + k] + v0 * P[k];
    acc[12 + k] = acc[12 + k] + v1 * P[k];
    acc[18 + k] = acc[18 + k] + q * P[k];
  }
}
// centroids from the coordinate sums; scales from the distance sums; false when a scale is not finite
OSFM_HD void dlt_centroids(const double* sums, int n, double* c) {
  for (int k = 0; k < 4; k++) c[k] = sums[k] / (double)n;
}
OSFM_HD bool dlt_frame(const double* c, const double* dist_sums, int n, DltFrame& f) {
  f.c1[0] = c[0], f.c1[1] = c[1], f.c2[0] = c[2], f.c2[1] = c[3];
  f.s1 = kSqrt2 / (dist_sums[0] / (double)n);
  f.s2 = kSqrt2 / (dist_sums[1] / (double)n);
  return finite_d(f.s1) && finite_d(f.s2);
}
// The eigenvector of the smallest eigenvalue of the normal matrix (the first one among equals), denormalised: H = T2^-1 Hn T1 with
// T = [s 0 -s c0; 0 s -s c1; 0 0 1].  The sign is the one that makes det H positive: a plane seen from the same side by both cameras
// has such a homography, and its projective denominator is then positive on the points in front of both.  false: an entry is not finite.
OSFM_HD bool dlt_solve(const double* acc, const DltFrame& f, double* H) {
  double A[81], w[9], V[81];
  // (loops of fixed length unrolled and no run-time index into A, w, V: they can then stay in registers on the device)
  OSFM_UNROLL for (int i = 0; i < 3; i++)
    OSFM_UNROLL for (int j = 0; j < 3; j++) {
      const int a = i < j ? i : j, b = i < j ? j : i;
      const int k = a == 0 ? b : (a == 1 ? b + 2 : 5);  // entry (i, j) of a symmetric 3 x 3 among its six sums: 0 1 2 / 1 3 4 / 2 4 5
      A[9 * i + j] = acc[k];
      A[9 * i + 3 + j] = 0.0;
      A[9 * i + 6 + j] = -acc[6 + k];
      A[9 * (3 + i) + j] = 0.0;
      A[9 * (3 + i) + 3 + j] = acc[k];
      A[9 * (3 + i) + 6 + j] = -acc[12 + k];
      A[9 * (6 + i) + j] = -acc[6 + k];
      A[9 * (6 + i) + 3 + j] = -acc[12 + k];
      A[9 * (6 + i) + 6 + j] = acc[18 + k];
    }
  jacobi_eig9(A, w, V);
  int lo = 0;
  double w_lo = w[0];
  OSFM_UNROLL for (int i = 1; i < 9; i++)
    if (w[i] < w_lo) {
      w_lo = w[i];
      lo = i;
    }
  double h[9], M[9];
  OSFM_UNROLL for (int i = 0; i < 9; i++) {
    double e = 0.0;
    OSFM_UNROLL for (int c = 0; c < 9; c++)
      if (c == lo) e = V[9 * i + c];
    h[i] = e;
  }
  for (int r = 0; r < 3; r++) {
    M[3 * r] = h[3 * r] * f.s1;
    M[3 * r + 1] = h[3 * r + 1] * f.s1;
    M[3 * r + 2] = h[3 * r + 2] - (M[3 * r] * f.c1[0] + M[3 * r + 1] * f.c1[1]);
  }
  for (int c = 0; c < 3; c++) {
    H[c] = M[c] / f.s2 + f.c2[0] * M[6 + c];
    H[3 + c] = M[3 + c] / f.s2 + f.c2[1] * M[6 + c];
    H[6 + c] = M[6 + c];
  }
  bool ok = true;
  for (int i = 0; i < 9; i++) ok = ok && finite_d(H[i]);
  if (!ok) return false;
  if (det3(H) < 0.0)
    for (int i = 0; i < 9; i++) H[i] = -H[i];
  return true;
}

// The normalised DLT over the rows idx[0 .. n-1] (idx == nullptr: rows 0 .. n-1), n >= 4, every sum from 0.0 over the rows in the order
// given.  x1 / x2: rows of two doubles.  Returns 1 and H (row-major), or 0: no model.
OSFM_HD int homography_dlt(const double* x1, const double* x2, const int* idx, int n, double* H) {
  if (n < kMinimalSamples) return 0;
  double sums[4] = {0.0, 0.0, 0.0, 0.0}, dist[2] = {0.0, 0.0}, c[4], acc[kDltSums];
  for (int k = 0; k < n; k++) dlt_add_coords(x1, x2, idx ? idx[k] : k, sums);
  dlt_centroids(sums, n, c);
  for (int k = 0; k < n; k++) dlt_add_dists(x1, x2, idx ? idx[k] : k, c, dist);
  DltFrame f;
  if (!dlt_frame(c, dist, n, f)) return 0;
  for (int k = 0; k < kDltSums; k++) acc[k] = 0.0;
  for (int k = 0; k < n; k++) dlt_add_normal(x1, x2, idx ? idx[k] : k, f, acc);
  return dlt_solve(acc, f, H) ? 1 : 0;
}

// The same over a pair's inlier list by a whole wavefront: the final fit.  W::sum_rows<K>(n, f, out) sums f's K terms over n items in
// a fixed order -- lane l takes items l, l + 64, ... from 0.0, then the 64 lanes are combined by a butterfly over xor 32, 16, ..., 1 --
// so the order differs from homography_dlt's (the two are different functions of the rows) but is the same on the host and the device.
// ws: 32 doubles next to the wavefront (LDS); H_out: 9 doubles there.  Returns the same on every lane.
template <class W>
OSFM_HD int homography_dlt_wave(W& w, double* ws, const double* x1, const double* x2, const int* list, int n, double* H_out, int* ok_out) {
  if (n < kMinimalSamples) return 0;
  w.template sum_rows<4>(n, [&](int k, double* acc) { dlt_add_coords(x1, x2, list[k], acc); }, ws);
  double c[4];
  dlt_centroids(ws, n, c);
  w.template sum_rows<2>(n, [&](int k, double* acc) { dlt_add_dists(x1, x2, list[k], c, acc); }, ws + 4);
  DltFrame f;
  if (!dlt_frame(c, ws + 4, n, f)) return 0;  // the same on every lane
  w.template sum_rows<kDltSums>(n, [&](int k, double* acc) { dlt_add_normal(x1, x2, list[k], f, acc); }, ws + 6);
  w.single([&]() { *ok_out = dlt_solve(ws + 6, f, H_out) ? 1 : 0; });
  return *ok_out;
}

// ---------------------------------------------------------------------------------------------------------------
// The model of loransac_walk.h's walk
// ---------------------------------------------------------------------------------------------------------------
// cv2.findHomography's inlier test: |x2 - pi(H x1)| < threshold; false when the projective denominator is <= 0 or anything is not finite
OSFM_HD bool homography_inlier(const double* H, const double* x1, const double* x2, double thr) {
  const double d = H[6] * x1[0] + H[7] * x1[1] + H[8];
  if (!(d > 0.0 && d <= kDblMax)) return false;
  const double px = (H[0] * x1[0] + H[1] * x1[1] + H[2]) / d, py = (H[3] * x1[0] + H[4] * x1[1] + H[5]) / d;
  const double ex = x2[0] - px, ey = x2[1] - py;
  const double e = sqrt(ex * ex + ey * ey);
  return e < thr;  // false for NaN; an infinite e is not below a finite threshold
}

struct Homography {
  static constexpr int kModelSize = 9, kMinimalSamples = osfm_pl::kMinimalSamples, kMaxModels = 1;
  static constexpr int kSlots = 64;    // speculative main iterations per block: one 4-point DLT (a 9 x 9 eigen-solve) per lane
  static constexpr int kLoBatch = 16;  // speculative LO iterations per block: the default 10 of a local optimisation fit one batch
  const double *x1, *x2;
  double thr;
  OSFM_HD int solve_minimal(const int* idx, int, double* out) const { return homography_dlt(x1, x2, idx, kMinimalSamples, out); }
  OSFM_HD void solve_nonminimal(const int* idx, int size, double* out) const {
    if (!homography_dlt(x1, x2, idx, size, out))
      for (int i = 0; i < 9; i++) out[i] = 0.0;  // a zero H has no inliers (its denominator is 0)
  }
  OSFM_HD bool inlier(const double* H, int i) const { return homography_inlier(H, x1 + 2 * i, x2 + 2 * i, thr); }
};

// ---------------------------------------------------------------------------------------------------------------
// multiview.motion_from_plane_homography (multiview.py:366-441).  H row-major; motions: 8 x (R, t, n, d); singular: d1, d2, d3.
// Returns 8, or 0 where the reference returns None (two singular values nearly equal; here also: not finite, or a middle one of 0).
// ---------------------------------------------------------------------------------------------------------------
OSFM_HD void matmul3(const double* A, const double* B, double* C) {  // row-major, 3-term sums left to right
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
OSFM_HD int plane_motions(const double* H, double* motions, double* singular) {
  double u[9], l[3], V[9], vh[9];
  jacobi_svd3(H, u, l, V);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) vh[3 * i + j] = V[3 * j + i];
  for (int j = 0; j < 3; j++) {  // the sign rule: the largest-magnitude entry of column j of u positive, row j of vh with it
    int big = 0;
    for (int i = 1; i < 3; i++)
      if (fabs(u[3 * i + j]) > fabs(u[3 * big + j])) big = i;
    if (u[3 * big + j] < 0.0)
      for (int i = 0; i < 3; i++) {
        u[3 * i + j] = -u[3 * i + j];
        vh[3 * j + i] = -vh[3 * j + i];
      }
  }
  const double d1 = l[0], d2 = l[1], d3 = l[2];
  for (int i = 0; i < 3; i++) singular[i] = l[i];
  if (!(d2 > 0.0 && d1 <= kDblMax)) return 0;
  const double s = det3(u) * det3(vh);
  if (d1 / d2 < 1.0001 || d2 / d3 < 1.0001) return 0;
  const double abs_x1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const double abs_x3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  for (int k = 0; k < 4; k++) {
    const double x1 = (k & 2) ? -abs_x1 : abs_x1, x3 = (k & 1) ? -abs_x3 : abs_x3;
    const double sin_term = x1 * x3 / d2;
    const double sin_theta = (d1 - d3) * sin_term;
    const double sin_phi = (d1 + d3) * sin_term;
    const double d1_x3_2 = d1 * (x3 * x3);
    const double d3_x1_2 = d3 * (x1 * x1);
    const double cos_theta = (d3_x1_2 + d1_x3_2) / d2;
    const double cos_phi = (d3_x1_2 - d1_x3_2) / d2;
    const double Rp_p[9] = {cos_theta, 0.0, -sin_theta, 0.0, 1.0, 0.0, sin_theta, 0.0, cos_theta};
    const double Rp_n[9] = {cos_phi, 0.0, sin_phi, 0.0, -1.0, 0.0, sin_phi, 0.0, -cos_phi};
    const double np_[3] = {x1, 0.0, x3};
    const double tp_p[3] = {(d1 - d3) * x1, (d1 - d3) * 0.0, (d1 - d3) * -x3};
    const double tp_n[3] = {(d1 + d3) * np_[0], (d1 + d3) * np_[1], (d1 + d3) * np_[2]};
    double *mp = motions + kMotionSize * (2 * k), *mn = mp + kMotionSize;
    double A[9], B[9];
    matmul3(u, Rp_p, A);
    matmul3(A, vh, B);
    for (int i = 0; i < 9; i++) mp[i] = s * B[i];
    matmul3(u, Rp_n, A);
    matmul3(A, vh, B);
    for (int i = 0; i < 9; i++) mn[i] = s * B[i];
    for (int i = 0; i < 3; i++) {
      mp[9 + i] = u[3 * i] * tp_p[0] + u[3 * i + 1] * tp_p[1] + u[3 * i + 2] * tp_p[2];
      mn[9 + i] = u[3 * i] * tp_n[0] + u[3 * i + 1] * tp_n[1] + u[3 * i + 2] * tp_n[2];
      const double ni = -(vh[i] * np_[0] + vh[3 + i] * np_[1] + vh[6 + i] * np_[2]);  // -vh^T np_
      mp[12 + i] = ni;
      mn[12 + i] = ni;
    }
    mp[15] = s * d2;
    mn[15] = -(s * d2);
  }
  return kMotions;
}

// H to middle singular value 1 and positive determinant.  false: the middle singular value is 0 or not finite (H has rank below 2)
OSFM_HD bool normalise_homography(double* H) {
  double U[9], S[3], V[9];
  jacobi_svd3(H, U, S, V);
  if (!(S[1] > 0.0 && S[0] <= kDblMax)) return false;
  for (int i = 0; i < 9; i++) H[i] = H[i] / S[1];
  if (det3(H) < 0.0)
    for (int i = 0; i < 9; i++) H[i] = -H[i];
  return true;
}

// the motion with the most inliers, the lowest index on ties
OSFM_HD int plane_pick(const int* counts) {
  int best = 0;
  for (int k = 1; k < kMotions; k++)
    if (counts[k] > counts[best]) best = k;
  return best;
}

// _two_view_reconstruction_inliers(b1, b2, R.T, -R.T.dot(t), threshold) of one motion: the pose handed to inlier_bearing
OSFM_HD void motion_scoring_pose(const double* motion, double* Rt, double* tt) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) Rt[3 * i + j] = motion[3 * j + i];
    tt[i] = -(motion[i] * motion[9] + motion[3 + i] * motion[10] + motion[6 + i] * motion[11]);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// One pair, one wavefront
// ---------------------------------------------------------------------------------------------------------------
struct PlaneOut {  // mirrors osfm_plane_result
  double H[9], singular[3];
  double R[9], t[3], rotation[3], translation[3];
  int32_t status, chosen, h_inliers, iterations, n_inliers;
  int32_t motion_inliers[kMotions];
  int32_t pad;
};

struct PlaneShared {  // LDS of a pair
  osfm_lo::WalkShared<Homography> walk;
  double ws[32], H[9], singular[3], motions[kMotions * kMotionSize];
  int ok, count;
};

struct PlaneArgs {
  const double *b1, *b2;      // bearings, total x 3
  const int64_t* offsets;     // n_pairs + 1
  const double* stop_bound;   // ShouldStop's bound per best inlier count; pair p reads n + 1 doubles at stop_bound + stop_off[p]
  const int64_t* stop_off;
  RngTable rng;               // raw outputs of std::mt19937(42)
  double thr;                 // the threshold: of the transfer error (normalised coordinates) and of the bearings' test (radians)
  int iterations, use_lo, lo_iterations, use_reduction;
  int* scratch;               // total ints: inlier lists of the pairs with more than kLdsInliers rows
  double *x1, *x2;            // total x 2 each: the normalised coordinates, written here
  double* motions;            // n_pairs x 8 x 16
  uint8_t* flags;             // 8 x total: flags[m * total + row] = the row is an inlier of motion m
  PlaneOut* out;
  uint8_t* mask;              // total: bit 0 inlier of H, bit 1 inlier of the picked motion
  int* overflow;              // set when the tabulated stream is too short
};

// the walk, the final fit, H with its scale fixed and the eight motions of pair p; mask bit 0
template <class W>
OSFM_HD void plane_ransac_pair(W& w, PlaneShared& sh, const PlaneArgs& A, int p) {
  const int64_t o = A.offsets[p];
  const int n = (int)(A.offsets[p + 1] - o);
  const double *b1 = A.b1 + 3 * o, *b2 = A.b2 + 3 * o;
  double *x1 = A.x1 + 2 * o, *x2 = A.x2 + 2 * o;
  w.parallel_for(n, [&](int i) { normalised_row(b1 + 3 * i, b2 + 3 * i, x1 + 2 * i, x2 + 2 * i); });
  int* inliers = n <= kLdsInliers ? sh.walk.inl : A.scratch + o;
  const Homography m{x1, x2, A.thr};
  osfm_lo::WalkResult<Homography> r;
  osfm_lo::walk(w, sh.walk, m, A, A.stop_bound + A.stop_off[p], n, inliers, r);
  int best = r.failed ? 0 : r.best;
  double H[9];
  for (int i = 0; i < 9; i++) H[i] = r.lo_model[i];
  int status = kPlaneOk;
  if (best < kMinimalSamples) {
    status = kPlaneNoHomography;
    best = 0;
  } else {
    // the final fit over all inliers of lo_model; kept when it has at least as many inliers (the newcomer wins ties, as in the walk)
    if (homography_dlt_wave(w, sh.ws, x1, x2, inliers, best, sh.H, &sh.ok)) {
      double Hf[9];
      for (int i = 0; i < 9; i++) Hf[i] = sh.H[i];
      auto fits = [&](int i) { return m.inlier(Hf, i); };
      const int cnt = w.count_if(n, fits);
      if (cnt >= best) {
        best = cnt;
        (void)w.compact(n, fits, inliers);
        for (int i = 0; i < 9; i++) H[i] = Hf[i];
      }
    }
    w.single([&]() {
      for (int i = 0; i < 9; i++) sh.H[i] = H[i];
      for (int i = 0; i < 3; i++) sh.singular[i] = 0.0;
      sh.count = 0;
      if (normalise_homography(sh.H)) sh.count = plane_motions(sh.H, sh.motions, sh.singular);
    });
    if (sh.count != kMotions) status = kPlaneDegenerate;
  }
  uint8_t* mask = A.mask + o;
  w.parallel_for(n, [&](int i) { mask[i] = 0; });
  w.parallel_for(best, [&](int i) { mask[inliers[i]] = 1; });
  if (status == kPlaneOk) {
    double* mo = A.motions + (size_t)p * kMotions * kMotionSize;
    w.parallel_for(kMotions * kMotionSize, [&](int i) { mo[i] = sh.motions[i]; });
  }
  w.single([&]() {
    PlaneOut& out = A.out[p];
    for (int i = 0; i < 9; i++) out.H[i] = status == kPlaneNoHomography ? 0.0 : sh.H[i];
    for (int i = 0; i < 3; i++) out.singular[i] = status == kPlaneNoHomography ? 0.0 : sh.singular[i];
    out.status = status;
    out.h_inliers = best;
    out.iterations = r.iterations;
    out.pad = 0;
    if (r.failed) *A.overflow = 1;
  });
}

// the rows of pair p that motion k explains: flags and the count.  Runs after plane_ransac_pair of the pair.
template <class W>
OSFM_HD void plane_motion_pair(W& w, const PlaneArgs& A, int p, int k, int64_t total) {
  const int64_t o = A.offsets[p];
  const int n = (int)(A.offsets[p + 1] - o);
  const double *b1 = A.b1 + 3 * o, *b2 = A.b2 + 3 * o;
  uint8_t* flags = A.flags + (size_t)k * total + o;
  int cnt = 0;
  if (A.out[p].status == kPlaneOk) {
    double Rt[9], tt[3];
    motion_scoring_pose(A.motions + ((size_t)p * kMotions + k) * kMotionSize, Rt, tt);
    const double thr = A.thr;
    cnt = w.count_if(n, [&](int i) {
      const bool ok = inlier_bearing(b1 + 3 * i, b2 + 3 * i, Rt, tt, thr) != 0;
      flags[i] = ok ? 1 : 0;
      return ok;
    });
  } else {
    w.parallel_for(n, [&](int i) { flags[i] = 0; });
  }
  w.single([&]() { A.out[p].motion_inliers[k] = cnt; });
}

// the choice, the record and mask bit 1 of pair p (one thread)
OSFM_HD void plane_decide_pair(const PlaneArgs& A, int p, int64_t total) {
  PlaneOut& out = A.out[p];
  const int64_t o = A.offsets[p];
  const int n = (int)(A.offsets[p + 1] - o);
  for (int i = 0; i < 9; i++) out.R[i] = 0.0;
  for (int i = 0; i < 3; i++) out.t[i] = out.rotation[i] = out.translation[i] = 0.0;
  out.chosen = -1;
  out.n_inliers = 0;
  if (out.status != kPlaneOk) return;
  const int k = plane_pick(out.motion_inliers);
  const double* mo = A.motions + ((size_t)p * kMotions + k) * kMotionSize;
  for (int i = 0; i < 9; i++) out.R[i] = mo[i];
  for (int i = 0; i < 3; i++) out.t[i] = out.translation[i] = mo[9 + i];
  rotmat_to_aa(out.R, out.rotation);
  out.chosen = k;
  out.n_inliers = out.motion_inliers[k];
  const uint8_t* flags = A.flags + (size_t)k * total + o;
  uint8_t* mask = A.mask + o;
  for (int i = 0; i < n; i++) mask[i] = (uint8_t)(mask[i] | (flags[i] << 1));
}

}  // namespace osfm_pl
