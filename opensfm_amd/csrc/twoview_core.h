// twoview_core.h -- the 5-point finish of bootstrap_reconstruction (two_view_reconstruction_5pt, opensfm/reconstruction.py:336-485)
// recombined from the leaves the calibrated matcher is pinned on (relpose_core.h: inlier_bearing, refinement_picks,
// refine_relative_pose, rotmat_to_aa; relpose_rounds.h: RefineShared / WaveRefineEval).  No solver of its own.  Written against the
// wave policy like robust_match_finish_wave: twoview.hip runs it with GpuWave (one wavefront per (pair, configuration)), the host
// tests with tests/native/loop_wave.h.  Every 3-term sum runs left to right, contraction off.
#pragma once
#include "relpose_rounds.h"

namespace osfm_rp {

enum { kTwoViewOk = 0, kTwoViewNoConfiguration = 1, kTwoViewUndecidable = 2 };
constexpr int kTwoViewMinInliers = 5;  // a configuration counts with MORE inliers than this (reconstruction.py:366, :459)

struct TwoViewOut {  // mirrors osfm_two_view_result
  double R[18], t[6];                 // per configuration: what the reference feeds to cv2.Rodrigues, and its t
  double rotation[3], translation[3];  // of the chosen configuration (angle-axis by rotmat_to_aa); zeros unless status is OK
  double lo_model[12];                 // the RANSAC's ScoreInfo::lo_model (zeros on given poses)
  int32_t status, chosen;
  int32_t n_inliers[2], refine_iterations[2];  // -1 / 0 for a configuration that was not run
  int32_t score, iterations;                   // of the RANSAC (zeros on given poses)
};

// multiview.relative_pose_ransac (multiview.py:494-516) on ScoreInfo::lo_model (3 x 4 row-major): R = R_lo^T, t = -R_lo^T t_lo
OSFM_HD void two_view_pose_from_lo_model(const double* lo, double* R, double* t) {
  for (int a = 0; a < 3; a++) {
    for (int b = 0; b < 3; b++) R[3 * a + b] = lo[4 * b + a];
    t[a] = -(lo[a] * lo[3] + lo[4 + a] * lo[7] + lo[8 + a] * lo[11]);
  }
}

// two_view_reconstruction_and_refinement (reconstruction.py:336-374) up to its cv2.Rodrigues: the given or the transposed pose, the
// correspondences that triangulate within `threshold`, with more than five of them relative_pose_optimize_nonlinear
// (multiview.py:541-553) over them and the inliers again.  all_pass: both inlier tests are skipped and every correspondence counts
// (pygeometry.relative_pose_refinement on its own).  Returns the inlier count; subset[0 .. count) ascending; R_out = R_curr^T,
// t_out = -R_curr^T t_curr; *refine_its = TinySolver iterations (0: not refined).
template <class W>
OSFM_HD int two_view_config_wave(W& w, RefineShared& s, const double* b1, const double* b2, int n, const double* R, const double* t, int transposed,
                                 double threshold, int refine_iterations, int all_pass, int* subset, double* R_out, double* t_out, int* refine_its) {
  double Rc[9], tc[3];
  if (transposed) {
    for (int a = 0; a < 3; a++) {
      for (int b = 0; b < 3; b++) Rc[3 * a + b] = R[3 * b + a];
      tc[a] = -(R[a] * t[0] + R[3 + a] * t[1] + R[6 + a] * t[2]);
    }
  } else {
    for (int i = 0; i < 9; i++) Rc[i] = R[i];
    for (int i = 0; i < 3; i++) tc[i] = t[i];
  }
  auto inliers = [&]() {
    if (all_pass) {
      w.parallel_for(n, [&](int i) { subset[i] = i; });
      return n;
    }
    return w.compact(n, [&](int i) { return inlier_bearing(b1 + 3 * i, b2 + 3 * i, Rc, tc, threshold) != 0; }, subset);
  };
  int cnt = inliers();
  *refine_its = 0;
  if (cnt > kTwoViewMinInliers) {
    double RT[12];
    for (int a = 0; a < 3; a++) {
      for (int b = 0; b < 3; b++) RT[4 * a + b] = Rc[3 * b + a];
      RT[4 * a + 3] = -(Rc[a] * tc[0] + Rc[3 + a] * tc[1] + Rc[6 + a] * tc[2]);
    }
    w.single([&]() { refinement_picks(cnt, s.picked); });
    WaveRefineEval<W> ev{w, s, b1, b2, subset};
    *refine_its = refine_relative_pose(RT, refine_iterations, ev, (double*)nullptr);
    for (int a = 0; a < 3; a++) {
      for (int b = 0; b < 3; b++) Rc[3 * a + b] = RT[4 * b + a];
      tc[a] = -(RT[a] * RT[3] + RT[4 + a] * RT[7] + RT[8 + a] * RT[11]);
    }
    cnt = inliers();
  }
  for (int a = 0; a < 3; a++) {
    for (int b = 0; b < 3; b++) R_out[3 * a + b] = Rc[3 * b + a];
    t_out[a] = -(Rc[a] * tc[0] + Rc[3 + a] * tc[1] + Rc[6 + a] * tc[2]);
  }
  return cnt;
}

// The choice between the configurations (reconstruction.py:458-485): n0 / n1 inliers of the given / the transposed one (n1 is not
// looked at without check_reversal).  -> status; *chosen = -1, 0 or 1.  A tie under reversal_ratio >= 1 picks the transposed one, as
// `0 if len1 > len2 else 1` does.
OSFM_HD int two_view_decide(int n0, int n1, int check_reversal, double reversal_ratio, int* chosen) {
  const bool v0 = n0 > kTwoViewMinInliers, v1 = check_reversal && n1 > kTwoViewMinInliers;
  *chosen = -1;
  if (v0 && v1) {
    const double ratio = (double)(n0 < n1 ? n0 : n1) / (double)(n0 > n1 ? n0 : n1);
    if (ratio > reversal_ratio) return kTwoViewUndecidable;
    *chosen = n0 > n1 ? 0 : 1;
    return kTwoViewOk;
  }
  if (v0 || v1) {
    *chosen = v0 ? 0 : 1;
    return kTwoViewOk;
  }
  return kTwoViewNoConfiguration;
}

// One pair after its configurations: the decision, the record and the mask bytes of its n correspondences (bit 0 / 1: inlier of
// configuration 0 / 1, bit 2: of the chosen one).  out.R / t / n_inliers / refine_iterations hold what the configurations left;
// list0 / list1: their inlier lists.
OSFM_HD void two_view_finish_pair(TwoViewOut& out, int n, int check_reversal, double reversal_ratio, const int* list0, const int* list1,
                                  uint8_t* mask) {
  if (!check_reversal) {
    for (int i = 0; i < 9; i++) out.R[9 + i] = 0.0;
    for (int i = 0; i < 3; i++) out.t[3 + i] = 0.0;
    out.n_inliers[1] = -1;
    out.refine_iterations[1] = 0;
  }
  int chosen;
  out.status = two_view_decide(out.n_inliers[0], out.n_inliers[1], check_reversal, reversal_ratio, &chosen);
  out.chosen = chosen;
  for (int i = 0; i < 3; i++) out.rotation[i] = out.translation[i] = 0.0;
  if (chosen >= 0) {
    rotmat_to_aa(out.R + 9 * chosen, out.rotation);
    for (int i = 0; i < 3; i++) out.translation[i] = out.t[3 * chosen + i];
  }
  for (int i = 0; i < n; i++) mask[i] = 0;
  for (int c = 0; c < (check_reversal ? 2 : 1); c++) {
    const int* list = c ? list1 : list0;
    const uint8_t bits = (uint8_t)((1 << c) | (c == chosen ? 4 : 0));
    for (int k = 0; k < out.n_inliers[c]; k++) mask[list[k]] |= bits;
  }
}

}  // namespace osfm_rp
