// twoview_host.cpp -- TEST INFRASTRUCTURE: compiles the two-view finish (opensfm_amd/csrc/twoview_core.h) for the HOST with loops in place
// of lanes, around the host rounds of the LO-RANSAC (relpose_core_host.cpp), so that tests/test_twoview_host.py can hold it bit for bit to
// the restatement of tests/twoview_cases.py without a GPU and tests/test_gpu_twoview.py can hold the GPU to it.  The driver below does
// what twoview.hip's does, pair by pair.  tests/native/twoview_main.cpp includes this file for its sanitizer run.
// Nothing in the product links or loads this file.
#include "relpose_core_host.cpp"

#include "../../opensfm_amd/csrc/twoview_core.h"

extern "C" {

// osfm_two_view_pairs on the host: poses null -> the RANSAC rounds first.  results: n_pairs TwoViewOut, mask: off[n_pairs] bytes.
int host_two_view_pairs(const double* b1, const double* b2, const int64_t* off, int n_pairs, const double* poses, double threshold,
                        double probability, int ransac_iterations, int use_lo, int lo_iterations, int refine_iterations, int check_reversal,
                        double reversal_ratio, int skip_inlier_tests, TwoViewOut* results, uint8_t* mask) {
  LoopWave w;
  RefineShared* rs = new RefineShared;
  for (int p = 0; p < n_pairs; p++) {
    const int64_t o = off[p];
    const int n = (int)(off[p + 1] - o);
    TwoViewOut& r = results[p];
    memset(&r, 0, sizeof r);
    if (n <= kTwoViewMinInliers) {
      r.status = kTwoViewNoConfiguration;
      r.chosen = r.n_inliers[0] = r.n_inliers[1] = -1;
      for (int i = 0; i < n; i++) mask[o + i] = 0;
      continue;
    }
    double pose[12];
    if (poses) {
      memcpy(pose, poses + 12 * (size_t)p, sizeof pose);
    } else {
      const int64_t one[2] = {0, n};
      HostRounds H(b1 + 3 * o, b2 + 3 * o, one, 1, threshold, ransac_iterations, probability, use_lo, lo_iterations, 5);
      H.run();
      const PairState& S = H.st[0];
      memcpy(r.lo_model, S.lo_model, sizeof r.lo_model);
      r.score = S.best_score;
      r.iterations = S.it;
      two_view_pose_from_lo_model(S.lo_model, pose, pose + 9);
    }
    std::vector<int> lists((size_t)2 * n);
    for (int c = 0; c < (check_reversal ? 2 : 1); c++) {
      int its = 0;
      r.n_inliers[c] = two_view_config_wave(w, *rs, b1 + 3 * o, b2 + 3 * o, n, pose, pose + 9, c, threshold, refine_iterations, skip_inlier_tests,
                                            lists.data() + (size_t)c * n, r.R + 9 * c, r.t + 3 * c, &its);
      r.refine_iterations[c] = its;
    }
    two_view_finish_pair(r, n, check_reversal, reversal_ratio, lists.data(), lists.data() + n, mask + o);
  }
  delete rs;
  return 0;
}

int host_two_view_decide(int n0, int n1, int check_reversal, double reversal_ratio, int* chosen) {
  return two_view_decide(n0, n1, check_reversal, reversal_ratio, chosen);
}
void host_aa_to_rotmat(const double* aa, double* R) { aa_to_rotmat(aa, R); }
int host_two_view_result_bytes() { return (int)sizeof(TwoViewOut); }
}
