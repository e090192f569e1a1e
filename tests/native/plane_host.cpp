// plane_host.cpp -- TEST INFRASTRUCTURE: compiles the plane-based two-view solve (opensfm_amd/csrc/plane_core.h) for the HOST with loops
// in place of lanes, so that tests/test_plane_host.py can hold it to the numpy restatement of tests/plane_cases.py without a GPU and
// tests/test_gpu_plane.py can hold the GPU to it bit for bit.  The driver below does what plane.hip's does, pair by pair.
// tests/native/plane_main.cpp includes this file for its sanitizer run.  Nothing in the product links or loads this file.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../opensfm_amd/csrc/plane_core.h"
#include "loop_wave.h"

using namespace osfm_pl;

namespace {

// LoopWave with the fixed-order sum of the final fit: "lane" l takes items l, l + 64, ... from 0.0, then the 64 lane sums are combined
// by a butterfly over xor 32, 16, ..., 1 -- the order of plane.hip's PlaneWave
struct PlaneLoopWave : LoopWave {
  template <int K, class F>
  void sum_rows(int n, F f, double* out) {
    constexpr int kLanes = 64;
    double acc[kLanes][K], next[kLanes][K];
    for (int l = 0; l < kLanes; l++) {
      for (int k = 0; k < K; k++) acc[l][k] = 0.0;
      for (int i = l; i < n; i += kLanes) f(i, acc[l]);
    }
    for (int m = kLanes / 2; m >= 1; m >>= 1) {
      for (int l = 0; l < kLanes; l++)
        for (int k = 0; k < K; k++) next[l][k] = acc[l][k] + acc[l ^ m][k];
      std::memcpy(acc, next, sizeof acc);
    }
    for (int k = 0; k < K; k++) out[k] = acc[0][k];
  }
};

}  // namespace

extern "C" {

int host_homography_dlt(const double* x1, const double* x2, const int* idx, int n, double* H) { return homography_dlt(x1, x2, idx, n, H); }
// the final fit's sum order over the rows list[0 .. n-1]
int host_homography_dlt_wave(const double* x1, const double* x2, const int* list, int n, double* H) {
  PlaneLoopWave w;
  double ws[32];
  int ok = 0;
  return homography_dlt_wave(w, ws, x1, x2, list, n, H, &ok);
}
int host_plane_motions(const double* H, double* motions, double* singular) { return plane_motions(H, motions, singular); }
int host_normalise_homography(double* H) { return normalise_homography(H) ? 1 : 0; }
int host_plane_pick(const int* counts) { return plane_pick(counts); }
void host_plane_aa_to_rotmat(const double* aa, double* R) { osfm_rp::aa_to_rotmat(aa, R); }
int host_plane_result_bytes() { return (int)sizeof(PlaneOut); }

// osfm_two_view_plane_pairs on the host.  results: n_pairs PlaneOut; mask: off[n_pairs] bytes.  -3: the generator table is too short.
int host_plane_pairs(const double* b1, const double* b2, const int64_t* off, int n_pairs, double threshold, double probability, int iterations,
                     int use_lo, int lo_iterations, int use_reduction, PlaneOut* results, uint8_t* mask) {
  PlaneLoopWave w;
  std::vector<PlaneShared> sh(1);
  int overflow = 0;
  for (int p = 0; p < n_pairs; p++) {
    const int64_t o = off[p];
    const int n = (int)(off[p + 1] - o);
    PlaneOut& r = results[p];
    std::memset(&r, 0, sizeof r);
    if (n < kMinimalSamples) {
      r.status = kPlaneNoHomography;
      r.chosen = -1;
      for (int i = 0; i < n; i++) mask[o + i] = 0;
      continue;
    }
    const int64_t one[2] = {0, n};
    std::vector<double> stop;
    std::vector<int64_t> stop_off;
    if (!stop_tables(one, 1, probability, kMinimalSamples, &stop, &stop_off)) return -1;
    std::vector<int> scratch((size_t)n);
    std::vector<double> x1((size_t)2 * n), x2((size_t)2 * n), motions((size_t)kMotions * kMotionSize);
    std::vector<uint8_t> flags((size_t)kMotions * n);
    const PlaneArgs A{b1 + 3 * o, b2 + 3 * o, one, stop.data(), stop_off.data(), rng_table<21>(), threshold, iterations, use_lo, lo_iterations,
                      use_reduction, scratch.data(), x1.data(), x2.data(), motions.data(), flags.data(), &r, mask + o, &overflow};
    plane_ransac_pair(w, sh[0], A, 0);
    for (int k = 0; k < kMotions; k++) plane_motion_pair(w, A, 0, k, n);
    plane_decide_pair(A, 0, n);
  }
  return overflow ? -3 : 0;
}
}
