// relrot_host.cpp -- TEST INFRASTRUCTURE: compiles the product's rotation-only LO-RANSAC (opensfm_amd/csrc/relrot_core.h) for the
// HOST with loops in place of lanes (the "header's round logic"), next to an independent sequential restatement of
// Estimate<RansacScoring, RelativeRotation> on this toolchain's real std::mt19937 / std::uniform_int_distribution, so that
// tests/test_relrot_host.py can compare the two bit for bit without a GPU.  Nothing in the product links or loads this file.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../opensfm_amd/csrc/relrot_core.h"
#include "loop_wave.h"

using namespace osfm_rr;

extern "C" {

void host_jacobi_svd3(const double* A, double* U, double* S, double* V) { jacobi_svd3(A, U, S, V); }
void host_svd3(const double* A, double* U, double* S, double* V) { osfm_rp::svd3(A, U, S, V); }
void host_rotation_model(const double* b1, const double* b2, const int* idx, int count, double* model, int* negated) {
  rotation_model(b1, b2, idx, count, model, negated);
}
// RotationBetweenPoints with osfm_rp::svd3 in place of the Eigen restatement (the DESIGN.md measurement only)
void host_rotation_model_svd3(const double* b1, const double* b2, const int* idx, int count, double* model, int* negated) {
  double qa[3] = {0, 0, 0}, pa[3] = {0, 0, 0}, M[9] = {0};
  for (int k = 0; k < count; k++)
    for (int a = 0; a < 3; a++) {
      qa[a] += b1[3 * idx[k] + a];
      pa[a] += b2[3 * idx[k] + a];
    }
  for (int a = 0; a < 3; a++) {
    qa[a] /= count;
    pa[a] /= count;
  }
  for (int k = 0; k < count; k++)
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) M[3 * i + j] += (b1[3 * idx[k] + i] - qa[i]) * (b2[3 * idx[k] + j] - pa[j]);
  double U[9], S[3], V[9], R[9];
  osfm_rp::svd3(M, U, S, V);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + U[3 * i + 2] * V[3 * j + 2];
  const double sign = osfm_rp::det3(R) < 0 ? -1.0 : 1.0;
  *negated = sign < 0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) model[3 * i + j] = sign * R[3 * j + i];
}
double host_rotation_error(const double* model, const double* x, const double* y) { return rotation_error(model, x, y); }
double host_rotation_chord(const double* lo_model, const double* x, const double* y) { return rotation_chord(lo_model, x, y); }

// relrot_core.h's walk for every pair of a batch (what rr_pairs_kernel runs, one "wavefront" after the other)
int host_relrot_pairs(const double* b1, const double* b2, const int64_t* offsets, int n_pairs, double threshold, double probability,
                      double chord, int iterations, int use_lo, int lo_iterations, int use_reduction, RelrotOut* out, uint8_t* mask) {
  std::vector<double> stop;
  std::vector<int64_t> stop_off;
  if (!stop_tables(offsets, n_pairs, probability, kMinimalSamples, &stop, &stop_off)) return -1;
  std::vector<int> scratch((size_t)std::max<int64_t>(offsets[n_pairs], 1));
  int overflow = 0;
  RelrotArgs A{b1, b2, offsets, stop.data(), stop_off.data(), rng_table<21>(), 1.0 - std::cos(threshold), chord,
               iterations, use_lo, lo_iterations, use_reduction, scratch.data(), out, mask, &overflow};
  LoopWave w;
  std::vector<RelrotShared> sh(1);  // per call: callers run batches on several threads
  for (int p = 0; p < n_pairs; p++) relrot_pair(w, sh[0], A, p);
  return overflow ? -3 : 0;
}

// Estimate<RansacScoring, RelativeRotation> restated sequentially (robust_estimator.h:37-119, random_sampler.h, scorer.h) on the real
// std::mt19937(42) and std::uniform_int_distribution, around the header's model numerics.  Returns the score.
int host_sequential_estimate(const double* b1, const double* b2, int n, double threshold, double probability, int iterations, int use_lo,
                             int lo_iterations, int use_reduction, double* model, double* lo_model, int* inliers, int* iterations_run) {
  std::mt19937 gen(42);
  auto sample = [&](int size, int range_max, std::vector<int>& idx) {
    std::uniform_int_distribution<std::mt19937::result_type> dist(0, range_max);
    idx.assign(size, 0);
    for (int i = 0; i < size; ++i) {
      do {
        idx[i] = (int)dist(gen);
      } while (std::find(idx.begin(), idx.begin() + i, idx[i]) != idx.begin() + i);
    }
  };
  const double thr = 1.0 - std::cos(threshold);
  auto score_of = [&](const double* m, std::vector<int>& list) {
    list.clear();
    for (int i = 0; i < n; i++)
      if (std::sqrt(rotation_error(m, b1 + 3 * i, b2 + 3 * i) * rotation_error(m, b1 + 3 * i, b2 + 3 * i)) < thr) list.push_back(i);
    return (int)list.size();
  };
  int best = 0;
  std::vector<int> best_list, list, idx;
  double bm[9] = {0}, blo[9] = {0};
  bool should_stop = false;
  int i = 0;
  for (; i < iterations && !should_stop; ++i) {
    sample(3, n - 1, idx);
    double m[9];
    rotation_model(b1, b2, idx.data(), 3, m);
    const int s = score_of(m, list);
    if (!(s < best)) {
      best = s;
      best_list = list;
      std::memcpy(bm, m, sizeof bm);
      std::memcpy(blo, m, sizeof blo);
    }
    if (s == best && (int)list.size() >= 3 && use_lo) {
      for (int k = 0; k < lo_iterations; ++k) {
        const std::vector<int> inl = best_list;
        const int size = std::max(std::min(12, int(best_list.size() * 0.5)), 3);
        sample(size, (int)inl.size() - 1, idx);
        std::vector<int> sel(size);
        for (int q = 0; q < size; q++) sel[q] = inl[idx[q]];
        double lm[9];
        rotation_model(b1, b2, sel.data(), size, lm);
        const int s2 = score_of(lm, list);
        if (!(s2 < best)) {
          best = s2;
          best_list = list;
          std::memcpy(blo, lm, sizeof blo);
        }
      }
    }
    if (use_reduction) {
      const double ratio = double(best_list.size()) / n;
      const double p1 = std::min(1.0 - std::numeric_limits<double>::epsilon(), 1.0 - std::pow(ratio, 3.0));
      should_stop = std::log(1.0 - probability) / std::log(p1) < i;
    }
  }
  std::memcpy(model, bm, sizeof bm);
  std::memcpy(lo_model, blo, sizeof blo);
  for (size_t k = 0; k < best_list.size(); k++) inliers[k] = best_list[k];
  *iterations_run = i;
  return best;
}

}  // extern "C"
