// abspose_host.cpp -- TEST INFRASTRUCTURE: compiles the product's absolute-pose LO-RANSAC (opensfm_amd/csrc/abspose_core.h) for the
// HOST with loops in place of lanes, next to an independent sequential restatement of Estimate<RansacScoring, AbsolutePose> on this
// toolchain's real std::mt19937 / std::uniform_int_distribution, so that tests/test_abspose_host.py can compare the two bit for bit
// without a GPU.  tests/native/abspose_main.cpp includes this file for its sanitizer run.  Nothing in the product links or loads it.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../opensfm_amd/csrc/abspose_core.h"
#include "loop_wave.h"

using namespace osfm_ap;

extern "C" {

// roots[0..3]: quartic_roots; roots[4..7]: after refine_quartic_roots.  Returns 0 where SolveQuartic refuses.
int host_quartic(const double* coefficients, double* roots) {
  if (!quartic_roots(coefficients, roots)) return 0;
  for (int i = 0; i < 4; i++) roots[4 + i] = roots[i];
  refine_quartic_roots(coefficients, roots + 4);
  return 1;
}
void host_ccbrt(const double* z, double* out) {
  const Cx r = ccbrt_principal(Cx{z[0], z[1]});
  out[0] = r.re, out[1] = r.im;
}
void host_csqrt(const double* z, double* out) {
  const Cx r = csqrt_principal(Cx{z[0], z[1]});
  out[0] = r.re, out[1] = r.im;
}
int host_p3p_coefficients(const double* b, const double* X, double* coefficients) {
  P3PSetup S;
  const int idx[3] = {0, 1, 2};
  const bool ok = p3p_setup(b, X, idx, S);
  for (int i = 0; i < 5; i++) coefficients[i] = ok ? S.coefficients[i] : 0.0;
  return ok;
}
int host_p3p_models(const double* b, const double* X, double* models) { return p3p_models(b, X, (double(*)[12])models); }
void host_npoints_model(const double* b, const double* X, int n, double* model) { npoints_model(b, X, nullptr, n, model); }
double host_abspose_error(const double* model, const double* b, const double* X) { return abspose_error(model, b, X); }
double host_abspose_chord(const double* lo_model, const double* b, const double* X) {
  double T[12];
  invert_model(lo_model, T);
  return abspose_chord(T, b, X);
}

// abspose_core.h's walk for every image of a batch (what ap_images_kernel runs, one "wavefront" after the other)
int host_abspose_images(const double* b, const double* X, const int64_t* offsets, int n_images, double threshold, double probability,
                        int iterations, int use_lo, int lo_iterations, int use_reduction, AbsposeOut* out, uint8_t* ransac_mask,
                        uint8_t* chord_mask) {
  std::vector<double> stop;
  std::vector<int64_t> stop_off;
  if (!stop_tables(offsets, n_images, probability, kMinimalSamples, &stop, &stop_off)) return -1;
  std::vector<int> scratch((size_t)std::max<int64_t>(offsets[n_images], 1));
  int overflow = 0;
  AbsposeArgs A{b, X, offsets, stop.data(), stop_off.data(), rng_table<21>(), 1.0 - std::cos(threshold), threshold,
                iterations, use_lo, lo_iterations, use_reduction, scratch.data(), out, ransac_mask, chord_mask, &overflow};
  LoopWave w;
  std::vector<AbsposeShared> sh(1);  // per call: callers run batches on several threads
  for (int p = 0; p < n_images; p++) abspose_image(w, sh[0], A, p);
  return overflow ? -3 : 0;
}

// Estimate<RansacScoring, AbsolutePose> restated sequentially (robust_estimator.h:37-119, random_sampler.h, scorer.h) on the real
// std::mt19937(42) and std::uniform_int_distribution, around the header's model numerics.  Returns the score.
// stats[0] += LO iterations that improved or tied, stats[1] += samples without a model.
int host_sequential_estimate(const double* b, const double* X, int n, double threshold, double probability, int iterations, int use_lo,
                             int lo_iterations, int use_reduction, double* model, double* lo_model, int* inliers, int* iterations_run,
                             int* stats) {
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
    for (int i = 0; i < n; i++) {
      const double e = abspose_error(m, b + 3 * i, X + 3 * i);
      if (std::sqrt(e * e) < thr) list.push_back(i);
    }
    return (int)list.size();
  };
  int best = 0;
  std::vector<int> best_list, list, idx;
  double bm[12] = {0}, blo[12] = {0};
  bool should_stop = false;
  int i = 0;
  for (; i < iterations && !should_stop; ++i) {
    sample(3, n - 1, idx);
    double sb[9], sX[9], models[4][12];
    for (int q = 0; q < 3; q++)
      for (int a = 0; a < 3; a++) {
        sb[3 * q + a] = b[3 * idx[q] + a];
        sX[3 * q + a] = X[3 * idx[q] + a];
      }
    const int count = p3p_models(sb, sX, models);
    if (count == 0) stats[1]++;
    for (int j = 0; j < count && !should_stop; ++j) {
      const double* m = models[j];
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
          std::vector<double> lb, lX;
          for (int q = 0; q < size; q++)
            for (int a = 0; a < 3; a++) {
              lb.push_back(b[3 * inl[idx[q]] + a]);
              lX.push_back(X[3 * inl[idx[q]] + a]);
            }
          double lm[12];
          npoints_model(lb.data(), lX.data(), nullptr, size, lm);
          const int s2 = score_of(lm, list);
          if (!(s2 < best)) {
            if (s2 > best || list != best_list) stats[0]++;
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
  }
  std::memcpy(model, bm, sizeof bm);
  std::memcpy(lo_model, blo, sizeof blo);
  for (size_t k = 0; k < best_list.size(); k++) inliers[k] = best_list[k];
  *iterations_run = i;
  return best;
}

}  // extern "C"
