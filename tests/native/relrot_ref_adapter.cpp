// relrot_ref_adapter.cpp -- TEST INFRASTRUCTURE: the reference's own LO-RANSAC template (robust_estimator.h, random_sampler.h,
// scorer.h, compiled at test time from where they lie, with the oracle's Eigen stand-in oracle/ref_adapters/stubs) around a
// RelativeRotation adapter over the product's model numerics (opensfm_amd/csrc/relrot_core.h).  The reference's own model header
// needs Eigen, which is not available, so what this pins is the control flow for 3-sample, 1-model estimators: the draws, ties,
// local optimisation and the stopping rule.  No reference source is copied.
#include <array>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#include "robust_estimator.h"
#include "../../opensfm_amd/csrc/relrot_core.h"

namespace {
struct Err {
  double v;
  double norm() const { return std::sqrt(v * v); }  // Eigen::Matrix<double, 1, 1>::norm()
};
struct RotationAdapter {  // RelativeRotation (robust/relative_rotation_model.h) over relrot_core.h
  using Type = std::array<double, 9>;
  using Data = std::pair<std::array<double, 3>, std::array<double, 3>>;
  static const int MINIMAL_SAMPLES = 3;
  static const int MAX_MODELS = 1;
  template <class IT>
  static int solve(IT begin, IT end, Type* models) {
    std::vector<double> x, y;
    std::vector<int> idx;
    for (IT it = begin; it != end; ++it) {
      idx.push_back((int)idx.size());
      for (int a = 0; a < 3; a++) {
        x.push_back(it->first[a]);
        y.push_back(it->second[a]);
      }
    }
    osfm_rr::rotation_model(x.data(), y.data(), idx.data(), (int)idx.size(), models[0].data());
    return 1;
  }
  template <class IT>
  static int Estimate(IT begin, IT end, Type* models) { return solve(begin, end, models); }
  template <class IT>
  static int EstimateNonMinimal(IT begin, IT end, Type* models) { return solve(begin, end, models); }
  template <class IT>
  static std::vector<Err> EvaluateModel(const Type& model, IT begin, IT end) {
    std::vector<Err> errors;
    for (IT it = begin; it != end; ++it) errors.push_back(Err{osfm_rr::rotation_error(model.data(), it->first.data(), it->second.data())});
    return errors;
  }
};
}  // namespace

extern "C" int ref_ransac_relative_rotation(const double* b1, const double* b2, int n, double threshold_angle, int iterations, double probability,
                                            int use_lo, int lo_iterations, int use_reduction, double* model, double* lo_model, int* inliers) {
  std::vector<RotationAdapter::Data> samples(n);
  for (int i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) {
      samples[i].first[a] = b1[3 * i + a];
      samples[i].second[a] = b2[3 * i + a];
    }
  RobustEstimatorParams params;
  params.iterations = iterations;
  params.probability = probability;
  params.use_local_optimization = use_lo != 0;
  params.use_iteration_reduction = use_reduction != 0;
  params.local_optimization_iterations = lo_iterations;
  RansacScoring scorer(1.0 - std::cos(threshold_angle));  // RelativeRotation::ThresholdAdapter
  const auto best = Estimate<RansacScoring, RotationAdapter>(samples, scorer, params);
  std::memcpy(model, best.model.data(), 9 * sizeof(double));
  std::memcpy(lo_model, best.lo_model.data(), 9 * sizeof(double));
  for (size_t i = 0; i < best.inliers_indices.size(); i++) inliers[i] = best.inliers_indices[i];
  return (int)best.score;
}
