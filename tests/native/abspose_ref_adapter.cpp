// abspose_ref_adapter.cpp -- TEST INFRASTRUCTURE: the reference's own LO-RANSAC template (robust_estimator.h, random_sampler.h,
// scorer.h, compiled at test time from where they lie, with the oracle's Eigen stand-in oracle/ref_adapters/stubs) around an
// AbsolutePose adapter (3 samples, up to 4 models) over the product's model numerics (opensfm_amd/csrc/abspose_core.h).  The
// reference's own model header needs Eigen, which is not available, so what this pins is the control flow for a 3-sample, 4-model
// estimator: the draws, the order of the models, ties, local optimisation and the stopping rule.  No reference source is copied.
#include <array>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#include "robust_estimator.h"
#include "../../opensfm_amd/csrc/abspose_core.h"

namespace {
struct Err {
  double v;
  double norm() const { return std::sqrt(v * v); }  // Eigen::Matrix<double, 1, 1>::norm()
};
struct AbsolutePoseAdapter {  // AbsolutePose (robust/absolute_pose_model.h) over abspose_core.h
  using Type = std::array<double, 12>;
  using Data = std::pair<std::array<double, 3>, std::array<double, 3>>;
  static const int MINIMAL_SAMPLES = 3;
  static const int MAX_MODELS = 4;
  template <class IT>
  static void rows(IT begin, IT end, std::vector<double>& b, std::vector<double>& X) {
    for (IT it = begin; it != end; ++it)
      for (int a = 0; a < 3; a++) {
        b.push_back(it->first[a]);
        X.push_back(it->second[a]);
      }
  }
  template <class IT>
  static int Estimate(IT begin, IT end, Type* models) {
    std::vector<double> b, X;
    rows(begin, end, b, X);
    double m[4][12];
    const int count = osfm_ap::p3p_models(b.data(), X.data(), m);
    for (int j = 0; j < count; j++) std::memcpy(models[j].data(), m[j], sizeof m[j]);
    return count;
  }
  template <class IT>
  static int EstimateNonMinimal(IT begin, IT end, Type* models) {
    std::vector<double> b, X;
    rows(begin, end, b, X);
    osfm_ap::npoints_model(b.data(), X.data(), nullptr, (int)(b.size() / 3), models[0].data());
    return 1;
  }
  template <class IT>
  static std::vector<Err> EvaluateModel(const Type& model, IT begin, IT end) {
    std::vector<Err> errors;
    for (IT it = begin; it != end; ++it) errors.push_back(Err{osfm_ap::abspose_error(model.data(), it->first.data(), it->second.data())});
    return errors;
  }
};
}  // namespace

extern "C" int ref_ransac_absolute_pose(const double* b, const double* X, int n, double threshold_angle, int iterations, double probability,
                                        int use_lo, int lo_iterations, int use_reduction, double* model, double* lo_model, int* inliers) {
  std::vector<AbsolutePoseAdapter::Data> samples(n);
  for (int i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) {
      samples[i].first[a] = b[3 * i + a];
      samples[i].second[a] = X[3 * i + a];
    }
  RobustEstimatorParams params;
  params.iterations = iterations;
  params.probability = probability;
  params.use_local_optimization = use_lo != 0;
  params.use_iteration_reduction = use_reduction != 0;
  params.local_optimization_iterations = lo_iterations;
  RansacScoring scorer(1.0 - std::cos(threshold_angle));  // AbsolutePose::ThresholdAdapter
  const auto best = Estimate<RansacScoring, AbsolutePoseAdapter>(samples, scorer, params);
  std::memcpy(model, best.model.data(), 12 * sizeof(double));
  std::memcpy(lo_model, best.lo_model.data(), 12 * sizeof(double));
  for (size_t i = 0; i < best.inliers_indices.size(); i++) inliers[i] = best.inliers_indices[i];
  return (int)best.score;
}
