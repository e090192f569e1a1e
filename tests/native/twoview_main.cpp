// twoview_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program of the host build of the two-view finish (twoview_host.cpp) over a small
// set of pairs -- none, the "more than 5" edge (5, 6), the wavefront edge of the compaction (64, 65) and one past the pick count of the
// refinement (101) -- built with -fsanitize=address,undefined and run as a child process by tests/test_twoview_host.py.  Both modes (RANSAC
// first, given poses) and both settings of check_reversal run; what comes back is checked for consistency with itself.
#include <cstdio>

#include "twoview_host.cpp"

namespace {
struct Lcg {  // inputs only: any numbers will do
  uint64_t s;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
  }
};

bool consistent(const TwoViewOut& r, int n, int check_reversal, double ratio, const uint8_t* mask) {
  if (n <= kTwoViewMinInliers) return r.status == kTwoViewNoConfiguration && r.chosen == -1 && r.n_inliers[0] == -1 && r.n_inliers[1] == -1;
  int chosen = -2, count[3] = {0, 0, 0};
  if (r.status != two_view_decide(r.n_inliers[0], r.n_inliers[1], check_reversal, ratio, &chosen) || chosen != r.chosen) return false;
  if (!check_reversal && r.n_inliers[1] != -1) return false;
  for (int i = 0; i < n; i++)
    for (int b = 0; b < 3; b++) count[b] += (mask[i] >> b) & 1;
  if (count[0] != r.n_inliers[0] || count[1] != (check_reversal ? r.n_inliers[1] : 0)) return false;
  return count[2] == (r.chosen >= 0 ? r.n_inliers[r.chosen] : 0);
}
}  // namespace

int main() {
  const int sizes[] = {0, 5, 6, 64, 65, 101};
  const int n_pairs = sizeof(sizes) / sizeof(sizes[0]);
  Lcg g{11};
  std::vector<double> b1, b2, poses;
  std::vector<int64_t> off{0};
  // second camera: x2 = R x1 + t; the pose handed over is its inverse (the second camera in the first)
  const double R[9] = {0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6}, t[3] = {0.3, -0.2, 0.1};
  for (int p = 0; p < n_pairs; p++) {
    for (int i = 0; i < sizes[p]; i++) {
      const double X[3] = {4 * g.next() - 2, 4 * g.next() - 2, 4 + 5 * g.next()};
      double x[3], y[3];
      const bool bad = sizes[p] > 12 && g.next() < 0.3;
      for (int a = 0; a < 3; a++) {
        x[a] = X[a] + 1e-3 * (g.next() - 0.5);
        y[a] = bad ? 2 * g.next() - 1 : R[3 * a] * X[0] + R[3 * a + 1] * X[1] + R[3 * a + 2] * X[2] + t[a] + 1e-3 * (g.next() - 0.5);
      }
      const double nx = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), ny = std::sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
      for (int a = 0; a < 3; a++) {
        b1.push_back(x[a] / nx);
        b2.push_back(y[a] / ny);
      }
    }
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) poses.push_back(R[3 * b + a]);
    for (int a = 0; a < 3; a++) poses.push_back(-(R[a] * t[0] + R[3 + a] * t[1] + R[6 + a] * t[2]));
    off.push_back(off.back() + sizes[p]);
  }
  std::vector<TwoViewOut> out(n_pairs);
  std::vector<uint8_t> mask(off.back() + 1);
  for (int variant = 0; variant < 4; variant++) {
    const int check_reversal = variant & 1, given = variant >> 1;
    const double ratio = 0.95;
    const int rc = host_two_view_pairs(b1.data(), b2.data(), off.data(), n_pairs, given ? poses.data() : nullptr, 0.004, 0.99, 1000, 1, 10, 1000,
                                       check_reversal, ratio, 0, out.data(), mask.data());
    if (rc != 0) {
      std::printf("twoview_main: host_two_view_pairs returned %d\n", rc);
      return 1;
    }
    for (int p = 0; p < n_pairs; p++) {
      if (!consistent(out[p], sizes[p], check_reversal, ratio, mask.data() + off[p])) {
        std::printf("twoview_main: pair %d (n = %d, variant %d) is not consistent with itself\n", p, sizes[p], variant);
        return 1;
      }
      if (given && sizes[p] > 5 && (out[p].status != kTwoViewOk || out[p].chosen != 0)) {
        std::printf("twoview_main: pair %d (n = %d, variant %d): the true pose was not chosen\n", p, sizes[p], variant);
        return 1;
      }
    }
  }
  // the refinement on its own: every correspondence counts
  if (host_two_view_pairs(b1.data(), b2.data(), off.data(), n_pairs, poses.data(), 0.004, 0.99, 1000, 1, 10, 20, 0, 1.0, 1, out.data(), mask.data()) != 0 ||
      out[5].n_inliers[0] != 101 || out[5].refine_iterations[0] < 1) {
    std::printf("twoview_main: the refinement without the inlier tests did not run over all 101 correspondences\n");
    return 1;
  }
  std::printf("twoview_main: ok\n");
  return 0;
}
