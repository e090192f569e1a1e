// plane_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program of the host build of the plane-based two-view solve (plane_host.cpp) over
// one mixed batch -- too few rows (3), the sample is the data (4), 5, the wavefront edge (63, 64, 65), 300, one above kLdsInliers
// (4097, the per-row scratch path), a pair behind the second camera and a pure rotation -- built with -fsanitize=address,undefined
// and run as a child process by tests/test_plane_host.py.  What comes back is checked for consistency with itself and with the scene.
#include <cstdio>

#include "plane_host.cpp"

namespace {
struct Lcg {  // inputs only: any numbers will do
  uint64_t s;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
  }
};
enum Kind { kPlane, kBehind, kRotation };
}  // namespace

int main() {
  const int sizes[] = {3, 4, 5, 63, 64, 65, 300, 4097, 12, 64};
  const Kind kinds[] = {kPlane, kPlane, kPlane, kPlane, kPlane, kPlane, kPlane, kPlane, kBehind, kRotation};
  const int n_pairs = sizeof(sizes) / sizeof(sizes[0]);
  Lcg g{5};
  // X2 = R X1 + t; the plane n . X1 = d
  const double R[9] = {0.9950, -0.0998, 0.0, 0.0998, 0.9950, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.5, -0.2, 0.1}, nrm[3] = {0.1, -0.05, 0.99}, d = 5.0;
  std::vector<double> b1, b2;
  std::vector<int> planted;  // per pair: the rows on the plane
  std::vector<int64_t> off{0};
  for (int p = 0; p < n_pairs; p++) {
    int good = 0;
    for (int i = 0; i < sizes[p]; i++) {
      const double ray[3] = {0.9 * g.next() - 0.45, 0.9 * g.next() - 0.45, 1.0};
      const double depth = d / (nrm[0] * ray[0] + nrm[1] * ray[1] + nrm[2] * ray[2]);
      const double X[3] = {ray[0] * depth, ray[1] * depth, depth};
      double y[3];
      const bool bad = kinds[p] == kPlane && sizes[p] > 5 && g.next() < 0.3;
      for (int a = 0; a < 3; a++) y[a] = R[3 * a] * X[0] + R[3 * a + 1] * X[1] + R[3 * a + 2] * X[2] + (kinds[p] == kRotation ? 0.0 : t[a]);
      if (bad) {
        y[0] = (g.next() - 0.5) * y[2];
        y[1] = (g.next() - 0.5) * y[2];
      }
      good += bad ? 0 : 1;
      const double nx = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), ny = std::sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
      for (int a = 0; a < 3; a++) {
        b1.push_back(X[a] / nx);
        b2.push_back((kinds[p] == kBehind ? -1.0 : 1.0) * y[a] / ny);
      }
    }
    planted.push_back(good);
    off.push_back(off.back() + sizes[p]);
  }
  std::vector<PlaneOut> out(n_pairs);
  std::vector<uint8_t> mask(off.back() + 1);
  for (int variant = 0; variant < 2; variant++) {  // with and without the local optimisation
    const int rc = host_plane_pairs(b1.data(), b2.data(), off.data(), n_pairs, 0.004, 0.99, 1000, variant == 0, 10, 1, out.data(), mask.data());
    if (rc != 0) {
      std::printf("plane_main: host_plane_pairs returned %d\n", rc);
      return 1;
    }
    for (int p = 0; p < n_pairs; p++) {
      const PlaneOut& r = out[p];
      int count[2] = {0, 0};
      for (int i = 0; i < sizes[p]; i++)
        for (int b = 0; b < 2; b++) count[b] += (mask[off[p] + i] >> b) & 1;
      const int want = sizes[p] < 4 || kinds[p] == kBehind ? kPlaneNoHomography : (kinds[p] == kRotation ? kPlaneDegenerate : kPlaneOk);
      bool ok = r.status == want && count[0] == r.h_inliers && count[1] == r.n_inliers;
      if (want == kPlaneOk)
        ok = ok && r.chosen == plane_pick(r.motion_inliers) && r.n_inliers == r.motion_inliers[r.chosen] && r.h_inliers >= planted[p] &&
             r.n_inliers >= planted[p];
      else
        ok = ok && r.chosen == -1 && r.n_inliers == 0;
      if (!ok) {
        std::printf("plane_main: pair %d (n = %d, variant %d): status %d, chosen %d, %d / %d inliers, %d on the plane\n", p, sizes[p], variant,
                    r.status, r.chosen, r.h_inliers, r.n_inliers, planted[p]);
        return 1;
      }
    }
  }
  std::printf("plane_main: ok\n");
  return 0;
}
