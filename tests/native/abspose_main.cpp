// abspose_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program of the host walk (abspose_host.cpp) over a small set of images, the
// smallest (n = 3) and one past the LDS inlier list (n = 4097) included, built with -fsanitize=address,undefined and run as a child
// process by tests/test_abspose_host.py.  Every image is also run through the sequential restatement and compared.
#include <cstdio>

#include "abspose_host.cpp"

namespace {
struct Lcg {  // inputs only: any numbers will do
  uint64_t s;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
  }
};
}  // namespace

int main() {
  const int sizes[] = {3, 4, 5, 6, 24, 63, 64, 65, 300, 4097};
  const int n_images = sizeof(sizes) / sizeof(sizes[0]);
  Lcg g{7};
  std::vector<double> b, X;
  std::vector<int64_t> off{0};
  const double R[9] = {0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6}, t[3] = {0.3, -0.2, 0.5};
  for (int p = 0; p < n_images; p++) {
    for (int i = 0; i < sizes[p]; i++) {
      double xc[3] = {4 * g.next() - 2, 4 * g.next() - 2, 4 + 5 * g.next()}, xw[3], v[3];
      for (int a = 0; a < 3; a++) xw[a] = R[a] * (xc[0] - t[0]) + R[3 + a] * (xc[1] - t[1]) + R[6 + a] * (xc[2] - t[2]);
      const bool bad = g.next() < 0.1 * p;  // 0 .. 90 % outliers
      for (int a = 0; a < 3; a++) v[a] = bad ? 2 * g.next() - 1 : xc[a] + 1e-3 * (g.next() - 0.5);
      const double nv = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      for (int a = 0; a < 3; a++) {
        b.push_back(v[a] / nv);
        X.push_back(xw[a]);
      }
    }
    if (p == 5)  // duplicate rows: samples without a model
      for (int i = 1; i < sizes[p]; i += 3)
        for (int a = 0; a < 3; a++) {
          b[3 * (off.back() + i) + a] = b[3 * off.back() + a];
          X[3 * (off.back() + i) + a] = X[3 * off.back() + a];
        }
    off.push_back(off.back() + sizes[p]);
  }
  std::vector<AbsposeOut> out(n_images);
  std::vector<uint8_t> rmask(off.back()), cmask(off.back());
  for (int variant = 0; variant < 2; variant++) {
    const int use_lo = variant == 0, use_reduction = variant == 0, iterations = variant == 0 ? 1000 : 60;
    const int rc = host_abspose_images(b.data(), X.data(), off.data(), n_images, 0.004, 0.99, iterations, use_lo, 10, use_reduction, out.data(),
                                       rmask.data(), cmask.data());
    if (rc != 0) {
      std::printf("abspose_main: host_abspose_images returned %d\n", rc);
      return 1;
    }
    for (int p = 0; p < n_images; p++) {
      double m[12], lo[12];
      std::vector<int> inl(sizes[p]);
      int it = 0, stats[2] = {0, 0};
      const int s = host_sequential_estimate(b.data() + 3 * off[p], X.data() + 3 * off[p], sizes[p], 0.004, 0.99, iterations, use_lo, 10,
                                             use_reduction, m, lo, inl.data(), &it, stats);
      bool same = s == out[p].score && it == out[p].iterations && !std::memcmp(m, out[p].model, sizeof m) && !std::memcmp(lo, out[p].lo_model, sizeof lo);
      int c = 0;
      for (int i = 0; i < sizes[p] && same; i++)
        if (rmask[off[p] + i]) same = c < s && inl[c++] == i;
      if (!same || c != s) {
        std::printf("abspose_main: image %d (n = %d, variant %d) differs from the sequential estimate\n", p, sizes[p], variant);
        return 1;
      }
    }
  }
  std::printf("abspose_main: ok\n");
  return 0;
}
