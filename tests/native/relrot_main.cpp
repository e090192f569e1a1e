// relrot_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program of the host walk (relrot_host.cpp) over a small set of pairs, the
// smallest (n = 3) and one past the LDS inlier list (n = 4097) included, built with -fsanitize=address,undefined and run as a child
// process by tests/test_relrot_host.py.  Every pair is also run through the sequential restatement and compared.
#include <cstdio>

#include "relrot_host.cpp"

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
  const int sizes[] = {3, 4, 5, 63, 64, 65, 300, 4097};
  const int n_pairs = sizeof(sizes) / sizeof(sizes[0]);
  Lcg g{7};
  std::vector<double> b1, b2;
  std::vector<int64_t> off{0};
  const double R[9] = {0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6};
  for (int p = 0; p < n_pairs; p++) {
    for (int i = 0; i < sizes[p]; i++) {
      double x[3] = {4 * g.next() - 2, 4 * g.next() - 2, 4 + 5 * g.next()}, y[3];
      const bool bad = g.next() < 0.125 * p;  // 0 .. 87 % outliers
      for (int a = 0; a < 3; a++) y[a] = bad ? 2 * g.next() - 1 : R[3 * a] * x[0] + R[3 * a + 1] * x[1] + R[3 * a + 2] * x[2] + 1e-3 * (g.next() - 0.5);
      const double nx = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), ny = std::sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
      for (int a = 0; a < 3; a++) {
        b1.push_back(x[a] / nx);
        b2.push_back(y[a] / ny);
      }
    }
    if (p == 3)  // duplicate correspondences: rank-deficient samples
      for (int i = 1; i < sizes[p]; i += 3)
        for (int a = 0; a < 3; a++) {
          b1[3 * (off.back() + i) + a] = b1[3 * off.back() + a];
          b2[3 * (off.back() + i) + a] = b2[3 * off.back() + a];
        }
    off.push_back(off.back() + sizes[p]);
  }
  std::vector<RelrotOut> out(n_pairs);
  std::vector<uint8_t> mask(off.back());
  for (int variant = 0; variant < 2; variant++) {
    const int use_lo = variant == 0, use_reduction = variant == 0, iterations = variant == 0 ? 1000 : 60;
    const int rc = host_relrot_pairs(b1.data(), b2.data(), off.data(), n_pairs, 0.016, 0.99, 0.016, iterations, use_lo, 10, use_reduction, out.data(),
                                     mask.data());
    if (rc != 0) {
      std::printf("relrot_main: host_relrot_pairs returned %d\n", rc);
      return 1;
    }
    for (int p = 0; p < n_pairs; p++) {
      double m[9], lo[9];
      std::vector<int> inl(sizes[p]);
      int it = 0;
      const int s = host_sequential_estimate(b1.data() + 3 * off[p], b2.data() + 3 * off[p], sizes[p], 0.016, 0.99, iterations, use_lo, 10, use_reduction,
                                             m, lo, inl.data(), &it);
      bool same = s == out[p].score && it == out[p].iterations && !std::memcmp(m, out[p].model, sizeof m) && !std::memcmp(lo, out[p].lo_model, sizeof lo);
      int c = 0;
      for (int i = 0; i < sizes[p] && same; i++)
        if (mask[off[p] + i]) same = c < s && inl[c++] == i;
      if (!same || c != s) {
        std::printf("relrot_main: pair %d (n = %d, variant %d) differs from the sequential estimate\n", p, sizes[p], variant);
        return 1;
      }
    }
  }
  std::printf("relrot_main: ok\n");
  return 0;
}
