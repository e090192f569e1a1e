// loop_wave.h -- TEST INFRASTRUCTURE shared by the host builds of the LO-RANSAC walks (relrot_host.cpp, abspose_host.cpp,
// relpose_core_host.cpp): the wave policy with loops in place of lanes, this toolchain's std::mt19937(42) stream tabulated as the
// device's is, and ShouldStop's bound tabulated per problem size.
#pragma once
#include <cstdint>
#include <random>
#include <unordered_map>
#include <vector>

#include "../../opensfm_amd/csrc/loransac_walk.h"
#include "../../opensfm_amd/csrc/relpose_core.h"  // max_iterations_for

namespace {

struct LoopWave {  // "lanes" are loop iterations; single() runs once
  template <class F> void single(F f) { f(); }
  template <class F> void parallel_for(int n, F f) { for (int i = 0; i < n; i++) f(i); }
  template <class P> int count_if(int n, P p) { int c = 0; for (int i = 0; i < n; i++) c += p(i) ? 1 : 0; return c; }
  template <class P> int compact(int n, P p, int* out) { int c = 0; for (int i = 0; i < n; i++) if (p(i)) out[c++] = i; return c; }
  template <class P> int compact_changed(int n, P p, int* out, int* changed) {
    int c = 0;
    for (int i = 0; i < n; i++)
      if (p(i)) {
        if (out[c] != i) *changed = 1;
        out[c++] = i;
      }
    return c;
  }
  int atomic_add(int* p, int v) { const int o = *p; *p += v; return o; }
  // the GPU stages a window of the stream in LDS; here a short one, so that both paths of RngView::get are exercised
  osfm_lo::RngView stage_rng(const osfm_lo::RngTable& T, uint32_t* buf, int pos, bool want) {
    int n = 0;
    if (want)
      for (; n < osfm_lo::kRngCache / 16 && pos + n < T.size; n++) buf[n] = T.tab[pos + n];
    return osfm_lo::RngView{T, buf, pos, n};
  }
};

// the first 2^kLog2 raw outputs of std::mt19937(42) (the device table, relpose.hip kRngTableSize, has 2^21)
template <int kLog2>
osfm_lo::RngTable rng_table() {
  static const std::vector<uint32_t> t = [] {  // (a function-local static: initialised once, also under threads)
    std::vector<uint32_t> v((size_t)1 << kLog2);
    std::mt19937 g(42);
    for (auto& x : v) x = (uint32_t)g();
    return v;
  }();
  return osfm_lo::RngTable{t.data(), (int)t.size()};
}

// ShouldStop's bound for every best inlier count 0 .. n, one table per distinct problem size (as osfm_stop_tables lays them out);
// false when a problem has fewer than minimal_samples rows
bool stop_tables(const int64_t* offsets, int n_problems, double probability, int minimal_samples, std::vector<double>* stop,
                        std::vector<int64_t>* stop_off) {
  std::unordered_map<int, int64_t> of_n;
  stop_off->assign((size_t)n_problems, 0);
  for (int p = 0; p < n_problems; p++) {
    const int n = (int)(offsets[p + 1] - offsets[p]);
    if (n < minimal_samples) return false;
    auto it = of_n.find(n);
    if (it == of_n.end()) {
      it = of_n.emplace(n, (int64_t)stop->size()).first;
      for (int c = 0; c <= n; c++) stop->push_back(osfm_rp::max_iterations_for(c, n, probability, minimal_samples));
    }
    (*stop_off)[(size_t)p] = it->second;
  }
  return true;
}

}  // namespace
