// loransac_walk.h -- robust::Estimate<RansacScoring, Model> (robust/robust_estimator.h:37-119) for ONE problem on ONE wavefront, and
// the sampler on the tabulated generator stream that every LO-RANSAC of this project draws from.
//
// walk<W, M> is instantiated by abspose_core.h (AbsolutePose: up to four models per sample, the non-minimal solver a batch at a
// time).  relrot_core.h keeps the same walk written out for RelativeRotation (as an instantiation its kernel measured slower, DESIGN.md
// 4d5) and relpose_rounds.h has a walk of its own, cut into kernels; both take the sampler from here.
//
// Everything is host + device: the tests compile the instantiations with g++ and a wave policy W whose "lanes" are loop iterations
// (tests/native/loop_wave.h), the kernels with gpu_wave.h's, one wavefront per problem.  W: single / parallel_for / count_if /
// compact / compact_changed / stage_rng.
#pragma once
#include "relpose_core.h"  // OSFM_HD

namespace osfm_lo {

constexpr int kLoSampleMax = 12; // lo_sample_size_clamp

// std::mt19937(42) is the same stream for every problem: its raw outputs are tabulated once and a generator "state" is an index into
// the table -- nothing to snapshot, rewind or replay.
struct RngTable {
  const uint32_t* tab;  // raw outputs of std::mt19937(42), in order
  int size;
};
constexpr int kRngCache = 512;  // stream entries a walk stages next to itself before it draws (LDS on the GPU)

// A window of the stream: entries [cache_pos, cache_pos + cache_n) come from `cache`, everything else from the table
struct RngView {
  RngTable T;
  const uint32_t* cache;
  int cache_pos, cache_n;
  OSFM_HD uint32_t get(int i) const {
    const unsigned k = (unsigned)(i - cache_pos);
    return k < (unsigned)cache_n ? cache[k] : T.tab[i];
  }
};

// RandomSamplesGenerator::GenerateOneSample (robust/random_sampler.h:27-37) on the tabulated stream: `size` distinct indices in
// [0, n) with std::uniform_int_distribution as libstdc++ >= 11 draws it (Lemire's multiply-shift with rejection).  Returns the
// stream position after the sample; *overflow is set when the table is too short (the caller then reports it).
OSFM_HD int draw_sample_tab(const RngView& V, int pos, int size, int n, int* idx, int* overflow) {
  for (int i = 0; i < size; i++) {
    int dup;
    do {
      const uint32_t range = (uint32_t)n;
      if (pos >= V.T.size) {
        *overflow = 1;
        for (int q = i; q < size; q++) idx[q] = q < n ? q : 0;
        return pos;
      }
      uint64_t product = (uint64_t)V.get(pos++) * (uint64_t)range;
      uint32_t low = (uint32_t)product;
      if (low < range) {
        const uint32_t threshold = (0u - range) % range;
        while (low < threshold) {
          if (pos >= V.T.size) {
            *overflow = 1;
            for (int q = i; q < size; q++) idx[q] = q < n ? q : 0;
            return pos;
          }
          product = (uint64_t)V.get(pos++) * (uint64_t)range;
          low = (uint32_t)product;
        }
      }
      idx[i] = (int)(uint32_t)(product >> 32);
      dup = 0;
      for (int j = 0; j < i; j++) dup |= idx[j] == idx[i];
    } while (dup);
  }
  return pos;
}
OSFM_HD int draw_sample_tab(const RngTable& T, int pos, int size, int n, int* idx, int* overflow) {
  const RngView V{T, nullptr, 0, 0};
  return draw_sample_tab(V, pos, size, n, idx, overflow);
}

// LO sample size: max(min(12, int(inliers * 0.5)), MINIMAL_SAMPLES)
OSFM_HD int lo_sample_size(int inliers, int minimal_samples) {
  int s = (int)(inliers * 0.5);
  if (s > kLoSampleMax) s = kLoSampleMax;
  return s < minimal_samples ? minimal_samples : s;
}

constexpr int kLdsInliers = 4096;  // inlier lists of problems up to this size stay in LDS; longer ones use per-row scratch

// ---------------------------------------------------------------------------------------------------------------
// The walk.  M is the problem: its data and threshold, and
//   kModelSize, kMinimalSamples, kMaxModels   doubles of a model, Model::MINIMAL_SAMPLES, Model::MAX_MODELS
//   kSlots                                    speculative main iterations per block (kSlots * kMaxModels lanes solve them)
//   kLoBatch                                  speculative LO iterations per block (one non-minimal solve per lane)
//   int solve_minimal(idx, root, out)         model `root` of the sample idx[kMinimalSamples]; returns the sample's number of models
//   void solve_nonminimal(idx, size, out)     the LO's model of idx[size]
//   bool inlier(model, i)                     RansacScoring on row i
// ---------------------------------------------------------------------------------------------------------------
template <class M>
struct WalkShared {  // LDS of a walk
  uint32_t rng[kRngCache];
  double models[M::kSlots][M::kMaxModels][M::kModelSize];
  int nmodels[M::kSlots];
  int sidx[M::kSlots][M::kMinimalSamples];
  int pos_after[M::kSlots];
  double lo[M::kLoBatch][M::kModelSize];
  int lidx[M::kLoBatch][kLoSampleMax];
  int lo_pos_after[M::kLoBatch];
  int overflow, changed;
  int inl[kLdsInliers];
};

template <class M>
struct WalkResult {
  double model[M::kModelSize], lo_model[M::kModelSize];
  int best, iterations;  // score (= length of the inlier list) and iterations run
  int failed;            // the tabulated stream was too short: the caller sets the batch's overflow flag
};

// The samples of the next B iterations are drawn by lane 0 and solved kMaxModels lanes per sample, assuming no local optimisation
// fires in between; when one does, the generator has moved and the remaining samples of the block are dropped (the next block draws
// from where the generator stands).  A local optimisation's samples are drawn kLoBatch at a time too, assuming none of them changes
// the inlier list, and solved one per lane; they are scored in order, and at the first one that changes the list the rest are redrawn
// from the generator position after it.  The decision sequence is the sequential one.
// A: the batch's arguments (RelrotArgs / AbsposeArgs: rng, iterations, use_lo, lo_iterations, use_reduction are read); n rows;
// stop_bound: the problem's table; inliers: n ints, the inlier list of the best score (ascending) when the walk returns.
template <class W, class M, class Args>
OSFM_HD void walk(W& w, WalkShared<M>& sh, const M& m, const Args& A, const double* stop_bound, int n, int* inliers, WalkResult<M>& r) {
  constexpr int kSize = M::kModelSize;
  auto is_inlier = [&](const double* mdl) { return [=](int i) { return m.inlier(mdl, i); }; };
  int pos = 0, it = 0, best = 0, width = 1, stop = 0, failed = 0;
  for (int i = 0; i < kSize; i++) r.model[i] = r.lo_model[i] = 0.0;
  // The window of the stream is staged at the generator's position before every speculative set of draws (a block of main samples,
  // a batch of LO samples).  Results do not depend on this: RngView::get falls back to the table.
  while (it < A.iterations && !stop && !failed) {
    int B = width < M::kSlots ? width : M::kSlots;
    if (B > A.iterations - it) B = A.iterations - it;
    RngView V = w.stage_rng(A.rng, sh.rng, pos, true);
    w.single([&]() {
      int q = pos, ovf = 0;
      for (int k = 0; k < B; k++) {
        q = draw_sample_tab(V, q, M::kMinimalSamples, n, sh.sidx[k], &ovf);
        sh.pos_after[k] = q;
      }
      sh.overflow = ovf;
    });
    if (sh.overflow) {
      failed = 1;
      break;
    }
    w.parallel_for(B * M::kMaxModels, [&](int j) {
      const int k = j / M::kMaxModels, root = j % M::kMaxModels;
      const int cnt = m.solve_minimal(sh.sidx[k], root, sh.models[k][root]);
      if (root == 0) sh.nmodels[k] = cnt;
    });
    int lo_fired = 0;
    for (int k = 0; k < B && !stop && !lo_fired && !failed; k++) {
      pos = sh.pos_after[k];
      const int nm = sh.nmodels[k];  // 0: the iteration still counts, and the stop flag stays as it is
      for (int j = 0; j < nm && !stop && !failed; j++) {
        double mk[kSize];
        for (int i = 0; i < kSize; i++) mk[i] = sh.models[k][j][i];
        const int cnt = w.count_if(n, is_inlier(mk));
        if (cnt >= best) {  // std::max(score, best_score): ties keep the newcomer
          best = cnt;
          (void)w.compact(n, is_inlier(mk), inliers);
          for (int i = 0; i < kSize; i++) r.model[i] = r.lo_model[i] = mk[i];
        }
        if (cnt == best && cnt >= M::kMinimalSamples && A.use_lo && A.lo_iterations > 0) {
          lo_fired = 1;
          int l = 0;
          while (l < A.lo_iterations && !failed) {
            const int size = lo_sample_size(best, M::kMinimalSamples);
            int nb = A.lo_iterations - l;
            if (nb > M::kLoBatch) nb = M::kLoBatch;
            V = w.stage_rng(A.rng, sh.rng, pos, true);
            w.single([&]() {
              int q = pos, ovf = 0;
              for (int s = 0; s < nb; s++) {
                int pick[kLoSampleMax];
                q = draw_sample_tab(V, q, size, best, pick, &ovf);
                for (int i = 0; i < size; i++) sh.lidx[s][i] = inliers[pick[i]];
                sh.lo_pos_after[s] = q;
              }
              sh.overflow = ovf;
            });
            if (sh.overflow) {
              failed = 1;
              break;
            }
            w.parallel_for(nb, [&](int s) { m.solve_nonminimal(sh.lidx[s], size, sh.lo[s]); });
            for (int s = 0; s < nb; s++) {
              pos = sh.lo_pos_after[s];
              l++;
              double lm[kSize];
              for (int i = 0; i < kSize; i++) lm[i] = sh.lo[s][i];
              const int c2 = w.count_if(n, is_inlier(lm));
              if (c2 >= best) {  // lo_score.model = best_score.model: only lo_model changes
                w.single([&]() { sh.changed = c2 != best; });
                best = c2;
                (void)w.compact_changed(n, is_inlier(lm), inliers, &sh.changed);
                for (int i = 0; i < kSize; i++) r.lo_model[i] = lm[i];
                if (sh.changed) break;  // the later samples were drawn from the list as it was
              }
            }
          }
        }
        if (A.use_reduction) stop = stop_bound[best] < (double)it;  // ShouldStop, after every scored model
      }
      it++;
    }
    // new bests come early and in bursts: speculate little right after a local optimisation, more once the blocks run through
    width = lo_fired ? it / 2 + 2 : 2 * B;
  }
  r.best = best;
  r.iterations = it;
  r.failed = failed;
}

}  // namespace osfm_lo
