// lo_batch.h -- the batch driver of the one-wavefront-per-problem LO-RANSAC kernels (relrot.hip, abspose.hip): the argument check,
// the device side of what RelrotArgs / AbsposeArgs have in common, the launch and the way back.  HIP only.
#pragma once
#include <math.h>

#include <vector>

#include "gpu_wave.h"
#include "loransac_walk.h"
#include "osfm_internal.h"

namespace osfm_lo {

struct BatchWords {  // how the messages name a problem and its rows: "pair" / "correspondences", "image" / "rows"
  const char *problem, *rows;
};

// P: osfm_relrot_params / osfm_abspose_params (the same fields)
template <class P>
int check_batch_args(const int64_t *offsets, int n_problems, const P *prm, int minimal_samples, BatchWords words, const char *who) {
  OSFM_REQUIRE(offsets && prm, OSFM_E_INVALID, "%s: null argument", who);
  OSFM_REQUIRE(n_problems >= 0, OSFM_E_INVALID, "%s: n_%ss < 0", who, words.problem);
  OSFM_REQUIRE(prm->iterations >= 0 && prm->lo_iterations >= 0 && prm->threshold > 0 && prm->probability > 0 && prm->probability < 1,
               OSFM_E_INVALID, "%s: bad parameters", who);
  if (n_problems == 0) return OSFM_OK;
  OSFM_REQUIRE(offsets[0] == 0, OSFM_E_INVALID, "%s: offsets[0] must be 0", who);
  for (int p = 0; p < n_problems; p++) {
    OSFM_REQUIRE(offsets[p + 1] - offsets[p] >= minimal_samples, OSFM_E_INVALID, "%s: %s %d has %lld %s (at least %d are needed to draw a sample)",
                 who, words.problem, p, (long long)(offsets[p + 1] - offsets[p]), words.rows, minimal_samples);
    OSFM_REQUIRE(offsets[p + 1] - offsets[p] <= (1 << 24), OSFM_E_INVALID, "%s: %s %d is too large", who, words.problem, p);
  }
  return OSFM_OK;
}

struct BatchArgs {  // the fields RelrotArgs / AbsposeArgs share, as run_batch sets them up (the pointers: device memory)
  const int64_t *offsets;
  const double *stop_bound;
  const int64_t *stop_off;
  RngTable rng;
  double thr, chord;
  int iterations, use_lo, lo_iterations, use_reduction;
  int *scratch, *overflow;
};

// The batch on device-resident rows (d_off: the offsets on the device); results (n_problems x result_bytes) and up to two masks of
// `total` bytes (null: not wanted) copied to the host.  launch(B, d_results, d_mask0, d_mask1) starts the kernel on st, one wavefront
// per problem.  timed_from_ev0: the caller has recorded ctx->ev[0] ahead of a kernel of its own.  The caller holds the context lock.
template <class P, class Launch>
int run_batch(osfm_ctx *ctx, hipStream_t st, const int64_t *d_off, const int64_t *offsets, int n_problems, const P *prm, int minimal_samples,
              void *results, size_t result_bytes, uint8_t *mask0, uint8_t *mask1, bool timed_from_ev0, double *kernel_ms, const char *who,
              Launch launch) {
  const int64_t total = offsets[n_problems];
  RngTable rng;
  OSFM_TRY(osfm_rng_table(ctx, &rng));
  std::vector<double> stop;
  std::vector<int64_t> stop_off;
  osfm_stop_tables(ctx, offsets, n_problems, prm->probability, minimal_samples, &stop, &stop_off);
  bool any_large = false;
  for (int p = 0; p < n_problems && !any_large; p++) any_large = offsets[p + 1] - offsets[p] > kLdsInliers;
  OsfmArena A;
  const auto d_stop = A.add<double>(stop.size());
  const auto d_stopoff = A.add<int64_t>(stop_off.size());
  const auto d_scratch = A.add<int>(any_large ? (size_t)total : 1);
  const auto d_out = A.add<char>((size_t)n_problems * result_bytes);
  const auto d_mask0 = A.add<uint8_t>(mask0 ? (size_t)total : 1), d_mask1 = A.add<uint8_t>(mask1 ? (size_t)total : 1);
  const auto d_flag = A.add<int>(4);
  OSFM_HIP(A.alloc(ctx));
  OSFM_HIP(A.upload(d_stop, stop.data(), st));
  OSFM_HIP(A.upload(d_stopoff, stop_off.data(), st));
  OSFM_HIP(hipMemsetAsync(d_flag, 0, d_flag.bytes, st));
  const BatchArgs B{d_off, d_stop, d_stopoff, rng, 1.0 - cos(prm->threshold), prm->inlier_chord, (int)prm->iterations, (int)prm->use_lo,
                    (int)prm->lo_iterations, (int)prm->use_iteration_reduction, d_scratch, d_flag};
  if (!timed_from_ev0) OSFM_HIP(hipEventRecord(ctx->ev[0], st));
  launch(B, (void *)d_out.get(), mask0 ? d_mask0.get() : nullptr, mask1 ? d_mask1.get() : nullptr);
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipEventRecord(ctx->ev[1], st));
  int flag = 0;
  OSFM_HIP(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipMemcpyAsync(results, d_out, d_out.bytes, hipMemcpyDeviceToHost, st));
  if (mask0) OSFM_HIP(hipMemcpyAsync(mask0, d_mask0, (size_t)total, hipMemcpyDeviceToHost, st));
  if (mask1) OSFM_HIP(hipMemcpyAsync(mask1, d_mask1, (size_t)total, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  OSFM_REQUIRE(flag == 0, OSFM_E_UNSUPPORTED, "%s: the tabulated mt19937 stream is too short for this input", who);
  return osfm_kernel_ms(ctx, kernel_ms);
}

}  // namespace osfm_lo
