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
  const size_t sizes[] = {stop.size() * 8, stop_off.size() * 8, any_large ? (size_t)total * 4 : 4, (size_t)n_problems * result_bytes,
                          mask0 ? (size_t)total : 1, mask1 ? (size_t)total : 1, 16};
  constexpr int kBuffers = sizeof(sizes) / sizeof(sizes[0]);
  size_t offs[kBuffers], arena_bytes = 0;
  for (int i = 0; i < kBuffers; i++) {
    offs[i] = arena_bytes;
    arena_bytes += (sizes[i] + 255) / 256 * 256;
  }
  OsfmPoolBuf arena;
  OSFM_HIP(arena.alloc(ctx, arena_bytes));
  char *base = (char *)arena.p;
  double *d_stop = (double *)(base + offs[0]);
  int64_t *d_stopoff = (int64_t *)(base + offs[1]);
  int *d_scratch = (int *)(base + offs[2]);
  void *d_out = base + offs[3];
  uint8_t *d_mask0 = mask0 ? (uint8_t *)(base + offs[4]) : nullptr;
  uint8_t *d_mask1 = mask1 ? (uint8_t *)(base + offs[5]) : nullptr;
  int *d_flag = (int *)(base + offs[6]);
  OSFM_HIP(hipMemcpyAsync(d_stop, stop.data(), stop.size() * 8, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_stopoff, stop_off.data(), stop_off.size() * 8, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemsetAsync(d_flag, 0, 16, st));
  const BatchArgs A{d_off, d_stop, d_stopoff, rng, 1.0 - cos(prm->threshold), prm->inlier_chord, (int)prm->iterations, (int)prm->use_lo,
                    (int)prm->lo_iterations, (int)prm->use_iteration_reduction, d_scratch, d_flag};
  if (!timed_from_ev0) OSFM_HIP(hipEventRecord(ctx->ev[0], st));
  launch(A, d_out, d_mask0, d_mask1);
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipEventRecord(ctx->ev[1], st));
  int flag = 0;
  OSFM_HIP(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipMemcpyAsync(results, d_out, (size_t)n_problems * result_bytes, hipMemcpyDeviceToHost, st));
  if (mask0) OSFM_HIP(hipMemcpyAsync(mask0, d_mask0, (size_t)total, hipMemcpyDeviceToHost, st));
  if (mask1) OSFM_HIP(hipMemcpyAsync(mask1, d_mask1, (size_t)total, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  OSFM_REQUIRE(flag == 0, OSFM_E_UNSUPPORTED, "%s: the tabulated mt19937 stream is too short for this input", who);
  if (kernel_ms) {
    float ms = 0.f;
    OSFM_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    *kernel_ms = ms;
  }
  return OSFM_OK;
}

}  // namespace osfm_lo
