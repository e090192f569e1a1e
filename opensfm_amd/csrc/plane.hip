// plane.hip -- the plane-based half of bootstrap_reconstruction's two-view step for a batch of pairs on gfx950.
//
// reference: reconstruction.two_view_reconstruction_plane_based (opensfm/reconstruction.py:298-333).  The numerics and what they do and do
// not restate are plane_core.h (host + device), the per-pair walk is loransac_walk.h, the batch driver lo_batch.h; this file adds the
// kernels and the C ABI.
//   pl_ransac_kernel   one wavefront per pair: normalised coordinates, the LO-RANSAC walk over 4-point DLTs (one 9 x 9 eigen-solve per
//                      lane), the final fit over all inliers, H with its scale fixed, its eight motions; mask bit 0
//   pl_motion_kernel   one wavefront per (pair, motion): the rows the motion explains (ballot + popcount; a byte per row, no atomics)
//   pl_decide_kernel   one thread per pair: the motion with the most inliers, the record, mask bit 1
// Pinned: a host build of plane_core.h against a numpy restatement (tests/test_plane_host.py), the GPU against that host build bit for
// bit (tests/test_gpu_plane.py).
#include <math.h>
#include <string.h>

#include <vector>

#include "lo_batch.h"
#include "plane_core.h"

using namespace osfm_pl;
using osfm_rp::kWave;

namespace {

static_assert(sizeof(PlaneOut) == sizeof(osfm_plane_result), "PlaneOut must mirror osfm_plane_result");
static_assert(sizeof(PlaneShared) <= 64 * 1024, "PlaneShared must fit the LDS of a workgroup");
static_assert(kWave == 64, "the butterfly of PlaneWave::sum_rows is written for 64 lanes");

// GpuWave with the fixed-order sum of the final fit: lane l takes items l, l + 64, ... from 0.0, then the lanes are combined by a
// butterfly over xor 32, 16, ..., 1 (a + b and b + a are the same bits, so every lane ends with the same sums).  out: LDS.
struct PlaneWave : osfm_rp::GpuWave {
  template <int K, class F>
  __device__ void sum_rows(int n, F f, double *out) {
    double acc[K];
    OSFM_UNROLL for (int k = 0; k < K; k++) acc[k] = 0.0;
    for (int i = lane; i < n; i += kWave) f(i, acc);
    OSFM_UNROLL for (int m = kWave / 2; m >= 1; m >>= 1)
      OSFM_UNROLL for (int k = 0; k < K; k++) acc[k] = acc[k] + __shfl_xor(acc[k], m, kWave);
    __syncthreads();
    if (lane == 0)
      OSFM_UNROLL for (int k = 0; k < K; k++) out[k] = acc[k];
    __syncthreads();
  }
};

__global__ __launch_bounds__(kWave) void pl_ransac_kernel(PlaneArgs A, int n_pairs) {
  const int p = (int)blockIdx.x;
  if (p >= n_pairs) return;
  __shared__ PlaneShared sh;
  PlaneWave w{{(int)threadIdx.x}};
  plane_ransac_pair(w, sh, A, p);
}

__global__ __launch_bounds__(kWave) void pl_motion_kernel(PlaneArgs A, int n_pairs, int64_t total) {
  const int p = (int)(blockIdx.x % (unsigned)n_pairs), k = (int)(blockIdx.x / (unsigned)n_pairs);
  if (k >= kMotions) return;
  PlaneWave w{{(int)threadIdx.x}};
  plane_motion_pair(w, A, p, k, total);
}

__global__ __launch_bounds__(256) void pl_decide_kernel(PlaneArgs A, int n_pairs, int64_t total) {
  const int p = (int)(blockIdx.x * 256 + threadIdx.x);
  if (p >= n_pairs) return;
  plane_decide_pair(A, p, total);
}

// the leaves, one lane each: the DLT over n rows; the decomposition of a given H
__global__ __launch_bounds__(kWave) void pl_dlt_kernel(const double *x1, const double *x2, int n, double *H, int *ok) {
  if (threadIdx.x != 0) return;
  double h[9];
  const int c = homography_dlt(x1, x2, nullptr, n, h);
  for (int i = 0; i < 9; i++) H[i] = c ? h[i] : 0.0;
  *ok = c;
}
__global__ __launch_bounds__(kWave) void pl_motions_kernel(const double *H, double *motions, int *count) {
  if (threadIdx.x != 0) return;
  double h[9], m[kMotions * kMotionSize], s[3];
  for (int i = 0; i < 9; i++) h[i] = H[i];
  const int c = plane_motions(h, m, s);
  for (int i = 0; i < kMotions * kMotionSize; i++) motions[i] = c ? m[i] : 0.0;
  *count = c;
}

struct Cameras {  // the camera table of the pixels call
  const int32_t *pair_cams, *cam_model;
  const double *cam_params;
  int n_cams;
};

int check_args(const osfm_ctx *ctx, const void *rows1, const void *rows2, const int64_t *offsets, int n_pairs, const osfm_plane_params *prm,
               const osfm_plane_result *results, const uint8_t *mask, const char *who) {
  OSFM_REQUIRE(ctx && offsets && prm && (n_pairs == 0 || results), OSFM_E_INVALID, "%s: null argument", who);
  OSFM_REQUIRE(n_pairs >= 0, OSFM_E_INVALID, "%s: n_pairs < 0", who);
  OSFM_REQUIRE(prm->iterations >= 0 && prm->lo_iterations >= 0 && prm->threshold > 0 && prm->probability > 0 && prm->probability < 1,
               OSFM_E_INVALID, "%s: bad parameters", who);
  if (n_pairs == 0) return OSFM_OK;
  OSFM_REQUIRE(offsets[0] == 0, OSFM_E_INVALID, "%s: offsets[0] must be 0", who);
  for (int p = 0; p < n_pairs; p++)
    OSFM_REQUIRE(offsets[p + 1] >= offsets[p] && offsets[p + 1] - offsets[p] <= (1 << 24), OSFM_E_INVALID, "%s: offsets must ascend (pair %d)", who,
                 p);
  OSFM_REQUIRE(offsets[n_pairs] == 0 || (rows1 && rows2 && mask), OSFM_E_INVALID, "%s: null correspondences / mask", who);
  return OSFM_OK;
}

// The batch after the argument checks.  rows1 / rows2: total x width doubles, bearings (width 3) or normalised image coordinates
// (width 2, with `cams`).  Pairs of fewer than four correspondences never reach the device: only the others are uploaded, as a batch
// of their own, and the results are put back in the caller's order (the arrangement of two_view_run, twoview.hip).
int plane_run(osfm_ctx *ctx, const double *rows1, const double *rows2, int width, const int64_t *offsets, int n_pairs, const Cameras *cams,
              const osfm_plane_params *prm, osfm_plane_result *results, uint8_t *mask, double *kernel_ms, const char *who) {
  std::vector<int> orig;  // the pairs that run
  for (int p = 0; p < n_pairs; p++)
    if (offsets[p + 1] - offsets[p] >= kMinimalSamples) orig.push_back(p);
  const int m = (int)orig.size();
  std::vector<int64_t> off_c;
  std::vector<double> rows1_c, rows2_c;
  std::vector<int32_t> pc_c;
  const int64_t *off = offsets;
  if (m < n_pairs) {  // the smaller batch
    off_c.assign(1, 0);
    for (int k = 0; k < m; k++) {
      const int64_t o = offsets[orig[k]], e = offsets[orig[k] + 1];
      rows1_c.insert(rows1_c.end(), rows1 + width * o, rows1 + width * e);
      rows2_c.insert(rows2_c.end(), rows2 + width * o, rows2 + width * e);
      if (cams) pc_c.insert(pc_c.end(), cams->pair_cams + 2 * (size_t)orig[k], cams->pair_cams + 2 * (size_t)orig[k] + 2);
      off_c.push_back(off_c.back() + (e - o));
    }
    off = off_c.data();
    rows1 = rows1_c.data();
    rows2 = rows2_c.data();
  }
  osfm_plane_result none;
  memset(&none, 0, sizeof none);
  none.status = OSFM_PLANE_NO_HOMOGRAPHY;
  none.chosen = -1;
  std::vector<osfm_plane_result> res_c((size_t)m);
  std::vector<uint8_t> mask_c;
  if (m > 0) {
    const int32_t *pair_cams = cams ? (m < n_pairs ? pc_c.data() : cams->pair_cams) : nullptr;
    const int64_t total = off[m];
    mask_c.resize((size_t)total);
    OSFM_CTX_LOCK(ctx);
    OSFM_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    OsfmArena A;
    const auto d_b1 = A.add<double>((size_t)total * 3);
    const auto d_b2 = A.add<double>((size_t)total * 3);
    const auto d_p1 = A.add<double>(cams ? (size_t)total * 2 : 0);
    const auto d_p2 = A.add<double>(cams ? (size_t)total * 2 : 0);
    const auto d_pc = A.add<int32_t>(cams ? (size_t)m * 2 : 0);
    const auto d_cm = A.add<int32_t>(cams ? (size_t)cams->n_cams : 0);
    const auto d_cp = A.add<double>(cams ? (size_t)cams->n_cams * 16 : 0);
    const auto d_off = A.add<int64_t>((size_t)m + 1);
    const auto d_x1 = A.add<double>((size_t)total * 2);
    const auto d_x2 = A.add<double>((size_t)total * 2);
    const auto d_motions = A.add<double>((size_t)m * kMotions * kMotionSize);
    const auto d_flags = A.add<uint8_t>((size_t)total * kMotions);
    OSFM_HIP(A.alloc(ctx));
    if (cams) {
      OSFM_HIP(A.upload(d_p1, rows1, st));
      OSFM_HIP(A.upload(d_p2, rows2, st));
      OSFM_HIP(A.upload(d_pc, pair_cams, st));
      OSFM_HIP(A.upload(d_cm, cams->cam_model, st));
      OSFM_HIP(A.upload(d_cp, cams->cam_params, st));
    } else {
      OSFM_HIP(A.upload(d_b1, rows1, st));
      OSFM_HIP(A.upload(d_b2, rows2, st));
    }
    OSFM_HIP(A.upload(d_off, off, st));
    if (cams) {  // the kernel time includes the bearings
      OSFM_HIP(hipEventRecord(ctx->ev[0], st));
      osfm_launch_pair_bearings(st, m, d_p1, d_p2, d_off, d_pc, d_cm, d_cp, d_b1, d_b2);
      OSFM_HIP(hipGetLastError());
    }
    // run_batch reads the fields of osfm_relrot_params; the chord is not used here
    const osfm_relrot_params walk_prm{prm->threshold, prm->probability, 0.0, prm->iterations, prm->use_lo, prm->lo_iterations,
                                      prm->use_iteration_reduction};
    const double threshold = prm->threshold;
    auto launch = [&](const osfm_lo::BatchArgs &B, void *d_out, uint8_t *d_mask, uint8_t *) {
      const PlaneArgs P{d_b1, d_b2, B.offsets, B.stop_bound, B.stop_off, B.rng, threshold, B.iterations, B.use_lo, B.lo_iterations, B.use_reduction,
                        B.scratch, d_x1, d_x2, d_motions, d_flags, (PlaneOut *)d_out, d_mask, B.overflow};
      hipLaunchKernelGGL(pl_ransac_kernel, dim3((unsigned)m), dim3(kWave), 0, st, P, m);
      hipLaunchKernelGGL(pl_motion_kernel, dim3((unsigned)(kMotions * (int64_t)m)), dim3(kWave), 0, st, P, m, total);
      hipLaunchKernelGGL(pl_decide_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, P, m, total);
    };
    OSFM_TRY(osfm_lo::run_batch(ctx, st, d_off, off, m, &walk_prm, kMinimalSamples, res_c.data(), sizeof(PlaneOut), mask_c.data(), nullptr,
                                cams != nullptr, kernel_ms, who, launch));
  }
  // nothing of the caller's is written before this point: a call that fails touches no output
  for (int p = 0; p < n_pairs; p++)
    if (offsets[p + 1] - offsets[p] < kMinimalSamples) {
      results[p] = none;
      if (offsets[p + 1] > offsets[p]) memset(mask + offsets[p], 0, (size_t)(offsets[p + 1] - offsets[p]));
    }
  for (int k = 0; k < m; k++) {
    results[orig[k]] = res_c[(size_t)k];
    memcpy(mask + offsets[orig[k]], mask_c.data() + off[k], (size_t)(off[k + 1] - off[k]));
  }
  return OSFM_OK;
}

}  // namespace

extern "C" int osfm_two_view_plane_pairs(osfm_ctx *ctx, const double *b1, const double *b2, const int64_t *offsets, int n_pairs,
                                         const osfm_plane_params *prm, osfm_plane_result *results, uint8_t *mask, double *kernel_ms) {
  const char *who = "osfm_two_view_plane_pairs";
  OSFM_TRY(check_args(ctx, b1, b2, offsets, n_pairs, prm, results, mask, who));
  if (n_pairs == 0) return OSFM_OK;
  double ms = 0.0;
  OSFM_TRY(plane_run(ctx, b1, b2, 3, offsets, n_pairs, nullptr, prm, results, mask, &ms, who));
  if (kernel_ms) *kernel_ms = ms;
  return OSFM_OK;
}

extern "C" int osfm_two_view_plane_pairs_pixels(osfm_ctx *ctx, const double *p1, const double *p2, const int64_t *offsets, int n_pairs,
                                                const int32_t *pair_cams, const int32_t *cam_model, const double *cam_params, int n_cams,
                                                const osfm_plane_params *prm, osfm_plane_result *results, uint8_t *mask, double *kernel_ms) {
  const char *who = "osfm_two_view_plane_pairs_pixels";
  OSFM_TRY(check_args(ctx, p1, p2, offsets, n_pairs, prm, results, mask, who));
  if (n_pairs == 0) return OSFM_OK;
  OSFM_REQUIRE(pair_cams && cam_model && cam_params && n_cams > 0, OSFM_E_INVALID, "%s: null camera table", who);
  OSFM_TRY(osfm_check_camera_table(cam_model, n_cams, pair_cams, n_pairs, 2, "pair", who));
  const Cameras cams{pair_cams, cam_model, cam_params, n_cams};
  double ms = 0.0;
  OSFM_TRY(plane_run(ctx, p1, p2, 2, offsets, n_pairs, &cams, prm, results, mask, &ms, who));
  if (kernel_ms) *kernel_ms = ms;
  return OSFM_OK;
}

extern "C" int osfm_homography_solve(osfm_ctx *ctx, const double *x1, const double *x2, int n, double *H_out, int *ok_out) {
  const char *who = "osfm_homography_solve";
  OSFM_REQUIRE(ctx && x1 && x2 && H_out && ok_out, OSFM_E_INVALID, "%s: null argument", who);
  OSFM_REQUIRE(n >= kMinimalSamples && n <= (1 << 24), OSFM_E_INVALID, "%s: %d rows (at least 4 are needed)", who, n);
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmArena A;
  const auto d_x1 = A.add<double>((size_t)n * 2);
  const auto d_x2 = A.add<double>((size_t)n * 2);
  const auto d_H = A.add<double>(9);
  const auto d_ok = A.add<int>(2);
  OSFM_HIP(A.alloc(ctx));
  OSFM_HIP(A.upload(d_x1, x1, st));
  OSFM_HIP(A.upload(d_x2, x2, st));
  hipLaunchKernelGGL(pl_dlt_kernel, dim3(1), dim3(kWave), 0, st, d_x1, d_x2, n, d_H, d_ok);
  OSFM_HIP(hipGetLastError());
  double H[9];
  int ok = 0;
  OSFM_HIP(hipMemcpyAsync(H, d_H, sizeof H, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipMemcpyAsync(&ok, d_ok, 4, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  memcpy(H_out, H, sizeof H);
  *ok_out = ok;
  return OSFM_OK;
}

extern "C" int osfm_plane_motions(osfm_ctx *ctx, const double *H, double *motions_out, int *count_out) {
  const char *who = "osfm_plane_motions";
  OSFM_REQUIRE(ctx && H && motions_out && count_out, OSFM_E_INVALID, "%s: null argument", who);
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmArena A;
  const auto d_H = A.add<double>(9);
  const auto d_m = A.add<double>(kMotions * kMotionSize);
  const auto d_c = A.add<int>(2);
  OSFM_HIP(A.alloc(ctx));
  OSFM_HIP(A.upload(d_H, H, st));
  hipLaunchKernelGGL(pl_motions_kernel, dim3(1), dim3(kWave), 0, st, d_H, d_m, d_c);
  OSFM_HIP(hipGetLastError());
  double m[kMotions * kMotionSize];
  int c = 0;
  OSFM_HIP(hipMemcpyAsync(m, d_m, sizeof m, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipMemcpyAsync(&c, d_c, 4, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  memcpy(motions_out, m, sizeof m);
  *count_out = c;
  return OSFM_OK;
}
