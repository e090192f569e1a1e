// twoview.hip -- bootstrap_reconstruction's two-view 5-point reconstruction for a batch of pairs on gfx950.
//
// reference: reconstruction.two_view_reconstruction_general up to the plane-based branch (opensfm/reconstruction.py:488-534):
//   multiview.relative_pose_ransac (multiview.py:494-516)            -> osfm_relpose_run_device, mode OSFM_RELPOSE_RANSAC (relpose.hip, untouched);
//                                                                     its results stay on the device
//   two_view_reconstruction_and_refinement (reconstruction.py:336-374) -> tv_config_kernel: one wavefront per (pair, configuration)
//   the choice between the configurations (reconstruction.py:458-485)  -> tv_decide_kernel: one thread per pair; record and mask bytes
// The numerics are twoview_core.h, which only recombines leaves of relpose_core.h / relpose_rounds.h.  Pinned: a host build of
// twoview_core.h is held bit for bit to a restatement composed from the CPU oracle's leaves (tests/test_twoview_host.py); the GPU to that
// host build -- statuses, choices, masks and the RANSAC bit for bit, the refined poses to 1e-6 (the device's sin / cos differ from the
// host's in the last bits) (tests/test_gpu_twoview.py).  Not pinned: cv2.Rodrigues' bit patterns (the angle-axis is rotmat_to_aa of the
// matrix the reference hands to it) and numpy's summation order in its 3 x 3 products (written out left to right here).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "osfm_internal.h"
#include "gpu_wave.h"
#include "twoview_core.h"

using namespace osfm_rp;

namespace {

static_assert(sizeof(TwoViewOut) == sizeof(osfm_two_view_result), "TwoViewOut must mirror osfm_two_view_result");

struct TvArgs {
  const double *b1, *b2;          // total x 3
  const int64_t *offsets;         // n_pairs + 1, from 0
  int n_pairs;
  const double *poses;            // n_pairs x 12 (R row-major, t), or null: from rp
  const osfm_relpose_result *rp;  // the RANSAC's results, or null
  double threshold, reversal_ratio;
  int refine_iterations, check_reversal, all_pass;
  int *lists;  // 2 x total: the inlier lists of configuration 0, then those of configuration 1
  TwoViewOut *out;
  uint8_t *mask;
};

// RefineShared in LDS and the registers of the refinement: the shape and budget of rp_finish_kernel (two wavefronts per SIMD)
__global__ __launch_bounds__(kWave, 2) void tv_config_kernel(TvArgs A) {
  __shared__ RefineShared sh;
  __shared__ double pose[12], Rt[12];
  const int p = (int)(blockIdx.x % (unsigned)A.n_pairs), c = (int)(blockIdx.x / (unsigned)A.n_pairs);
  GpuWave w{(int)threadIdx.x};
  const int64_t o = A.offsets[p];
  const int n = (int)(A.offsets[p + 1] - o);
  if (w.lane == 0) {
    if (A.poses)
      for (int i = 0; i < 12; i++) pose[i] = A.poses[12 * (size_t)p + i];
    else
      two_view_pose_from_lo_model(A.rp[p].lo_model, pose, pose + 9);
  }
  __syncthreads();
  int *subset = A.lists + (size_t)c * A.offsets[A.n_pairs] + o;
  int it = 0;
  const int cnt = two_view_config_wave(w, sh, A.b1 + 3 * o, A.b2 + 3 * o, n, pose, pose + 9, c, A.threshold, A.refine_iterations, A.all_pass,
                                       subset, Rt, Rt + 9, &it);
  __syncthreads();
  if (w.lane == 0) {
    TwoViewOut &r = A.out[p];
    for (int i = 0; i < 9; i++) r.R[9 * c + i] = Rt[i];
    for (int i = 0; i < 3; i++) r.t[3 * c + i] = Rt[9 + i];
    r.n_inliers[c] = cnt;
    r.refine_iterations[c] = it;
  }
}

__global__ __launch_bounds__(256) void tv_decide_kernel(TvArgs A) {
  const int p = (int)(blockIdx.x * 256 + threadIdx.x);
  if (p >= A.n_pairs) return;
  TwoViewOut &r = A.out[p];
  for (int i = 0; i < 12; i++) r.lo_model[i] = A.rp ? A.rp[p].lo_model[i] : 0.0;
  r.score = A.rp ? A.rp[p].score : 0;
  r.iterations = A.rp ? A.rp[p].iterations : 0;
  const int64_t o = A.offsets[p], total = A.offsets[A.n_pairs];
  two_view_finish_pair(r, (int)(A.offsets[p + 1] - o), A.check_reversal, A.reversal_ratio, A.lists + o, A.lists + total + o, A.mask + o);
}

struct Cameras {  // the camera table of the pixels call
  const int32_t *pair_cams, *cam_model;
  const double *cam_params;
  int n_cams;
};

int check_args(const osfm_ctx *ctx, const void *rows1, const void *rows2, const int64_t *offsets, int n_pairs, const osfm_two_view_params *prm,
               const osfm_two_view_result *results, const uint8_t *mask, const char *who) {
  OSFM_REQUIRE(ctx && offsets && prm && (n_pairs == 0 || results), OSFM_E_INVALID, "%s: null argument", who);
  OSFM_REQUIRE(n_pairs >= 0, OSFM_E_INVALID, "%s: n_pairs < 0", who);
  OSFM_REQUIRE(prm->lo_iterations <= kLoIterMax, OSFM_E_UNSUPPORTED, "%s: more than %d local optimisation iterations", who, kLoIterMax);
  OSFM_REQUIRE(prm->ransac_iterations >= 0 && prm->lo_iterations >= 0 && prm->refine_iterations >= 0 && prm->threshold > 0 &&
                   prm->probability > 0 && prm->probability < 1 && prm->reversal_ratio == prm->reversal_ratio,
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
// (width 2, with `cams`).  Pairs of five or fewer correspondences never reach the device: only the others are uploaded, as a batch
// of their own, and the results are put back in the caller's order.
int two_view_run(osfm_ctx *ctx, const double *rows1, const double *rows2, int width, const int64_t *offsets, int n_pairs, const Cameras *cams,
                 const double *poses, const osfm_two_view_params *prm, osfm_two_view_result *results, uint8_t *mask, double *kernel_ms) {
  std::vector<int> orig;  // the pairs that run
  for (int p = 0; p < n_pairs; p++)
    if (offsets[p + 1] - offsets[p] > kTwoViewMinInliers) orig.push_back(p);
  const int m = (int)orig.size();
  std::vector<int64_t> off_c;
  std::vector<double> rows1_c, rows2_c, poses_c;
  std::vector<int32_t> pc_c;
  const int64_t *off = offsets;
  if (m < n_pairs) {  // the smaller batch
    off_c.assign(1, 0);
    for (int k = 0; k < m; k++) {
      const int64_t o = offsets[orig[k]], e = offsets[orig[k] + 1];
      rows1_c.insert(rows1_c.end(), rows1 + width * o, rows1 + width * e);
      rows2_c.insert(rows2_c.end(), rows2 + width * o, rows2 + width * e);
      if (poses) poses_c.insert(poses_c.end(), poses + 12 * (size_t)orig[k], poses + 12 * (size_t)orig[k] + 12);
      if (cams) pc_c.insert(pc_c.end(), cams->pair_cams + 2 * (size_t)orig[k], cams->pair_cams + 2 * (size_t)orig[k] + 2);
      off_c.push_back(off_c.back() + (e - o));
    }
    off = off_c.data();
    rows1 = rows1_c.data();
    rows2 = rows2_c.data();
    if (poses) poses = poses_c.data();
    osfm_two_view_result none;
    memset(&none, 0, sizeof none);
    none.status = OSFM_TWO_VIEW_NO_CONFIGURATION;
    none.chosen = none.n_inliers[0] = none.n_inliers[1] = -1;
    for (int p = 0; p < n_pairs; p++)
      if (offsets[p + 1] - offsets[p] <= kTwoViewMinInliers) {
        results[p] = none;
        if (offsets[p + 1] > offsets[p]) memset(mask + offsets[p], 0, (size_t)(offsets[p + 1] - offsets[p]));
      }
  }
  if (m == 0) return OSFM_OK;
  const int32_t *pair_cams = cams ? (m < n_pairs ? pc_c.data() : cams->pair_cams) : nullptr;
  const int64_t total = off[m];
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
  const auto d_poses = A.add<double>(poses ? (size_t)m * 12 : 0);
  const auto d_rp = A.add<osfm_relpose_result>(poses ? 0 : (size_t)m);
  const auto d_rmask = A.add<uint8_t>(poses ? 0 : (size_t)total);  // the RANSAC's own inlier mask: not part of the result
  const auto d_lists = A.add<int>((size_t)total * 2);
  const auto d_out = A.add<TwoViewOut>((size_t)m);  // d_out and d_mask lie one after the other: one copy brings both back
  const auto d_mask = A.add<uint8_t>((size_t)total);
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
  if (poses) OSFM_HIP(A.upload(d_poses, poses, st));
  OSFM_HIP(hipEventRecord(ctx->ev[0], st));
  if (cams) {  // the kernel time includes the bearings
    osfm_launch_pair_bearings(st, m, d_p1, d_p2, d_off, d_pc, d_cm, d_cp, d_b1, d_b2);
    OSFM_HIP(hipGetLastError());
  }
  if (!poses) {
    const osfm_relpose_params rp{prm->threshold, prm->probability, prm->ransac_iterations, prm->use_lo, prm->lo_iterations, 0};
    constexpr int kBatch = 65536;  // bounds the work space of the rounds, as in osfm_relpose_pairs
    for (int p0 = 0; p0 < m; p0 += kBatch)
      OSFM_TRY(osfm_relpose_run_device(ctx, st, d_b1, d_b2, d_off.get() + p0, off + p0, std::min(kBatch, m - p0), &rp, OSFM_RELPOSE_RANSAC, d_rmask,
                                       d_rp.get() + p0, nullptr));
  }
  const int n_cfg = prm->check_reversal ? 2 : 1;
  const TvArgs T{d_b1, d_b2, d_off, m, poses ? d_poses.get() : nullptr, poses ? nullptr : d_rp.get(), prm->threshold, prm->reversal_ratio,
                 (int)prm->refine_iterations, prm->check_reversal ? 1 : 0, prm->skip_inlier_tests ? 1 : 0, d_lists, d_out, d_mask};
  hipLaunchKernelGGL(tv_config_kernel, dim3((unsigned)(n_cfg * (int64_t)m)), dim3(kWave), 0, st, T);
  hipLaunchKernelGGL(tv_decide_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, T);
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipEventRecord(ctx->ev[1], st));
  const size_t out_bytes = d_mask.offset - d_out.offset + (size_t)total;
  std::vector<uint8_t> back(out_bytes);
  OSFM_HIP(hipMemcpyAsync(back.data(), d_out.get(), out_bytes, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  const uint8_t *mask_back = back.data() + (d_mask.offset - d_out.offset);
  for (int k = 0; k < m; k++) {
    memcpy(&results[orig[k]], back.data() + (size_t)k * sizeof(TwoViewOut), sizeof(TwoViewOut));
    memcpy(mask + offsets[orig[k]], mask_back + off[k], (size_t)(off[k + 1] - off[k]));
  }
  return osfm_kernel_ms(ctx, kernel_ms);
}

}  // namespace

extern "C" int osfm_two_view_pairs(osfm_ctx *ctx, const double *b1, const double *b2, const int64_t *offsets, int n_pairs, const double *poses,
                                   const osfm_two_view_params *prm, osfm_two_view_result *results, uint8_t *mask, double *kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_TRY(check_args(ctx, b1, b2, offsets, n_pairs, prm, results, mask, "osfm_two_view_pairs"));
  if (n_pairs == 0) return OSFM_OK;
  return two_view_run(ctx, b1, b2, 3, offsets, n_pairs, nullptr, poses, prm, results, mask, kernel_ms);
}

extern "C" int osfm_two_view_pairs_pixels(osfm_ctx *ctx, const double *p1, const double *p2, const int64_t *offsets, int n_pairs,
                                          const int32_t *pair_cams, const int32_t *cam_model, const double *cam_params, int n_cams,
                                          const double *poses, const osfm_two_view_params *prm, osfm_two_view_result *results, uint8_t *mask,
                                          double *kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_TRY(check_args(ctx, p1, p2, offsets, n_pairs, prm, results, mask, "osfm_two_view_pairs_pixels"));
  if (n_pairs == 0) return OSFM_OK;
  OSFM_REQUIRE(pair_cams && cam_model && cam_params && n_cams > 0, OSFM_E_INVALID, "osfm_two_view_pairs_pixels: null camera table");
  OSFM_TRY(osfm_check_camera_table(cam_model, n_cams, pair_cams, n_pairs, 2, "pair", "osfm_two_view_pairs_pixels"));
  const Cameras cams{pair_cams, cam_model, cam_params, n_cams};
  return two_view_run(ctx, p1, p2, 2, offsets, n_pairs, &cams, poses, prm, results, mask, kernel_ms);
}
