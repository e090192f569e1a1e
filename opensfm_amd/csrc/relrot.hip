// relrot.hip -- rotation-only LO-RANSAC for a batch of image pairs on gfx950: the ranking of reconstruction.compute_image_pairs.
//
// The numerics and the per-pair walk live in relrot_core.h, the sampler on the tabulated stream in loransac_walk.h (both host + device),
// the GPU wave policy in gpu_wave.h and the batch driver in lo_batch.h; this file adds the kernels and the C ABI.  One wavefront per pair: lane 0 draws the samples of the next block of iterations, every lane solves one 3-point model,
// all lanes score each model over the pair's correspondences (ballot + popcount, inlier list compacted in order), and the same
// launch ends with the rotation-only inlier count and the reconstructability score.
#include <math.h>

#include "lo_batch.h"
#include "relrot_core.h"

using namespace osfm_rr;
using osfm_rp::GpuWave;
using osfm_rp::kWave;

namespace {

static_assert(sizeof(RelrotOut) == sizeof(osfm_relrot_result), "RelrotOut must mirror osfm_relrot_result");

__global__ __launch_bounds__(kWave) void rr_pairs_kernel(RelrotArgs A, int n_pairs) {
  const int p = (int)blockIdx.x;
  if (p >= n_pairs) return;
  __shared__ RelrotShared sh;
  GpuWave w{(int)threadIdx.x};
  relrot_pair(w, sh, A, p);
}

// bearings of both sides of every pair from normalised image coordinates: one workgroup per pair, the pair's two cameras from the
// camera table (osfm_rp::pixel_bearing_generic, the code of osfm_pixel_bearings)
__global__ __launch_bounds__(256) void rr_bearings_kernel(const double *__restrict__ p1, const double *__restrict__ p2, const int64_t *offsets,
                                                          const int32_t *pair_cams, const int32_t *cam_model, const double *cam_params,
                                                          double *b1, double *b2) {
  const int p = (int)blockIdx.x;
  const int64_t o = offsets[p], e = offsets[p + 1];
  const int c1 = pair_cams[2 * p], c2 = pair_cams[2 * p + 1];
  const int m1 = cam_model[c1], m2 = cam_model[c2];
  const double *par1 = cam_params + 16 * (size_t)c1, *par2 = cam_params + 16 * (size_t)c2;
  for (int64_t i = o + threadIdx.x; i < e; i += blockDim.x) {
    osfm_rp::pixel_bearing_generic(m1, par1, p1[2 * i], p1[2 * i + 1], b1 + 3 * i);
    osfm_rp::pixel_bearing_generic(m2, par2, p2[2 * i], p2[2 * i + 1], b2 + 3 * i);
  }
}

int check_args(const int64_t *offsets, int n_pairs, const osfm_relrot_params *prm, const char *who) {
  return osfm_lo::check_batch_args(offsets, n_pairs, prm, kMinimalSamples, {"pair", "correspondences"}, who);
}

// The batch on device-resident bearings; results and mask copied to the host.  The caller holds the context lock.
int run_device(osfm_ctx *ctx, hipStream_t st, const double *d_b1, const double *d_b2, const int64_t *d_off, const int64_t *offsets, int n_pairs,
               const osfm_relrot_params *prm, osfm_relrot_result *results, uint8_t *mask, bool timed_from_ev0, double *kernel_ms) {
  auto launch = [&](const osfm_lo::BatchArgs &B, void *d_out, uint8_t *d_mask, uint8_t *) {
    const RelrotArgs A{d_b1, d_b2, B.offsets, B.stop_bound, B.stop_off, B.rng, B.thr, B.chord, B.iterations, B.use_lo, B.lo_iterations,
                       B.use_reduction, B.scratch, (RelrotOut *)d_out, d_mask, B.overflow};
    hipLaunchKernelGGL(rr_pairs_kernel, dim3((unsigned)n_pairs), dim3(kWave), 0, st, A, n_pairs);
  };
  return osfm_lo::run_batch(ctx, st, d_off, offsets, n_pairs, prm, kMinimalSamples, results, sizeof(RelrotOut), mask, nullptr,
                            timed_from_ev0, kernel_ms, "osfm_relrot_pairs", launch);
}

}  // namespace

// rr_bearings_kernel for the pair drivers (this file's, twoview.hip's): everything device-resident, enqueued on st
void osfm_launch_pair_bearings(hipStream_t st, int n_pairs, const double *d_p1, const double *d_p2, const int64_t *d_off, const int32_t *d_pair_cams,
                               const int32_t *d_cam_model, const double *d_cam_params, double *d_b1, double *d_b2) {
  hipLaunchKernelGGL(rr_bearings_kernel, dim3((unsigned)n_pairs), dim3(256), 0, st, d_p1, d_p2, d_off, d_pair_cams, d_cam_model, d_cam_params, d_b1,
                     d_b2);
}

extern "C" int osfm_relrot_pairs(osfm_ctx *ctx, const double *b1, const double *b2, const int64_t *offsets, int n_pairs,
                                 const osfm_relrot_params *prm, osfm_relrot_result *results, uint8_t *mask, double *kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_REQUIRE(ctx, OSFM_E_INVALID, "osfm_relrot_pairs: null context");
  OSFM_TRY(check_args(offsets, n_pairs, prm, "osfm_relrot_pairs"));
  if (n_pairs == 0) return OSFM_OK;
  OSFM_REQUIRE(b1 && b2 && results, OSFM_E_INVALID, "osfm_relrot_pairs: null bearings / results");
  const int64_t total = offsets[n_pairs];
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmDevBuf d_b1, d_b2, d_off;
  OSFM_HIP(d_b1.alloc((size_t)total * 24));
  OSFM_HIP(d_b2.alloc((size_t)total * 24));
  OSFM_HIP(d_off.alloc((size_t)(n_pairs + 1) * 8));
  OSFM_HIP(hipMemcpyAsync(d_b1.p, b1, (size_t)total * 24, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_b2.p, b2, (size_t)total * 24, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_off.p, offsets, (size_t)(n_pairs + 1) * 8, hipMemcpyHostToDevice, st));
  return run_device(ctx, st, d_b1.as<double>(), d_b2.as<double>(), d_off.as<int64_t>(), offsets, n_pairs, prm, results, mask, false, kernel_ms);
}

extern "C" int osfm_relrot_pairs_pixels(osfm_ctx *ctx, const double *p1, const double *p2, const int64_t *offsets, int n_pairs,
                                        const int32_t *pair_cams, const int32_t *cam_model, const double *cam_params, int n_cams,
                                        const osfm_relrot_params *prm, osfm_relrot_result *results, uint8_t *mask, double *kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_REQUIRE(ctx, OSFM_E_INVALID, "osfm_relrot_pairs_pixels: null context");
  OSFM_TRY(check_args(offsets, n_pairs, prm, "osfm_relrot_pairs_pixels"));
  if (n_pairs == 0) return OSFM_OK;
  OSFM_REQUIRE(p1 && p2 && results && pair_cams && cam_model && cam_params && n_cams > 0, OSFM_E_INVALID,
               "osfm_relrot_pairs_pixels: null argument");
  OSFM_TRY(osfm_check_camera_table(cam_model, n_cams, pair_cams, n_pairs, 2, "pair", "osfm_relrot_pairs_pixels"));
  const int64_t total = offsets[n_pairs];
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmDevBuf d_p1, d_p2, d_b1, d_b2, d_off, d_pc, d_cm, d_cp;
  OSFM_HIP(d_p1.alloc((size_t)total * 16));
  OSFM_HIP(d_p2.alloc((size_t)total * 16));
  OSFM_HIP(d_b1.alloc((size_t)total * 24));
  OSFM_HIP(d_b2.alloc((size_t)total * 24));
  OSFM_HIP(d_off.alloc((size_t)(n_pairs + 1) * 8));
  OSFM_HIP(d_pc.alloc((size_t)n_pairs * 8));
  OSFM_HIP(d_cm.alloc((size_t)n_cams * 4));
  OSFM_HIP(d_cp.alloc((size_t)n_cams * 16 * 8));
  OSFM_HIP(hipMemcpyAsync(d_p1.p, p1, (size_t)total * 16, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_p2.p, p2, (size_t)total * 16, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_off.p, offsets, (size_t)(n_pairs + 1) * 8, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_pc.p, pair_cams, (size_t)n_pairs * 8, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_cm.p, cam_model, (size_t)n_cams * 4, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_cp.p, cam_params, (size_t)n_cams * 16 * 8, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipEventRecord(ctx->ev[0], st));  // the kernel time includes the bearings
  osfm_launch_pair_bearings(st, n_pairs, d_p1.as<double>(), d_p2.as<double>(), d_off.as<int64_t>(), d_pc.as<int32_t>(), d_cm.as<int32_t>(),
                            d_cp.as<double>(), d_b1.as<double>(), d_b2.as<double>());
  OSFM_HIP(hipGetLastError());
  return run_device(ctx, st, d_b1.as<double>(), d_b2.as<double>(), d_off.as<int64_t>(), offsets, n_pairs, prm, results, mask, true, kernel_ms);
}
