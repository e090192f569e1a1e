// abspose.hip -- absolute-pose (P3P) LO-RANSAC for a batch of candidate images on gfx950: the estimator of reconstruction.resect.
//
// The numerics live in abspose_core.h, the per-image walk in loransac_walk.h (both host + device), the GPU wave policy in gpu_wave.h
// and the batch driver in lo_batch.h; this file adds the kernels and the C ABI.  One wavefront per image: lane 0 draws the samples of the next block of iterations, four lanes share a
// sample (one root of its quartic each), all lanes score each model over the image's rows (ballot + popcount, inlier list compacted
// in order); a local optimisation's Lu-Hager solves run one per lane; the same launch ends with resect's inlier test on chords.
#include <math.h>

#include "abspose_core.h"
#include "lo_batch.h"

using namespace osfm_ap;
using osfm_rp::GpuWave;
using osfm_rp::kWave;

namespace {

static_assert(sizeof(AbsposeOut) == sizeof(osfm_abspose_result), "AbsposeOut must mirror osfm_abspose_result");
static_assert(sizeof(AbsposeShared) <= 64 * 1024, "AbsposeShared must fit the LDS of a workgroup");

__global__ __launch_bounds__(kWave) void ap_images_kernel(AbsposeArgs A, int n_images) {
  const int p = (int)blockIdx.x;
  if (p >= n_images) return;
  __shared__ AbsposeShared sh;
  GpuWave w{(int)threadIdx.x};
  abspose_image(w, sh, A, p);
}

// bearings of every row from normalised image coordinates: one workgroup per image, the image's camera from the camera table
// (osfm_rp::pixel_bearing_generic, the code of osfm_pixel_bearings)
__global__ __launch_bounds__(256) void ap_bearings_kernel(const double *__restrict__ xy, const int64_t *offsets, const int32_t *image_cam,
                                                          const int32_t *cam_model, const double *cam_params, double *b) {
  const int p = (int)blockIdx.x;
  const int64_t o = offsets[p], e = offsets[p + 1];
  const int c = image_cam[p];
  const int m = cam_model[c];
  const double *par = cam_params + 16 * (size_t)c;
  for (int64_t i = o + threadIdx.x; i < e; i += blockDim.x) osfm_rp::pixel_bearing_generic(m, par, xy[2 * i], xy[2 * i + 1], b + 3 * i);
}

// the leaf solvers on n rows: kind 0 = AbsolutePoseThreePoints on rows 0 .. 2 (one root per lane), kind 1 = AbsolutePoseNPoints
__global__ __launch_bounds__(kWave) void ap_solve_kernel(const double *b, const double *X, int n, int kind, double *models, int *count) {
  const int lane = (int)threadIdx.x;
  if (kind == 0) {
    if (lane < kMaxModels) {
      const int idx[3] = {0, 1, 2};
      double m[12];
      const int c = p3p_model_of_root(b, X, idx, lane, m);
      for (int i = 0; i < 12; i++) models[12 * lane + i] = c ? m[i] : 0.0;
      if (lane == 0) *count = c;
    }
  } else if (lane == 0) {
    double m[12];
    npoints_model(b, X, nullptr, n, m);
    for (int i = 0; i < 12; i++) models[i] = m[i];
    *count = 1;
  }
}

int check_args(const int64_t *offsets, int n_images, const osfm_abspose_params *prm, const char *who) {
  return osfm_lo::check_batch_args(offsets, n_images, prm, kMinimalSamples, {"image", "rows"}, who);
}

// The batch on device-resident bearings and points; results and masks copied to the host.  The caller holds the context lock.
int run_device(osfm_ctx *ctx, hipStream_t st, const double *d_b, const double *d_X, const int64_t *d_off, const int64_t *offsets, int n_images,
               const osfm_abspose_params *prm, osfm_abspose_result *results, uint8_t *ransac_mask, uint8_t *chord_mask, bool timed_from_ev0,
               double *kernel_ms, const char *who) {
  auto launch = [&](const osfm_lo::BatchArgs &B, void *d_out, uint8_t *d_rmask, uint8_t *d_cmask) {
    const AbsposeArgs A{d_b, d_X, B.offsets, B.stop_bound, B.stop_off, B.rng, B.thr, B.chord, B.iterations, B.use_lo, B.lo_iterations,
                        B.use_reduction, B.scratch, (AbsposeOut *)d_out, d_rmask, d_cmask, B.overflow};
    hipLaunchKernelGGL(ap_images_kernel, dim3((unsigned)n_images), dim3(kWave), 0, st, A, n_images);
  };
  return osfm_lo::run_batch(ctx, st, d_off, offsets, n_images, prm, kMinimalSamples, results, sizeof(AbsposeOut), ransac_mask,
                            chord_mask, timed_from_ev0, kernel_ms, who, launch);
}

}  // namespace

extern "C" int osfm_abspose_images(osfm_ctx *ctx, const double *bearings, const double *points, const int64_t *offsets, int n_images,
                                   const osfm_abspose_params *prm, osfm_abspose_result *results, uint8_t *ransac_mask, uint8_t *chord_mask,
                                   double *kernel_ms) {
  const char *who = "osfm_abspose_images";
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_REQUIRE(ctx, OSFM_E_INVALID, "%s: null context", who);
  OSFM_TRY(check_args(offsets, n_images, prm, who));
  if (n_images == 0) return OSFM_OK;
  OSFM_REQUIRE(bearings && points && results, OSFM_E_INVALID, "%s: null bearings / points / results", who);
  const int64_t total = offsets[n_images];
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmDevBuf d_b, d_X, d_off;
  OSFM_HIP(d_b.alloc((size_t)total * 24));
  OSFM_HIP(d_X.alloc((size_t)total * 24));
  OSFM_HIP(d_off.alloc((size_t)(n_images + 1) * 8));
  OSFM_HIP(hipMemcpyAsync(d_b.p, bearings, (size_t)total * 24, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_X.p, points, (size_t)total * 24, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_off.p, offsets, (size_t)(n_images + 1) * 8, hipMemcpyHostToDevice, st));
  return run_device(ctx, st, d_b.as<double>(), d_X.as<double>(), d_off.as<int64_t>(), offsets, n_images, prm, results, ransac_mask, chord_mask,
                    false, kernel_ms, who);
}

extern "C" int osfm_abspose_images_pixels(osfm_ctx *ctx, const double *xy, const double *points, const int64_t *offsets, int n_images,
                                          const int32_t *image_cam, const int32_t *cam_model, const double *cam_params, int n_cams,
                                          const osfm_abspose_params *prm, osfm_abspose_result *results, uint8_t *ransac_mask,
                                          uint8_t *chord_mask, double *kernel_ms) {
  const char *who = "osfm_abspose_images_pixels";
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_REQUIRE(ctx, OSFM_E_INVALID, "%s: null context", who);
  OSFM_TRY(check_args(offsets, n_images, prm, who));
  if (n_images == 0) return OSFM_OK;
  OSFM_REQUIRE(xy && points && results && image_cam && cam_model && cam_params && n_cams > 0, OSFM_E_INVALID, "%s: null argument", who);
  OSFM_TRY(osfm_check_camera_table(cam_model, n_cams, image_cam, n_images, 1, "image", who));
  const int64_t total = offsets[n_images];
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmDevBuf d_xy, d_b, d_X, d_off, d_ic, d_cm, d_cp;
  OSFM_HIP(d_xy.alloc((size_t)total * 16));
  OSFM_HIP(d_b.alloc((size_t)total * 24));
  OSFM_HIP(d_X.alloc((size_t)total * 24));
  OSFM_HIP(d_off.alloc((size_t)(n_images + 1) * 8));
  OSFM_HIP(d_ic.alloc((size_t)n_images * 4));
  OSFM_HIP(d_cm.alloc((size_t)n_cams * 4));
  OSFM_HIP(d_cp.alloc((size_t)n_cams * 16 * 8));
  OSFM_HIP(hipMemcpyAsync(d_xy.p, xy, (size_t)total * 16, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_X.p, points, (size_t)total * 24, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_off.p, offsets, (size_t)(n_images + 1) * 8, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_ic.p, image_cam, (size_t)n_images * 4, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_cm.p, cam_model, (size_t)n_cams * 4, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_cp.p, cam_params, (size_t)n_cams * 16 * 8, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipEventRecord(ctx->ev[0], st));  // the kernel time includes the bearings
  hipLaunchKernelGGL(ap_bearings_kernel, dim3((unsigned)n_images), dim3(256), 0, st, d_xy.as<double>(), d_off.as<int64_t>(), d_ic.as<int32_t>(),
                     d_cm.as<int32_t>(), d_cp.as<double>(), d_b.as<double>());
  OSFM_HIP(hipGetLastError());
  return run_device(ctx, st, d_b.as<double>(), d_X.as<double>(), d_off.as<int64_t>(), offsets, n_images, prm, results, ransac_mask, chord_mask,
                    true, kernel_ms, who);
}

extern "C" int osfm_abspose_solve(osfm_ctx *ctx, const double *bearings, const double *points, int n, int kind, double *models_out,
                                  int *count_out) {
  const char *who = "osfm_abspose_solve";
  OSFM_REQUIRE(ctx && bearings && points && models_out && count_out, OSFM_E_INVALID, "%s: null argument", who);
  OSFM_REQUIRE(kind == 0 || kind == 1, OSFM_E_INVALID, "%s: kind must be 0 (three points) or 1 (n points)", who);
  OSFM_REQUIRE(n >= 3 && n <= (1 << 24), OSFM_E_INVALID, "%s: %d rows (at least 3 are needed)", who, n);
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmDevBuf d_b, d_X, d_m, d_c;
  OSFM_HIP(d_b.alloc((size_t)n * 24));
  OSFM_HIP(d_X.alloc((size_t)n * 24));
  OSFM_HIP(d_m.alloc(kMaxModels * 12 * 8));
  OSFM_HIP(d_c.alloc(8));
  OSFM_HIP(hipMemcpyAsync(d_b.p, bearings, (size_t)n * 24, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemcpyAsync(d_X.p, points, (size_t)n * 24, hipMemcpyHostToDevice, st));
  OSFM_HIP(hipMemsetAsync(d_m.p, 0, kMaxModels * 12 * 8, st));
  hipLaunchKernelGGL(ap_solve_kernel, dim3(1), dim3(kWave), 0, st, d_b.as<double>(), d_X.as<double>(), n, kind, d_m.as<double>(), d_c.as<int>());
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipMemcpyAsync(models_out, d_m.p, (size_t)(kind == 0 ? kMaxModels : 1) * 12 * 8, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipMemcpyAsync(count_out, d_c.p, 4, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  return OSFM_OK;
}
