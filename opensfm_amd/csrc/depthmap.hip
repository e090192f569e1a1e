// depthmap.hip -- raw depthmaps and their cleaning on gfx950: dense::DepthmapEstimator (ComputeBruteForce, ComputePatchMatch,
// ComputePatchMatchSample) and dense::DepthmapCleaner::Clean of opensfm/src/dense/src/depthmap.cc for a batch of shots in one call --
// what dense.compute_depthmap and dense.clean_depthmap do shot by shot, one CPU thread each.
//
// The numerics live in depthmap_core.h (host + device); this file adds the lanes, the kernels and the C ABI.
//   dm_brute_kernel   one lane per interior pixel, grid (pixel blocks, problems): a pixel's planes and views in the reference's order;
//   dm_patch_kernel   ONE workgroup per problem.  The reference's raster sweep is sequential: pixel (i, j) of a forward pass reads
//                     (i - 1, j) and (i, j - 1), final values of that pass, so the pixels of one anti-diagonal i + j = c are
//                     independent and a diagonal wavefront gives the sequential result; the backward pass is its mirror image.  Sample
//                     mode: one lane per pixel of the diagonal, one workgroup barrier per diagonal.  Otherwise lanes cover pixels x
//                     views: per candidate, every (pixel, view) score goes to a scratch row, barrier, the pixel's lane takes the
//                     maximum in ascending view order with the reference's strict > (the lowest view wins a tie), barrier.
//                     The chip is filled by the batch: no grid-wide wait, no cooperative launch, no spinning on memory.
//   dm_clean_kernel   one lane per pixel, grid (pixel blocks, problems).
// A pixel's result never depends on the grid or on another problem: a batch gives, byte for byte, what single calls give.
#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "depthmap_core.h"
#include "osfm_internal.h"

using namespace osfm_dm;

namespace {

constexpr int kPixelBlock = 256;
constexpr int kPatchBlock = 512;

__global__ __launch_bounds__(kPixelBlock) void dm_brute_kernel(const Problem *__restrict__ probs, const View *__restrict__ views, Tables tab, Params prm,
                                                               Out out) {
  const Problem &P = probs[blockIdx.y];
  const int hpz = (prm.patch_size - 1) / 2, ih = P.h - 2 * hpz, iw = P.w - 2 * hpz;
  const int64_t idx = (int64_t)blockIdx.x * kPixelBlock + threadIdx.x;
  if (idx >= (int64_t)ih * iw) return;
  brute_force_pixel(views, P, tab, prm, out, hpz + (int)(idx / iw), hpz + (int)(idx % iw));
}

__global__ __launch_bounds__(kPatchBlock) void dm_patch_kernel(const Problem *__restrict__ probs, const View *__restrict__ views, Tables tab, Params prm,
                                                               Out out, float *__restrict__ scratch) {
  const Problem &P = probs[blockIdx.x];
  const int tid = (int)threadIdx.x;
  const int hpz = (prm.patch_size - 1) / 2, ih = P.h - 2 * hpz, iw = P.w - 2 * hpz;  // the host launches no problem without an interior
  const int nv = P.n_views - 1;
  const bool sample = sample_mode(P, prm);
  float *scores = scratch + P.scr0;               // (pixel of the diagonal) x (other view)
  float *median = scores + (int64_t)(ih < iw ? ih : iw) * (nv > 0 ? nv : 1);  // w x h
  for (int idx = tid; idx < ih * iw; idx += kPatchBlock) init_pixel(views, P, tab, prm, out, hpz + idx / iw, hpz + idx % iw);
  __syncthreads();
  for (int pass = 0; pass < 2 * prm.iterations; pass++) {
    const bool backward = (pass & 1) != 0;
    const int sweep = 1 + pass;
    for (int c = 0; c <= ih + iw - 2; c++) {
      const int lo = c - iw + 1 > 0 ? c - iw + 1 : 0, hi = c < ih - 1 ? c : ih - 1;
      const int n = hi - lo + 1;
      // pixel p of the diagonal: interior row lo + p, column c - row; mirrored in a backward pass
      if (sample) {
        for (int p = tid; p < n; p += kPatchBlock) {
          const int ii = lo + p, jj = c - ii;
          update_pixel_sample(views, P, tab, prm, out, sweep, backward, hpz + (backward ? ih - 1 - ii : ii), hpz + (backward ? iw - 1 - jj : jj));
        }
        __syncthreads();
        continue;
      }
      for (int cand = 0; cand < kCandidates - 1; cand++) {
        for (int item = tid; item < n * nv; item += kPatchBlock) {
          const int p = item / nv, other = 1 + item % nv;
          const int ii = lo + p, jj = c - ii;
          const int i = hpz + (backward ? ih - 1 - ii : ii), j = hpz + (backward ? iw - 1 - jj : jj);
          float plane[3];
          int unused;
          if (candidate(P, tab, prm, out, sweep, backward, i, j, cand, plane, &unused))
            scores[item] = image_score(views[P.view0], views[P.view0 + other], P.Kinv, tab.weight, hpz, i, j, plane);
        }
        __syncthreads();
        for (int p = tid; p < n; p += kPatchBlock) {
          const int ii = lo + p, jj = c - ii;
          const int i = hpz + (backward ? ih - 1 - ii : ii), j = hpz + (backward ? iw - 1 - jj : jj);
          float plane[3];
          int unused;
          if (!candidate(P, tab, prm, out, sweep, backward, i, j, cand, plane, &unused)) continue;
          float score = -1.0f;
          int nghbr = 0;
          for (int other = 1; other <= nv; other++) {
            const float s = scores[p * nv + other - 1];
            if (s > score) {
              score = s;
              nghbr = other;
            }
          }
          check_candidate(out, P, i, j, plane, score, nghbr);
        }
        __syncthreads();
      }
    }
  }
  // PostProcess
  const float *depth = out.depth + P.pix0;
  for (int idx = tid; idx < P.w * P.h; idx += kPatchBlock) median[idx] = median5(depth, P.w, P.h, idx / P.w, idx % P.w);
  __syncthreads();
  for (int idx = tid; idx < P.w * P.h; idx += kPatchBlock) out.depth[P.pix0 + idx] = post_process(depth[idx], median[idx]);
}

__global__ __launch_bounds__(kPixelBlock) void dm_clean_kernel(const CleanProblem *__restrict__ probs, const CleanView *__restrict__ views, float threshold,
                                                               int min_consistent, float *__restrict__ clean) {
  const CleanProblem &P = probs[blockIdx.y];
  const int64_t idx = (int64_t)blockIdx.x * kPixelBlock + threadIdx.x;
  if (idx >= (int64_t)P.w * P.h) return;
  clean[P.pix0 + idx] = clean_pixel(views, P, threshold, min_consistent, (int)(idx / P.w), (int)(idx % P.w));
}

// ---- the tables ----
// Phi^-1(p) by bisection on erfc: the interval halves until it no longer shrinks (the error of erfc, a few 1e-16, moves the root by less
// than 1e-12 relative anywhere in the table)
double normal_quantile(double p) {
  double lo = -10.0, hi = 10.0;
  for (int it = 0; it < 200; it++) {
    const double mid = 0.5 * (lo + hi);
    if (mid <= lo || mid >= hi) break;
    if (0.5 * erfc(-mid / sqrt(2.0)) < p) lo = mid; else hi = mid;
  }
  return 0.5 * (lo + hi);
}

struct HostTables {
  std::vector<float> normal, factor, weight;
};
const HostTables &host_tables() {
  static HostTables T;
  static std::once_flag once;
  std::call_once(once, [] {
    T.normal.resize(kQuantiles);
    for (int m = 0; m < kQuantiles / 2; m++) {  // antisymmetric by construction
      const float q = (float)normal_quantile(((double)m + 0.5) / (double)kQuantiles);
      T.normal[m] = q;
      T.normal[kQuantiles - 1 - m] = -q;
    }
    T.factor.resize((size_t)kPerturb * kQuantiles);
    for (int k = 0; k < kPerturb; k++)
      for (int m = 0; m < kQuantiles; m++) T.factor[(size_t)k * kQuantiles + m] = (float)exp((double)(depth_range(k) * T.normal[m]));
    T.weight.resize((size_t)256 * kR2);
    const float dcolor_factor = 1.0f / (2 * 50.0f * 50.0f), dx_factor = 1.0f / (2 * 5.0f * 5.0f);
    for (int dc = 0; dc < 256; dc++)
      for (int r2 = 0; r2 < kR2; r2++) {
        const float dcolor = (float)dc;
        const float arg = -dcolor * dcolor * dcolor_factor - (float)r2 * dx_factor;  // depthmap.cc:473, in float
        T.weight[(size_t)dc * kR2 + r2] = (float)exp((double)arg);
      }
  });
  return T;
}
void init_depth_table(double min_depth, double max_depth, float *out) {
  const double a = log(min_depth), b = log(max_depth);
  for (int m = 0; m < kQuantiles; m++) out[m] = (float)exp(a + (b - a) * (((double)m + 0.5) / (double)kQuantiles));
}

bool finite_all(const double *v, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (!finite_d(v[k])) return false;
  return true;
}

// what both calls check of a batch's views
int check_views(int n_problems, const int32_t *view_offsets, const double *K, const double *R, const double *t, const void *const *data,
                const int32_t *widths, const int32_t *heights, const char *who) {
  OSFM_REQUIRE(view_offsets, OSFM_E_INVALID, "%s: null view_offsets", who);
  OSFM_REQUIRE(view_offsets[0] == 0, OSFM_E_INVALID, "%s: view_offsets[0] must be 0", who);
  OSFM_REQUIRE(n_problems <= 65535, OSFM_E_INVALID, "%s: more than 65535 problems in one call", who);
  for (int b = 0; b < n_problems; b++) {
    const int n = view_offsets[b + 1] - view_offsets[b];
    OSFM_REQUIRE(n >= 0, OSFM_E_INVALID, "%s: view_offsets decrease at problem %d", who, b);
    OSFM_REQUIRE(n <= kMaxViews, OSFM_E_INVALID, "%s: problem %d has %d views, more than %d", who, b, n, kMaxViews);
  }
  const int nv = view_offsets[n_problems];
  if (nv == 0) return OSFM_OK;
  OSFM_REQUIRE(K && R && t && data && widths && heights, OSFM_E_INVALID, "%s: null argument", who);
  OSFM_REQUIRE(finite_all(K, (size_t)nv * 9) && finite_all(R, (size_t)nv * 9) && finite_all(t, (size_t)nv * 3), OSFM_E_INVALID,
               "%s: a K, R or t is not finite", who);
  for (int v = 0; v < nv; v++) {
    OSFM_REQUIRE(widths[v] >= 0 && heights[v] >= 0 && (int64_t)widths[v] * heights[v] < ((int64_t)1 << 30), OSFM_E_INVALID,
                 "%s: view %d is %d x %d", who, v, widths[v], heights[v]);
    OSFM_REQUIRE(data[v] || (int64_t)widths[v] * heights[v] == 0, OSFM_E_INVALID, "%s: view %d has no data", who, v);
  }
  return OSFM_OK;
}

}  // namespace

extern "C" void osfm_depthmap_params_default(osfm_depthmap_params *p) {
  if (!p) return;
  p->min_depth = 0.0;
  p->max_depth = 0.0;
  p->min_patch_sd = 1.0;
  p->min_correlation_score = 0.1;
  p->same_depth_threshold = 0.01;
  p->method = OSFM_DEPTHMAP_PATCH_MATCH_SAMPLE;
  p->resolution = 640;
  p->num_neighbors = 10;
  p->num_matching_views = 6;
  p->patchmatch_iterations = 3;
  p->patch_size = 7;
  p->min_consistent_views = 3;
  p->num_depth_planes = 100;
  p->pad = 0;
}

extern "C" int osfm_depthmap_tables(double min_depth, double max_depth, float *normal, float *factor, float *weight, float *init_depth) {
  const HostTables &T = host_tables();
  if (normal) memcpy(normal, T.normal.data(), T.normal.size() * sizeof(float));
  if (factor) memcpy(factor, T.factor.data(), T.factor.size() * sizeof(float));
  if (weight) memcpy(weight, T.weight.data(), T.weight.size() * sizeof(float));
  if (init_depth) {
    OSFM_REQUIRE(min_depth > 0.0 && max_depth >= min_depth && finite_d(max_depth), OSFM_E_INVALID,
                 "osfm_depthmap_tables: the depth range must satisfy 0 < min_depth <= max_depth");
    init_depth_table(min_depth, max_depth, init_depth);
  }
  return OSFM_OK;
}

extern "C" int osfm_depthmap_estimate(osfm_ctx *ctx, int n_problems, const int32_t *view_offsets, const double *K, const double *R, const double *t,
                                      const uint8_t *const *images, const uint8_t *const *masks, const int32_t *widths, const int32_t *heights,
                                      const double *min_depth, const double *max_depth, const osfm_depthmap_params *params, uint64_t seed,
                                      float *const *depth, float *const *plane, float *const *score, int32_t *const *nghbr, double *kernel_ms) {
  const char *who = "osfm_depthmap_estimate";
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_REQUIRE(ctx && params, OSFM_E_INVALID, "%s: null context or params", who);
  OSFM_REQUIRE(n_problems >= 0, OSFM_E_INVALID, "%s: n_problems < 0", who);
  const osfm_depthmap_params &p = *params;
  OSFM_REQUIRE(p.method >= OSFM_DEPTHMAP_BRUTE_FORCE && p.method <= OSFM_DEPTHMAP_PATCH_MATCH_SAMPLE, OSFM_E_INVALID, "%s: unknown method %d", who,
               p.method);
  OSFM_REQUIRE(p.patch_size >= 3 && p.patch_size % 2 == 1, OSFM_E_INVALID,
               "%s: patch_size %d must be odd and at least 3 (the reference reads stale or foreign memory otherwise)", who, p.patch_size);
  OSFM_REQUIRE(p.patch_size <= kMaxPatch, OSFM_E_INVALID, "%s: patch_size %d is above %d", who, p.patch_size, kMaxPatch);
  OSFM_REQUIRE(p.num_depth_planes >= 1, OSFM_E_INVALID, "%s: num_depth_planes < 1", who);
  OSFM_REQUIRE(p.patchmatch_iterations >= 0, OSFM_E_INVALID, "%s: patchmatch_iterations < 0", who);
  OSFM_REQUIRE(p.min_patch_sd == p.min_patch_sd, OSFM_E_INVALID, "%s: min_patch_sd is NaN", who);
  if (n_problems == 0) return OSFM_OK;
  OSFM_TRY(check_views(n_problems, view_offsets, K, R, t, (const void *const *)images, widths, heights, who));
  OSFM_REQUIRE(min_depth && max_depth && depth && plane && score && nghbr, OSFM_E_INVALID, "%s: null argument", who);
  const int hpz = (p.patch_size - 1) / 2;
  const bool patchmatch = p.method != OSFM_DEPTHMAP_BRUTE_FORCE;

  // the problems with an interior go to the device; the others are zeros
  std::vector<Problem> probs;
  std::vector<int> prob_of;  // index in the batch
  std::vector<View> views;
  std::vector<float> init_tables;
  std::vector<size_t> image_off, mask_off;
  size_t image_bytes = 0, mask_bytes = 0;
  int64_t n_pix = 0, n_scratch = 0, max_interior = 0;
  // the whole batch is checked before any output is touched: a refused call leaves the caller's buffers as they were
  for (int b = 0; b < n_problems; b++) {
    const int v0 = view_offsets[b], n = view_offsets[b + 1] - v0;
    if (n == 0) continue;
    const size_t px = (size_t)widths[v0] * heights[v0];
    OSFM_REQUIRE(px == 0 || (masks && masks[v0] && depth[b] && plane[b] && score[b] && nghbr[b]), OSFM_E_INVALID,
                 "%s: problem %d has no mask or no outputs", who, b);
    OSFM_REQUIRE(min_depth[b] > 0.0 && max_depth[b] >= min_depth[b] && finite_d(max_depth[b]), OSFM_E_INVALID,
                 "%s: problem %d: the depth range must satisfy 0 < min_depth <= max_depth", who, b);
  }
  for (int b = 0; b < n_problems; b++) {
    const int v0 = view_offsets[b], n = view_offsets[b + 1] - v0;
    if (n == 0) continue;
    const int w = widths[v0], h = heights[v0];
    const size_t px = (size_t)w * h;
    if (px) {
      memset(depth[b], 0, px * sizeof(float));
      memset(plane[b], 0, 3 * px * sizeof(float));
      memset(score[b], 0, px * sizeof(float));
      memset(nghbr[b], 0, px * sizeof(int32_t));
    }
    const int ih = h - 2 * hpz, iw = w - 2 * hpz;
    if (ih < 1 || iw < 1) continue;
    Problem P;
    memset(&P, 0, sizeof(P));
    inverse3_cv(K + 9 * (size_t)v0, P.Kinv);
    P.min_depth = min_depth[b];
    P.max_depth = max_depth[b];
    P.view0 = (int64_t)views.size();
    P.pix0 = n_pix;
    P.scr0 = n_scratch;
    P.n_views = n;
    P.w = w;
    P.h = h;
    n_pix += (int64_t)px;
    n_scratch += (int64_t)(ih < iw ? ih : iw) * (n > 1 ? n - 1 : 1) + (int64_t)px;
    if ((int64_t)ih * iw > max_interior) max_interior = (int64_t)ih * iw;
    for (int o = 0; o < n; o++) {
      View V;
      memset(&V, 0, sizeof(V));
      memcpy(V.K, K + 9 * (size_t)(v0 + o), sizeof(V.K));
      baked_view(R + 9 * (size_t)v0, t + 3 * (size_t)v0, R + 9 * (size_t)(v0 + o), t + 3 * (size_t)(v0 + o), V.Q, V.a);
      V.w = widths[v0 + o];
      V.h = heights[v0 + o];
      views.push_back(V);
      image_off.push_back(image_bytes);
      image_bytes += osfm_round256((size_t)V.w * V.h);
    }
    mask_off.push_back(mask_bytes);
    mask_bytes += osfm_round256(px);
    if (patchmatch) {
      init_tables.resize(init_tables.size() + kQuantiles);
      init_depth_table(P.min_depth, P.max_depth, init_tables.data() + init_tables.size() - kQuantiles);
    }
    probs.push_back(P);
    prob_of.push_back(b);
  }
  if (probs.empty()) return OSFM_OK;
  const HostTables &T = host_tables();

  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmArena A;
  const auto d_probs = A.add<Problem>(probs.size());
  const auto d_views = A.add<View>(views.size());
  const auto d_normal = A.add<float>(T.normal.size()), d_factor = A.add<float>(T.factor.size()), d_weight = A.add<float>(T.weight.size());
  const auto d_init = A.add<float>(init_tables.size());
  const auto d_images = A.add<uint8_t>(image_bytes), d_masks = A.add<uint8_t>(mask_bytes);
  const auto d_depth = A.add<float>((size_t)n_pix), d_plane = A.add<float>(3 * (size_t)n_pix), d_score = A.add<float>((size_t)n_pix);
  const auto d_nghbr = A.add<int32_t>((size_t)n_pix);
  const auto d_scratch = A.add<float>(patchmatch ? (size_t)n_scratch : 0);
  OSFM_HIP(A.alloc(ctx));
  for (size_t q = 0; q < probs.size(); q++) {
    const int v0 = view_offsets[prob_of[q]];
    probs[q].mask = d_masks.get() + mask_off[q];
    probs[q].init_depth = patchmatch ? d_init.get() + q * kQuantiles : nullptr;
    OSFM_HIP(hipMemcpyAsync(d_masks.get() + mask_off[q], masks[v0], (size_t)probs[q].w * probs[q].h, hipMemcpyHostToDevice, st));
    for (int o = 0; o < probs[q].n_views; o++) {
      View &V = views[(size_t)probs[q].view0 + o];
      V.image = d_images.get() + image_off[(size_t)probs[q].view0 + o];
      if ((size_t)V.w * V.h)
        OSFM_HIP(hipMemcpyAsync(d_images.get() + image_off[(size_t)probs[q].view0 + o], images[v0 + o], (size_t)V.w * V.h, hipMemcpyHostToDevice, st));
    }
  }
  OSFM_HIP(A.upload(d_probs, probs.data(), st));
  OSFM_HIP(A.upload(d_views, views.data(), st));
  OSFM_HIP(A.upload(d_normal, T.normal.data(), st));
  OSFM_HIP(A.upload(d_factor, T.factor.data(), st));
  OSFM_HIP(A.upload(d_weight, T.weight.data(), st));
  OSFM_HIP(A.upload(d_init, init_tables.data(), st));
  OSFM_HIP(hipMemsetAsync(d_depth, 0, d_depth.bytes, st));
  OSFM_HIP(hipMemsetAsync(d_plane, 0, d_plane.bytes, st));
  OSFM_HIP(hipMemsetAsync(d_score, 0, d_score.bytes, st));
  OSFM_HIP(hipMemsetAsync(d_nghbr, 0, d_nghbr.bytes, st));
  const Tables tab{d_normal, d_factor, d_weight};
  const Params prm{seed, (int)p.patch_size, (int)p.patchmatch_iterations, (int)p.num_depth_planes, (int)p.method,
                   (float)p.min_patch_sd * (float)p.min_patch_sd};
  const Out out{d_depth, d_plane, d_score, d_nghbr};
  OSFM_HIP(hipEventRecord(ctx->ev[0], st));
  if (patchmatch)
    hipLaunchKernelGGL(dm_patch_kernel, dim3((unsigned)probs.size()), dim3(kPatchBlock), 0, st, d_probs.get(), d_views.get(), tab, prm, out,
                       d_scratch.get());
  else
    hipLaunchKernelGGL(dm_brute_kernel, dim3((unsigned)((max_interior + kPixelBlock - 1) / kPixelBlock), (unsigned)probs.size()), dim3(kPixelBlock), 0,
                       st, d_probs.get(), d_views.get(), tab, prm, out);
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipEventRecord(ctx->ev[1], st));
  for (size_t q = 0; q < probs.size(); q++) {
    const int b = prob_of[q];
    const size_t px = (size_t)probs[q].w * probs[q].h, at = (size_t)probs[q].pix0;
    OSFM_HIP(hipMemcpyAsync(depth[b], d_depth.get() + at, px * sizeof(float), hipMemcpyDeviceToHost, st));
    OSFM_HIP(hipMemcpyAsync(plane[b], d_plane.get() + 3 * at, 3 * px * sizeof(float), hipMemcpyDeviceToHost, st));
    OSFM_HIP(hipMemcpyAsync(score[b], d_score.get() + at, px * sizeof(float), hipMemcpyDeviceToHost, st));
    OSFM_HIP(hipMemcpyAsync(nghbr[b], d_nghbr.get() + at, px * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  OSFM_HIP(hipStreamSynchronize(st));
  return osfm_kernel_ms(ctx, kernel_ms);
}

extern "C" int osfm_depthmap_clean(osfm_ctx *ctx, int n_problems, const int32_t *view_offsets, const double *K, const double *R, const double *t,
                                   const float *const *depths, const int32_t *widths, const int32_t *heights, const osfm_depthmap_params *params,
                                   float *const *clean, double *kernel_ms) {
  const char *who = "osfm_depthmap_clean";
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_REQUIRE(ctx && params, OSFM_E_INVALID, "%s: null context or params", who);
  OSFM_REQUIRE(n_problems >= 0, OSFM_E_INVALID, "%s: n_problems < 0", who);
  OSFM_REQUIRE(params->same_depth_threshold == params->same_depth_threshold, OSFM_E_INVALID, "%s: same_depth_threshold is NaN", who);
  if (n_problems == 0) return OSFM_OK;
  OSFM_TRY(check_views(n_problems, view_offsets, K, R, t, (const void *const *)depths, widths, heights, who));
  OSFM_REQUIRE(clean, OSFM_E_INVALID, "%s: null clean", who);
  std::vector<CleanProblem> probs;
  std::vector<int> prob_of;
  std::vector<CleanView> views;
  std::vector<size_t> depth_off;
  size_t depth_floats = 0;
  int64_t n_pix = 0, max_pix = 0;
  for (int b = 0; b < n_problems; b++) {
    const int v0 = view_offsets[b], n = view_offsets[b + 1] - v0;
    if (n == 0) continue;
    const int64_t px = (int64_t)widths[v0] * heights[v0];
    if (px == 0) continue;
    OSFM_REQUIRE(clean[b], OSFM_E_INVALID, "%s: problem %d has no output", who, b);
    CleanProblem P;
    memset(&P, 0, sizeof(P));
    inverse3_cv(K + 9 * (size_t)v0, P.Kinv);
    P.view0 = (int64_t)views.size();
    P.pix0 = n_pix;
    P.n_views = n;
    P.w = widths[v0];
    P.h = heights[v0];
    n_pix += px;
    if (px > max_pix) max_pix = px;
    for (int o = 0; o < n; o++) {
      CleanView V;
      memset(&V, 0, sizeof(V));
      memcpy(V.K, K + 9 * (size_t)(v0 + o), sizeof(V.K));
      memcpy(V.R, R + 9 * (size_t)(v0 + o), sizeof(V.R));
      memcpy(V.t, t + 3 * (size_t)(v0 + o), sizeof(V.t));
      V.w = widths[v0 + o];
      V.h = heights[v0 + o];
      views.push_back(V);
      depth_off.push_back(depth_floats);
      depth_floats += osfm_round256((size_t)V.w * V.h * sizeof(float)) / sizeof(float);
    }
    probs.push_back(P);
    prob_of.push_back(b);
  }
  if (probs.empty()) return OSFM_OK;
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmArena A;
  const auto d_probs = A.add<CleanProblem>(probs.size());
  const auto d_views = A.add<CleanView>(views.size());
  const auto d_depths = A.add<float>(depth_floats);
  const auto d_clean = A.add<float>((size_t)n_pix);
  OSFM_HIP(A.alloc(ctx));
  for (size_t q = 0; q < probs.size(); q++) {
    const int v0 = view_offsets[prob_of[q]];
    for (int o = 0; o < probs[q].n_views; o++) {
      CleanView &V = views[(size_t)probs[q].view0 + o];
      V.depth = d_depths.get() + depth_off[(size_t)probs[q].view0 + o];
      if ((size_t)V.w * V.h)
        OSFM_HIP(hipMemcpyAsync(d_depths.get() + depth_off[(size_t)probs[q].view0 + o], depths[v0 + o], (size_t)V.w * V.h * sizeof(float),
                                hipMemcpyHostToDevice, st));
    }
  }
  OSFM_HIP(A.upload(d_probs, probs.data(), st));
  OSFM_HIP(A.upload(d_views, views.data(), st));
  OSFM_HIP(hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(dm_clean_kernel, dim3((unsigned)((max_pix + kPixelBlock - 1) / kPixelBlock), (unsigned)probs.size()), dim3(kPixelBlock), 0, st,
                     d_probs.get(), d_views.get(), (float)params->same_depth_threshold, (int)params->min_consistent_views, d_clean.get());
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipEventRecord(ctx->ev[1], st));
  for (size_t q = 0; q < probs.size(); q++)
    OSFM_HIP(hipMemcpyAsync(clean[prob_of[q]], d_clean.get() + probs[q].pix0, (size_t)probs[q].w * probs[q].h * sizeof(float), hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  return osfm_kernel_ms(ctx, kernel_ms);
}
