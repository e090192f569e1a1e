// prune.hip -- pruning and merging of depthmaps on gfx950: dense::DepthmapPruner::Prune of opensfm/src/dense/src/depthmap.cc for a batch
// of shots in one call, the merged cloud of the batch as its result -- what dense.prune_depthmap does shot by shot and
// dense.merge_depthmaps concatenates.
//
// The per-pixel rule lives in prune_core.h (host + device); this file adds the lanes, the ordered compaction and the C ABI.  The
// reference's raster-ordered push_back is a prefix sum over the keep flags:
//   dp_mark_kernel     one lane per pixel of view 0, grid (pixel blocks, problems): the keep flag of every pixel and, per workgroup,
//                      the number of flags set (wavefront __shfl_up scans joined through LDS);
//   dp_scan_kernel     ONE workgroup: the block counts, in batch order, become exclusive int64 row offsets, kScanChunk counts at a time
//                      with a running carry; then the rows of every problem;
//   dp_scatter_kernel  the grid of the first kernel: every workgroup ranks its flags again and writes the four outputs of a kept pixel
//                      at row offset + rank.  The point and the normal are computed again, not parked: 24 bytes per pixel less to move.
// A row's place is fixed by the data alone: no atomic decides it, two runs are byte-equal and a batch gives what its single calls give.
// Synchronisation is __syncthreads() and kernel boundaries: no cooperative launch, no grid-wide wait, no spinning on memory.  No lane
// leaves a kernel before a barrier the rest of its workgroup reaches: lanes past the end of a problem stay, with keep = 0 (a workgroup
// that lies wholly past the end of its problem leaves together).
#include <math.h>
#include <string.h>

#include <vector>

#include "osfm_internal.h"
#include "prune_core.h"

using namespace osfm_dm;

namespace {

constexpr int kPixelBlock = 256;             // lanes, and pixels, of a workgroup of the mark and scatter kernels
constexpr int kWaves = kPixelBlock / 64;
constexpr int kScanChunk = 512;              // lanes of the scan kernel's workgroup = block counts it scans per step

// exclusive rank of `v` among the lanes of the workgroup (in lane order) and the workgroup's sum, for n_waves wavefronts of 64 lanes;
// every lane of the workgroup calls it
template <int n_waves>
__device__ int block_exclusive_scan(int v, int *sum) {
  __shared__ int wave_sum[n_waves];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  int incl = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, (unsigned)d);
    if (lane >= d) incl += up;
  }
  __syncthreads();  // the sums of an earlier call have been read
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < n_waves; w++) {
    if (w < wave) before += wave_sum[w];
    all += wave_sum[w];
  }
  *sum = all;
  return before + incl - v;
}

__global__ __launch_bounds__(kPixelBlock) void dp_mark_kernel(const PruneProblem *__restrict__ probs, const PruneView *__restrict__ views,
                                                              float same_depth_threshold, uint8_t *__restrict__ flags,
                                                              int32_t *__restrict__ block_count) {
  const PruneProblem &P = probs[blockIdx.y];
  const int64_t n_pix = (int64_t)P.w * P.h;
  if ((int64_t)blockIdx.x * kPixelBlock >= n_pix) return;  // the whole workgroup
  const int64_t idx = (int64_t)blockIdx.x * kPixelBlock + threadIdx.x;
  int keep = 0;
  if (idx < n_pix) {
    keep = prune_pixel(views, P, same_depth_threshold, (int)(idx / P.w), (int)(idx % P.w)) ? 1 : 0;
    flags[P.pix0 + idx] = (uint8_t)keep;
  }
  int sum;
  block_exclusive_scan<kWaves>(keep, &sum);
  if (threadIdx.x == 0) block_count[P.blk0 + blockIdx.x] = sum;
}

// offsets[k] = rows before block k for k = 0 .. n_blocks (the last: the rows of the batch);  rows[q] = rows of problem q, whose blocks
// are first_block[q] .. first_block[q + 1] - 1
__global__ __launch_bounds__(kScanChunk) void dp_scan_kernel(const int32_t *__restrict__ block_count, int64_t n_blocks, int64_t *__restrict__ offsets,
                                                             const int64_t *__restrict__ first_block, int n_problems, int64_t *__restrict__ rows) {
  int64_t carry = 0;
  for (int64_t base = 0; base < n_blocks; base += kScanChunk) {
    const int64_t k = base + threadIdx.x;
    const int v = k < n_blocks ? block_count[k] : 0;
    int sum;
    const int before = block_exclusive_scan<kScanChunk / 64>(v, &sum);
    if (k < n_blocks) offsets[k] = carry + before;
    carry += sum;
  }
  if (threadIdx.x == 0) offsets[n_blocks] = carry;
  __syncthreads();
  for (int q = (int)threadIdx.x; q < n_problems; q += kScanChunk) rows[q] = offsets[first_block[q + 1]] - offsets[first_block[q]];
}

__global__ __launch_bounds__(kPixelBlock) void dp_scatter_kernel(const PruneProblem *__restrict__ probs, const PruneView *__restrict__ views,
                                                                 const uint8_t *__restrict__ flags, const int64_t *__restrict__ offsets,
                                                                 float *__restrict__ points, float *__restrict__ normals,
                                                                 uint8_t *__restrict__ colors, uint8_t *__restrict__ labels) {
  const PruneProblem &P = probs[blockIdx.y];
  const int64_t n_pix = (int64_t)P.w * P.h;
  if ((int64_t)blockIdx.x * kPixelBlock >= n_pix) return;  // the whole workgroup
  const int64_t idx = (int64_t)blockIdx.x * kPixelBlock + threadIdx.x;
  const int keep = idx < n_pix ? (int)flags[P.pix0 + idx] : 0;
  int sum;
  const int rank = block_exclusive_scan<kWaves>(keep, &sum);
  if (!keep) return;  // (past the last barrier)
  const int64_t row = offsets[P.blk0 + blockIdx.x] + rank;
  float point[3], normal[3];
  uint8_t color[3], label;
  prune_emit(views, P, (int)(idx / P.w), (int)(idx % P.w), point, normal, color, &label);
  for (int k = 0; k < 3; k++) {
    points[3 * row + k] = point[k];
    normals[3 * row + k] = normal[k];
    colors[3 * row + k] = color[k];
  }
  labels[row] = label;
}

bool finite_all(const double *v, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (!finite_d(v[k])) return false;
  return true;
}

// what osfm_depthmap_clean checks of a batch's views, with the pruner's four arrays per view
int check_views(int n_problems, const int32_t *view_offsets, const double *K, const double *R, const double *t, const float *const *depths,
                const float *const *planes, const uint8_t *const *colors, const uint8_t *const *labels, const int32_t *widths,
                const int32_t *heights, const char *who) {
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
  OSFM_REQUIRE(K && R && t && depths && planes && colors && labels && widths && heights, OSFM_E_INVALID, "%s: null argument", who);
  OSFM_REQUIRE(finite_all(K, (size_t)nv * 9) && finite_all(R, (size_t)nv * 9) && finite_all(t, (size_t)nv * 3), OSFM_E_INVALID,
               "%s: a K, R or t is not finite", who);
  for (int v = 0; v < nv; v++) {
    OSFM_REQUIRE(widths[v] >= 0 && heights[v] >= 0 && (int64_t)widths[v] * heights[v] < ((int64_t)1 << 30), OSFM_E_INVALID,
                 "%s: view %d is %d x %d", who, v, widths[v], heights[v]);
    OSFM_REQUIRE((depths[v] && planes[v]) || (int64_t)widths[v] * heights[v] == 0, OSFM_E_INVALID, "%s: view %d has no depth or no plane", who, v);
  }
  for (int b = 0; b < n_problems; b++) {
    const int v = view_offsets[b];
    if (view_offsets[b + 1] == v || (int64_t)widths[v] * heights[v] == 0) continue;
    OSFM_REQUIRE(colors[v] && labels[v], OSFM_E_INVALID, "%s: the first view of problem %d has no colour or no label", who, b);
  }
  return OSFM_OK;
}

}  // namespace

extern "C" int osfm_depthmap_prune(osfm_ctx *ctx, int n_problems, const int32_t *view_offsets, const double *K, const double *R, const double *t,
                                   const float *const *depths, const float *const *planes, const uint8_t *const *colors,
                                   const uint8_t *const *labels, const int32_t *widths, const int32_t *heights, const osfm_depthmap_params *params,
                                   int64_t capacity, float *points, float *normals, uint8_t *out_colors, uint8_t *out_labels, int64_t *counts,
                                   double *kernel_ms) {
  const char *who = "osfm_depthmap_prune";
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_REQUIRE(ctx && params, OSFM_E_INVALID, "%s: null context or params", who);
  OSFM_REQUIRE(n_problems >= 0, OSFM_E_INVALID, "%s: n_problems < 0", who);
  OSFM_REQUIRE(params->same_depth_threshold == params->same_depth_threshold, OSFM_E_INVALID, "%s: same_depth_threshold is NaN", who);
  OSFM_REQUIRE(capacity >= 0, OSFM_E_INVALID, "%s: capacity < 0", who);
  if (n_problems == 0) return OSFM_OK;
  OSFM_TRY(check_views(n_problems, view_offsets, K, R, t, depths, planes, colors, labels, widths, heights, who));
  OSFM_REQUIRE(counts, OSFM_E_INVALID, "%s: null counts", who);
  for (int b = 0; b < n_problems; b++) counts[b] = 0;
  std::vector<PruneProblem> probs;
  std::vector<int> prob_of;
  std::vector<PruneView> views;
  std::vector<size_t> depth_off, color_off;  // per view in floats, per problem in bytes
  std::vector<int64_t> first_block;
  size_t depth_floats = 0, color_bytes = 0;
  int64_t n_pix = 0, max_pix = 0, n_blocks = 0;
  for (int b = 0; b < n_problems; b++) {
    const int v0 = view_offsets[b], n = view_offsets[b + 1] - v0;
    if (n == 0) continue;
    const int64_t px = (int64_t)widths[v0] * heights[v0];
    if (px == 0) continue;
    PruneProblem P;
    memset(&P, 0, sizeof(P));
    inverse3_cv(K + 9 * (size_t)v0, P.Kinv);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) P.Rinv[3 * r + c] = (float)R[9 * (size_t)v0 + 3 * c + r];
    P.view0 = (int64_t)views.size();
    P.pix0 = n_pix;
    P.blk0 = n_blocks;
    P.n_views = n;
    P.w = widths[v0];
    P.h = heights[v0];
    first_block.push_back(n_blocks);
    n_pix += px;
    n_blocks += (px + kPixelBlock - 1) / kPixelBlock;
    if (px > max_pix) max_pix = px;
    for (int o = 0; o < n; o++) {
      PruneView V;
      memset(&V, 0, sizeof(V));
      memcpy(V.K, K + 9 * (size_t)(v0 + o), sizeof(V.K));
      memcpy(V.R, R + 9 * (size_t)(v0 + o), sizeof(V.R));
      memcpy(V.t, t + 3 * (size_t)(v0 + o), sizeof(V.t));
      V.w = widths[v0 + o];
      V.h = heights[v0 + o];
      views.push_back(V);
      depth_off.push_back(depth_floats);
      depth_floats += 4 * (osfm_round256((size_t)V.w * V.h * sizeof(float)) / sizeof(float));  // the depth, then the plane
    }
    color_off.push_back(color_bytes);
    color_bytes += 4 * osfm_round256((size_t)px);  // the colour, then the label
    probs.push_back(P);
    prob_of.push_back(b);
  }
  if (probs.empty()) return OSFM_OK;
  first_block.push_back(n_blocks);
  const int64_t row_cap = capacity < n_pix ? capacity : n_pix;
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmArena A;
  const auto d_probs = A.add<PruneProblem>(probs.size());
  const auto d_views = A.add<PruneView>(views.size());
  const auto d_depths = A.add<float>(depth_floats);
  const auto d_colors = A.add<uint8_t>(color_bytes);
  const auto d_flags = A.add<uint8_t>((size_t)n_pix);
  const auto d_block_count = A.add<int32_t>((size_t)n_blocks);
  const auto d_offsets = A.add<int64_t>((size_t)n_blocks + 1);
  const auto d_first_block = A.add<int64_t>(first_block.size());
  const auto d_rows = A.add<int64_t>(probs.size());
  const auto d_points = A.add<float>(3 * (size_t)row_cap);
  const auto d_normals = A.add<float>(3 * (size_t)row_cap);
  const auto d_out_colors = A.add<uint8_t>(3 * (size_t)row_cap);
  const auto d_out_labels = A.add<uint8_t>((size_t)row_cap);
  OSFM_HIP(A.alloc(ctx));
  for (size_t q = 0; q < probs.size(); q++) {
    const int v0 = view_offsets[prob_of[q]];
    for (int o = 0; o < probs[q].n_views; o++) {
      PruneView &V = views[(size_t)probs[q].view0 + o];
      const size_t px = (size_t)V.w * V.h, stride = osfm_round256(px * sizeof(float)) / sizeof(float);
      float *base = d_depths.get() + depth_off[(size_t)probs[q].view0 + o];
      V.depth = base;
      V.plane = base + stride;
      if (px) {
        OSFM_HIP(hipMemcpyAsync(base, depths[v0 + o], px * sizeof(float), hipMemcpyHostToDevice, st));
        OSFM_HIP(hipMemcpyAsync(base + stride, planes[v0 + o], 3 * px * sizeof(float), hipMemcpyHostToDevice, st));
      }
    }
    const size_t px = (size_t)probs[q].w * probs[q].h;
    uint8_t *base = d_colors.get() + color_off[q];
    probs[q].color = base;
    probs[q].label = base + 3 * osfm_round256(px);
    OSFM_HIP(hipMemcpyAsync(base, colors[v0], 3 * px, hipMemcpyHostToDevice, st));
    OSFM_HIP(hipMemcpyAsync(base + 3 * osfm_round256(px), labels[v0], px, hipMemcpyHostToDevice, st));
  }
  OSFM_HIP(A.upload(d_probs, probs.data(), st));
  OSFM_HIP(A.upload(d_views, views.data(), st));
  OSFM_HIP(A.upload(d_first_block, first_block.data(), st));
  const dim3 grid((unsigned)((max_pix + kPixelBlock - 1) / kPixelBlock), (unsigned)probs.size());
  OSFM_HIP(hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(dp_mark_kernel, grid, dim3(kPixelBlock), 0, st, d_probs.get(), d_views.get(), (float)params->same_depth_threshold, d_flags.get(),
                     d_block_count.get());
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipEventRecord(ctx->ev[2], st));
  hipLaunchKernelGGL(dp_scan_kernel, dim3(1), dim3(kScanChunk), 0, st, d_block_count.get(), n_blocks, d_offsets.get(), d_first_block.get(),
                     (int)probs.size(), d_rows.get());
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipEventRecord(ctx->ev[3], st));
  // the rows come back first: only that many rows of the four outputs cross the bus
  std::vector<int64_t> rows(probs.size());
  OSFM_HIP(hipMemcpyAsync(rows.data(), d_rows.get(), rows.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  int64_t total = 0;
  for (size_t q = 0; q < probs.size(); q++) {
    counts[prob_of[q]] = rows[q];
    total += rows[q];
  }
  OSFM_REQUIRE(total <= capacity, OSFM_E_INVALID, "%s: the batch keeps %lld rows, the buffers hold %lld", who, (long long)total, (long long)capacity);
  OSFM_REQUIRE(total == 0 || (points && normals && out_colors && out_labels), OSFM_E_INVALID, "%s: null output", who);
  OSFM_HIP(hipEventRecord(ctx->ev[4], st));
  if (total) {
    hipLaunchKernelGGL(dp_scatter_kernel, grid, dim3(kPixelBlock), 0, st, d_probs.get(), d_views.get(), d_flags.get(), d_offsets.get(), d_points.get(),
                       d_normals.get(), d_out_colors.get(), d_out_labels.get());
    OSFM_HIP(hipGetLastError());
  }
  OSFM_HIP(hipEventRecord(ctx->ev[1], st));
  if (total) {
    OSFM_HIP(hipMemcpyAsync(points, d_points.get(), 3 * (size_t)total * sizeof(float), hipMemcpyDeviceToHost, st));
    OSFM_HIP(hipMemcpyAsync(normals, d_normals.get(), 3 * (size_t)total * sizeof(float), hipMemcpyDeviceToHost, st));
    OSFM_HIP(hipMemcpyAsync(out_colors, d_out_colors.get(), 3 * (size_t)total, hipMemcpyDeviceToHost, st));
    OSFM_HIP(hipMemcpyAsync(out_labels, d_out_labels.get(), (size_t)total, hipMemcpyDeviceToHost, st));
  }
  OSFM_HIP(hipStreamSynchronize(st));
  if (kernel_ms) {
    double split[3];
    OSFM_TRY(osfm_depthmap_prune_split_ms(ctx, split));
    *kernel_ms = split[0] + split[1] + split[2];
  }
  return OSFM_OK;
}

// mark, scan and scatter of the context's last osfm_depthmap_prune that launched kernels (the host waits between the scan and the
// scatter: their sum, not the span, is the call's kernel time)
extern "C" int osfm_depthmap_prune_split_ms(osfm_ctx *ctx, double *ms) {
  OSFM_REQUIRE(ctx && ms, OSFM_E_INVALID, "osfm_depthmap_prune_split_ms: null argument");
  OSFM_CTX_LOCK(ctx);
  const int pair[3][2] = {{0, 2}, {2, 3}, {4, 1}};
  for (int k = 0; k < 3; k++) {
    float v = 0.f;
    OSFM_HIP(hipEventElapsedTime(&v, ctx->ev[pair[k][0]], ctx->ev[pair[k][1]]));
    ms[k] = v;
  }
  return OSFM_OK;
}
