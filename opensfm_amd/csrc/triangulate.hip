// triangulate.hip -- triangulation of reconstruction tracks on gfx950: TrackTriangulator.triangulate (opensfm/reconstruction.py:1032-1073,
// `triangulation_type: FULL`) for every track of a batch in one call -- what triangulate_shot_features and retriangulate do track by track.
//
// The numerics and the per-track walk live in triangulate_core.h (host + device); this file adds the lane policies, the kernels and the
// C ABI.
//   tri_group_kernel  a group of kGroup = 8 lanes per track (eight tracks per wavefront, the shape of cloud.hip) for the tracks of at
//                     most kGroupObs observations;
//   tri_wave_kernel   one wavefront per track for the longer ones (a compacted list the host builds while it checks the offsets).
// A lane loads the observations i = lane, lane + G, ... of its track ONCE -- for osfm_triangulate_tracks that is where the bearing
// b = pixel_bearing(xy), w = R^T b and o = -R^T t are computed and where the row is validated -- and parks (o, w) in LDS, where the pair
// test, the midpoint sums, the two per-observation tests and every evaluation of the refinement read them.  Only a track longer than
// the kWaveObs observations a wavefront's LDS slice holds loads the overhang again.
// Sums: every lane adds its observations in ascending order, then a butterfly over the group (log2 G xor-shuffles): the order depends
// on the track's length alone (which kernel, which lane), never on the grid or on timing; no atomics on floating-point values.
//
// `triangulation_type: ROBUST` (TrackTriangulator.triangulate_robust, the walk of triangulate_robust.h) runs on the same two shapes:
// tri_group_robust_kernel and tri_wave_robust_kernel share the row loaders, stage() and the host-side split.  The candidate and best
// masks belong to the lane that owns the observation: one 32-bit word per lane (bit 16 * which + i / G) -- a register in the group
// kernel (at most 4 observations per lane), an LDS word per lane in the wavefront kernel (8 staged observations per lane) -- and, for
// the overhang past kWaveObs, bit `which` of the observation's byte of the output mask, which the same lane alone reads and writes.
#include <math.h>

#include <vector>

#include "osfm_internal.h"
#include "triangulate_core.h"
#include "triangulate_robust.h"

using namespace osfm_tri;

namespace {

constexpr int kGroup = 8;  // lanes per short track
#ifndef OSFM_TRI_GROUP_OBS
#define OSFM_TRI_GROUP_OBS 32  // the measured split: 8 is 7 x slower on 10-observation tracks, 16 ties, 64 loses occupancy to LDS
#endif
constexpr int kGroupObs = OSFM_TRI_GROUP_OBS;  // longest track of the group kernel
constexpr int kGroupPitch = kGroupObs + 1;     // LDS doubles per group and component (odd: the groups of a wavefront start on different banks)
constexpr int kBlock = 256;
constexpr int kGroupsPerBlock = kBlock / kGroup;
constexpr int kWave = 64;
constexpr int kWaveObs = 512;  // observations of a long track kept in LDS (24 KiB)
constexpr int kMaxTrack = 1 << 24;

// rows that are world-space origins and bearings already
struct BearingRows {
  const double *centers, *bearings;
  __device__ __forceinline__ bool load(int64_t row, double *o, double *w) const {
    for (int k = 0; k < 3; k++) {
      o[k] = centers[3 * row + k];
      w[k] = bearings[3 * row + k];
    }
    return true;
  }
};

// rows that are (shot, normalised image point): Camera::Bearing, then into the world with the shot's pose; false for a row that cannot
// be evaluated (shot index outside the table, non-finite point or pose)
struct PixelRows {
  const double *shot_pose;
  const int32_t *shot_camera, *cam_model;
  const double *cam_params;
  const int32_t *obs_shot;
  const double *obs_xy;
  int n_shots;
  __device__ __forceinline__ bool load(int64_t row, double *o, double *w) const {
    const int s = obs_shot[row];
    const double x = obs_xy[2 * row], y = obs_xy[2 * row + 1];
    bool ok = s >= 0 && s < n_shots && finite_d(x) && finite_d(y);
    double P[12];
    for (int k = 0; k < 12; k++) {
      P[k] = ok ? shot_pose[12 * (size_t)s + k] : NAN;
      ok = ok && finite_d(P[k]);
    }
    if (!ok) {
      for (int k = 0; k < 3; k++) o[k] = w[k] = NAN;
      return false;
    }
    const int c = shot_camera[s];
    double b[3];
    osfm_rp::pixel_bearing_generic(cam_model[c], cam_params + 16 * (size_t)c, x, y, b);
    for (int k = 0; k < 3; k++) {
      w[k] = (P[k] * b[0] + P[3 + k] * b[1]) + P[6 + k] * b[2];       // R^T b
      o[k] = -((P[k] * P[9] + P[3 + k] * P[10]) + P[6 + k] * P[11]);  // Pose::GetOrigin: -R^T t
    }
    return true;
  }
};

// G lanes on one track; (o, w) of observation i < cap at sh[c * plane + i], c = 0 .. 5.  Overhang: the track may be longer than cap
template <int G, bool Overhang, class Rows>
struct LaneTrack {
  int n, lane, cap, plane;
  const double *sh;
  Rows rows;
  int64_t row0;
  __device__ __forceinline__ int first() const { return lane; }
  __device__ __forceinline__ int stride() const { return G; }
  __device__ __forceinline__ void at(int i, double *o, double *w) const {
    if (!Overhang || i < cap) {
      for (int k = 0; k < 3; k++) {
        o[k] = sh[k * plane + i];
        w[k] = sh[(3 + k) * plane + i];
      }
    } else {
      again(row0 + i, o, w);
    }
  }
  // the overhang of a track longer than the LDS slice (validated when the track was staged); out of line: one copy, not one per reader
  __device__ __attribute__((noinline)) void again(int64_t row, double *o, double *w) const { (void)rows.load(row, o, w); }
  template <class F>
  __device__ __forceinline__ void each(F f) const {
    for (int i = lane; i < n; i += G) {
      double o[3], w[3];
      at(i, o, w);
      f(i, o, w);
    }
  }
  __device__ __forceinline__ void sum(double *v, int m) const {
    for (int mask = 1; mask < G; mask <<= 1)
      for (int k = 0; k < m; k++) v[k] += __shfl_xor(v[k], mask, 64);
  }
  __device__ __forceinline__ int lowest(int key) const {
    for (int mask = 1; mask < G; mask <<= 1) {
      const int other = __shfl_xor(key, mask, 64);
      key = other < key ? other : key;
    }
    return key;
  }
  __device__ __forceinline__ bool any(bool b) const {
    int v = b ? 1 : 0;
    for (int mask = 1; mask < G; mask <<= 1) v |= __shfl_xor(v, mask, 64);
    return v != 0;
  }
};

struct Out {
  double *points;
  uint8_t *status;
  int32_t *iterations;
  int *bad;  // set when a row could not be evaluated
  const double *initial;  // osfm_triangulate_refine: n_tracks x 3 starting points -- PointRefinement alone, no test; else null
};

// lanes lane, lane + G, ... of a track's first `cap` observations into LDS
template <int G, class Rows>
__device__ __forceinline__ void stage(const Rows &rows, int64_t row0, int n, int cap, int lane, double *sh, int plane, int *bad) {
  bool ok = true;
  for (int i = lane; i < n; i += G) {
    double o[3], w[3];
    ok = rows.load(row0 + i, o, w) && ok;
    if (i < cap)
      for (int k = 0; k < 3; k++) {
        sh[k * plane + i] = o[k];
        sh[(3 + k) * plane + i] = w[k];
      }
  }
  if (!ok) atomicOr(bad, 1);
}

template <class Track>
__device__ __forceinline__ void solve_and_store(Track &trk, const Params &prm, int64_t t, const Out &out) {
  double X[3] = {NAN, NAN, NAN};
  int iterations = 0;
  int status = kOk;
  if (out.initial) {
    for (int k = 0; k < 3; k++) X[k] = out.initial[3 * t + k];
    iterations = refine(trk, prm.iterations, X);
  } else {
    status = triangulate_track(trk, prm, X, &iterations);
  }
  if (trk.lane != 0) return;
  for (int k = 0; k < 3; k++) out.points[3 * t + k] = X[k];
  out.status[t] = (uint8_t)status;
  out.iterations[t] = iterations;
}

template <class Rows>
__global__ __launch_bounds__(kBlock) void tri_group_kernel(Rows rows, const int64_t *__restrict__ offsets, int n_tracks, Params prm, Out out) {
  __shared__ double sh[6 * kGroupsPerBlock * kGroupPitch];
  const int g = (int)threadIdx.x / kGroup, lane = (int)threadIdx.x % kGroup;
  const int64_t t = (int64_t)blockIdx.x * kGroupsPerBlock + g;
  const int64_t row0 = t < n_tracks ? offsets[t] : 0;
  const int64_t len = t < n_tracks ? offsets[t + 1] - row0 : 0;
  const bool mine = t < n_tracks && len <= kGroupObs;  // the same on every lane of the group
  const int n = mine ? (int)len : 0;
  constexpr int plane = kGroupsPerBlock * kGroupPitch;
  double *slice = sh + g * kGroupPitch;
  stage<kGroup>(rows, row0, n, kGroupObs, lane, slice, plane, out.bad);
  __syncthreads();
  if (!mine) return;
  LaneTrack<kGroup, false, Rows> trk{n, lane, kGroupObs, plane, slice, rows, row0};
  solve_and_store(trk, prm, t, out);
}

template <class Rows>
__global__ __launch_bounds__(kWave) void tri_wave_kernel(Rows rows, const int64_t *__restrict__ offsets, const int32_t *__restrict__ long_tracks,
                                                         Params prm, Out out) {
  __shared__ double sh[6 * kWaveObs];
  const int lane = (int)threadIdx.x;
  const int64_t t = long_tracks[blockIdx.x];
  const int64_t row0 = offsets[t];
  const int n = (int)(offsets[t + 1] - row0);
  stage<kWave>(rows, row0, n, kWaveObs, lane, sh, kWaveObs, out.bad);
  __syncthreads();
  LaneTrack<kWave, true, Rows> trk{n, lane, kWaveObs, kWaveObs, sh, rows, row0};
  solve_and_store(trk, prm, t, out);
}

// ---- ROBUST ----
// LaneTrack plus the two masks of triangulate_robust.h; Overhang says which kernel: the word in a register or in LDS
template <int G, bool Overhang, class Rows>
struct RobustLaneTrack : LaneTrack<G, Overhang, Rows> {
  uint32_t reg;    // group kernel: this lane's mask word
  uint32_t *word;  // wavefront kernel: this lane's mask word in LDS
  uint8_t *bytes;  // wavefront kernel: the track's bytes of the output mask, bit `which` of byte i for i >= cap
  __device__ __forceinline__ bool bit(int which, int i) const {
    if (Overhang && i >= this->cap) return (bytes[i] >> which) & 1;
    return ((Overhang ? *word : reg) >> (16 * which + i / G)) & 1;
  }
  __device__ __forceinline__ void set_bit(int which, int i, bool b) {
    if (Overhang && i >= this->cap) {
      bytes[i] = (uint8_t)((bytes[i] & ~(1 << which)) | ((b ? 1 : 0) << which));
      return;
    }
    const uint32_t m = 1u << (16 * which + i / G);
    if (Overhang)
      *word = b ? (*word | m) : (*word & ~m);
    else
      reg = b ? (reg | m) : (reg & ~m);
  }
};
static_assert(kGroupObs / kGroup <= 16 && kWaveObs / kWave <= 16, "a mask has 16 bits per lane");

struct RobustOut {
  double *points;
  uint8_t *status, *mask;
  int32_t *n_inliers, *tries;
  int *bad;              // set when a row could not be evaluated or a draw lies outside [0, 1)
  const double *draws;   // n_tracks x 11, or null: robust_draw(seed, t, k)
  uint64_t seed;
};

template <class Track>
__device__ __forceinline__ void solve_and_store_robust(Track &trk, const Params &prm, int64_t t, int64_t row0, const RobustOut &out) {
  double X[3] = {NAN, NAN, NAN};
  int n_inliers = 0, tries = 0;
  const Draws11 draw{out.draws ? out.draws + kRobustTries * t : nullptr, out.seed, t};
  int status = triangulate_track_robust(trk, prm, draw, X, &n_inliers, &tries);
  if (status == kBadDraws) {
    if (trk.lane == 0) atomicOr(out.bad, 1);
    status = kNoConsensus;
  }
  for (int i = trk.first(); i < trk.n; i += trk.stride()) out.mask[row0 + i] = (status == kOk && trk.bit(kBest, i)) ? 1 : 0;
  if (trk.lane != 0) return;
  for (int k = 0; k < 3; k++) out.points[3 * t + k] = X[k];
  out.status[t] = (uint8_t)status;
  out.n_inliers[t] = n_inliers;
  out.tries[t] = tries;
}

template <class Rows>
__global__ __launch_bounds__(kBlock) void tri_group_robust_kernel(Rows rows, const int64_t *__restrict__ offsets, int n_tracks, Params prm,
                                                                  RobustOut out) {
  __shared__ double sh[6 * kGroupsPerBlock * kGroupPitch];
  const int g = (int)threadIdx.x / kGroup, lane = (int)threadIdx.x % kGroup;
  const int64_t t = (int64_t)blockIdx.x * kGroupsPerBlock + g;
  const int64_t row0 = t < n_tracks ? offsets[t] : 0;
  const int64_t len = t < n_tracks ? offsets[t + 1] - row0 : 0;
  const bool mine = t < n_tracks && len <= kGroupObs;  // the same on every lane of the group
  const int n = mine ? (int)len : 0;
  constexpr int plane = kGroupsPerBlock * kGroupPitch;
  double *slice = sh + g * kGroupPitch;
  stage<kGroup>(rows, row0, n, kGroupObs, lane, slice, plane, out.bad);
  __syncthreads();
  if (!mine) return;
  RobustLaneTrack<kGroup, false, Rows> trk{{n, lane, kGroupObs, plane, slice, rows, row0}, 0u, nullptr, nullptr};
  solve_and_store_robust(trk, prm, t, row0, out);
}

template <class Rows>
__global__ __launch_bounds__(kWave) void tri_wave_robust_kernel(Rows rows, const int64_t *__restrict__ offsets,
                                                                const int32_t *__restrict__ long_tracks, Params prm, RobustOut out) {
  __shared__ double sh[6 * kWaveObs];
  __shared__ uint32_t words[kWave];
  const int lane = (int)threadIdx.x;
  const int64_t t = long_tracks[blockIdx.x];
  const int64_t row0 = offsets[t];
  const int n = (int)(offsets[t + 1] - row0);
  stage<kWave>(rows, row0, n, kWaveObs, lane, sh, kWaveObs, out.bad);
  words[lane] = 0u;
  __syncthreads();
  RobustLaneTrack<kWave, true, Rows> trk{{n, lane, kWaveObs, kWaveObs, sh, rows, row0}, 0u, words + lane, out.mask + row0};
  solve_and_store_robust(trk, prm, t, row0, out);
}

int check_args(const int64_t *offsets, int n_tracks, const osfm_triangulate_params *p, const char *who) {
  OSFM_REQUIRE(p, OSFM_E_INVALID, "%s: null params", who);
  OSFM_REQUIRE(n_tracks >= 0, OSFM_E_INVALID, "%s: n_tracks < 0", who);
  OSFM_REQUIRE(p->refinement_iterations >= 0, OSFM_E_INVALID, "%s: refinement_iterations < 0", who);
  OSFM_REQUIRE(p->min_angle_deg >= 0.0 && p->min_angle_deg <= 180.0, OSFM_E_INVALID, "%s: min_angle_deg must lie in [0, 180]", who);
  OSFM_REQUIRE(!(p->threshold != p->threshold) && !(p->min_depth != p->min_depth), OSFM_E_INVALID, "%s: threshold / min_depth is NaN", who);
  if (n_tracks == 0) return OSFM_OK;
  OSFM_REQUIRE(offsets, OSFM_E_INVALID, "%s: null track_offsets", who);
  OSFM_REQUIRE(offsets[0] == 0, OSFM_E_INVALID, "%s: track_offsets[0] must be 0", who);
  for (int t = 0; t < n_tracks; t++) {
    OSFM_REQUIRE(offsets[t + 1] >= offsets[t], OSFM_E_INVALID, "%s: track_offsets decrease at track %d", who, t);
    OSFM_REQUIRE(offsets[t + 1] - offsets[t] <= kMaxTrack, OSFM_E_UNSUPPORTED, "%s: track %d has more than 2^24 observations", who, t);
  }
  return OSFM_OK;
}

// the tracks of the wavefront kernel
std::vector<int32_t> split_long(const int64_t *offsets, int n_tracks) {
  std::vector<int32_t> long_tracks;
  for (int t = 0; t < n_tracks; t++)
    if (offsets[t + 1] - offsets[t] > kGroupObs) long_tracks.push_back(t);
  return long_tracks;
}

// What the plain and the robust call differ in on the host side: the struct the kernels write through and its buffers in the arena,
// the optional input (`initial` / `draws`), the mask, the pair of kernels, the way back and what a refusal says.
struct PlainCall {
  using DeviceOut = Out;
  template <class Rows>
  static constexpr auto group_kernel = &tri_group_kernel<Rows>;
  template <class Rows>
  static constexpr auto wave_kernel = &tri_wave_kernel<Rows>;
  static constexpr const char *refusal = "%s: an observation names a shot outside the table, or it or its shot's pose is not finite";
  const double *initial;  // n_tracks x 3, or null
  double *points;
  uint8_t *status;
  int32_t *iterations_used;
  OsfmArena::Slot<double> d_points, d_initial;
  OsfmArena::Slot<uint8_t> d_status;
  OsfmArena::Slot<int32_t> d_iterations;
  int check(int64_t, const char *who) const {
    OSFM_REQUIRE(points && status && iterations_used, OSFM_E_INVALID, "%s: null points / status / iterations_used", who);
    return OSFM_OK;
  }
  void declare(OsfmArena &A, size_t n_tracks, size_t) {
    d_points = A.add<double>(3 * n_tracks);
    d_status = A.add<uint8_t>(n_tracks);
    d_iterations = A.add<int32_t>(n_tracks);
    d_initial = A.add<double>(initial ? 3 * n_tracks : 0);
  }
  int stage(const OsfmArena &A, int *d_bad, hipStream_t st, Out *out) const {
    OSFM_HIP(A.upload(d_initial, initial, st));
    *out = Out{d_points, d_status, d_iterations, d_bad, initial ? d_initial.get() : nullptr};
    return OSFM_OK;
  }
  int fetch(const Out &out, hipStream_t st) const {
    OSFM_HIP(hipMemcpyAsync(points, out.points, d_points.bytes, hipMemcpyDeviceToHost, st));
    OSFM_HIP(hipMemcpyAsync(status, out.status, d_status.bytes, hipMemcpyDeviceToHost, st));
    OSFM_HIP(hipMemcpyAsync(iterations_used, out.iterations, d_iterations.bytes, hipMemcpyDeviceToHost, st));
    return OSFM_OK;
  }
};

struct RobustCall {
  using DeviceOut = RobustOut;
  template <class Rows>
  static constexpr auto group_kernel = &tri_group_robust_kernel<Rows>;
  template <class Rows>
  static constexpr auto wave_kernel = &tri_wave_robust_kernel<Rows>;
  static constexpr const char *refusal =
      "%s: an observation names a shot outside the table, it or its shot's pose is not finite, or a draw lies outside [0, 1)";
  const double *draws;  // n_tracks x 11, or null
  uint64_t seed;
  double *points;
  uint8_t *status, *inlier_mask;
  int32_t *n_inliers, *tries_used;
  OsfmArena::Slot<double> d_points, d_draws;
  OsfmArena::Slot<uint8_t> d_status, d_mask;
  OsfmArena::Slot<int32_t> d_inliers, d_tries;
  int check(int64_t n_obs, const char *who) const {
    OSFM_REQUIRE(points && status && n_inliers && tries_used, OSFM_E_INVALID, "%s: null points / status / n_inliers / tries_used", who);
    OSFM_REQUIRE(n_obs == 0 || inlier_mask, OSFM_E_INVALID, "%s: null inlier_mask", who);
    return OSFM_OK;
  }
  void declare(OsfmArena &A, size_t n_tracks, size_t n_obs) {
    d_points = A.add<double>(3 * n_tracks);
    d_status = A.add<uint8_t>(n_tracks);
    d_inliers = A.add<int32_t>(n_tracks);
    d_tries = A.add<int32_t>(n_tracks);
    d_mask = A.add<uint8_t>(n_obs);
    d_draws = A.add<double>(draws ? kRobustTries * n_tracks : 0);
  }
  int stage(const OsfmArena &A, int *d_bad, hipStream_t st, RobustOut *out) const {
    OSFM_HIP(A.upload(d_draws, draws, st));
    if (d_mask.bytes) OSFM_HIP(hipMemsetAsync(d_mask, 0, d_mask.bytes, st));
    *out = RobustOut{d_points, d_status, d_mask, d_inliers, d_tries, d_bad, draws ? d_draws.get() : nullptr, seed};
    return OSFM_OK;
  }
  int fetch(const RobustOut &out, hipStream_t st) const {
    OSFM_HIP(hipMemcpyAsync(points, out.points, d_points.bytes, hipMemcpyDeviceToHost, st));
    OSFM_HIP(hipMemcpyAsync(status, out.status, d_status.bytes, hipMemcpyDeviceToHost, st));
    OSFM_HIP(hipMemcpyAsync(n_inliers, out.n_inliers, d_inliers.bytes, hipMemcpyDeviceToHost, st));
    OSFM_HIP(hipMemcpyAsync(tries_used, out.tries, d_tries.bytes, hipMemcpyDeviceToHost, st));
    if (d_mask.bytes) OSFM_HIP(hipMemcpyAsync(inlier_mask, out.mask, d_mask.bytes, hipMemcpyDeviceToHost, st));
    return OSFM_OK;
  }
};

// Both kernels of `call` over rows that are on the device already.  The caller holds the context lock and has recorded nothing on
// ev[0] / ev[1].
template <class Rows, class Call>
int run_device(osfm_ctx *ctx, hipStream_t st, const Rows &rows, const int64_t *offsets, int n_tracks, const osfm_triangulate_params *p, Call call,
               double *kernel_ms, const char *who) {
  const std::vector<int32_t> long_tracks = split_long(offsets, n_tracks);
  const size_t n_long = long_tracks.size();
  OsfmArena A;
  const auto d_off = A.add<int64_t>((size_t)n_tracks + 1);
  const auto d_long = A.add<int32_t>(n_long);
  const auto d_bad = A.add<int>(4);
  call.declare(A, (size_t)n_tracks, (size_t)offsets[n_tracks]);
  OSFM_HIP(A.alloc(ctx));
  typename Call::DeviceOut out;
  OSFM_TRY(call.stage(A, d_bad, st, &out));
  OSFM_HIP(A.upload(d_off, offsets, st));
  OSFM_HIP(A.upload(d_long, long_tracks.data(), st));
  OSFM_HIP(hipMemsetAsync(out.bad, 0, d_bad.bytes, st));
  const Params prm{p->threshold, p->min_angle_deg * M_PI / 180.0, p->min_depth, (int)p->refinement_iterations};
  OSFM_HIP(hipEventRecord(ctx->ev[0], st));
  if (n_long < (size_t)n_tracks) {
    hipLaunchKernelGGL((Call::template group_kernel<Rows>), dim3((unsigned)((n_tracks + kGroupsPerBlock - 1) / kGroupsPerBlock)), dim3(kBlock), 0, st,
                       rows, d_off, n_tracks, prm, out);
    OSFM_HIP(hipGetLastError());
  }
  if (n_long) {
    hipLaunchKernelGGL((Call::template wave_kernel<Rows>), dim3((unsigned)n_long), dim3(kWave), 0, st, rows, d_off, d_long, prm, out);
    OSFM_HIP(hipGetLastError());
  }
  OSFM_HIP(hipEventRecord(ctx->ev[1], st));
  int bad = 0;
  OSFM_HIP(hipMemcpyAsync(&bad, out.bad, 4, hipMemcpyDeviceToHost, st));
  OSFM_TRY(call.fetch(out, st));
  OSFM_HIP(hipStreamSynchronize(st));
  OSFM_TRY(osfm_kernel_ms(ctx, kernel_ms));
  OSFM_REQUIRE(bad == 0, OSFM_E_INVALID, Call::refusal, who);
  return OSFM_OK;
}

// the tables and rows of a pixel call, checked and on their way to the device (the caller holds the context lock; `in` owns the memory)
int upload_pixel_rows(osfm_ctx *ctx, const double *shot_pose, const int32_t *shot_camera, int n_shots, const int32_t *cam_model,
                      const double *cam_params, int n_cams, const int32_t *obs_shot, const double *obs_xy, int64_t n_obs, OsfmArena &in,
                      PixelRows *rows, const char *who) {
  OSFM_REQUIRE(n_obs == 0 || (shot_pose && shot_camera && cam_model && cam_params && obs_shot && obs_xy && n_shots > 0 && n_cams > 0),
               OSFM_E_INVALID, "%s: null argument", who);
  OSFM_TRY(osfm_check_camera_table(cam_model, n_cams, shot_camera, n_shots, 1, "shot", who));
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const auto d_pose = in.add<double>((size_t)n_shots * 12);
  const auto d_shot_camera = in.add<int32_t>((size_t)n_shots);
  const auto d_cam_model = in.add<int32_t>((size_t)n_cams);
  const auto d_cam_params = in.add<double>((size_t)n_cams * 16);
  const auto d_obs_shot = in.add<int32_t>((size_t)n_obs);
  const auto d_obs_xy = in.add<double>((size_t)n_obs * 2);
  OSFM_HIP(in.alloc(ctx));
  OSFM_HIP(in.upload(d_pose, shot_pose, st));
  OSFM_HIP(in.upload(d_shot_camera, shot_camera, st));
  OSFM_HIP(in.upload(d_cam_model, cam_model, st));
  OSFM_HIP(in.upload(d_cam_params, cam_params, st));
  OSFM_HIP(in.upload(d_obs_shot, obs_shot, st));
  OSFM_HIP(in.upload(d_obs_xy, obs_xy, st));
  *rows = PixelRows{d_pose, d_shot_camera, d_cam_model, d_cam_params, d_obs_shot, d_obs_xy, n_shots};
  return OSFM_OK;
}

// an entry point over bearings: the checks, centers and bearings to the device, then both kernels of `call`
template <class Call>
int bearings_call(osfm_ctx *ctx, const double *centers, const double *bearings, const int64_t *track_offsets, int n_tracks,
                  const osfm_triangulate_params *params, const Call &call, double *kernel_ms, const char *who) {
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_REQUIRE(ctx, OSFM_E_INVALID, "%s: null context", who);
  OSFM_TRY(check_args(track_offsets, n_tracks, params, who));
  if (n_tracks == 0) return OSFM_OK;
  const int64_t n_obs = track_offsets[n_tracks];
  OSFM_TRY(call.check(n_obs, who));
  OSFM_REQUIRE(n_obs == 0 || (centers && bearings), OSFM_E_INVALID, "%s: null centers / bearings", who);
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmArena in;
  const auto d_centers = in.add<double>((size_t)n_obs * 3), d_bearings = in.add<double>((size_t)n_obs * 3);
  OSFM_HIP(in.alloc(ctx));
  OSFM_HIP(in.upload(d_centers, centers, st));
  OSFM_HIP(in.upload(d_bearings, bearings, st));
  return run_device(ctx, st, BearingRows{d_centers, d_bearings}, track_offsets, n_tracks, params, call, kernel_ms, who);
}

// an entry point over pixels: the checks, the tables and observations to the device, then both kernels of `call`
template <class Call>
int tracks_call(osfm_ctx *ctx, const double *shot_pose, const int32_t *shot_camera, int n_shots, const int32_t *cam_model, const double *cam_params,
                int n_cams, const int32_t *obs_shot, const double *obs_xy, const int64_t *track_offsets, int n_tracks,
                const osfm_triangulate_params *params, const Call &call, double *kernel_ms, const char *who) {
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_REQUIRE(ctx, OSFM_E_INVALID, "%s: null context", who);
  OSFM_TRY(check_args(track_offsets, n_tracks, params, who));
  OSFM_REQUIRE(n_shots >= 0 && n_cams >= 0, OSFM_E_INVALID, "%s: negative size", who);
  if (n_tracks == 0) return OSFM_OK;
  const int64_t n_obs = track_offsets[n_tracks];
  OSFM_TRY(call.check(n_obs, who));
  OSFM_CTX_LOCK(ctx);
  PixelRows rows;
  OsfmArena in;
  OSFM_TRY(upload_pixel_rows(ctx, shot_pose, shot_camera, n_shots, cam_model, cam_params, n_cams, obs_shot, obs_xy, n_obs, in, &rows, who));
  return run_device(ctx, ctx->stream, rows, track_offsets, n_tracks, params, call, kernel_ms, who);
}

}  // namespace

extern "C" void osfm_triangulate_params_default(osfm_triangulate_params *p) {
  if (!p) return;
  p->threshold = 0.006;
  p->min_angle_deg = 1.0;
  p->min_depth = 0.001;
  p->refinement_iterations = 10;
  p->pad = 0;
}

extern "C" int osfm_triangulate_bearings(osfm_ctx *ctx, const double *centers, const double *bearings, const int64_t *track_offsets, int n_tracks,
                                         const osfm_triangulate_params *params, double *points, uint8_t *status, int32_t *iterations_used,
                                         double *kernel_ms) {
  return bearings_call(ctx, centers, bearings, track_offsets, n_tracks, params, PlainCall{nullptr, points, status, iterations_used}, kernel_ms,
                       "osfm_triangulate_bearings");
}

extern "C" int osfm_triangulate_tracks(osfm_ctx *ctx, const double *shot_pose, const int32_t *shot_camera, int n_shots, const int32_t *cam_model,
                                       const double *cam_params, int n_cams, const int32_t *obs_shot, const double *obs_xy,
                                       const int64_t *track_offsets, int n_tracks, const osfm_triangulate_params *params, double *points,
                                       uint8_t *status, int32_t *iterations_used, double *kernel_ms) {
  return tracks_call(ctx, shot_pose, shot_camera, n_shots, cam_model, cam_params, n_cams, obs_shot, obs_xy, track_offsets, n_tracks, params,
                     PlainCall{nullptr, points, status, iterations_used}, kernel_ms, "osfm_triangulate_tracks");
}

extern "C" int osfm_triangulate_refine(osfm_ctx *ctx, const double *centers, const double *bearings, const int64_t *track_offsets, int n_tracks,
                                       const double *initial, int refinement_iterations, double *points, int32_t *iterations_used,
                                       double *kernel_ms) {
  const char *who = "osfm_triangulate_refine";
  osfm_triangulate_params p;
  osfm_triangulate_params_default(&p);
  p.refinement_iterations = refinement_iterations;
  OSFM_REQUIRE(n_tracks <= 0 || initial, OSFM_E_INVALID, "%s: null initial points", who);
  std::vector<uint8_t> status((size_t)(n_tracks > 0 ? n_tracks : 0));
  return bearings_call(ctx, centers, bearings, track_offsets, n_tracks, &p, PlainCall{n_tracks > 0 ? initial : nullptr, points, status.data(), iterations_used},
                       kernel_ms, who);
}

extern "C" int osfm_triangulate_bearings_robust(osfm_ctx *ctx, const double *centers, const double *bearings, const int64_t *track_offsets,
                                                int n_tracks, const osfm_triangulate_params *params, const double *draws, uint64_t seed,
                                                double *points, uint8_t *status, uint8_t *inlier_mask, int32_t *n_inliers, int32_t *tries_used,
                                                double *kernel_ms) {
  return bearings_call(ctx, centers, bearings, track_offsets, n_tracks, params,
                       RobustCall{draws, seed, points, status, inlier_mask, n_inliers, tries_used}, kernel_ms, "osfm_triangulate_bearings_robust");
}

extern "C" int osfm_triangulate_tracks_robust(osfm_ctx *ctx, const double *shot_pose, const int32_t *shot_camera, int n_shots,
                                              const int32_t *cam_model, const double *cam_params, int n_cams, const int32_t *obs_shot,
                                              const double *obs_xy, const int64_t *track_offsets, int n_tracks,
                                              const osfm_triangulate_params *params, const double *draws, uint64_t seed, double *points,
                                              uint8_t *status, uint8_t *inlier_mask, int32_t *n_inliers, int32_t *tries_used, double *kernel_ms) {
  return tracks_call(ctx, shot_pose, shot_camera, n_shots, cam_model, cam_params, n_cams, obs_shot, obs_xy, track_offsets, n_tracks, params,
                     RobustCall{draws, seed, points, status, inlier_mask, n_inliers, tries_used}, kernel_ms, "osfm_triangulate_tracks_robust");
}
