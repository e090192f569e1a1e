// cloud.hip -- culling of the final point cloud on gfx950: the two filters grow_reconstruction runs after its last bundle
// (opensfm/reconstruction.py:1590-1594 -> sfm/src/map_helpers.cc).
//
// osfm_points_conditioning (FilterBadlyConditionedPoints + ComputePointInverseCovariance)
//   host    stable counting sort of the observations by landmark (ascending input order inside a landmark);
//   cond_obs_kernel       one thread per sorted observation: the unit ray normalize(X - origin) and the six distinct entries of J^T J
//                         (J = camera-frame Jacobian of ba_math.h times R; the spherical one written out here), stored SoA -- the work
//                         per thread does not depend on the track length;
//   cond_landmark_kernel  a group of kGroup = 8 lanes per landmark (eight landmarks per wavefront): the pair-angle search with the outer
//                         index split across the lanes and a group-wide "found" after every block of eight outer indices, the ordered sum
//                         of the J^T J entries (lane l takes observations l, l + 8, ..., then a three-step butterfly: a fixed order, no
//                         atomics), and on every lane the determinant, the cyclic Jacobi and cond;
//   host    mean / sigma / threshold sequentially in landmark order (std::accumulate in the reference).
//
// osfm_points_isolation (RemoveIsolatedPoints)
//   host    float32 cast, a uniform grid over the 2 % .. 98 % box of every axis (points outside it are clamped into the border cells, so a
//           few far points do not blow the cells up), counting sort of the points by cell;
//   knn_ring_kernel      one thread per query in cell order, the k + 1 best distances in registers (statically indexed insertion list),
//                        Chebyshev rings of cells outward; a query stops after ring r when its (k + 1)-th distance is below
//                        (0.99 r h)^2 -- everything unvisited is at least r h away along one axis -- or when the rings covered the grid;
//   knn_brute_kernel     the queries still open after kRingBudget rings (compacted list): one wavefront per query over all points, then a
//                        k + 1 round merge of the 64 lanes' lists;
//   host    mean / sigma / threshold sequentially in input order.
#include <math.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ba_math.h"
#include "osfm_internal.h"

namespace {

constexpr int kGroup = 8;       // lanes per landmark
constexpr int kBlock = 256;
constexpr int kRingBudget = 4;  // rings 0 .. 4 (9^3 cells) before a query goes to the brute-force pass
constexpr double kMaxCond = 1000.0;

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }

// ------------------------------------------------------------------------------------------------------------------------------
// conditioning
// ------------------------------------------------------------------------------------------------------------------------------
// derivative of SphericalProjection::Forward (camera_projections_functions.h:214-223: lon = atan2(x, z), lat = atan2(-y, hypot(x, z)),
// (lon, -lat) / 2 pi) with respect to the camera-frame point
__device__ __forceinline__ void spherical_jacobian(const double *Xc, double *J) {
  const double x = Xc[0], y = Xc[1], z = Xc[2];
  const double rt2 = x * x + z * z, rt = sqrt(rt2), R2 = rt2 + y * y;
  const double two_pi = 2.0 * M_PI;
  J[0] = z / (two_pi * rt2);
  J[1] = 0.0;
  J[2] = -x / (two_pi * rt2);
  J[3] = -(x * y) / (two_pi * R2 * rt);
  J[4] = rt / (two_pi * R2);
  J[5] = -(y * z) / (two_pi * R2 * rt);
}

__global__ __launch_bounds__(kBlock) void cond_obs_kernel(const double *__restrict__ points, const double *__restrict__ shot_pose,
                                                          const int32_t *__restrict__ shot_camera, const int32_t *__restrict__ cam_model,
                                                          const double *__restrict__ cam_params, const int32_t *__restrict__ s_shot,
                                                          const int32_t *__restrict__ s_point, int64_t n_obs, double *__restrict__ rays,
                                                          double *__restrict__ jtj) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_obs) return;
  const int s = s_shot[i];
  const double *X = points + 3 * (size_t)s_point[i];
  const double *P = shot_pose + 12 * (size_t)s;
  double R[9], t[3];
  for (int k = 0; k < 9; k++) R[k] = P[k];
  for (int k = 0; k < 3; k++) t[k] = P[9 + k];
  // Pose::GetOrigin: -R^T t
  double d[3], Xc[3];
  for (int k = 0; k < 3; k++) d[k] = X[k] - (-(R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2]));
  const double n2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  if (n2 > 0.0) {  // Eigen's normalized(): a zero vector stays zero
    const double n = sqrt(n2);
    for (int k = 0; k < 3; k++) d[k] = d[k] / n;
  }
  for (int k = 0; k < 3; k++) rays[(size_t)k * n_obs + i] = d[k];
  for (int k = 0; k < 3; k++) Xc[k] = R[3 * k] * X[0] + R[3 * k + 1] * X[1] + R[3 * k + 2] * X[2] + t[k];
  const int c = shot_camera[s], model = cam_model[c];
  double Jc[6], out[2];
  if (model == OSFM_CAMERA_SPHERICAL)
    spherical_jacobian(Xc, Jc);
  else
    osfm_ba::project_generic<true>(model, cam_params + 16 * (size_t)c, Xc, out, Jc);
  double J[6];  // 2 x 3 with respect to the world point: Jc R
  for (int r = 0; r < 2; r++)
    for (int k = 0; k < 3; k++) J[3 * r + k] = Jc[3 * r] * R[k] + Jc[3 * r + 1] * R[3 + k] + Jc[3 * r + 2] * R[6 + k];
  int e = 0;
  for (int a = 0; a < 3; a++)
    for (int b = a; b < 3; b++, e++) jtj[(size_t)e * n_obs + i] = J[a] * J[b] + J[3 + a] * J[3 + b];  // 00 01 02 11 12 22
}

template <class T>
__device__ __forceinline__ T group_xor(T v, int mask) {
  return __shfl_xor(v, mask, 64);
}

// geometry::AngleBetweenVectors(u, v) > rad (triangulation.cc:66-73): acos only where the cosine is within 1e-9 of cos(rad) -- acos is
// monotone with |d acos / dc| >= 1, so outside that band the comparison is decided by the cosine
__device__ __forceinline__ bool angle_exceeds(const double *u, const double *v, double rad, double cosr) {
  const double c = (u[0] * v[0] + u[1] * v[1] + u[2] * v[2]) /
                   sqrt((u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
  if (fabs(c) >= 1.0) return 0.0 > rad;
  if (c > cosr + 1e-9) return false;
  if (c < cosr - 1e-9) return true;
  return acos(c) > rad;  // (a NaN cosine lands here: false)
}

// eigenvalues of the symmetric 3 x 3 (a00 a01 a02 a11 a12 a22) by cyclic Jacobi: smallest and largest
__device__ __forceinline__ void sym3_extreme_eigenvalues(const double *h, double *lo, double *hi) {
  double a[3][3] = {{h[0], h[1], h[2]}, {h[1], h[3], h[4]}, {h[2], h[4], h[5]}};
  for (int sweep = 0; sweep < 16; sweep++) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    if (!(off > 1e-18 * (fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2])))) break;
#pragma unroll
    for (int pq = 0; pq < 3; pq++) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2, r = 3 - p - q;
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
      a[p][p] -= tt * apq;
      a[q][q] += tt * apq;
      a[p][q] = a[q][p] = 0.0;
      const double arp = a[r][p], arq = a[r][q];
      a[r][p] = a[p][r] = c * arp - s * arq;
      a[r][q] = a[q][r] = s * arp + c * arq;
    }
  }
  *lo = fmin(a[0][0], fmin(a[1][1], a[2][2]));
  *hi = fmax(a[0][0], fmax(a[1][1], a[2][2]));
  if (!(finite_d(a[0][0]) && finite_d(a[1][1]) && finite_d(a[2][2]))) *lo = *hi = NAN;
}

__global__ __launch_bounds__(kBlock) void cond_landmark_kernel(const int64_t *__restrict__ start, const double *__restrict__ rays,
                                                               const double *__restrict__ jtj, int64_t n_obs, int n_points, double rad, double cosr,
                                                               double min_abs_det, double *__restrict__ cond, uint8_t *__restrict__ reason) {
  const int64_t lm = (int64_t)blockIdx.x * (kBlock / kGroup) + threadIdx.x / kGroup;
  const int lane = (int)threadIdx.x % kGroup;
  const bool live = lm < n_points;
  const int64_t b = live ? start[lm] : 0;
  const int L = live ? (int)(start[lm + 1] - b) : 0;  // the same on every lane of the group
  const double *rx = rays + b, *ry = rays + n_obs + b, *rz = rays + 2 * n_obs + b;
  // some pair of rays wider than the limit?  lane l takes the outer indices l, l + 8, ...; the group agrees after every block of eight
  int found = 0;
  for (int base = 0; base + 1 < L; base += kGroup) {
    const int i = base + lane;
    if (i + 1 < L) {
      const double u[3] = {rx[i], ry[i], rz[i]};
      for (int j = i + 1; j < L; j++) {
        const double v[3] = {rx[j], ry[j], rz[j]};
        if (angle_exceeds(u, v, rad, cosr)) {
          found = 1;
          break;
        }
      }
    }
    for (int m = 1; m < kGroup; m <<= 1) found |= group_xor(found, m);
    if (found) break;
  }
  // H = sum J^T J: lane l sums its observations in ascending order, then the butterfly -- the same order in every run
  double h[6] = {0, 0, 0, 0, 0, 0};
  for (int i = lane; i < L; i += kGroup)
    for (int e = 0; e < 6; e++) h[e] += jtj[(size_t)e * n_obs + b + i];
  for (int m = 1; m < kGroup; m <<= 1)
    for (int e = 0; e < 6; e++) h[e] += group_xor(h[e], m);
  if (!live || lane != 0) return;
  double cnd = NAN;
  uint8_t why = 0;
  bool fin = true;
  for (int e = 0; e < 6; e++) fin = fin && finite_d(h[e]);
  if (!found) {
    why = 1;
  } else if (!fin) {
    why = 2;
  } else {
    // Eigen's 3 x 3 determinant (bruteforce_det3_helper): sum of m(0, a) (m(1, b) m(2, c) - m(1, c) m(2, b))
    const double det = h[0] * (h[3] * h[5] - h[4] * h[4]) - h[1] * (h[1] * h[5] - h[4] * h[2]) + h[2] * (h[1] * h[4] - h[3] * h[2]);
    if (!finite_d(det) || fabs(det) < min_abs_det) {
      why = 3;
    } else {
      double lo, hi;
      sym3_extreme_eigenvalues(h, &lo, &hi);
      if (!(lo > 0.0) || !finite_d(lo) || !finite_d(hi)) {
        why = 4;
      } else {
        cnd = fmin(sqrt(hi / lo), kMaxCond);
        if (!finite_d(cnd)) {
          cnd = NAN;
          why = 4;
        }
      }
    }
  }
  cond[lm] = cnd;
  reason[lm] = why;
}

// ------------------------------------------------------------------------------------------------------------------------------
// isolation
// ------------------------------------------------------------------------------------------------------------------------------
struct Grid {
  float lo[3];
  int n[3];
  double h;
};
struct __attribute__((aligned(16))) CellPoint {  // one 16-byte load
  float x, y, z;
  int32_t index;  // of the point in the caller's order
};
static_assert(sizeof(CellPoint) == 16, "CellPoint is loaded as one dwordx4");

// squared L2 distance in float32 as vl_kdtree's distance function accumulates it on a build without FMA: ((dx*dx) + dy*dy) + dz*dz
__device__ __forceinline__ float dist2_f32(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  float acc = dx * dx;
  acc = acc + dy * dy;
  acc = acc + dz * dz;
  return acc;
}

// The k1 = k + 1 smallest values seen, ascending in v[CAP - k1 .. CAP - 1]; the slots below hold -inf, which stops the insertion's
// compare-and-swap chain, so every index is a compile-time constant and the list stays in registers.
template <int CAP>
struct Best {
  float v[CAP];
  __device__ __forceinline__ void init(int k1) {
#pragma unroll
    for (int i = 0; i < CAP; i++) v[i] = i < CAP - k1 ? -INFINITY : INFINITY;
  }
  __device__ __forceinline__ float worst() const { return v[CAP - 1]; }
  __device__ __forceinline__ void insert(float d) {
    if (!(d < v[CAP - 1])) return;
    v[CAP - 1] = d;
#pragma unroll
    for (int i = CAP - 1; i > 0; i--) {
      const float hi = v[i], lo = v[i - 1];
      const bool sw = hi < lo;
      v[i] = sw ? lo : hi;
      v[i - 1] = sw ? hi : lo;
    }
  }
  // the smallest dropped, the other k summed in ascending order in float64, divided by k
  __device__ __forceinline__ double average(int k1) const {
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < CAP; i++)
      if (i > CAP - k1) sum += (double)v[i];
    return sum / (double)(k1 - 1);
  }
};

template <int CAP>
__global__ __launch_bounds__(kBlock) void knn_ring_kernel(const CellPoint *__restrict__ pts /* sorted by cell */,
                                                          const int32_t *__restrict__ cell_start, Grid g, int n, int k1,
                                                          double *__restrict__ avg, int32_t *__restrict__ open_list, int32_t *__restrict__ open_count) {
  const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (q >= n) return;
  const CellPoint me = pts[q];
  int c[3];
  {
    const float p[3] = {me.x, me.y, me.z};
    for (int a = 0; a < 3; a++) {
      const double t = ((double)p[a] - (double)g.lo[a]) / g.h;
      c[a] = g.n[a] == 1 || !(t > 0.0) ? 0 : t >= (double)g.n[a] ? g.n[a] - 1 : (int)t;
    }
  }
  Best<CAP> best;
  best.init(k1);
  bool done = false;
  for (int r = 0; r <= kRingBudget && !done; r++) {
    for (int dz = -r; dz <= r; dz++) {
      const int z = c[2] + dz;
      if (z < 0 || z >= g.n[2]) continue;
      for (int dy = -r; dy <= r; dy++) {
        const int y = c[1] + dy;
        if (y < 0 || y >= g.n[1]) continue;
        const int row = (z * g.n[1] + y) * g.n[0];
        const bool shell = dz == -r || dz == r || dy == -r || dy == r;
        // a shell row is one run of cells (x is the fastest index: their points are contiguous); an inner row has the two end cells
        const int x0 = c[0] - r, x1 = c[0] + r;
        for (int part = 0; part < (shell ? 1 : 2); part++) {
          int xa = shell ? x0 : (part == 0 ? x0 : x1), xb = shell ? x1 : xa;
          if (!shell && (xa < 0 || xa >= g.n[0])) continue;
          xa = xa < 0 ? 0 : xa;
          xb = xb >= g.n[0] ? g.n[0] - 1 : xb;
          if (xa > xb) continue;
          const int e = cell_start[row + xb + 1];
          for (int j = cell_start[row + xa]; j < e; j++) {
            const CellPoint o = pts[j];
            best.insert(dist2_f32(me.x, me.y, me.z, o.x, o.y, o.z));
          }
        }
      }
    }
    // Everything not visited yet lies in a cell at least r + 1 away along some axis: its cell coordinate t (clamped cells included: a
    // clamped t only lies further out) differs from this query's by more than r, so it is more than r h away.  The float32 distance is
    // within 4 ulp-relative of the exact one and the cell coordinates are formed in float64: the 1 % margin covers both many times over.
    const double bound = 0.99 * (double)r * g.h;
    const bool covered = c[0] - r <= 0 && c[0] + r >= g.n[0] - 1 && c[1] - r <= 0 && c[1] + r >= g.n[1] - 1 && c[2] - r <= 0 && c[2] + r >= g.n[2] - 1;
    done = covered || (double)best.worst() < bound * bound;
  }
  if (done)
    avg[me.index] = best.average(k1);
  else
    open_list[atomicAdd(open_count, 1)] = q;
}

// one wavefront per open query: every lane keeps the best of its share of all points, then k1 rounds take the smallest head of the 64 lists
template <int CAP>
__global__ __launch_bounds__(64) void knn_brute_kernel(const CellPoint *__restrict__ pts, const int32_t *__restrict__ open_list, int n, int k1,
                                                       double *__restrict__ avg) {
  const int lane = (int)threadIdx.x;
  const CellPoint me = pts[open_list[blockIdx.x]];
  Best<CAP> best;
  best.init(k1);
  for (int j = lane; j < n; j += 64) {
    const CellPoint o = pts[j];
    best.insert(dist2_f32(me.x, me.y, me.z, o.x, o.y, o.z));
  }
  for (int s = 0; s < CAP - k1; s++) {  // the list to the front: v[0 .. k1 - 1] ascending, +inf behind
#pragma unroll
    for (int i = 0; i + 1 < CAP; i++) best.v[i] = best.v[i + 1];
    best.v[CAP - 1] = INFINITY;
  }
  double sum = 0.0;
  for (int round = 0; round < k1; round++) {
    // distances are >= 0 (or +inf): their bit patterns order like the values; the lane index breaks ties, so exactly one lane pops
    unsigned long long key = ((unsigned long long)__builtin_bit_cast(unsigned, best.v[0]) << 32) | (unsigned)lane;
    for (int m = 1; m < 64; m <<= 1) {
      const unsigned long long other = __shfl_xor(key, m, 64);
      key = other < key ? other : key;
    }
    if ((int)(key & 63u) == lane) {
#pragma unroll
      for (int i = 0; i + 1 < CAP; i++) best.v[i] = best.v[i + 1];
      best.v[CAP - 1] = INFINITY;
    }
    if (round > 0) sum += (double)__builtin_bit_cast(float, (unsigned)(key >> 32));
  }
  if (lane == 0) avg[me.index] = sum / (double)(k1 - 1);
}

template <int CAP>
int launch_knn(osfm_ctx *ctx, hipStream_t st, const CellPoint *d_pts, const int32_t *d_cell_start, const Grid &g, int n, int k1, double *d_avg,
               int32_t *d_open, int32_t *d_count, double *ms_out) {
  OSFM_HIP(hipMemsetAsync(d_count, 0, 4, st));
  OSFM_HIP(hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL((knn_ring_kernel<CAP>), dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, d_pts, d_cell_start, g, n, k1, d_avg,
                     d_open, d_count);
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipEventRecord(ctx->ev[1], st));
  int n_open = 0;
  OSFM_HIP(hipMemcpyAsync(&n_open, d_count, 4, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  OSFM_REQUIRE(n_open >= 0 && n_open <= n, OSFM_E_NUMERIC, "osfm_points_isolation: %d open queries of %d", n_open, n);
  float ms = 0.f, ms2 = 0.f;
  if (n_open > 0) {
    OSFM_HIP(hipEventRecord(ctx->ev[2], st));
    hipLaunchKernelGGL((knn_brute_kernel<CAP>), dim3((unsigned)n_open), dim3(64), 0, st, d_pts, d_open, n, k1, d_avg);
    OSFM_HIP(hipGetLastError());
    OSFM_HIP(hipEventRecord(ctx->ev[3], st));
    OSFM_HIP(hipStreamSynchronize(st));
    OSFM_HIP(hipEventElapsedTime(&ms2, ctx->ev[2], ctx->ev[3]));
  }
  OSFM_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
  *ms_out = (double)ms + (double)ms2;
  return OSFM_OK;
}

// mean + multiplier * population sigma of the finite-or-not values v[i] with use[i], accumulated in index order (std::accumulate)
double stat_threshold(const double *v, const uint8_t *skip, int n, double multiplier) {
  double sum = 0.0;
  int64_t m = 0;
  for (int i = 0; i < n; i++)
    if (!skip || !skip[i]) {
      sum += v[i];
      m++;
    }
  if (m == 0) return NAN;
  const double mean = sum / (double)m;
  double ss = 0.0;
  for (int i = 0; i < n; i++)
    if (!skip || !skip[i]) ss += (v[i] - mean) * (v[i] - mean);
  return mean + multiplier * sqrt(ss / (double)m);
}

}  // namespace

extern "C" int osfm_points_conditioning(osfm_ctx *ctx, const double *points, int n_points, const double *shot_pose, const int32_t *shot_camera,
                                        int n_shots, const int32_t *cam_model, const double *cam_params, int n_cams, const int32_t *obs_shot,
                                        const int32_t *obs_point, int64_t n_obs, double min_angle_deg, double min_abs_det, double *cond,
                                        uint8_t *reason, double *threshold, int *n_removed, double *kernel_ms) {
  const char *who = "osfm_points_conditioning";
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_REQUIRE(ctx && threshold && n_removed, OSFM_E_INVALID, "%s: null argument", who);
  *threshold = NAN;
  *n_removed = 0;
  OSFM_REQUIRE(n_points >= 0 && n_shots >= 0 && n_cams >= 0 && n_obs >= 0, OSFM_E_INVALID, "%s: negative size", who);
  OSFM_REQUIRE(min_angle_deg >= 0.0 && min_angle_deg <= 180.0, OSFM_E_INVALID, "%s: min_angle_deg must lie in [0, 180]", who);
  OSFM_REQUIRE(!(min_abs_det != min_abs_det), OSFM_E_INVALID, "%s: min_abs_det is NaN", who);
  if (n_points == 0) return OSFM_OK;
  OSFM_REQUIRE(points && cond && reason, OSFM_E_INVALID, "%s: null points / cond / reason", who);
  if (n_obs == 0) {  // no landmark has a pair of rays
    for (int i = 0; i < n_points; i++) {
      cond[i] = NAN;
      reason[i] = 1;
    }
    *n_removed = n_points;
    return OSFM_OK;
  }
  OSFM_REQUIRE(shot_pose && shot_camera && cam_model && cam_params && obs_shot && obs_point && n_shots > 0 && n_cams > 0, OSFM_E_INVALID,
               "%s: null argument", who);
  OSFM_TRY(osfm_check_camera_table(cam_model, n_cams, shot_camera, n_shots, 1, "shot", who));
  // stable counting sort by landmark
  std::vector<int64_t> start((size_t)n_points + 1, 0);
  for (int64_t i = 0; i < n_obs; i++) {
    OSFM_REQUIRE(obs_point[i] >= 0 && obs_point[i] < n_points && obs_shot[i] >= 0 && obs_shot[i] < n_shots, OSFM_E_INVALID,
                 "%s: observation %lld names a shot or point outside the tables", who, (long long)i);
    start[(size_t)obs_point[i] + 1]++;
  }
  for (int p = 0; p < n_points; p++) start[(size_t)p + 1] += start[(size_t)p];
  std::vector<int32_t> s_shot((size_t)n_obs), s_point((size_t)n_obs);
  {
    std::vector<int64_t> fill(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < n_obs; i++) {
      const int64_t at = fill[(size_t)obs_point[i]]++;
      s_shot[(size_t)at] = obs_shot[i];
      s_point[(size_t)at] = obs_point[i];
    }
  }
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmArena A;
  const auto d_points = A.add<double>((size_t)n_points * 3);
  const auto d_pose = A.add<double>((size_t)n_shots * 12);
  const auto d_shot_camera = A.add<int32_t>((size_t)n_shots);
  const auto d_cam_model = A.add<int32_t>((size_t)n_cams);
  const auto d_cam_params = A.add<double>((size_t)n_cams * 16);
  const auto d_s_shot = A.add<int32_t>((size_t)n_obs);
  const auto d_s_point = A.add<int32_t>((size_t)n_obs);
  const auto d_start = A.add<int64_t>((size_t)n_points + 1);
  const auto d_rays = A.add<double>((size_t)n_obs * 3);
  const auto d_jtj = A.add<double>((size_t)n_obs * 6);
  const auto d_cond = A.add<double>((size_t)n_points);
  const auto d_reason = A.add<uint8_t>((size_t)n_points);
  OSFM_HIP(A.alloc(ctx));
  OSFM_HIP(A.upload(d_points, points, st));
  OSFM_HIP(A.upload(d_pose, shot_pose, st));
  OSFM_HIP(A.upload(d_shot_camera, shot_camera, st));
  OSFM_HIP(A.upload(d_cam_model, cam_model, st));
  OSFM_HIP(A.upload(d_cam_params, cam_params, st));
  OSFM_HIP(A.upload(d_s_shot, s_shot.data(), st));
  OSFM_HIP(A.upload(d_s_point, s_point.data(), st));
  OSFM_HIP(A.upload(d_start, start.data(), st));
  const double rad = min_angle_deg * M_PI / 180.0;
  OSFM_HIP(hipEventRecord(ctx->ev[0], st));
  hipLaunchKernelGGL(cond_obs_kernel, dim3((unsigned)((n_obs + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, d_points, d_pose,
                     d_shot_camera, d_cam_model, d_cam_params, d_s_shot, d_s_point, n_obs, d_rays, d_jtj);
  OSFM_HIP(hipGetLastError());
  constexpr int kPerBlock = kBlock / kGroup;
  hipLaunchKernelGGL(cond_landmark_kernel, dim3((unsigned)((n_points + kPerBlock - 1) / kPerBlock)), dim3(kBlock), 0, st, d_start, d_rays,
                     d_jtj, n_obs, n_points, rad, cos(rad), min_abs_det, d_cond, d_reason);
  OSFM_HIP(hipGetLastError());
  OSFM_HIP(hipEventRecord(ctx->ev[1], st));
  OSFM_HIP(hipMemcpyAsync(cond, d_cond, d_cond.bytes, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipMemcpyAsync(reason, d_reason, d_reason.bytes, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  OSFM_TRY(osfm_kernel_ms(ctx, kernel_ms));
  const double thr = stat_threshold(cond, reason, n_points, 1.0);
  int removed = 0;
  for (int i = 0; i < n_points; i++) {
    if (reason[i] == 0 && cond[i] > thr) reason[i] = 5;
    removed += reason[i] != 0;
  }
  *threshold = thr;
  *n_removed = removed;
  return OSFM_OK;
}

extern "C" int osfm_points_isolation(osfm_ctx *ctx, const double *points, int n_points, int k, double *avg, uint8_t *removed, double *threshold,
                                     int *n_removed, double *kernel_ms) {
  const char *who = "osfm_points_isolation";
  if (kernel_ms) *kernel_ms = 0.0;
  OSFM_REQUIRE(ctx && threshold && n_removed, OSFM_E_INVALID, "%s: null argument", who);
  *threshold = NAN;
  *n_removed = 0;
  OSFM_REQUIRE(n_points >= 0, OSFM_E_INVALID, "%s: n_points < 0", who);
  OSFM_REQUIRE(k >= 1 && k <= 31, OSFM_E_INVALID, "%s: k = %d is outside 1 .. 31", who, k);
  OSFM_REQUIRE(n_points <= (1 << 29), OSFM_E_UNSUPPORTED, "%s: more than 2^29 points", who);
  if (n_points == 0) return OSFM_OK;
  OSFM_REQUIRE(points && avg && removed, OSFM_E_INVALID, "%s: null points / avg / removed", who);
  const int n = n_points;
  std::vector<float> f((size_t)n * 3);
  for (size_t i = 0; i < (size_t)n * 3; i++) {
    f[i] = static_cast<float>(points[i]);
    OSFM_REQUIRE(fabsf(f[i]) <= 3.4028234663852886e38f, OSFM_E_INVALID, "%s: point %lld has a coordinate that is not finite as a float32", who,
                 (long long)(i / 3));
  }
  memset(removed, 0, (size_t)n);
  if (n <= k) {  // RemoveIsolatedPoints returns before it computes anything
    for (int i = 0; i < n; i++) avg[i] = NAN;
    return OSFM_OK;
  }
  // the grid: the 2 % .. 98 % box of every axis, cells of ~max(4, (k + 1) / 2) points (so that a cloud without extent along one or two
  // axes still finds its k + 1 neighbours within the ring budget), at most 1024 cells per axis and ~2 n in all; an axis without extent
  // gets one cell.  Points outside the box fall into the border cells.
  Grid g;
  double ext[3];
  {
    std::vector<float> axis((size_t)n);
    const size_t qa = (size_t)(0.02 * (double)(n - 1)), qb = (size_t)n - 1 - qa;
    for (int a = 0; a < 3; a++) {
      for (int i = 0; i < n; i++) axis[(size_t)i] = f[3 * (size_t)i + a];
      std::nth_element(axis.begin(), axis.begin() + qa, axis.end());
      const float lo = axis[qa];
      std::nth_element(axis.begin(), axis.begin() + qb, axis.end());
      g.lo[a] = lo;
      ext[a] = (double)axis[qb] - (double)lo;
    }
  }
  {
    double vol = 1.0, max_ext = 0.0;
    int dims = 0;
    for (int a = 0; a < 3; a++)
      if (ext[a] > 0.0) {
        vol *= ext[a];
        dims++;
        max_ext = std::max(max_ext, ext[a]);
      }
    double h = dims ? pow(vol * (double)std::max(4, (k + 1) / 2) / (double)n, 1.0 / dims) : 1.0;
    h = std::max(h, max_ext / 1023.0);
    if (!(h > 0.0) || !(h <= 1.7976931348623157e308)) {
      h = 1.0;
      ext[0] = ext[1] = ext[2] = 0.0;
    }
    for (;;) {
      int64_t total = 1;
      for (int a = 0; a < 3; a++) {
        g.n[a] = ext[a] > 0.0 ? (int)std::min(1024.0, floor(ext[a] / h) + 1.0) : 1;
        total *= g.n[a];
      }
      if (total <= 2 * (int64_t)n + 64) break;
      h *= 1.25;
    }
    g.h = h;
  }
  const int64_t n_cells = (int64_t)g.n[0] * g.n[1] * g.n[2];
  // counting sort by cell (the same arithmetic as the kernel's)
  std::vector<int32_t> cell((size_t)n), cell_start((size_t)n_cells + 1, 0);
  for (int i = 0; i < n; i++) {
    int c[3];
    for (int a = 0; a < 3; a++) {
      const double t = ((double)f[3 * (size_t)i + a] - (double)g.lo[a]) / g.h;
      c[a] = g.n[a] == 1 || !(t > 0.0) ? 0 : t >= (double)g.n[a] ? g.n[a] - 1 : (int)t;
    }
    cell[(size_t)i] = (c[2] * g.n[1] + c[1]) * g.n[0] + c[0];
    cell_start[(size_t)cell[(size_t)i] + 1]++;
  }
  for (int64_t c = 0; c < n_cells; c++) cell_start[(size_t)c + 1] += cell_start[(size_t)c];
  std::vector<float> sorted((size_t)n * 4);
  {
    std::vector<int32_t> fill(cell_start.begin(), cell_start.end() - 1);
    for (int i = 0; i < n; i++) {
      const size_t at = (size_t)fill[(size_t)cell[(size_t)i]]++;
      sorted[4 * at] = f[3 * (size_t)i];
      sorted[4 * at + 1] = f[3 * (size_t)i + 1];
      sorted[4 * at + 2] = f[3 * (size_t)i + 2];
      memcpy(&sorted[4 * at + 3], &i, 4);
    }
  }
  OSFM_CTX_LOCK(ctx);
  OSFM_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  OsfmArena A;
  const auto d_pts = A.add<CellPoint>((size_t)n);
  const auto d_cell_start = A.add<int32_t>((size_t)n_cells + 1);
  const auto d_avg = A.add<double>((size_t)n);
  const auto d_open = A.add<int32_t>((size_t)n);
  const auto d_count = A.add<int32_t>(4);
  OSFM_HIP(A.alloc(ctx));
  OSFM_HIP(A.upload(d_pts, (const CellPoint *)sorted.data(), st));
  OSFM_HIP(A.upload(d_cell_start, cell_start.data(), st));
  const int k1 = k + 1;
  double ms = 0.0;
  if (k1 <= 8)
    OSFM_TRY(launch_knn<8>(ctx, st, d_pts, d_cell_start, g, n, k1, d_avg, d_open, d_count, &ms));
  else if (k1 <= 16)
    OSFM_TRY(launch_knn<16>(ctx, st, d_pts, d_cell_start, g, n, k1, d_avg, d_open, d_count, &ms));
  else
    OSFM_TRY(launch_knn<32>(ctx, st, d_pts, d_cell_start, g, n, k1, d_avg, d_open, d_count, &ms));
  OSFM_HIP(hipMemcpyAsync(avg, d_avg, d_avg.bytes, hipMemcpyDeviceToHost, st));
  OSFM_HIP(hipStreamSynchronize(st));
  if (kernel_ms) *kernel_ms = ms;
  const double thr = stat_threshold(avg, nullptr, n, 1.25);
  int count = 0;
  for (int i = 0; i < n; i++) {
    removed[i] = avg[i] > thr ? 1 : 0;
    count += removed[i];
  }
  *threshold = thr;
  *n_removed = count;
  return OSFM_OK;
}
