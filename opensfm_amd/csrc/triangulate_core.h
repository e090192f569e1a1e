// triangulate_core.h -- the per-track numerics of TrackTriangulator.triangulate (opensfm/reconstruction.py:1032-1073): the ray-angle test,
// the midpoint solve and its two per-observation tests (geometry/src/triangulation.cc:139-178, geometry/triangulation.h:58-82) and
// PointRefinement (triangulation.cc:13-60, 221-233).
//
// PointRefinement is Ceres' TinySolver over the 3n residuals normalize(X - o_i) - w_i with the Jacobian of Normalize::ForwardDerivatives
// (geometry/transformations_functions.h:265-305).  Neither Ceres nor Eigen is available to this project, so TinySolver is RESTATED here
// from its published description, the way relrot_core.h restates Eigen's SVD: residual negated, Jacobi scaling 1 / (1 + column norm) from
// the first evaluation, g = J^T e, cost = |e|^2 / 2, stop at the start on max|g| < 1e-10 or cost < eps, u = 1 / 1e4, v = 2, the loop
// `for (it = 1; it < max_num_iterations; ++it)` (iterations - 1 steps), the diagonal u * clamp(JtJ_ii, 1e-6, 1e32), a 3 x 3 LDL^T solve,
// dx = scaling .* step, stop on |dx| < 1e-8 (|x| + 1e-8), rho = (2 cost - |f(x + dx)|^2) / (step . (2 g - JtJ step)); on rho > 0 accept,
// stop on |cost change| < 1e-6, re-evaluate, repeat the gradient and cost tests, u *= max(1/3, 1 - (2 rho - 1)^3), v = 2; otherwise
// u *= v, v *= 2.  The restatement has NOT been compared with the Ceres source; the tests pin its result against the quantity it
// approximates (the minimiser of sum |normalize(X - o_i) - w_i|^2 at 50 digits), not against itself.  Two places are not literal:
//   - J^T J and J^T e are summed unscaled and scaled afterwards (TinySolver scales the columns of J first): one pass per evaluation;
//   - the LDL^T is unpivoted (Eigen's pivots on the diagonal): the matrix is J^T J plus a positive diagonal.
// Both change roundings only.
//
// The walk is written once, over a TRACK POLICY that owns the lanes working on one track:
//   int n                                   observations of the track (the same on every lane)
//   each(f)                                 f(i, o, w) for this lane's observations, ascending
//   at(i, o, w)                             any observation (the pair test reads its partner)
//   first() / stride()                      this lane's first observation index and the distance to its next
//   sum(v, m)                               v[0..m) summed over the lanes in a fixed order; every lane gets the same bits
//   lowest(k)                               the smallest k over the lanes;  any(b)  whether any lane has b
// triangulate.hip supplies the GPU policies (a lane group or a wavefront); a single-lane policy serves host callers.
#pragma once
#include <math.h>
#include <stdint.h>

#include "relpose_core.h"  // OSFM_HD

namespace osfm_tri {

enum Status { kOk = 0, kTooFew = 1, kRayAngle = 2, kReprojection = 3, kDepth = 4, kNotFinite = 5 };

struct Params {
  double threshold;  // radians
  double min_angle;  // radians
  double min_depth;
  int iterations;    // TinySolver's max_num_iterations
};

OSFM_HD bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }

// geometry::AngleBetweenVectors (triangulation.cc:66-73)
OSFM_HD double angle_between(const double *u, const double *v) {
  const double c = (u[0] * v[0] + u[1] * v[1] + u[2] * v[2]) /
                   sqrt((u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
  if (fabs(c) >= 1.0) return 0.0;
  return acos(c);
}

// Normalize::Forward (transformations_functions.h:266-272): SquaredNorm is x^2 + y^2
OSFM_HD void normalize_forward(const double *p, double *out) {
  const double inv_norm = 1.0 / sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
  for (int k = 0; k < 3; k++) out[k] = p[k] * inv_norm;
}

// the inverse of a 3 x 3 by cofactors and 1 / det, as Eigen's fixed-size inverse (compute_inverse_size3)
OSFM_HD void inverse3(const double *m, double *inv) {
  const double c00 = m[4] * m[8] - m[5] * m[7], c10 = m[5] * m[6] - m[3] * m[8], c20 = m[3] * m[7] - m[4] * m[6];
  const double invdet = 1.0 / (c00 * m[0] + c10 * m[1] + c20 * m[2]);
  inv[0] = c00 * invdet;
  inv[3] = c10 * invdet;
  inv[6] = c20 * invdet;
  inv[1] = (m[2] * m[7] - m[1] * m[8]) * invdet;
  inv[4] = (m[0] * m[8] - m[2] * m[6]) * invdet;
  inv[7] = (m[1] * m[6] - m[0] * m[7]) * invdet;
  inv[2] = (m[1] * m[5] - m[2] * m[4]) * invdet;
  inv[5] = (m[2] * m[3] - m[0] * m[5]) * invdet;
  inv[8] = (m[0] * m[4] - m[1] * m[3]) * invdet;
}

// TriangulateBearingsMidpointSolve from its three sums: S = BBt (00 01 02 11 12 22), BBtA (3), A (3)
OSFM_HD void midpoint_from_sums(const double *S, int n, double *X) {
  const double B[9] = {S[0], S[1], S[2], S[1], S[3], S[4], S[2], S[4], S[5]};
  const double *BA = S + 6, *A = S + 9;
  double C[9], Cinv[9];
  for (int k = 0; k < 9; k++) C[k] = ((k % 4 == 0) ? (double)n : 0.0) - B[k];
  inverse3(C, Cinv);
  for (int r = 0; r < 3; r++) {
    double acc = 0.0, sub = 0.0;  // ((I + BBt Cinv) A)_r / n - (Cinv BBtA)_r
    for (int c = 0; c < 3; c++) {
      const double bc = (B[3 * r] * Cinv[c] + B[3 * r + 1] * Cinv[3 + c]) + B[3 * r + 2] * Cinv[6 + c];
      acc += ((r == c ? 1.0 : 0.0) + bc) * A[c];
      sub += Cinv[3 * r + c] * BA[c];
    }
    X[r] = acc / (double)n - sub;
  }
}

// A x = b for a symmetric positive definite 3 x 3 (a00 a01 a02 a11 a12 a22) by LDL^T
OSFM_HD void ldlt3_solve(const double *a, const double *b, double *x) {
  const double d0 = a[0], l10 = a[1] / d0, l20 = a[2] / d0;
  const double d1 = a[3] - l10 * l10 * d0, l21 = (a[4] - l20 * l10 * d0) / d1;
  const double d2 = a[5] - l20 * l20 * d0 - l21 * l21 * d1;
  const double y0 = b[0], y1 = b[1] - l10 * y0, y2 = b[2] - l20 * y0 - l21 * y1;
  const double z2 = y2 / d2, z1 = y1 / d1, z0 = y0 / d0;
  x[2] = z2;
  x[1] = z1 - l21 * x[2];
  x[0] = z0 - l10 * x[1] - l20 * x[2];
}

// One evaluation of the cost function at X: this lane's share of J^T J (6), J^T e (3) and |e|^2 (1) into v[10], e = -(normalize(X - o) - w)
template <class Track>
OSFM_HD void evaluate(Track &trk, const double *X, bool with_jacobian, double *v) {
  for (int k = 0; k < 10; k++) v[k] = 0.0;
  trk.each([&](int, const double *o, const double *w) {
    const double p[3] = {X[0] - o[0], X[1] - o[1], X[2] - o[2]};
    double t[3], e[3];
    normalize_forward(p, t);
    for (int k = 0; k < 3; k++) e[k] = -(t[k] - w[k]);
    v[9] += (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    if (!with_jacobian) return;
    const double x = p[0], y = p[1], z = p[2], x2 = x * x, y2 = y * y, z2 = z * z;
    const double norm2 = x2 + y2 + z2, norm = sqrt(norm2), s = 1.0 / (norm * norm2);
    const double J[9] = {(y2 + z2) * s, (-x * y) * s, (-x * z) * s, (-y * x) * s, (x2 + z2) * s, (-y * z) * s, (-z * x) * s, (-z * y) * s, (x2 + y2) * s};
    int q = 0;
    for (int a = 0; a < 3; a++)
      for (int b = a; b < 3; b++, q++) v[q] += (J[a] * J[b] + J[3 + a] * J[3 + b]) + J[6 + a] * J[6 + b];
    for (int a = 0; a < 3; a++) v[6 + a] += (J[a] * e[0] + J[3 + a] * e[1]) + J[6 + a] * e[2];
  });
  if (with_jacobian)
    trk.sum(v, 10);
  else
    trk.sum(v + 9, 1);
}

struct Solver {
  double scaling[3], jtj[6], g[3], cost, gmax;
};

// TinySolver::Update: v from evaluate(); the scaling is fixed by the first call
OSFM_HD void solver_update(Solver &s, const double *v, bool first) {
  if (first)
    for (int a = 0; a < 3; a++) s.scaling[a] = 1.0 / (1.0 + sqrt(v[a == 0 ? 0 : a == 1 ? 3 : 5]));
  int q = 0;
  for (int a = 0; a < 3; a++)
    for (int b = a; b < 3; b++, q++) s.jtj[q] = v[q] * s.scaling[a] * s.scaling[b];
  for (int a = 0; a < 3; a++) s.g[a] = v[6 + a] * s.scaling[a];
  s.gmax = fmax(fabs(s.g[0]), fmax(fabs(s.g[1]), fabs(s.g[2])));  // (Eigen's maxCoeff: a NaN is not larger than anything)
  s.cost = v[9] / 2.0;
}

// PointRefinement: X in place; returns TinySolver's summary.iterations
template <class Track>
OSFM_HD int refine(Track &trk, int max_num_iterations, double *X) {
  constexpr double kGradientTolerance = 1e-10, kParameterTolerance = 1e-8, kFunctionTolerance = 1e-6, kCostThreshold = 2.220446049250313e-16;
  Solver s;
  double v[10];
  evaluate(trk, X, true, v);
  solver_update(s, v, true);
  if (s.gmax < kGradientTolerance) return 0;
  if (s.cost < kCostThreshold) return 0;
  double u = 1.0 / 1e4, vv = 2.0;
  int it = 1;
  for (; it < max_num_iterations; it++) {
    double reg[6] = {s.jtj[0], s.jtj[1], s.jtj[2], s.jtj[3], s.jtj[4], s.jtj[5]};
    const int diag[3] = {0, 3, 5};
    for (int a = 0; a < 3; a++) {
      const double lm = sqrt(u * fmin(fmax(s.jtj[diag[a]], 1e-6), 1e32));
      reg[diag[a]] += lm * lm;
    }
    double step[3], dx[3], xn[3];
    ldlt3_solve(reg, s.g, step);
    for (int a = 0; a < 3; a++) dx[a] = s.scaling[a] * step[a];
    const double xnorm = sqrt((X[0] * X[0] + X[1] * X[1]) + X[2] * X[2]), dxnorm = sqrt((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]);
    if (dxnorm < kParameterTolerance * (xnorm + kParameterTolerance)) break;
    for (int a = 0; a < 3; a++) xn[a] = X[a] + dx[a];
    evaluate(trk, xn, false, v);
    const double cost_change = 2.0 * s.cost - v[9];
    const double js[3] = {(s.jtj[0] * step[0] + s.jtj[1] * step[1]) + s.jtj[2] * step[2], (s.jtj[1] * step[0] + s.jtj[3] * step[1]) + s.jtj[4] * step[2],
                          (s.jtj[2] * step[0] + s.jtj[4] * step[1]) + s.jtj[5] * step[2]};
    const double model_cost_change =
        (step[0] * (2.0 * s.g[0] - js[0]) + step[1] * (2.0 * s.g[1] - js[1])) + step[2] * (2.0 * s.g[2] - js[2]);
    const double rho = cost_change / model_cost_change;
    if (rho > 0.0) {
      for (int a = 0; a < 3; a++) X[a] = xn[a];
      if (fabs(cost_change) < kFunctionTolerance) break;
      evaluate(trk, X, true, v);
      solver_update(s, v, false);
      if (s.gmax < kGradientTolerance) break;
      if (s.cost < kCostThreshold) break;
      const double tmp = 2.0 * rho - 1.0;
      u = u * fmax(1.0 / 3.0, 1.0 - tmp * tmp * tmp);
      vv = 2.0;
    } else {
      u *= vv;
      vv *= 2.0;
    }
  }
  return it;
}

// One track: status, the point (untouched unless the status is kOk) and the solver's iteration count
template <class Track>
OSFM_HD int triangulate_track(Track &trk, const Params &prm, double *X, int *iterations) {
  *iterations = 0;
  const int n = trk.n;
  if (n < 2) return kTooFew;
  // some pair (i, j < i) with an angle in [min_angle, pi - min_angle]: the outer index spread over the lanes, agreed after every round
  bool found = false;
  for (int base = 0; base < n && !found; base += trk.stride()) {
    const int i = base + trk.first();
    bool mine = false;
    if (i < n) {
      double oi[3], wi[3], oj[3], wj[3];
      trk.at(i, oi, wi);
      for (int j = 0; j < i && !mine; j++) {
        trk.at(j, oj, wj);
        const double angle = angle_between(wi, wj);
        mine = angle >= prm.min_angle && angle <= M_PI - prm.min_angle;
      }
    }
    found = trk.any(mine);
  }
  if (!found) return kRayAngle;
  double S[12];
  for (int k = 0; k < 12; k++) S[k] = 0.0;
  trk.each([&](int, const double *o, const double *w) {
    int q = 0;
    for (int a = 0; a < 3; a++)
      for (int b = a; b < 3; b++, q++) S[q] += w[a] * w[b];
    for (int a = 0; a < 3; a++) S[6 + a] += ((w[a] * w[0]) * o[0] + (w[a] * w[1]) * o[1]) + (w[a] * w[2]) * o[2];
    for (int a = 0; a < 3; a++) S[9 + a] += o[a];
  });
  trk.sum(S, 12);
  double P[3];
  midpoint_from_sums(S, n, P);
  // the first observation that fails, and on which test: key = 2 i (angle) or 2 i + 1 (depth)
  int key = 2 * n;
  trk.each([&](int i, const double *o, const double *w) {
    if (key != 2 * n) return;
    const double p[3] = {P[0] - o[0], P[1] - o[1], P[2] - o[2]};
    if (angle_between(p, w) > prm.threshold)
      key = 2 * i;
    else if ((p[0] * w[0] + p[1] * w[1]) + p[2] * w[2] < prm.min_depth)
      key = 2 * i + 1;
  });
  key = trk.lowest(key);
  if (key != 2 * n) return (key & 1) ? kDepth : kReprojection;
  if (!(finite_d(P[0]) && finite_d(P[1]) && finite_d(P[2]))) return kNotFinite;
  *iterations = refine(trk, prm.iterations, P);
  if (!(finite_d(P[0]) && finite_d(P[1]) && finite_d(P[2]))) return kNotFinite;
  for (int k = 0; k < 3; k++) X[k] = P[k];
  return kOk;
}

}  // namespace osfm_tri
