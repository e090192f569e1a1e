// abspose_core.h -- absolute-pose (P3P) LO-RANSAC of candidate images: the estimator behind reconstruction.resect.
//
// reference: reconstruction.resect (opensfm/reconstruction.py:695-762) -> multiview.absolute_pose_ransac (opensfm/multiview.py:468-491)
// -> pyrobust.ransac_absolute_pose (robust/src/instanciations.cc:67-83) = Estimate<RansacScoring, AbsolutePose>
// (robust/robust_estimator.h:37-119) with AbsolutePose (robust/absolute_pose_model.h): 3-point samples, 0 or 4 models from the
// three-point solver of Ke & Roumeliotis (geometry/absolute_pose.h:15-122), the Lu-Hager iteration (:144-189) as the non-minimal
// solver of the local optimisation; then the inlier count of resect on bearing chords.
//
// Everything is host + device, with the discipline of relrot_core.h: tests/native/abspose_host.cpp compiles this header with g++ and
// runs the very same per-image walk (loransac_walk.h over AbsposeModel) with loops in place of lanes; abspose.hip runs it with one wavefront
// per image.  Contraction is
// off, every 3-term sum is evaluated left to right, and the decision path uses only + - * / sqrt (frexp / ldexp are exact), so host
// and device give the same bits.
//
// Numerics that cannot be pinned here.
//  * Eigen: the 3 x 3 products, norms and JacobiSVD of the reference are restated (jacobi_svd3, relrot_core.h); the inverse of
//    I - F1 in TranslationBetweenPoints is restated as Eigen's fixed-size 3 x 3 inverse (cofactors of the first column give the
//    determinant, every entry is a cofactor times 1 / det) from memory of Eigen 3.3 / 3.4 and is NOT verified against Eigen.
//  * libstdc++ / libm: SolveQuartic (foundation/src/numeric.cc:30-66) calls std::pow on complex numbers (a principal square root
//    and a principal cube root) and divides complex numbers; device libm and glibc differ in the last bit of such calls, and one bit
//    in a root can move a row across the threshold.  quartic_roots evaluates the reference's formula (Q1 .. Q7 and the four
//    .real() / 4 expressions, in its order) in complex arithmetic built from real sqrt only: csqrt_principal from
//    sqrt((|z| +- re) / 2); ccbrt_principal as |z|^(1/3) (Newton from an exponent-scaled start) times the cube root of the unit
//    part (Newton on w^3 = u started at sqrt(sqrt(u)), whose argument theta / 4 lies within 15 degrees of theta / 3: the principal
//    branch, the one std::pow(z, 1 / 3) picks).  The branch decides the ORDER of the four roots and the order decides ties between
//    the models of a sample, so the order is the reference's; the five Newton-Raphson steps of RefineQuarticRoots then absorb the
//    last-bit differences in the values.  The last bits of libstdc++'s own pow / complex division are not reproduced.
// What the tests pin is therefore: this header on the GPU == this header on the host, bit for bit; the decision sequence (draws,
// model order, ties, LO, stopping) == the reference's own robust_estimator.h / random_sampler.h / scorer.h compiled with this
// toolchain around these numerics; the quartic against a 50-digit evaluation of the same formulas.
//
// Divergence: with fewer than 3 rows the reference's sampler loops forever; the C ABI rejects such images (OSFM_E_INVALID).
// A sample for which the reference returns no model, and a batch of iterations that all do, leave model / lo_model at zero here
// (the reference's are uninitialised).
#pragma once
#include "relrot_core.h"

namespace osfm_ap {

using osfm_lo::kLdsInliers;
using osfm_lo::kRngCache;
using osfm_lo::RngTable;
using osfm_lo::RngView;
using osfm_rr::closest_rotation;
using osfm_rr::rotation_between_points;

constexpr int kMinimalSamples = 3;  // AbsolutePose::MINIMAL_SAMPLES
constexpr int kMaxModels = 4;       // AbsolutePose::MAX_MODELS
constexpr int kNPointsIterations = 100;
constexpr int kCbrtSteps = 8;       // Newton steps of either cube root: quadratic convergence from a start within 26 % / 15 degrees

// ---------------------------------------------------------------------------------------------------------------
// small vectors, as Eigen evaluates them (sums left to right)
// ---------------------------------------------------------------------------------------------------------------
OSFM_HD double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
OSFM_HD void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
OSFM_HD double norm3(const double* a) { return sqrt(dot3(a, a)); }
OSFM_HD void normalized3(const double* a, double* out) {  // MatrixBase::normalized(): a / sqrt(z) when z > 0, a itself otherwise
  const double z = dot3(a, a);
  if (z > 0.0) {
    const double s = sqrt(z);
    for (int i = 0; i < 3; i++) out[i] = a[i] / s;
  } else {
    for (int i = 0; i < 3; i++) out[i] = a[i];
  }
}
OSFM_HD void matmul3(const double* A, const double* B, double* C) {  // row-major
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
OSFM_HD void matvec3(const double* A, const double* x, double* y) {
  for (int i = 0; i < 3; i++) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
}
OSFM_HD void matTvec3(const double* A, const double* x, double* y) {  // A^T x
  for (int i = 0; i < 3; i++) y[i] = A[i] * x[0] + A[3 + i] * x[1] + A[6 + i] * x[2];
}

// ---------------------------------------------------------------------------------------------------------------
// complex arithmetic from + - * / sqrt
// ---------------------------------------------------------------------------------------------------------------
struct Cx {
  double re, im;
};
OSFM_HD Cx cx_mul(Cx a, Cx b) { return Cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
OSFM_HD Cx cx_div(Cx a, Cx b) {
  const double d = b.re * b.re + b.im * b.im;
  return Cx{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
OSFM_HD double cx_abs(Cx z) {  // scaled by the larger component: no overflow or underflow of the squares
  const double ar = fabs(z.re), ai = fabs(z.im);
  const double s = ar > ai ? ar : ai;
  if (!(s > 0.0) || !(s <= 1.79769313486231570815e308)) return ar + ai;  // 0, inf, NaN
  const double x = z.re / s, y = z.im / s;
  return s * sqrt(x * x + y * y);
}
// principal square root: real part >= 0; on the negative real axis the result is +i sqrt(-re) (an imaginary part of +0 or -0 alike)
OSFM_HD Cx csqrt_principal(Cx z) {
  if (z.re == 0.0 && z.im == 0.0) return Cx{0.0, 0.0};
  const double m = cx_abs(z);
  const double t = sqrt((m + fabs(z.re)) / 2.0);
  if (z.re >= 0.0) return Cx{t, z.im / (2.0 * t)};
  return Cx{fabs(z.im) / (2.0 * t), z.im < 0.0 ? -t : t};
}
// x^(1/3) of a finite x > 0: x = f 2^(3 q + r), f in [0.5, 1), r in {0, 1, 2}; Newton on y^3 = f 2^r in [0.5, 4) from y = 1
OSFM_HD double cbrt_positive(double x) {
  int e;
  const double f = frexp(x, &e);
  int q = e / 3, r = e - 3 * q;
  if (r < 0) {
    r += 3;
    q -= 1;
  }
  const double g = ldexp(f, r);
  double y = 1.0;
  for (int k = 0; k < kCbrtSteps + 2; k++) y = (2.0 * y + g / (y * y)) / 3.0;
  return ldexp(y, q);
}
// principal cube root: argument theta / 3 for theta in (-pi, pi]
OSFM_HD Cx ccbrt_principal(Cx z) {
  const double m = cx_abs(z);
  if (m == 0.0) return Cx{0.0, 0.0};
  if (!(m <= 1.79769313486231570815e308)) return Cx{m - m, m - m};  // not finite: NaN
  const Cx u{z.re / m, z.im / m};
  Cx w = csqrt_principal(csqrt_principal(u));
  for (int k = 0; k < kCbrtSteps; k++) {  // w <- (2 w + u / w^2) / 3
    const Cx q = cx_div(u, cx_mul(w, w));
    w = Cx{(2.0 * w.re + q.re) / 3.0, (2.0 * w.im + q.im) / 3.0};
  }
  const double r = cbrt_positive(m);
  return Cx{r * w.re, r * w.im};
}

// foundation::SolveQuartic: coefficients c[0] + c[1] x + ... + c[4] x^4; false when all four discriminant terms are below epsilon
OSFM_HD bool quartic_roots(const double* coefficients, double* roots) {
  const double eps = 2.220446049250313e-16;
  const double a = fabs(coefficients[4]) > eps ? coefficients[4] : eps;
  const double b = coefficients[3] / a;
  const double c = coefficients[2] / a;
  const double d = coefficients[1] / a;
  const double e = coefficients[0] / a;
  const double Q1 = c * c - 3. * b * d + 12. * e;
  const double Q2 = 2. * c * c * c - 9. * b * c * d + 27. * d * d + 27. * b * b * e - 72. * c * e;
  const double Q3 = 8. * b * c - 16. * d - 2. * b * b * b;
  const double Q4 = 3. * b * b - 8. * c;
  if (fabs(Q1) < eps && fabs(Q2) < eps && fabs(Q3) < eps && fabs(Q4) < eps) return false;
  Cx s = csqrt_principal(Cx{Q2 * Q2 / 4. - Q1 * Q1 * Q1, 0.0});
  const Cx Q5 = ccbrt_principal(Cx{Q2 / 2. + s.re, s.im});
  const Cx q15 = cx_div(Cx{Q1, 0.0}, Q5);
  const Cx Q6{(q15.re + Q5.re) / 3., (q15.im + Q5.im) / 3.};
  s = csqrt_principal(Cx{Q4 / 12. + Q6.re, Q6.im});
  const Cx Q7{2. * s.re, 2. * s.im};
  const Cx q37 = cx_div(Cx{Q3, 0.0}, Q7);
  const double base = 4. * Q4 / 6.;
  const Cx sm = csqrt_principal(Cx{base - 4. * Q6.re - q37.re, -(4. * Q6.im) - q37.im});
  const Cx sp = csqrt_principal(Cx{base - 4. * Q6.re + q37.re, -(4. * Q6.im) + q37.im});
  roots[0] = (-b - Q7.re - sm.re) / 4.;
  roots[1] = (-b - Q7.re + sm.re) / 4.;
  roots[2] = (-b + Q7.re - sp.re) / 4.;
  roots[3] = (-b + Q7.re + sp.re) / 4.;
  return true;
}

// foundation::RefineQuarticRoots: five Newton-Raphson steps (foundation/newton_raphson.h, scalar case: the decrement is f / f', 0 when
// f' == 0; a decrement below 1e-20 ends the iteration)
OSFM_HD void refine_quartic_roots(const double* c, double* roots) {
  for (int r = 0; r < 4; r++) {
    double x = roots[r];
    for (int i = 0; i < 5; i++) {
      const double f = (((c[4] * x + c[3]) * x + c[2]) * x + c[1]) * x + c[0];
      const double x2 = x * x;
      const double x3 = x2 * x;
      const double df = 4.0 * c[4] * x3 + 3.0 * c[3] * x2 + 2.0 * c[2] * x + c[1];
      const double decr = df == 0. ? 0. : f / df;
      if (fabs(decr) < 1e-20) break;
      x -= decr;
    }
    roots[r] = x;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// AbsolutePoseThreePoints.  b / X: rows of 3 doubles; idx: the three rows of the sample.
// ---------------------------------------------------------------------------------------------------------------
struct P3PSetup {  // everything the four back-substitutions share
  double coefficients[5], roots[4];
  double g1, g2, g3, g4, g5, g6, g7, sigma, k3_b3;
  double c_barre[9], c_barre_barre[9], p3[3], b3[3];
};

// RotationMatrixAroundAxis (geometry/src/absolute_pose.cc), row-major
OSFM_HD void rotation_around_axis(double cos_theta, double sin_theta, const double* v, double* R) {
  const double omc = 1.0 - cos_theta;
  R[0] = cos_theta + v[0] * v[0] * omc;
  R[3] = -v[2] * sin_theta + v[0] * v[1] * omc;
  R[6] = v[1] * sin_theta + v[0] * v[2] * omc;
  R[1] = v[2] * sin_theta + v[0] * v[1] * omc;
  R[4] = cos_theta + v[1] * v[1] * omc;
  R[7] = -v[0] * sin_theta + v[1] * v[2] * omc;
  R[2] = -v[1] * sin_theta + v[0] * v[2] * omc;
  R[5] = v[0] * sin_theta + v[1] * v[2] * omc;
  R[8] = cos_theta + v[2] * v[2] * omc;
}

// the part up to RefineQuarticRoots: false where the reference returns no model
OSFM_HD bool p3p_setup(const double* b, const double* X, const int* idx, P3PSetup& S) {
  const double *b1 = b + 3 * idx[0], *b2 = b + 3 * idx[1], *b3 = b + 3 * idx[2];
  const double *p1 = X + 3 * idx[0], *p2 = X + 3 * idx[1], *p3 = X + 3 * idx[2];
  double d12[3], u1[3], u2[3], k1[3], k3[3], b1xb2[3], v1[3], v2[3], u1_k1[3], k3s[3];
  for (int i = 0; i < 3; i++) {
    d12[i] = p1[i] - p2[i];
    u1[i] = p1[i] - p3[i];
    u2[i] = p2[i] - p3[i];
  }
  normalized3(d12, k1);
  cross3(b1, b2, b1xb2);
  normalized3(b1xb2, k3);
  cross3(b1, b3, v1);
  cross3(b2, b3, v2);
  cross3(u1, k1, u1_k1);
  const double sigma = norm3(u1_k1);
  if (sigma == 0.0) return false;
  for (int i = 0; i < 3; i++) k3s[i] = u1_k1[i] / sigma;
  const double k3_b3 = dot3(k3, b3);
  if (k3_b3 == 0.0) return false;
  const double b1_b2 = norm3(b1xb2);
  const double f11 = sigma * k3_b3;
  const double f21 = sigma * dot3(b1, b2) * k3_b3;
  const double f22 = sigma * k3_b3 * b1_b2;
  const double f13 = sigma * dot3(v1, k3);
  const double f23 = sigma * dot3(v2, k3);
  const double f24 = dot3(u2, k1) * k3_b3 * b1_b2;
  const double f15 = -dot3(u1, k1) * k3_b3;
  const double f25 = -dot3(u2, k1) * dot3(b1, b2) * k3_b3;
  const double g1 = f13 * f22;
  const double g2 = f13 * f25 - f15 * f23;
  const double g3 = f11 * f23 - f13 * f21;
  const double g4 = -f13 * f24;
  const double g5 = f11 * f22;
  const double g6 = f11 * f25 - f15 * f21;
  const double g7 = -f15 * f24;
  S.coefficients[4] = g5 * g5 + g1 * g1 + g3 * g3;
  S.coefficients[3] = 2.0 * (g5 * g6 + g1 * g2 + g3 * g4);
  S.coefficients[2] = g6 * g6 + 2.0 * g5 * g7 + g2 * g2 + g4 * g4 - g1 * g1 - g3 * g3;
  S.coefficients[1] = 2.0 * (g6 * g7 - g1 * g2 - g3 * g4);
  S.coefficients[0] = g7 * g7 - g2 * g2 - g4 * g4;
  if (!quartic_roots(S.coefficients, S.roots)) return false;
  refine_quartic_roots(S.coefficients, S.roots);
  double k1xk3s[3], b1xk3[3];
  cross3(k1, k3s, k1xk3s);
  cross3(b1, k3, b1xk3);
  for (int i = 0; i < 3; i++) {
    S.c_barre[3 * i] = k1[i];  // columns k1, k3'', k1 x k3''
    S.c_barre[3 * i + 1] = k3s[i];
    S.c_barre[3 * i + 2] = k1xk3s[i];
    S.c_barre_barre[i] = b1[i];  // rows b1, k3, b1 x k3
    S.c_barre_barre[3 + i] = k3[i];
    S.c_barre_barre[6 + i] = b1xk3[i];
    S.p3[i] = p3[i];
    S.b3[i] = b3[i];
  }
  S.g1 = g1, S.g2 = g2, S.g3 = g3, S.g4 = g4, S.g5 = g5, S.g6 = g6, S.g7 = g7, S.sigma = sigma, S.k3_b3 = k3_b3;
  return true;
}

// the back-substitution of root j: model = [R^T | -R^T t], row-major 3 x 4 (NaN where sqrt(1 - root^2) is: the reference pushes it)
OSFM_HD void p3p_back(const P3PSetup& S, int j, double* model) {
  const double cos_theta_1 = S.roots[j];
  const double sin_theta_1 = (S.k3_b3 < 0.0 ? -1.0 : 1.0) * sqrt(1.0 - cos_theta_1 * cos_theta_1);
  const double t = sin_theta_1 / (S.g5 * (cos_theta_1 * cos_theta_1) + S.g6 * cos_theta_1 + S.g7);
  const double cos_theta_3 = t * (S.g1 * cos_theta_1 + S.g2);
  const double sin_theta_3 = t * (S.g3 * cos_theta_1 + S.g4);
  const double e1[3] = {1.0, 0.0, 0.0}, e2[3] = {0.0, 1.0, 0.0};
  double c1[9], c2[9], A[9], B[9], R[9];
  rotation_around_axis(cos_theta_1, sin_theta_1, e1, c1);
  rotation_around_axis(cos_theta_3, sin_theta_3, e2, c2);
  matmul3(S.c_barre, c1, A);
  matmul3(A, c2, B);
  matmul3(B, S.c_barre_barre, A);
  closest_rotation(A, R);
  double Rb3[3], tr[3], Rtt[3];
  matvec3(R, S.b3, Rb3);
  const double f = (S.sigma * sin_theta_1) / S.k3_b3;
  for (int i = 0; i < 3; i++) tr[i] = S.p3[i] - f * Rb3[i];
  matTvec3(R, tr, Rtt);
  for (int i = 0; i < 3; i++) {
    for (int k = 0; k < 3; k++) model[4 * i + k] = R[3 * k + i];
    model[4 * i + 3] = -Rtt[i];
  }
}

OSFM_HD int p3p_models_idx(const double* b, const double* X, const int* idx, double (*models)[12]) {
  P3PSetup S;
  if (!p3p_setup(b, X, idx, S)) return 0;
  for (int j = 0; j < kMaxModels; j++) p3p_back(S, j, models[j]);
  return kMaxModels;
}
// AbsolutePoseThreePoints on three bearings / points: 0 or 4 models
OSFM_HD int p3p_models(const double* b, const double* X, double (*models)[12]) {
  const int idx[3] = {0, 1, 2};
  return p3p_models_idx(b, X, idx, models);
}
// root j of the sample alone (the lanes of a sample each take one): the number of models the sample has
OSFM_HD int p3p_model_of_root(const double* b, const double* X, const int* idx, int j, double* model) {
  P3PSetup S;
  if (!p3p_setup(b, X, idx, S)) return 0;
  p3p_back(S, j, model);
  return kMaxModels;
}

// ---------------------------------------------------------------------------------------------------------------
// AbsolutePoseNPoints (Lu-Hager) over the rows idx[0 .. count-1] (idx == nullptr: rows 0 .. count-1).  model = [R | t], row-major 3 x 4.
// ---------------------------------------------------------------------------------------------------------------
// Eigen's fixed-size 3 x 3 inverse, restated (see the head of this file)
OSFM_HD void inverse3(const double* m, double* inv) {
  auto cof = [&](int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[3 * i1 + j1] * m[3 * i2 + j2] - m[3 * i1 + j2] * m[3 * i2 + j1];
  };
  const double c0 = cof(0, 0), c1 = cof(1, 0), c2 = cof(2, 0);
  const double det = c0 * m[0] + c1 * m[3] + c2 * m[6];
  const double invdet = 1.0 / det;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) inv[3 * i + j] = cof(j, i) * invdet;
}
// F = v v^T / (v . v)
OSFM_HD void line_projector(const double* v, double* F) {
  const double vv = dot3(v, v);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) F[3 * i + j] = (v[i] * v[j]) / vv;
}
OSFM_HD void translation_between_points(const double* b, const double* X, const int* idx, int count, const double* R, double* t) {
  double F1[9], F2[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < 9; i++) F1[i] = 0.0;
  for (int k = 0; k < count; k++) {
    const int m = idx ? idx[k] : k;
    double F[9], G[9], GR[9], y[3];
    line_projector(b + 3 * m, F);
    for (int i = 0; i < 9; i++) {
      F1[i] += F[i];
      G[i] = F[i] - ((i % 4 == 0) ? 1.0 : 0.0);
    }
    matmul3(G, R, GR);
    matvec3(GR, X + 3 * m, y);
    for (int i = 0; i < 3; i++) F2[i] += y[i];
  }
  double A[9], Ai[9];
  for (int i = 0; i < 3; i++) F2[i] /= (double)count;
  for (int i = 0; i < 9; i++) {
    F1[i] /= (double)count;
    A[i] = ((i % 4 == 0) ? 1.0 : 0.0) - F1[i];
  }
  inverse3(A, Ai);
  matvec3(Ai, F2, t);
}
OSFM_HD void npoints_model(const double* b, const double* X, const int* idx, int count, double* model) {
  auto row = [=](int k) { return idx ? idx[k] : k; };
  auto bearing = [=](int k, double* v) {
    for (int a = 0; a < 3; a++) v[a] = b[3 * row(k) + a];
  };
  auto point = [=](int k, double* v) {
    for (int a = 0; a < 3; a++) v[a] = X[3 * row(k) + a];
  };
  double qa[3] = {0.0, 0.0, 0.0}, pa[3] = {0.0, 0.0, 0.0};  // ComputeAverage
  for (int k = 0; k < count; k++) {
    double q[3], p[3];
    bearing(k, q);
    point(k, p);
    for (int a = 0; a < 3; a++) {
      qa[a] += q[a];
      pa[a] += p[a];
    }
  }
  for (int a = 0; a < 3; a++) {
    qa[a] /= (double)count;
    pa[a] /= (double)count;
  }
  double s_num = 0., s_denum = 0.;
  for (int k = 0; k < count; k++) {
    double q[3], p[3];
    bearing(k, q);
    point(k, p);
    for (int a = 0; a < 3; a++) {
      q[a] = q[a] - qa[a];
      p[a] = p[a] - pa[a];
    }
    const double pn = norm3(p), qn = norm3(q);
    s_num += pn * pn;
    s_denum += qn * qn;
  }
  const double scale = sqrt(s_num / s_denum);
  double R[9], t[3], Rp[3];
  rotation_between_points(bearing, point, count, R);
  matvec3(R, pa, Rp);
  for (int a = 0; a < 3; a++) t[a] = scale * qa[a] - Rp[a];
  OSFM_NOUNROLL for (int it = 0; it < kNPointsIterations; it++) {
    const double* Rc = R;
    const double* tc = t;
    auto projected = [=](int k, double* y) {  // q = F (R p + t)
      const int m = row(k);
      double F[9], v[3];
      line_projector(b + 3 * m, F);
      matvec3(Rc, X + 3 * m, v);
      for (int i = 0; i < 3; i++) v[i] = v[i] + tc[i];
      matvec3(F, v, y);
    };
    double Rn[9], tn[3], dlt[3];
    rotation_between_points(projected, point, count, Rn);
    for (int i = 0; i < 9; i++) R[i] = Rn[i];
    translation_between_points(b, X, idx, count, R, tn);
    for (int a = 0; a < 3; a++) dlt[a] = tn[a] - t[a];
    const double rel_delta = norm3(dlt) / norm3(t);
    if (rel_delta < 1e-7) break;
    for (int a = 0; a < 3; a++) t[a] = tn[a];
  }
  for (int i = 0; i < 3; i++) {
    for (int k = 0; k < 3; k++) model[4 * i + k] = R[3 * i + k];
    model[4 * i + 3] = t[i];
  }
}

// AbsolutePose::Evaluate: e = 1 - normalized(b) . normalized(R X + t); RansacScoring: an inlier when |e| < thr (= 1 - cos(threshold))
OSFM_HD double abspose_error(const double* model, const double* b, const double* X) {
  double v[3], bn[3], pn[3];
  for (int r = 0; r < 3; r++) v[r] = (model[4 * r] * X[0] + model[4 * r + 1] * X[1] + model[4 * r + 2] * X[2]) + model[4 * r + 3];
  normalized3(b, bn);
  normalized3(v, pn);
  return 1.0 - dot3(bn, pn);
}
OSFM_HD bool abspose_ransac_inlier(const double* model, const double* b, const double* X, double thr) {
  return fabs(abspose_error(model, b, X)) < thr;
}
// multiview.absolute_pose_ransac's inversion of a model [R | t]: [R^T | -R^T t]
OSFM_HD void invert_model(const double* model, double* inv) {
  const double t[3] = {model[3], model[7], model[11]};
  for (int i = 0; i < 3; i++) {
    const double s = model[i] * t[0] + model[4 + i] * t[1] + model[8 + i] * t[2];
    for (int k = 0; k < 3; k++) inv[4 * i + k] = model[4 * k + i];
    inv[4 * i + 3] = -s;
  }
}
// resect's inlier test on T = invert_model(lo_model) = [R_c | o]: r = R_c^T (X - o) left to right, normalised; |r - b|.
// (numpy goes through BLAS for the product, which may fuse or reorder: a row within a few ulp of the chord can fall either way there.)
OSFM_HD double abspose_chord(const double* T, const double* b, const double* X) {
  double d[3], r[3];
  for (int i = 0; i < 3; i++) d[i] = X[i] - T[4 * i + 3];
  for (int i = 0; i < 3; i++) r[i] = T[i] * d[0] + T[4 + i] * d[1] + T[8 + i] * d[2];
  const double n = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  for (int i = 0; i < 3; i++) d[i] = r[i] / n - b[i];
  return sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

// ---------------------------------------------------------------------------------------------------------------
// One image, one wavefront: loransac_walk.h's walk over AbsolutePose, then resect's inlier test.
// ---------------------------------------------------------------------------------------------------------------
struct AbsposeModel {  // AbsolutePose on the rows of one image
  static constexpr int kModelSize = 12, kMinimalSamples = osfm_ap::kMinimalSamples, kMaxModels = osfm_ap::kMaxModels;
  static constexpr int kSlots = 16;    // speculative main iterations per block: four lanes per sample, one per root of the quartic
  static constexpr int kLoBatch = 64;  // speculative LO iterations per block: one Lu-Hager solve per lane (up to 100 dependent SVDs:
                                       // the latency of this walk)
  const double *b, *X;
  double thr;
  OSFM_HD int solve_minimal(const int* idx, int root, double* out) const { return p3p_model_of_root(b, X, idx, root, out); }
  OSFM_HD void solve_nonminimal(const int* idx, int size, double* out) const { npoints_model(b, X, idx, size, out); }
  OSFM_HD bool inlier(const double* model, int i) const { return abspose_ransac_inlier(model, b + 3 * i, X + 3 * i, thr); }
};
using AbsposeShared = osfm_lo::WalkShared<AbsposeModel>;

struct AbsposeOut {  // mirrors osfm_abspose_result
  double model[12], lo_model[12];
  int32_t score, iterations, num_inliers;
};

struct AbsposeArgs {
  const double* b;            // bearings, total x 3
  const double* X;            // points, total x 3
  const int64_t* offsets;     // n_images + 1
  const double* stop_bound;   // ShouldStop's bound per best inlier count; image i reads n + 1 doubles at stop_bound + stop_off[i]
  const int64_t* stop_off;
  RngTable rng;               // raw outputs of std::mt19937(42)
  double thr;                 // 1 - cos(threshold)
  double chord;               // resect's inlier chord (= threshold); <= 0: skipped, num_inliers = -1
  int iterations, use_lo, lo_iterations, use_reduction;
  int* scratch;               // total ints: inlier lists of the images with more than kLdsInliers rows
  AbsposeOut* out;
  uint8_t* ransac_mask;       // total, or null: the estimator's inliers
  uint8_t* chord_mask;        // total, or null: resect's inliers
  int* overflow;              // set when the tabulated stream is too short
};

// Estimate<RansacScoring, AbsolutePose> for image p, and resect's inlier test on the inverted lo_model
template <class W>
OSFM_HD void abspose_image(W& w, AbsposeShared& sh, const AbsposeArgs& A, int p) {
  const int64_t o = A.offsets[p];
  const int n = (int)(A.offsets[p + 1] - o);
  const double *b = A.b + 3 * o, *X = A.X + 3 * o;
  int* inliers = n <= kLdsInliers ? sh.inl : A.scratch + o;
  osfm_lo::WalkResult<AbsposeModel> r;
  osfm_lo::walk(w, sh, AbsposeModel{b, X, A.thr}, A, A.stop_bound + A.stop_off[p], n, inliers, r);
  int ninl = -1;
  double T[12];
  invert_model(r.lo_model, T);
  const double chord = A.chord;
  auto chord_inlier = [&](int i) { return abspose_chord(T, b + 3 * i, X + 3 * i) < chord; };
  const bool tail = !r.failed && chord > 0.0;
  if (tail) ninl = w.count_if(n, chord_inlier);
  if (A.ransac_mask) {
    uint8_t* mask = A.ransac_mask + o;
    w.parallel_for(n, [&](int i) { mask[i] = 0; });
    w.parallel_for(r.failed ? 0 : r.best, [&](int i) { mask[inliers[i]] = 1; });
  }
  if (A.chord_mask) {
    uint8_t* mask = A.chord_mask + o;
    w.parallel_for(n, [&](int i) { mask[i] = (tail && chord_inlier(i)) ? 1 : 0; });
  }
  w.single([&]() {
    AbsposeOut& out = A.out[p];
    for (int i = 0; i < 12; i++) {
      out.model[i] = r.model[i];
      out.lo_model[i] = r.lo_model[i];
    }
    out.score = r.best;
    out.iterations = r.iterations;
    out.num_inliers = ninl;
    if (r.failed) *A.overflow = 1;
  });
}

}  // namespace osfm_ap
