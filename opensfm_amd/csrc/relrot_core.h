// relrot_core.h -- rotation-only LO-RANSAC of image pairs (the ranking of reconstruction.compute_image_pairs).
//
// reference: reconstruction.compute_image_pairs (opensfm/reconstruction.py:208-244) -> two_view_reconstruction_rotation_only
// (:387-412) -> multiview.relative_pose_ransac_rotation_only (opensfm/multiview.py:520-540) -> pyrobust.ransac_relative_rotation
// (robust/src/instanciations.cc:50-64) = Estimate<RansacScoring, RelativeRotation> (robust/robust_estimator.h:37-119) with
// RelativeRotation (robust/relative_rotation_model.h): 3-point samples, 1 model, RotationBetweenPoints(sample)^T
// (geometry/transform.h:9-40); then _two_view_rotation_inliers (reconstruction.py:377-384) and pairwise_reconstructability (:193-200).
//
// Everything is host + device: tests/native/relrot_host.cpp compiles this header with g++ and runs the very same per-pair walk
// with loops in place of lanes; relrot.hip runs it with one wavefront per pair.  Contraction is off (-ffp-contract=off in
// build.sh), so host and device give the same bits.
//
// Numerics that cannot be pinned here.  The reference computes the model with Eigen (JacobiSVD<Matrix3d>, 3 x 3 products), and
// Eigen is not available to this project.  jacobi_svd3 below restates Eigen's two-sided Jacobi SVD (real 2 x 2 Jacobi SVD per
// (p, q) pair, threshold 2 eps * max |diagonal|, sign fix of U, descending sort) from memory of Eigen 3.3 / 3.4; it is not
// verified against Eigen.  Every 3-term sum (matrix products, dot products) is evaluated left to right; Eigen's unrollers may
// pair the terms differently.  What the tests pin is therefore: this header on the GPU == this header on the host, bit for bit;
// the decision sequence (draws, ties, LO, stopping) == the reference's own robust_estimator.h / random_sampler.h / scorer.h
// compiled with this toolchain around these numerics.
//
// The negation quirk.  RotationBetweenPoints returns R = U V^T and negates the WHOLE matrix when det R < 0.  A minimal sample's
// M = sum q p^T has rank <= 2 (three centred points are coplanar), so the sign of det(U V^T) is the product of the signs the SVD
// happens to give the null-space pair (u3, v3): for about half of the samples the hypothesis is -U V^T.  For an exact rotation R
// that is R followed by a half-turn about R n, n the normal of the plane through the sample's first bearings: it maps a sample's
// first bearing to a point at dot product 2 h^2 - 1 with the second (h: distance of that plane from the origin), and it explains only
// the correspondences whose second bearing lies within about half the threshold angle of the axis +-R n.  This is reproduced
// literally (DESIGN.md §4d2 gives the fraction of samples that take the branch, counted by rotation_model's `negated` flag, with
// this SVD and with osfm_rp::svd3, which completes U by u1 x u2 and would make the branch follow its column sort instead).
//
// Divergence: with fewer than 3 correspondences the reference's sampler loops forever (it cannot draw 3 distinct indices); the
// C ABI rejects such pairs (OSFM_E_INVALID) instead.
#pragma once
#include "loransac_walk.h"

namespace osfm_rr {

using osfm_lo::draw_sample_tab;
using osfm_lo::kLdsInliers;
using osfm_lo::kLoSampleMax;
using osfm_lo::kRngCache;
using osfm_lo::lo_sample_size;
using osfm_lo::RngTable;
using osfm_lo::RngView;

constexpr int kMinimalSamples = 3;  // RelativeRotation::MINIMAL_SAMPLES
constexpr int kSlots = 64;          // speculative main iterations per block: one 3-point solve per lane

// ---------------------------------------------------------------------------------------------------------------
// Eigen::JacobiSVD<Matrix3d>(A, ComputeFullU | ComputeFullV), restated (see above).  A, U, V row-major; S descending.
// A Jacobi rotation (c, s) applied "in the plane" of x, y:  x' = c x + s y,  y' = -s x + c y.
// ---------------------------------------------------------------------------------------------------------------
OSFM_HD void rot_rows(double* M, int p, int q, double c, double s) {  // M.applyOnTheLeft(p, q, J)
  for (int k = 0; k < 3; k++) {
    const double x = M[3 * p + k], y = M[3 * q + k];
    M[3 * p + k] = c * x + s * y;
    M[3 * q + k] = -s * x + c * y;
  }
}
OSFM_HD void rot_cols(double* M, int p, int q, double c, double s) {  // M.applyOnTheRight(p, q, J): the plane rotation of J^T
  for (int k = 0; k < 3; k++) {
    const double x = M[3 * k + p], y = M[3 * k + q];
    M[3 * k + p] = c * x - s * y;
    M[3 * k + q] = s * x + c * y;
  }
}
// JacobiRotation::makeJacobi(x, y, z): the rotation that diagonalises the symmetric [[x, y], [y, z]]
OSFM_HD void make_jacobi(double x, double y, double z, double* c, double* s) {
  const double deno = 2.0 * fabs(y);
  if (deno < 2.2250738585072014e-308) {
    *c = 1.0;
    *s = 0.0;
    return;
  }
  const double tau = (x - z) / deno;
  const double w = sqrt(tau * tau + 1.0);
  const double t = tau > 0.0 ? 1.0 / (tau + w) : 1.0 / (tau - w);
  const double sign_t = t > 0.0 ? 1.0 : -1.0;
  const double n = 1.0 / sqrt(t * t + 1.0);
  *s = -sign_t * (y / fabs(y)) * fabs(t) * n;
  *c = n;
}
OSFM_HD void jacobi_svd3(const double* A, double* U, double* S, double* V) {
  double scale = 0.0;
  for (int i = 0; i < 9; i++) scale = fabs(A[i]) > scale ? fabs(A[i]) : scale;
  for (int i = 0; i < 9; i++) U[i] = V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  if (!(scale <= 1.79769313486231570815e308)) {  // not finite (Eigen reports InvalidInput): identity factors
    for (int i = 0; i < 3; i++) S[i] = 0.0;
    return;
  }
  if (scale == 0.0) scale = 1.0;
  double W[9];
  for (int i = 0; i < 9; i++) W[i] = A[i] / scale;
  const double considerAsZero = 2.2250738585072014e-308, precision = 2.0 * 2.220446049250313e-16;
  double maxDiag = 0.0;
  for (int i = 0; i < 3; i++) maxDiag = fabs(W[4 * i]) > maxDiag ? fabs(W[4 * i]) : maxDiag;
  bool finished = false;
  OSFM_NOUNROLL for (int sweep = 0; sweep < 64 && !finished; sweep++) {  // Eigen: until no pair is above the threshold
    finished = true;
    for (int p = 1; p < 3; p++)
      for (int q = 0; q < p; q++) {
        const double threshold = considerAsZero > precision * maxDiag ? considerAsZero : precision * maxDiag;
        if (!(fabs(W[3 * p + q]) > threshold || fabs(W[3 * q + p]) > threshold)) continue;
        finished = false;
        // real_2x2_jacobi_svd(W, p, q): m = [[W(p,p), W(p,q)], [W(q,p), W(q,q)]]
        double m00 = W[3 * p + p], m01 = W[3 * p + q], m10 = W[3 * q + p], m11 = W[3 * q + q];
        double c1, s1;
        const double t = m00 + m11, d = m10 - m01;
        if (fabs(d) < considerAsZero) {
          s1 = 0.0;
          c1 = 1.0;
        } else {
          const double u = t / d;
          const double tmp = sqrt(1.0 + u * u);
          s1 = 1.0 / tmp;
          c1 = u / tmp;
        }
        {  // m.applyOnTheLeft(0, 1, rot1)
          const double x0 = m00, x1 = m01, y0 = m10, y1 = m11;
          m00 = c1 * x0 + s1 * y0;
          m01 = c1 * x1 + s1 * y1;
          m10 = -s1 * x0 + c1 * y0;
          m11 = -s1 * x1 + c1 * y1;
        }
        double cr, sr;
        make_jacobi(m00, m01, m11, &cr, &sr);
        // j_left = rot1 * j_right.transpose()  (JacobiRotation::operator*, transpose = (c, -s))
        const double cl = c1 * cr - s1 * (-sr), sl = c1 * (-sr) + s1 * cr;
        rot_rows(W, p, q, cl, sl);    // m_workMatrix.applyOnTheLeft(p, q, j_left)
        rot_cols(U, p, q, cl, -sl);   // m_matrixU.applyOnTheRight(p, q, j_left.transpose())
        rot_cols(W, p, q, cr, sr);    // m_workMatrix.applyOnTheRight(p, q, j_right)
        rot_cols(V, p, q, cr, sr);    // m_matrixV.applyOnTheRight(p, q, j_right)
        const double dp = fabs(W[4 * p]), dq = fabs(W[4 * q]);
        const double dm = dp > dq ? dp : dq;
        maxDiag = maxDiag > dm ? maxDiag : dm;
      }
  }
  for (int i = 0; i < 3; i++) {
    const double a = W[4 * i];
    S[i] = fabs(a);
    if (a < 0.0)
      for (int k = 0; k < 3; k++) U[3 * k + i] = -U[3 * k + i];
  }
  for (int i = 0; i < 3; i++) S[i] *= scale;
  for (int i = 0; i < 3; i++) {  // descending; the first maximum wins; stops at an exactly zero maximum
    int pos = i;
    for (int j = i + 1; j < 3; j++)
      if (S[j] > S[pos]) pos = j;
    if (S[pos] == 0.0) break;
    if (pos != i) {
      const double ts = S[i];
      S[i] = S[pos];
      S[pos] = ts;
      for (int k = 0; k < 3; k++) {
        const double tu = U[3 * k + i], tv = V[3 * k + i];
        U[3 * k + i] = U[3 * k + pos];
        U[3 * k + pos] = tu;
        V[3 * k + i] = V[3 * k + pos];
        V[3 * k + pos] = tv;
      }
    }
  }
}

// ClosestRotationMatrix (foundation/src/numeric.cc:11-19) and the tail of RotationBetweenPoints: R = U V^T (3-term sums left to right),
// the WHOLE matrix negated when det R < 0.  R row-major; negated (optional): whether that branch was taken.
OSFM_HD void closest_rotation(const double* M, double* R, int* negated = nullptr) {
  double U[9], S[3], V[9];
  jacobi_svd3(M, U, S, V);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + U[3 * i + 2] * V[3 * j + 2];
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[3] * (R[1] * R[8] - R[7] * R[2]) + R[6] * (R[1] * R[5] - R[4] * R[2]);
  const double sign = det < 0.0 ? -1.0 : 1.0;
  if (negated) *negated = det < 0.0;
  for (int i = 0; i < 9; i++) R[i] = R[i] * sign;
}

// RotationBetweenPoints (geometry/transform.h:21-40) over `count` pairs; first(k, v) / second(k, v) write the two vectors of pair k to v[3]
// (they are called twice per pair: once for the centroids, once for M).  Operation order: centroids = sum in order, then / count;
// M(i, j) = sum over the pairs (from 0.0) of q_i p_j with q = first - centroid, p = second - centroid; closest_rotation(M).  Not transposed.
template <class FA, class FB>
OSFM_HD void rotation_between_points(FA first, FB second, int count, double* R, int* negated = nullptr) {
  double qa[3] = {0.0, 0.0, 0.0}, pa[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < count; k++) {
    double q[3], p[3];
    first(k, q);
    second(k, p);
    for (int a = 0; a < 3; a++) {
      qa[a] += q[a];
      pa[a] += p[a];
    }
  }
  for (int a = 0; a < 3; a++) {
    qa[a] /= (double)count;
    pa[a] /= (double)count;
  }
  double M[9];
  for (int i = 0; i < 9; i++) M[i] = 0.0;
  for (int k = 0; k < count; k++) {
    double q[3], p[3];
    first(k, q);
    second(k, p);
    for (int a = 0; a < 3; a++) {
      q[a] = q[a] - qa[a];
      p[a] = p[a] - pa[a];
    }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) M[3 * i + j] += q[i] * p[j];
  }
  closest_rotation(M, R, negated);
}

// RotationBetweenPoints over the correspondences idx[0 .. count-1] (first = b1, second = b2), transposed: the RelativeRotation model
// (row-major).  negated (optional): set to whether the det R < 0 branch was taken.
OSFM_HD void rotation_model(const double* b1, const double* b2, const int* idx, int count, double* model, int* negated = nullptr) {
  double R[9];
  auto first = [=](int k, double* v) {
    for (int a = 0; a < 3; a++) v[a] = b1[3 * idx[k] + a];
  };
  auto second = [=](int k, double* v) {
    for (int a = 0; a < 3; a++) v[a] = b2[3 * idx[k] + a];
  };
  rotation_between_points(first, second, count, R, negated);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) model[3 * i + j] = R[3 * j + i];
}

// RelativeRotation::Evaluate: e = 1 - (model first) . second; RansacScoring: an inlier when |e| < thr (= 1 - cos(threshold))
OSFM_HD double rotation_error(const double* model, const double* x, const double* y) {
  double v[3];
  for (int r = 0; r < 3; r++) v[r] = model[3 * r] * x[0] + model[3 * r + 1] * x[1] + model[3 * r + 2] * x[2];
  return 1.0 - (v[0] * y[0] + v[1] * y[1] + v[2] * y[2]);
}
OSFM_HD bool rotation_ransac_inlier(const double* model, const double* x, const double* y, double thr) {
  return fabs(rotation_error(model, x, y)) < thr;
}
// _two_view_rotation_inliers with R = lo_model^T: |R b2 - b1| < chord.  (R b2)_r = sum_k lo_model(k, r) b2_k left to right, then
// the difference, then sqrt((d0^2 + d1^2) + d2^2).  (numpy goes through BLAS for R.dot(b2.T), which may fuse or reorder: a
// correspondence within a few ulp of the chord can fall either way there.)
OSFM_HD double rotation_chord(const double* lo_model, const double* x, const double* y) {
  double d[3];
  for (int r = 0; r < 3; r++) d[r] = (lo_model[r] * y[0] + lo_model[3 + r] * y[1] + lo_model[6 + r] * y[2]) - x[r];
  return sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}
// pairwise_reconstructability (reconstruction.py:193-200)
OSFM_HD int pairwise_reconstructability(int common_tracks, int rotation_inliers) {
  const int outliers = common_tracks - rotation_inliers;
  const double ratio = (double)outliers / (double)common_tracks;
  return ratio >= 0.3 ? outliers : 0;
}
// ---------------------------------------------------------------------------------------------------------------
// One pair, one wavefront (policy W as in loransac_walk.h: single / parallel_for / count_if / compact / stage_rng).  This is the walk of
// loransac_walk.h written out for one model per sample and a local optimisation solved one sample at a time: as an instantiation of
// walk<W, M> rr_pairs_kernel measured 3.9 % slower on the MI355X, and what the template changed was not found.
// ---------------------------------------------------------------------------------------------------------------
struct RelrotOut {  // mirrors osfm_relrot_result
  double model[9], lo_model[9];
  int32_t score, iterations, n_rotation_inliers, reconstructability;
};

struct RelrotShared {  // LDS of a walk
  uint32_t rng[kRngCache];
  double models[kSlots][9];
  int sidx[kSlots][kMinimalSamples];
  int pos_after[kSlots];
  double lo[9];
  int lidx[kLoSampleMax];
  int lo_pos, overflow;
  int inl[kLdsInliers];
};

struct RelrotArgs {
  const double* b1;  // bearings as handed over (first / second of the samples), total x 3
  const double* b2;
  const int64_t* offsets;     // n_pairs + 1
  const double* stop_bound;   // ShouldStop's bound per best inlier count; pair p reads n + 1 doubles at stop_bound + stop_off[p]
  const int64_t* stop_off;
  RngTable rng;               // raw outputs of std::mt19937(42)
  double thr;                 // 1 - cos(threshold)
  double chord;               // inlier chord of the rotation-only count (<= 0: skipped)
  int iterations, use_lo, lo_iterations, use_reduction;
  int* scratch;               // total ints: inlier lists of the pairs with more than kLdsInliers correspondences
  RelrotOut* out;
  uint8_t* mask;              // total, or null
  int* overflow;              // set when the tabulated stream is too short
};

// Estimate<RansacScoring, RelativeRotation> for pair p.  The samples of the next `width` iterations are drawn by lane 0 and solved
// one per lane, assuming no local optimisation fires in between; when one does, the generator has moved and the remaining slots of
// the block are dropped (the next block draws from where the generator stands) -- the decision sequence is the sequential one.
template <class W>
OSFM_HD void relrot_pair(W& w, RelrotShared& sh, const RelrotArgs& A, int p) {
  const int64_t o = A.offsets[p];
  const int n = (int)(A.offsets[p + 1] - o);
  const double *b1 = A.b1 + 3 * o, *b2 = A.b2 + 3 * o;
  int* inliers = n <= kLdsInliers ? sh.inl : A.scratch + o;
  const double* stop_bound = A.stop_bound + A.stop_off[p];
  const double thr = A.thr;
  auto is_inlier = [&](const double* mdl) { return [=](int i) { return rotation_ransac_inlier(mdl, b1 + 3 * i, b2 + 3 * i, thr); }; };
  int pos = 0, it = 0, best = 0, width = 1, stop = 0, failed = 0;
  double model[9], lo_model[9];
  for (int i = 0; i < 9; i++) model[i] = lo_model[i] = 0.0;
  while (it < A.iterations && !stop && !failed) {
    int B = width < kSlots ? width : kSlots;
    if (B > A.iterations - it) B = A.iterations - it;
    const RngView V = w.stage_rng(A.rng, sh.rng, pos, true);
    w.single([&]() {
      int q = pos, ovf = 0;
      for (int k = 0; k < B; k++) {
        q = draw_sample_tab(V, q, kMinimalSamples, n, sh.sidx[k], &ovf);
        sh.pos_after[k] = q;
      }
      sh.overflow = ovf;
    });
    if (sh.overflow) {
      failed = 1;
      break;
    }
    w.parallel_for(B, [&](int k) { rotation_model(b1, b2, sh.sidx[k], kMinimalSamples, sh.models[k]); });
    int lo_fired = 0;
    for (int k = 0; k < B && !stop && !lo_fired && !failed; k++) {
      pos = sh.pos_after[k];
      double mk[9];
      for (int i = 0; i < 9; i++) mk[i] = sh.models[k][i];
      const int cnt = w.count_if(n, is_inlier(mk));
      if (cnt >= best) {  // std::max(score, best_score): ties keep the newcomer
        best = cnt;
        (void)w.compact(n, is_inlier(mk), inliers);
        for (int i = 0; i < 9; i++) model[i] = lo_model[i] = mk[i];
      }
      if (cnt == best && cnt >= kMinimalSamples && A.use_lo && A.lo_iterations > 0) {
        lo_fired = 1;
        const RngView V2 = w.stage_rng(A.rng, sh.rng, pos, true);
        for (int l = 0; l < A.lo_iterations; l++) {
          const int size = lo_sample_size(best, kMinimalSamples);
          w.single([&]() {
            int pick[kLoSampleMax], ovf = 0;
            sh.lo_pos = draw_sample_tab(V2, pos, size, best, pick, &ovf);
            for (int i = 0; i < size; i++) sh.lidx[i] = inliers[pick[i]];
            sh.overflow = ovf;
          });
          if (sh.overflow) {
            failed = 1;
            break;
          }
          pos = sh.lo_pos;
          w.parallel_for(1, [&](int) { rotation_model(b1, b2, sh.lidx, size, sh.lo); });
          double lm[9];
          for (int i = 0; i < 9; i++) lm[i] = sh.lo[i];
          const int c2 = w.count_if(n, is_inlier(lm));
          if (c2 >= best) {  // lo_score.model = best_score.model: only lo_model changes
            best = c2;
            (void)w.compact(n, is_inlier(lm), inliers);
            for (int i = 0; i < 9; i++) lo_model[i] = lm[i];
          }
        }
      }
      if (A.use_reduction) stop = stop_bound[best] < (double)it;
      it++;
    }
    // new bests come early and in bursts: speculate little right after a local optimisation, more once the blocks run through
    width = lo_fired ? it / 2 + 2 : 2 * B;
  }
  int nrot = -1, recon = 0;
  if (A.chord > 0.0 && !failed) {
    const double chord = A.chord;
    nrot = w.count_if(n, [&](int i) { return rotation_chord(lo_model, b1 + 3 * i, b2 + 3 * i) < chord; });
    recon = pairwise_reconstructability(n, nrot);
  }
  if (A.mask) {
    uint8_t* mask = A.mask + o;
    w.parallel_for(n, [&](int i) { mask[i] = 0; });
    w.parallel_for(failed ? 0 : best, [&](int i) { mask[inliers[i]] = 1; });
  }
  w.single([&]() {
    RelrotOut& r = A.out[p];
    for (int i = 0; i < 9; i++) {
      r.model[i] = model[i];
      r.lo_model[i] = lo_model[i];
    }
    r.score = best;
    r.iterations = it;
    r.n_rotation_inliers = nrot;
    r.reconstructability = recon;
    if (failed) *A.overflow = 1;
  });
}

}  // namespace osfm_rr
