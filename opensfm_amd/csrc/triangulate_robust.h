// triangulate_robust.h -- TrackTriangulator.triangulate_robust (opensfm/reconstruction.py:922-1030, `triangulation_type: ROBUST`) for one
// track, over the numerics and the track policy of triangulate_core.h.  Restated literally, quirks included:
//   n < 2: no point.  C = n (n - 1) / 2 pairs (i < j), lexicographic.  Up to kRobustTries = 11 tries, one uniform draw u each:
//   id = int(u * (C - 1)) (a double product, truncated: the last pair is never drawn unless C == 1); an id that an earlier try drew costs
//   the try and nothing else.  TriangulateBearingsMidpoint on the rows (i, j) of rank id alone; invalid ends the try; a valid midpoint
//   goes through PointRefinement over the two rows -> X.  Inliers of X over all rows: |(X - o_k) / |X - o_k| - w_k| < threshold (a chord,
//   strict).  Only when there are more of them than the best so far: new_X = PointRefinement over the inlier rows from X (the midpoint
//   the reference computes over the inliers first is dead code), ls_inliers of new_X over all rows; the best becomes (ls_inliers, new_X)
//   if there are strictly more of them, else (inliers, X).  ratio = |best| / n; stop on ratio == 1, else on
//   log(1 - 0.99) / log(1 - ratio^2) <= i with i the FIRST INDEX OF THE SAMPLED PAIR (the reference's loop variable is shadowed by
//   `i, j = ...`).  After the loop a best of more than one inlier is the point, and exactly the best inliers observe it.
// The tried-ids set needs no storage: every earlier try's id is in it (drawn anew or drawn again), so it is {id(u_k) : k < try} and the
// draws are at hand.
//
// Randomness: track t owns the draws 11 t .. 11 t + 10, either the caller's or robust_draw(seed, t, k) below -- a pure integer function,
// so a track's result never depends on another track or on the grid.
//
// A robust track policy is a track policy of triangulate_core.h plus two masks over the observations, kCandidate and kBest, owned by
// the lane that owns the observation (first(), first() + stride(), ...):
//   bit(which, i) / set_bit(which, i, b)    for an observation of THIS lane only
// MaskedTrack is the view of one mask under which refine() and evaluate() run unchanged: each() skips the rows outside the mask, sum()
// is the policy's -- per lane ascending, then its butterfly -- so the order of a sum is a function of the track's length and the mask.
#pragma once
#include "triangulate_core.h"

namespace osfm_tri {

enum { kNoConsensus = 6 };  // no valid sample, or a best of fewer than 2 inliers
enum { kCandidate = 0, kBest = 1 };
constexpr int kRobustTries = 11;  // "0.99 proba, 60% inliers"
constexpr int kBadDraws = -1;     // triangulate_track_robust: a draw outside [0, 1) or not finite; nothing else was done

// draw k of track t: splitmix64's finaliser over seed + 0x9E3779B97F4A7C15 (11 t + k + 1) (mod 2^64), the top 53 bits scaled by 2^-53
OSFM_HD double robust_draw(uint64_t seed, int64_t t, int k) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(11 * t + k + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * 0x1p-53;
}

// the 11 draws of one track: the caller's, or generated
struct Draws11 {
  const double *given;  // this track's 11 values, or null
  uint64_t seed;
  int64_t t;
  OSFM_HD double operator()(int k) const { return given ? given[k] : robust_draw(seed, t, k); }
};

// pairs (i < j) of n in lexicographic order: those with a first index below i number i (2 n - i - 1) / 2
OSFM_HD int64_t pairs_before(int64_t i, int64_t n) { return i * (2 * n - i - 1) / 2; }

// rank id -> (i, j), 0 <= id < n (n - 1) / 2, n <= 2^24: the root of pairs_before(i) = id in doubles (every operand below 2^51, so only
// the square root rounds), then an integer fix-up
OSFM_HD void unrank_pair(int64_t id, int n, int *pi, int *pj) {
  const double b = 2.0 * (double)n - 1.0;
  int64_t i = (int64_t)((b - sqrt(b * b - 8.0 * (double)id)) / 2.0);
  i = i < 0 ? 0 : i > n - 2 ? n - 2 : i;
  while (pairs_before(i, n) > id) i--;
  while (pairs_before(i + 1, n) <= id) i++;
  *pi = (int)i;
  *pj = (int)(i + 1 + (id - pairs_before(i, n)));
}

// two rows on one lane: every lane of a group runs the two-view solve redundantly, like the 3 x 3 algebra
struct PairTrack {
  int n;
  double o[2][3], w[2][3];
  OSFM_HD int first() const { return 0; }
  OSFM_HD int stride() const { return 1; }
  OSFM_HD void at(int i, double *oo, double *ww) const {
    for (int k = 0; k < 3; k++) {
      oo[k] = o[i][k];
      ww[k] = w[i][k];
    }
  }
  template <class F>
  OSFM_HD void each(F f) const {
    for (int i = 0; i < 2; i++) f(i, o[i], w[i]);
  }
  OSFM_HD void sum(double *, int) const {}
  OSFM_HD int lowest(int key) const { return key; }
  OSFM_HD bool any(bool b) const { return b; }
};

template <class Track>
struct MaskedTrack {
  Track &base;
  int which, n;
  template <class F>
  OSFM_HD void each(F f) const {
    base.each([&](int i, const double *o, const double *w) {
      if (base.bit(which, i)) f(i, o, w);
    });
  }
  OSFM_HD void sum(double *v, int m) const { base.sum(v, m); }
};

// the inliers of X into mask `which`; their number (the same on every lane)
template <class Track>
OSFM_HD int mark_inliers(Track &trk, const double *X, double threshold, int which) {
  double count = 0.0;  // (summed as a double by the policy's one reduction: exact)
  trk.each([&](int i, const double *o, const double *w) {
    const double p[3] = {X[0] - o[0], X[1] - o[1], X[2] - o[2]};
    const double norm = sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
    const double d[3] = {p[0] / norm - w[0], p[1] / norm - w[1], p[2] / norm - w[2]};
    const bool in = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < threshold;
    trk.set_bit(which, i, in);
    count += in ? 1.0 : 0.0;
  });
  trk.sum(&count, 1);
  return (int)count;
}

// One track: status (kOk, kTooFew, kNotFinite, kNoConsensus, or kBadDraws), the point (untouched unless kOk), the number of best
// inliers (mask kBest holds them; 0 unless kOk) and the tries made (draws consumed).
template <class Track>
OSFM_HD int triangulate_track_robust(Track &trk, const Params &prm, const Draws11 &draw, double *X, int *n_inliers, int *tries_used) {
  *n_inliers = *tries_used = 0;
  for (int k = 0; k < kRobustTries; k++) {
    const double u = draw(k);
    if (!(u >= 0.0 && u < 1.0)) return kBadDraws;
  }
  const int n = trk.n;
  if (n < 2) return kTooFew;
  const int64_t C = (int64_t)n * (n - 1) / 2;
  const double log_pout = log(1.0 - 0.99);
  int best = 0, tries = 0;
  double P[3] = {NAN, NAN, NAN};
  while (tries < kRobustTries) {
    const int attempt = tries++;
    const int64_t id = (int64_t)(draw(attempt) * (double)(C - 1));
    bool tried = false;
    for (int k = 0; k < attempt; k++) tried = tried || (int64_t)(draw(k) * (double)(C - 1)) == id;
    if (tried) continue;
    int i, j;
    unrank_pair(id, n, &i, &j);
    PairTrack two;
    two.n = 2;
    trk.at(i, two.o[0], two.w[0]);
    trk.at(j, two.o[1], two.w[1]);
    double Xs[3];
    int unused;
    if (triangulate_track(two, prm, Xs, &unused) != kOk) continue;
    const int inliers = mark_inliers(trk, Xs, prm.threshold, kCandidate);
    if (inliers <= best) continue;
    double Xn[3] = {Xs[0], Xs[1], Xs[2]};
    MaskedTrack<Track> subset{trk, kCandidate, inliers};
    (void)refine(subset, prm.iterations, Xn);
    const int ls_inliers = mark_inliers(trk, Xn, prm.threshold, kBest);
    if (ls_inliers > inliers) {
      best = ls_inliers;
      for (int k = 0; k < 3; k++) P[k] = Xn[k];
    } else {
      best = inliers;
      for (int k = 0; k < 3; k++) P[k] = Xs[k];
      for (int q = trk.first(); q < n; q += trk.stride()) trk.set_bit(kBest, q, trk.bit(kCandidate, q));
    }
    const double ratio = (double)best / (double)n;
    if (ratio == 1.0) break;
    if (log_pout / log(1.0 - ratio * ratio) <= (double)i) break;
  }
  *tries_used = tries;
  if (best < 2) return kNoConsensus;
  if (!(finite_d(P[0]) && finite_d(P[1]) && finite_d(P[2]))) return kNotFinite;
  *n_inliers = best;
  for (int k = 0; k < 3; k++) X[k] = P[k];
  return kOk;
}

}  // namespace osfm_tri
