// ba_generic.inc -- the streaming Schur solver of ba.hip for EVERYTHING sfm::BAHelpers::Bundle builds (included by ba.hip inside its
// anonymous namespace, after the kernels of the [k1 k2 focal] configuration and before the host side).
//
// osfm_ba_solve's kernels are specialised for one situation: perspective / fisheye cameras with three intrinsics, one shot per pose, a
// camera block of three columns.  What bundle::BundleAdjuster::Run (opensfm/src/bundle/src/bundle_adjuster.cc:595-1121) is handed by
// BAHelpers::Bundle (opensfm/src/sfm/src/ba_helpers.cc:581-763) on a calibrated data set is wider: any of the ten projection types with
// up to 16 free native parameters (camera_instances.h:127-160), rig cameras composed with rig instances (error_utils.h:68-85), GPS
// priors through a per-camera similarity bias (bias.h:33-53), control points (point priors), depth priors, the 3-row bearing residual
// of spherical cameras, compass / inclinometer priors.  Round 4 sent all of that to a DENSE reduced system factorised by rocSOLVER --
// O(n^2) memory, no scaling.  Here the same problems run through the streaming solver's own linear algebra:
//
//   unknowns      x = [6 per rig INSTANCE (the band, co-visibility order) | NB border unknowns: free rig cameras (6 each), free cameras
//                 (their native parameters), free biases (7 each)]; points eliminated on the fly (Hhat_p, never stored as a matrix)
//   observation   rows of NR = 2 (3 with a spherical camera) residuals, stored SoA in point-major order like the fast path (round 6: the
//                 per-instance kernels recompute the rows they need, gen_sm_row, instead of reading a second, shot-major copy):
//                 res NR | Jp NR x 3 | Jc NR x 6 (instance pose) | Jb NR x KW (the border columns the observation's view touches:
//                 camera parameters, then the rig camera pose), KW = the widest view.  With NR = 2 the first 20 components are the
//                 fast path's layout: the band assembly on the matrix cores (band_mfma_kernel) and the per-shot assembly run unchanged.
//   priors        every non-reprojection residual family (camera, rig camera, position through the bias, up vector, pan / tilt /
//                 roll) is differentiated by dual numbers, one thread per block, and lands in three small arrays: PI (6 x 6 per
//                 instance), Bpri (border x instance rows), Cpri (border x border); the mat-vec applies them explicitly.
//   linear solve  the streaming solver's: exact band (cyclic reduction in LDS / over dense clusters), the border eliminated exactly
//                 (Sigma = C - B^T A^-1 B, NB <= kGenMaxNB), PCG on the implicit Schur complement to confirm / as the fallback.
//
// The mat-vec, gradients and costs are atomics-free (fixed summation orders); only the prior blocks (a handful of terms per entry) are
// accumulated with atomics.

constexpr int kGenMaxKW = 22;  // 16 native camera parameters + the 6 of a rig camera pose
constexpr int kGenMaxNB = 100;  // border unknowns the exact elimination carries: Sigma's augmented array [Sigma | I] (NB x 2 NB doubles) in one workgroup's
                                // 160 KB of LDS (round 6; 64 until round 5 -- seven Brown cameras; now eleven).  Every cost of the exact border grows with NB
                                // (its columns' passes over the observations, (NB + 1) / 7 walks of the cyclic reduction, NB^2 dot products): beyond this
                                // the band still preconditions the instance block, the border rows are Jacobi-preconditioned and CG carries the coupling

#define GA(o, c) d.Jpm[(long)(c) * d.M + (o)]

__device__ __forceinline__ void gen_atomic_add(double *p, double v) { atomicAdd(p, v); }

// ---- residual rows of one observation ---------------------------------------------------------------------------------------------
// res (nres <= 3), Jp (3 x 3), Ji (3 x 6, instance pose), Jr (3 x 6, rig camera pose), K (3 x 16, camera parameters); rows beyond nres are
// zero.  WorldToCameraCoordinatesRig (error_utils.h:68-85): Xc = R_rc (R_i (X - t_i) - t_rc) with the rotation blocks of
// shot_rot_kernel (R = R(-r), dR[k] = dR / da_k, a = -r).  kind 0: reprojection (2-D through project_full, or the unit bearing of a
// spherical camera, projection_errors.h:208-246); 1 / 2: RelativeDepthError on z / on the norm (relative_depth_error.h:21-39).
// MODEL >= 0: every camera of the problem has that projection type (the common case: one camera model per data set) -- the branches of
// project_full and the widths of its parameter Jacobian fold at compile time
template <bool JAC, int MODEL = -1>
__device__ __forceinline__ void gen_rows(const Dev &d, const double *cam, const double *rcp, const double *poses, const double *pts, int v, int p,
                                         int kind, double ox, double oy, double sigma, double *res, int &nres, double *Jp, double *Ji, double *Jr,
                                         double *K, double *Xc_out = nullptr) {
  const GenDev &g = d.g;
  const int s = g.view_inst[v], q = g.view_rc[v], c = g.view_cam[v];
  const int model = MODEL >= 0 ? MODEL : d.cam_model[c];
  const double *X = pts + 3 * (long)p, *pi = poses + 6 * (long)s, *pr = rcp + 6 * (long)q;
  const double *Ri = d.shotR + 36 * (long)s, *dRi = Ri + 9;
  const double *Rr = g.rcR + 36 * (long)q, *dRr = Rr + 9;
  const bool use_rc = g.rc_useful[q] != 0;
  const double qv[3] = {X[0] - pi[3], X[1] - pi[4], X[2] - pi[5]};
  double Xi[3], Xc[3], w[3] = {0, 0, 0};
#pragma unroll
  for (int a = 0; a < 3; a++) Xi[a] = Ri[3 * a] * qv[0] + Ri[3 * a + 1] * qv[1] + Ri[3 * a + 2] * qv[2];
  if (use_rc) {
#pragma unroll
    for (int a = 0; a < 3; a++) w[a] = Xi[a] - pr[3 + a];
#pragma unroll
    for (int a = 0; a < 3; a++) Xc[a] = Rr[3 * a] * w[0] + Rr[3 * a + 1] * w[1] + Rr[3 * a + 2] * w[2];
  } else {
#pragma unroll
    for (int a = 0; a < 3; a++) Xc[a] = Xi[a];
  }
  if (Xc_out) {
    Xc_out[0] = Xc[0];
    Xc_out[1] = Xc[1];
    Xc_out[2] = Xc[2];
  }
  double A[9];  // d residual / d Xc
  const double is = 1.0 / sigma;
  if (JAC)
    for (int e = 0; e < 48; e++) K[e] = 0.0;
  if (kind != 0) {
    nres = 1;
    const double n = sqrt(Xc[0] * Xc[0] + Xc[1] * Xc[1] + Xc[2] * Xc[2]);
    res[0] = is * ((kind == 2 ? n : Xc[2]) - ox);
    res[1] = res[2] = 0.0;
    if (JAC) {
      for (int e = 0; e < 9; e++) A[e] = 0.0;
      if (kind == 2) {
        for (int e = 0; e < 3; e++) A[e] = is * Xc[e] / n;
      } else {
        A[2] = is;
      }
    }
  } else if (model == OSFM_CAMERA_SPHERICAL) {
    nres = 3;
    const double n2 = Xc[0] * Xc[0] + Xc[1] * Xc[1] + Xc[2] * Xc[2], n = sqrt(n2);
    const double lon = ox * 2 * M_PI, lat = -oy * 2 * M_PI;
    const double b[3] = {cos(lat) * sin(lon), -sin(lat), cos(lat) * cos(lon)};
    for (int a = 0; a < 3; a++) res[a] = is * (Xc[a] / n - b[a]);
    if (JAC)
      for (int a = 0; a < 3; a++)
        for (int e = 0; e < 3; e++) A[3 * a + e] = is * ((a == e ? 1.0 : 0.0) - Xc[a] * Xc[e] / n2) / n;
  } else {
    nres = 2;
    double out[2], JX[6], JK[32];
    project_full<JAC>(model, cam + 16 * (long)c, Xc, out, JX, JK);
    res[0] = is * (out[0] - ox);
    res[1] = is * (out[1] - oy);
    res[2] = 0.0;
    if (JAC) {
      for (int e = 0; e < 6; e++) A[e] = is * JX[e];
      for (int e = 6; e < 9; e++) A[e] = 0.0;
      for (int e = 0; e < 32; e++) K[e] = is * JK[e];
    }
  }
  if (!JAC) return;
  double B[9];  // d residual / d Xi
  if (use_rc) {
    for (int a = 0; a < 3; a++)
      for (int e = 0; e < 3; e++) B[3 * a + e] = A[3 * a] * Rr[e] + A[3 * a + 1] * Rr[3 + e] + A[3 * a + 2] * Rr[6 + e];
    for (int a = 0; a < 3; a++) {
      for (int k = 0; k < 3; k++) {
        double u[3];
        for (int e = 0; e < 3; e++) u[e] = dRr[9 * k + 3 * e] * w[0] + dRr[9 * k + 3 * e + 1] * w[1] + dRr[9 * k + 3 * e + 2] * w[2];
        Jr[6 * a + k] = -(A[3 * a] * u[0] + A[3 * a + 1] * u[1] + A[3 * a + 2] * u[2]);  // the pose stores r, the map rotates by a = -r
      }
      for (int e = 0; e < 3; e++) Jr[6 * a + 3 + e] = -B[3 * a + e];
    }
  } else {
    for (int e = 0; e < 9; e++) B[e] = A[e];
    for (int e = 0; e < 18; e++) Jr[e] = 0.0;
  }
  for (int a = 0; a < 3; a++) {
    for (int e = 0; e < 3; e++) {
      const double t = B[3 * a] * Ri[e] + B[3 * a + 1] * Ri[3 + e] + B[3 * a + 2] * Ri[6 + e];
      Jp[3 * a + e] = t;
      Ji[6 * a + 3 + e] = -t;
    }
    for (int k = 0; k < 3; k++) {
      double u[3];
      for (int e = 0; e < 3; e++) u[e] = dRi[9 * k + 3 * e] * qv[0] + dRi[9 * k + 3 * e + 1] * qv[1] + dRi[9 * k + 3 * e + 2] * qv[2];
      Ji[6 * a + k] = -(B[3 * a] * u[0] + B[3 * a + 1] * u[1] + B[3 * a + 2] * u[2]);
    }
  }
}

__global__ void gen_rc_rot_kernel(Dev d, const double *rcp) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= d.g.NRC) return;
  rot_and_derivs(rcp + 6 * q, d.g.rcR + 36 * (long)q, d.g.rcR + 36 * (long)q + 9);
}

// The border slots of point-major row o in the COMPACT layout: jb[e][i] = wt (is JK[16 e + i]) for the camera's nkc parameters (0 beyond; a constant camera
// has none), rebuilt from the row's Xc and wt, the observation's sigma and the camera at the linearisation point (g.cam) -- what gen_eval_kernel stores in
// the full layout, operation by operation
template <int MODEL>
__device__ __forceinline__ void gen_compact_jb(const Dev &d, long o, int vw, double (&jb)[2][16], int &nkc) {
  const GenDev &g = d.g;
  const int c = g.view_cam[vw];
  nkc = g.cam_col[c] >= 0 ? model_num_params(MODEL) : 0;
  const double Xc[3] = {GA(o, g.oJb), GA(o, g.oJb + 1), GA(o, g.oJb + 2)};
  const double wt = GA(o, g.oJb + 3), is = 1.0 / d.o_sigma[o];
  double out[2], JX[6], JK[32];
  project_full<true>(MODEL, g.cam + 16 * (long)c, Xc, out, JX, JK);
#pragma unroll
  for (int e = 0; e < 2; e++)
#pragma unroll
    for (int i = 0; i < 16; i++) jb[e][i] = i < nkc ? wt * (is * JK[16 * e + i]) : 0.0;
}
__device__ __forceinline__ double gen_pick16(const double (&a)[16], int slot) {
  double v = 0.0;
#pragma unroll
  for (int i = 0; i < 16; i++) v = slot == i ? a[i] : v;
  return v;
}

// residuals (+ Jacobian rows), robust corrector, cost partials: the generic twin of eval_kernel.  Component layout of a row:
// [0, NR) residual | [oJp, oJp + 3 NR) Jp | [oJc, oJc + 6 NR) Jc | [oJb + e KW + i] border slot i of residual row e.
// COMPACT (round 6; one 2-D projection type for every camera, no depth priors, no free rig camera): the border slots -- 2 KW doubles per observation,
// 144 B for a Brown camera -- are not stored; the row keeps the point in the camera frame and the robust weight (Xc | wt at the slots' place, 32 B) and
// the readers of the slots (pass A of the mat-vec, the back-substitution, the border's point pass) rebuild them with project_full on the same Xc:
// wt (is JK), the expressions of this kernel, the same bits (gen_compact_jb)
template <int NR, bool JAC, int MODEL = -1, bool COMPACT = false>
__global__ void __launch_bounds__(TPB) gen_eval_kernel(Dev d, const double *cam, const double *rcp, const double *poses, const double *pts, int loss,
                                                        double a) {
  __shared__ double lds[8];
  const GenDev &g = d.g;
  const long o = (long)blockIdx.x * TPB + threadIdx.x;
  double acc[2] = {0.0, 0.0};
  if (o < d.M) {
    const int v = g.o_view[o], p = d.o_point[o];
    const int kind = g.o_kind ? g.o_kind[o] : 0;
    const double sg = d.o_sigma[o];
    double res[3], Jp[9], Ji[18], Jr[18], K[48], Xc[3];
    int nres;
    gen_rows<JAC, MODEL>(d, cam, rcp, poses, pts, v, p, kind, d.o_x[o], d.o_y[o], sg, res, nres, Jp, Ji, Jr, K, Xc);
    const double sq = res[0] * res[0] + res[1] * res[1] + res[2] * res[2];
    double rho, rho1;
    loss_eval(loss, a, sq, rho, rho1);
    acc[0] = 0.5 * rho;
    acc[1] = kind == 0 ? sq * sg * sg : 0.0;
    if (JAC) {
      const double wt = sqrt(rho1);
      const int c = g.view_cam[v], q = g.view_rc[v];
      const int nkc = g.cam_col[c] >= 0 ? model_num_params(MODEL >= 0 ? MODEL : d.cam_model[c]) : 0;
      const bool rc_free = g.rc_col[q] >= 0 && g.rc_useful[q];
      double *dst = d.Jpm + o;
      const long M = d.M;
#pragma unroll
      for (int e = 0; e < NR; e++) dst[(long)e * M] = wt * res[e];
#pragma unroll
      for (int e = 0; e < NR; e++)
#pragma unroll
        for (int j = 0; j < 3; j++) dst[(long)(g.oJp + 3 * e + j) * M] = wt * Jp[3 * e + j];
      // (the instance's translation columns are -Jp exactly -- gen_rows forms them so -- and are not stored: their readers take Jp with the other sign, the same
      //  bits; 48 B per observation less to write here and to read in pass A of the mat-vec and in the band assembly)
#pragma unroll
      for (int e = 0; e < NR; e++)
#pragma unroll
        for (int j = 0; j < 3; j++) dst[(long)(g.oJc + 6 * e + j) * M] = wt * Ji[6 * e + j];
      if (COMPACT) {
        dst[(long)(g.oJb + 0) * M] = Xc[0];
        dst[(long)(g.oJb + 1) * M] = Xc[1];
        dst[(long)(g.oJb + 2) * M] = Xc[2];
        dst[(long)(g.oJb + 3) * M] = wt;
      }
#pragma unroll
      for (int e = 0; e < NR; e++) {
        if (COMPACT) break;
        const long base = g.oJb + (long)e * g.KW;
#pragma unroll
        for (int i = 0; i < 16; i++)
          if (i < nkc) dst[(base + i) * M] = wt * K[16 * e + i];
#pragma unroll
        for (int k = 0; k < 6; k++)
          if (rc_free) dst[(base + nkc + k) * M] = wt * Jr[6 * e + k];
        for (int i = nkc + (rc_free ? 6 : 0); i < g.KW; i++) dst[(base + i) * M] = 0.0;
      }
      if (d.Epm) {  // E_o = Jc_o^T Jp_o (6 x 3), the per-shot band assembly's operand
        double *E = d.Epm + 18 * o;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) {
            double t = 0.0;
#pragma unroll
            for (int e = 0; e < NR; e++) t += (wt * Ji[6 * e + i]) * (wt * Jp[3 * e + j]);
            E[3 * i + j] = t;
          }
      }
    }
  }
  block_sum<2, TPB>(acc, lds);
  if (threadIdx.x == 0) {
    d.partial[2 * blockIdx.x] = acc[0];
    d.partial[2 * blockIdx.x + 1] = acc[1];
  }
}

// The row of shot-major position k (an observation of view vw, uniform over the wavefront) as gen_eval_kernel stores it in the point-major
// copy -- residual | Jp | Jc | border slots, all times the robust weight -- recomputed at the CURRENT parameters (g.cam, g.rc, d.poses, d.pts and
// the rotation blocks of that point).  The per-instance kernels (gradient, pass B of the mat-vec and of the border's columns, block Jacobi) read
// a second, shot-major copy of the rows until round 5: a second evaluation launch and (10 + KW) NR doubles per observation written, then re-read by
// every pass.  Same device function, same operands: the same bits.  wt < 0: the weight is formed here from `loss` (the gradient kernel, which
// leaves it in sm_wt for the others); the return value is the weight used.
// MODEL >= 0: every camera of the problem has that projection type (as in gen_eval_kernel): project_full's branches and the border slots' layout fold
// at compile time -- the unspecialised rows index their parameter Jacobian dynamically (scratch memory, one wave per SIMD).
template <int NR, int KWT, bool WANT_B, int MODEL = -1>
__device__ __forceinline__ double gen_sm_row(const Dev &d, int vw, long k, double wt, int loss, double la, double (&res)[NR], double (&Jp)[NR][3], double (&Jc)[NR][6],
                                             double (&Jb)[NR][KWT]) {
  const GenDev &g = d.g;
  double r3[3], jp9[9], ji[18], jr[18], K[48];
  int nres;
  gen_rows<true, MODEL>(d, g.cam, g.rc, d.poses, d.pts, vw, d.sm_point[k], g.sm_kind ? g.sm_kind[k] : 0, d.sm_x[k], d.sm_y[k], d.sm_sigma[k], r3, nres, jp9, ji, jr, K);
  if (wt < 0) {
    double rho, rho1;
    loss_eval(loss, la, r3[0] * r3[0] + r3[1] * r3[1] + r3[2] * r3[2], rho, rho1);
    wt = sqrt(rho1);
  }
#pragma unroll
  for (int e = 0; e < NR; e++) {
    res[e] = wt * r3[e];
#pragma unroll
    for (int j = 0; j < 3; j++) Jp[e][j] = wt * jp9[3 * e + j];
#pragma unroll
    for (int j = 0; j < 6; j++) Jc[e][j] = wt * ji[6 * e + j];
  }
  if (WANT_B) {
    const int c = g.view_cam[vw], q = g.view_rc[vw];
    const bool cam_free = g.cam_col[c] >= 0;
    const int nkc = cam_free ? model_num_params(MODEL >= 0 ? MODEL : d.cam_model[c]) : 0;
    const bool rc_free = g.rc_col[q] >= 0 && g.rc_useful[q];
#pragma unroll
    for (int e = 0; e < NR; e++)
#pragma unroll
      for (int i = 0; i < KWT; i++) {
        double val = 0.0;
        if (i < 16 && i < nkc) val = wt * K[16 * e + (i < 16 ? i : 0)];
        if (rc_free) {  // the rig camera's six columns follow the camera's nkc
#pragma unroll
          for (int kk = 0; kk < 6; kk++)
            if (i - nkc == kk) val = wt * jr[6 * e + kk];
        }
        Jb[e][i] = val;
      }
  }
  return wt;
}

// plain residuals with sigma = 1 (ComputeReprojectionErrors, bundle_adjuster.cc:1196-1208), three per row, point-major order
__global__ void gen_reproj_kernel(Dev d, double *out) {
  const long o = (long)blockIdx.x * TPB + threadIdx.x;
  if (o >= d.M) return;
  const GenDev &g = d.g;
  const int kind = g.o_kind ? g.o_kind[o] : 0;
  double res[3], dummy[1];
  int nres;
  gen_rows<false>(d, g.cam, g.rc, d.poses, d.pts, g.o_view[o], d.o_point[o], kind, d.o_x[o], d.o_y[o], 1.0, res, nres, dummy, dummy, dummy, dummy);
  for (int e = 0; e < 3; e++) out[3 * o + e] = kind == 0 ? res[e] : 0.0;
}

// ---- dual numbers for the prior families (what the reference's autodiff does) -----------------------------------------------------
template <int N>
struct Jet {
  double v, d[N];
};
template <int N>
__device__ __forceinline__ Jet<N> jc(double c) {
  Jet<N> r;
  r.v = c;
  for (int i = 0; i < N; i++) r.d[i] = 0.0;
  return r;
}
template <int N>
__device__ __forceinline__ Jet<N> jv(double c, int k) {
  Jet<N> r = jc<N>(c);
  r.d[k] = 1.0;
  return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator+(Jet<N> a, const Jet<N> &b) {
  a.v += b.v;
  for (int i = 0; i < N; i++) a.d[i] += b.d[i];
  return a;
}
template <int N>
__device__ __forceinline__ Jet<N> operator-(Jet<N> a, const Jet<N> &b) {
  a.v -= b.v;
  for (int i = 0; i < N; i++) a.d[i] -= b.d[i];
  return a;
}
template <int N>
__device__ __forceinline__ Jet<N> operator*(const Jet<N> &a, const Jet<N> &b) {
  Jet<N> r;
  r.v = a.v * b.v;
  for (int i = 0; i < N; i++) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator*(Jet<N> a, double c) {
  a.v *= c;
  for (int i = 0; i < N; i++) a.d[i] *= c;
  return a;
}
template <int N>
__device__ __forceinline__ Jet<N> operator/(const Jet<N> &a, const Jet<N> &b) {
  Jet<N> r;
  const double ib = 1.0 / b.v;
  r.v = a.v * ib;
  for (int i = 0; i < N; i++) r.d[i] = (a.d[i] - r.v * b.d[i]) * ib;
  return r;
}
template <int N>
__device__ __forceinline__ Jet<N> jsqrt(const Jet<N> &a) {
  Jet<N> r;
  r.v = sqrt(a.v);
  const double h = 0.5 / r.v;
  for (int i = 0; i < N; i++) r.d[i] = a.d[i] * h;
  return r;
}
template <int N>
__device__ __forceinline__ Jet<N> jsin(const Jet<N> &a) {
  Jet<N> r;
  r.v = sin(a.v);
  const double c = cos(a.v);
  for (int i = 0; i < N; i++) r.d[i] = a.d[i] * c;
  return r;
}
template <int N>
__device__ __forceinline__ Jet<N> jcos(const Jet<N> &a) {
  Jet<N> r;
  r.v = cos(a.v);
  const double s = -sin(a.v);
  for (int i = 0; i < N; i++) r.d[i] = a.d[i] * s;
  return r;
}
template <int N>
__device__ __forceinline__ Jet<N> jatan2(const Jet<N> &y, const Jet<N> &x) {
  Jet<N> r;
  r.v = atan2(y.v, x.v);
  const double den = 1.0 / (x.v * x.v + y.v * y.v);
  for (int i = 0; i < N; i++) r.d[i] = (x.v * y.d[i] - y.v * x.d[i]) * den;
  return r;
}
template <int N>
__device__ __forceinline__ Jet<N> jasin(const Jet<N> &a) {
  Jet<N> r;
  r.v = asin(a.v);
  const double k = 1.0 / sqrt(1.0 - a.v * a.v);
  for (int i = 0; i < N; i++) r.d[i] = a.d[i] * k;
  return r;
}
// DiffBetweenAngles (error_utils.h:88-97)
template <int N>
__device__ __forceinline__ Jet<N> jdiff_angles(const Jet<N> &a, double b) {
  Jet<N> dd = a;
  dd.v -= b;
  if (dd.v > M_PI) dd.v -= 2 * M_PI;
  else if (dd.v < -M_PI) dd.v += 2 * M_PI;
  return dd;
}
template <int N>
__device__ __forceinline__ Jet<N> jlog(const Jet<N> &a) {
  Jet<N> r;
  r.v = log(a.v);
  const double ia = 1.0 / a.v;
  for (int i = 0; i < N; i++) r.d[i] = a.d[i] * ia;
  return r;
}
// ceres::AngleAxisRotatePoint
template <int N>
__device__ void j_rotate(const Jet<N> *aa, const Jet<N> *pt, Jet<N> *out) {
  const Jet<N> th2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  if (th2.v > kEps) {
    const Jet<N> th = jsqrt(th2), ct = jcos(th), st = jsin(th), ti = jc<N>(1.0) / th;
    const Jet<N> w[3] = {aa[0] * ti, aa[1] * ti, aa[2] * ti};
    const Jet<N> wxp[3] = {w[1] * pt[2] - w[2] * pt[1], w[2] * pt[0] - w[0] * pt[2], w[0] * pt[1] - w[1] * pt[0]};
    const Jet<N> tmp = (w[0] * pt[0] + w[1] * pt[1] + w[2] * pt[2]) * (jc<N>(1.0) - ct);
    for (int i = 0; i < 3; i++) out[i] = pt[i] * ct + wxp[i] * st + w[i] * tmp;
  } else {
    const Jet<N> wxp[3] = {aa[1] * pt[2] - aa[2] * pt[1], aa[2] * pt[0] - aa[0] * pt[2], aa[0] * pt[1] - aa[1] * pt[0]};
    for (int i = 0; i < 3; i++) out[i] = pt[i] + wxp[i];
  }
}
// ceres::AngleAxisToQuaternion / QuaternionProduct / QuaternionToAngleAxis: MultRotations (error_utils.h:14-24)
template <int N>
__device__ void j_aa_to_quat(const Jet<N> *aa, Jet<N> *q) {
  const Jet<N> th2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  if (th2.v > 0.0) {
    const Jet<N> th = jsqrt(th2), half = th * 0.5, k = jsin(half) / th;
    q[0] = jcos(half);
    for (int i = 0; i < 3; i++) q[1 + i] = aa[i] * k;
  } else {
    q[0] = jc<N>(1.0);
    for (int i = 0; i < 3; i++) q[1 + i] = aa[i] * 0.5;
  }
}
template <int N>
__device__ void j_quat_to_aa(const Jet<N> *q, Jet<N> *aa) {
  const Jet<N> s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (s2.v > 0.0) {
    const Jet<N> s = jsqrt(s2);
    const Jet<N> two_theta = (q[0].v < 0.0 ? jatan2(jc<N>(0.0) - s, jc<N>(0.0) - q[0]) : jatan2(s, q[0])) * 2.0;
    const Jet<N> k = two_theta / s;
    for (int i = 0; i < 3; i++) aa[i] = q[1 + i] * k;
  } else {
    for (int i = 0; i < 3; i++) aa[i] = q[1 + i] * 2.0;
  }
}
template <int N>
__device__ void j_mult_rotations(const Jet<N> *r1, const Jet<N> *r2, Jet<N> *out) {
  Jet<N> a[4], b[4], c[4];
  j_aa_to_quat(r1, a);
  j_aa_to_quat(r2, b);
  c[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  c[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  c[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  c[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  j_quat_to_aa(c, out);
}

// Normal-equation contribution of one prior block: nres residuals r with Jacobian rows over up to two parameter blocks (reduced start
// index ia / ib, sizes na / nb; an index < 0 = constant block).  Entries between two instance unknowns go to PI (a prior never couples
// two instances), instance x border to Bpri (border-major, 6 S per row), border x border to Cpri; the gradient to gpri.
// (border x border entries and the border's gradient are hit by EVERY instance that shares the block -- 5 000 position priors through
// one bias: same-address global atomics took 1.2 ms per evaluation -- so they are first added up in the workgroup's LDS copy `lc`
// (NB x NB, then NB gradient entries) and flushed once per workgroup; lc == nullptr -- a border too wide for that copy, kGenPriorLdsMaxNB --
// adds to Cpri / gpri directly)
template <int N>
__device__ void gen_add_block(const Dev &d, double *lc, const Jet<N> *r, int nres, double wt, int ia, int na, int ib, int nb) {
  const GenDev &g = d.g;
  const int n6 = d.cam0;
  for (int x = 0; x < na + nb; x++) {
    const int gx = x < na ? (ia < 0 ? -1 : ia + x) : (ib < 0 ? -1 : ib + x - na);
    if (gx < 0) continue;
    double gsum = 0.0;
    for (int e = 0; e < nres; e++) gsum += wt * r[e].d[x] * wt * r[e].v;
    if (gx >= n6) gen_atomic_add(lc ? lc + g.NB * g.NB + (gx - n6) : g.gpri + gx, gsum);
    else gen_atomic_add(g.gpri + gx, gsum);
    for (int y = 0; y < na + nb; y++) {
      const int gy = y < na ? (ia < 0 ? -1 : ia + y) : (ib < 0 ? -1 : ib + y - na);
      if (gy < 0) continue;
      double h = 0.0;
      for (int e = 0; e < nres; e++) h += wt * r[e].d[x] * wt * r[e].d[y];
      if (gx < n6 && gy < n6) {
        gen_atomic_add(g.PI + 36 * (long)(gx / 6) + 6 * (gx % 6) + (gy % 6), h);
      } else if (gx >= n6 && gy >= n6) {
        gen_atomic_add(lc ? lc + (gx - n6) * g.NB + (gy - n6) : g.Cpri + (long)(gx - n6) * g.NB + (gy - n6), h);
      } else if (gx >= n6) {  // (border, instance): stored once, from the border's side
        gen_atomic_add(g.Bpri + (long)(gx - n6) * n6 + gy, h);
      }
    }
  }
}

// The prior families, one thread per block.  Threads [0, NC): camera prior (+ the dual camera's barrier); [NC, NC + NRC): rig camera
// pose prior; then S instances: position prior through the bias; then NV views: absolute up vector; then 3 NV: pan / tilt / roll.
// mode 0: cost only (*cost_out += ...); 1: cost + normal equations; 2: model change, *cost_out -= u (r + u / 2), u = J y (y = the
// unscaled reduced step)
constexpr int kGenPriorLdsMaxNB = 72;  // (72^2 + 72) doubles = 42 KB: under the 64 KB a launch gets without an attribute
// Private copies of that LDS array, thread t adds to copy t % copies (round 6).  The 5 000 position priors of configs[4] reach the border through ONE
// bias: 256 threads of a workgroup adding to the same 56 addresses was 180 us of same-address LDS atomics per evaluation; sixteen copies: the
// largest power of two whose copies stay under 60 KB
// Workgroups of one wavefront (round 6): a thread is one prior block -- a long serial piece of jet arithmetic -- and the 5 000 position priors of
// configs[4] were 20 workgroups of 256 on 20 of the 256 CUs; 64 threads spread them over 79.
constexpr int kGenPriorTPB = 64;
__host__ __device__ inline int gen_prior_copies(int NB) {
  const int nlc = NB * NB + NB;
  int c = 16;
  while (c > 1 && (long)c * nlc * 8 > 60 * 1024) c >>= 1;
  return c;
}
__global__ void gen_prior_kernel(Dev d, const double *cam, const double *bias, const double *rcp, const double *instp, int mode, const double *y,
                                 double *cost_out) {
  const GenDev &g = d.g;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int NC = d.NC, NRC = g.NRC, NI = d.S, NV = g.NV, n6 = d.cam0;
  extern __shared__ __attribute__((aligned(16))) double pri_lc_mem[];  // mode 1, NB <= kGenPriorLdsMaxNB: NB x NB + NB, the workgroup's share of Cpri and of the border gradient
  const bool use_lc = mode == 1 && g.NB <= kGenPriorLdsMaxNB;
  const int nlc = g.NB * g.NB + g.NB, copies = gen_prior_copies(g.NB);
  double *pri_lc = use_lc ? pri_lc_mem + (long)(threadIdx.x & (copies - 1)) * nlc : nullptr;
  if (use_lc) {
    for (int q = threadIdx.x; q < nlc * copies; q += blockDim.x) pri_lc_mem[q] = 0.0;
    __syncthreads();
  }
  double cost = 0.0, mc = 0.0;
  auto finish = [&](auto *r, int nres, double wt, int ia, int na, int ib, int nb) {
    using J = std::remove_pointer_t<decltype(r)>;
    constexpr int N = sizeof(J::d) / sizeof(double);
    if (mode == 1) gen_add_block<N>(d, pri_lc, r, nres, wt, ia, na, ib, nb);
    if (mode == 2)
      for (int e = 0; e < nres; e++) {
        double u = 0.0;
        for (int x = 0; x < na + nb; x++) {
          const int gx = x < na ? (ia < 0 ? -1 : ia + x) : (ib < 0 ? -1 : ib + x - na);
          if (gx >= 0) u += wt * r[e].d[x] * y[gx];
        }
        mc -= u * (wt * r[e].v + 0.5 * u);
      }
  };
  auto inst_index = [&](int i) { return (d.shot_fixed && d.shot_fixed[i]) ? -1 : 6 * i; };
  auto border_index = [&](int col) { return col < 0 ? -1 : n6 + col; };
  if (t < NC) {  // ---- camera prior: (p - prior) / sigma, log(p / prior) / sigma for focal and aspect ratio (bundle_adjuster.cc:568-593) ----
    const int c = t, model = d.cam_model[c], nk = model_num_params(model);
    {  // (a constant camera's prior still counts in the cost: Ceres folds residual blocks over constant blocks into its fixed cost)
      int proj, kind, nd, na;
      model_layout(model, proj, kind, nd, na);
      const int ifocal = (proj == 2 ? 1 : 0) + nd;
      // Residual k depends on parameter k alone (the dual camera's barrier, residual nk, on parameter 0): a jet of ONE derivative per residual
      // carries everything (round 6).  Seventeen Jet<16> in scratch memory, every product of the 16 x 16 block formed by this one thread and
      // 256 atomic additions of mostly zeros were 60 us (cost only) to 160 us (normal equations) of EVERY prior evaluation at configs[4] --
      // its other 25 000 threads had long finished.  The component of a wide jet and the one-wide jet go through the same operations: the same
      // bits; the sums over the residuals below skip terms that are exactly zero.
      Jet<1> r[17];
      for (int k = 0; k < nk; k++) {
        const Jet<1> v = jv<1>(cam[16 * c + k], 0);
        const double scale = 1.0 / fmax(g.cam_sigma[16 * c + k], kEps);
        const bool logarithmic = (k == ifocal) || (na == 4 && k == ifocal + 1);
        r[k] = (logarithmic ? jlog(v / jc<1>(g.cam_prior[16 * c + k])) : v - jc<1>(g.cam_prior[16 * c + k])) * scale;
      }
      int nres = nk;
      if (model == OSFM_CAMERA_DUAL) {  // ParameterBarrier(0, 1) on the transition (parameters_errors.h:21-38)
        const Jet<1> v = jv<1>(cam[16 * c], 0);
        r[nres++] = jlog(v + jc<1>(1e-10)) + jlog(jc<1>(1.0 + 1e-10) - v) + jc<1>(2.0 * log(0.5));
      }
      for (int e = 0; e < nres; e++) cost += 0.5 * r[e].v * r[e].v;
      const int col = g.cam_col[c];
      if (col >= 0 && mode == 1) {
        for (int x = 0; x < nk; x++) {
          double gsum = 0.0, h = 0.0;
          gsum += r[x].d[0] * r[x].v;
          h += r[x].d[0] * r[x].d[0];
          if (x == 0 && nres > nk) {
            gsum += r[nk].d[0] * r[nk].v;
            h += r[nk].d[0] * r[nk].d[0];
          }
          gen_atomic_add(pri_lc ? pri_lc + g.NB * g.NB + (col + x) : g.gpri + n6 + col + x, gsum);
          gen_atomic_add(pri_lc ? pri_lc + (col + x) * g.NB + (col + x) : g.Cpri + (long)(col + x) * g.NB + (col + x), h);
        }
      }
      if (col >= 0 && mode == 2)
        for (int e = 0; e < nres; e++) {
          double u = 0.0;
          u += r[e].d[0] * y[n6 + col + (e < nk ? e : 0)];
          mc -= u * (r[e].v + 0.5 * u);
        }
    }
  } else if (t < NC + NRC) {  // ---- rig camera pose prior ----
    const int q = t - NC;
    if (g.rc_prior && g.rc_sigma) {
      Jet<6> r[6];
      for (int k = 0; k < 6; k++) r[k] = (jv<6>(rcp[6 * q + k], k) - jc<6>(g.rc_prior[6 * q + k])) * (1.0 / fmax(g.rc_sigma[6 * q + k], kEps));
      for (int e = 0; e < 6; e++) cost += 0.5 * r[e].v * r[e].v;
      finish(r, 6, 1.0, border_index(g.rc_col[q]), 6, -1, 0);
    }
  } else if (t < NC + NRC + NI) {  // ---- instance position prior through the bias: t - (s R(b) gps + t_b) (bias.h:33-53) ----
    const int i = t - NC - NRC;
    if (g.gps && g.gps_sigma && g.gps_sigma[3 * i] > 0) {
      const int bc = g.inst_bias_cam[i];
      const double *b = bias + 7 * (long)bc;
      const int ii = inst_index(i), bi = border_index(g.bias_col[bc]);
      {
        constexpr int N = 13;  // instance 6 | bias 7
        Jet<N> rot[3], tb[3], gp[3], rg[3], r[3];
        for (int k = 0; k < 3; k++) {
          rot[k] = jv<N>(b[k], 6 + k);
          tb[k] = jv<N>(b[3 + k], 9 + k);
          gp[k] = jc<N>(g.gps[3 * i + k]);
        }
        const Jet<N> sc = jv<N>(b[6], 12);
        j_rotate(rot, gp, rg);
        for (int k = 0; k < 3; k++) r[k] = (jv<N>(instp[6 * i + 3 + k], 3 + k) - (sc * rg[k] + tb[k])) * (1.0 / fmax(g.gps_sigma[3 * i + k], kEps));
        for (int e = 0; e < 3; e++) cost += 0.5 * r[e].v * r[e].v;
        finish(r, 3, 1.0, ii, 6, bi, 7);
      }
    }
  } else if (t < NC + NRC + NI + NV) {  // ---- absolute up vector, CauchyLoss(1) (absolute_motion_errors.h:12-39) ----
    const int s = t - NC - NRC - NI;
    if (g.up && g.up_sigma && g.up_sigma[s] > 0) {
      const int i = g.view_inst[s], q = g.view_rc[s];
      const int ii = inst_index(i), qi = border_index(g.rc_col[q]);
      {
        constexpr int N = 12;  // instance 6 | rig camera 6
        Jet<N> ri[3], rr[3], R[3], acc[3], z[3], r[3];
        const double *u0 = g.up + 3 * (long)s;
        const double nrm = sqrt(u0[0] * u0[0] + u0[1] * u0[1] + u0[2] * u0[2]);
        for (int k = 0; k < 3; k++) {
          ri[k] = jv<N>(instp[6 * i + k], k);
          rr[k] = jv<N>(rcp[6 * q + k], 6 + k);
          acc[k] = jc<N>(u0[k] / nrm);
        }
        j_mult_rotations(ri, rr, R);
        j_rotate(R, acc, z);
        const double is = 1.0 / g.up_sigma[s];
        for (int k = 0; k < 3; k++) r[k] = (z[k] - jc<N>(k == 2 ? 1.0 : 0.0)) * is;
        const double sq = r[0].v * r[0].v + r[1].v * r[1].v + r[2].v * r[2].v;
        double rho, rho1;
        loss_eval(OSFM_LOSS_CAUCHY, 1.0, sq, rho, rho1);
        cost += 0.5 * rho;
        finish(r, 3, sqrt(rho1), ii, 6, qi, 6);
      }
    }
  } else if (t < NC + NRC + NI + 4 * NV) {  // ---- absolute pan / tilt / roll of a view, CauchyLoss(1) each (absolute_motion_errors.h:40-137) ----
    const int u = t - NC - NRC - NI - NV, which = u / NV, s = u % NV;
    const double *ang = which == 0 ? g.pan : (which == 1 ? g.tilt : g.roll), *sg = which == 0 ? g.pan_sigma : (which == 1 ? g.tilt_sigma : g.roll_sigma);
    if (ang && sg && sg[s] > 0) {
      const int i = g.view_inst[s], q = g.view_rc[s];
      const int ii = inst_index(i), qi = border_index(g.rc_col[q]);
      {
        constexpr int N = 12;
        Jet<N> ri[3], rr[3], R[3], r[1];
        for (int k = 0; k < 3; k++) {
          ri[k] = jv<N>(instp[6 * i + k], k);
          rr[k] = jv<N>(rcp[6 * q + k], 6 + k);
        }
        j_mult_rotations(ri, rr, R);
        const Jet<N> ex[3] = {jc<N>(1.0), jc<N>(0.0), jc<N>(0.0)}, ez[3] = {jc<N>(0.0), jc<N>(0.0), jc<N>(1.0)};
        Jet<N> zw[3];
        j_rotate(R, ez, zw);
        const double is = 1.0 / sg[s];
        bool zero = false;
        if (which == 0) {  // PanAngleError
          if (fabs(zw[0].v) < 1e-8 && fabs(zw[1].v) < 1e-8) zero = true;
          else r[0] = jdiff_angles(jatan2(zw[0], zw[1]), ang[s]) * is;
        } else if (which == 1) {  // TiltAngleError
          const Jet<N> l = jsqrt(zw[0] * zw[0] + zw[1] * zw[1]);
          r[0] = jdiff_angles(jc<N>(0.0) - jatan2(zw[2], l), ang[s]) * is;
        } else {  // RollAngleError
          Jet<N> xw[3];
          j_rotate(R, ex, xw);
          Jet<N> a0 = zw[1], a1 = jc<N>(0.0) - zw[0];
          const Jet<N> la = jsqrt(a0 * a0 + a1 * a1);
          if (la.v < 1e-5) {
            zero = true;
          } else {
            a0 = a0 / la;
            a1 = a1 / la;
            const Jet<N> b0 = jc<N>(0.0) - xw[2] * a1, b1 = xw[2] * a0, b2 = xw[0] * a1 - xw[1] * a0;  // Rt_ex x (a0, a1, 0)
            const Jet<N> sin_roll = zw[0] * b0 + zw[1] * b1 + zw[2] * b2;
            if (sin_roll.v <= -(1.0 - 1e-5)) zero = true;
            else r[0] = jdiff_angles(jasin(sin_roll), ang[s]) * is;
          }
        }
        if (!zero) {
          double rho, rho1;
          loss_eval(OSFM_LOSS_CAUCHY, 1.0, r[0].v * r[0].v, rho, rho1);
          cost += 0.5 * rho;
          finish(r, 1, sqrt(rho1), ii, 6, qi, 6);
        }
      }
    }
  }
  double v = mode == 2 ? mc : cost;
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  if ((threadIdx.x & 63) == 0 && v != 0.0) gen_atomic_add(cost_out, v);
  if (use_lc) {
    __syncthreads();
    for (int q = threadIdx.x; q < nlc; q += blockDim.x) {
      double a = 0.0;
      for (int c = 0; c < copies; c++) a += pri_lc_mem[(long)c * nlc + q];
      if (a != 0.0) gen_atomic_add(q < g.NB * g.NB ? g.Cpri + q : g.gpri + n6 + (q - g.NB * g.NB), a);
    }
  }
}

// point priors = ground control points (bundle_adjuster.cc:688-707): cost (mode 0) or the model change of the step d_pt (mode 2)
__global__ void gen_point_prior_kernel(Dev d, const double *pts, int mode, double *out) {
  const GenDev &g = d.g;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  double v = 0.0;
  if (p < d.P && g.pt_prior_sigma[3 * (long)p] > 0) {
    const bool fixed = d.point_fixed && d.point_fixed[p];
    const int n = g.pt_prior_alt[p] ? 3 : 2;
    for (int a = 0; a < n; a++) {
      const double sc = 1.0 / fmax(g.pt_prior_sigma[3 * (long)p + a], kEps);
      const double r = sc * (pts[3 * (long)p + a] - g.pt_prior[3 * (long)p + a]);
      if (mode == 0) {
        v += 0.5 * r * r;  // (a constant point's prior still counts: Ceres' fixed cost)
      } else if (!fixed) {
        const double u = sc * d.d_pt[3 * (long)p + a];
        v -= u * (r + 0.5 * u);
      }
    }
  }
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  if ((threadIdx.x & 63) == 0 && v != 0.0) gen_atomic_add(out, v);
}

// ---- gradients -----------------------------------------------------------------------------------------------------------------------
// per point: gradient and J^T J block from the rows (the partition and summation order of point_grad_kernel), plus the point prior
template <int NR>
__global__ void __launch_bounds__(kCoopObs) gen_point_grad_kernel(Dev d) {
  __shared__ double c[9][kCoopObs];
  const GenDev &g = d.g;
  const int tid = threadIdx.x;
  const int p0 = d.wg_pt[blockIdx.x], p1 = d.wg_pt[blockIdx.x + 1];
  const long o0 = d.pt_off[p0], o1 = d.pt_off[p1];
  auto products = [&](long o, double (&v)[9]) {
    double r[NR], jp[NR][3];
#pragma unroll
    for (int e = 0; e < NR; e++) {
      r[e] = GA(o, e);
#pragma unroll
      for (int j = 0; j < 3; j++) jp[e][j] = GA(o, g.oJp + 3 * e + j);
    }
#pragma unroll
    for (int q = 0; q < 9; q++) v[q] = 0.0;
#pragma unroll
    for (int e = 0; e < NR; e++) {
#pragma unroll
      for (int j = 0; j < 3; j++) v[j] += jp[e][j] * r[e];
      v[3] += jp[e][0] * jp[e][0];
      v[4] += jp[e][0] * jp[e][1];
      v[5] += jp[e][0] * jp[e][2];
      v[6] += jp[e][1] * jp[e][1];
      v[7] += jp[e][1] * jp[e][2];
      v[8] += jp[e][2] * jp[e][2];
    }
  };
  auto finish = [&](int p, double (&acc)[9]) {
    if (g.pt_prior_sigma && g.pt_prior_sigma[3 * (long)p] > 0 && !(d.point_fixed && d.point_fixed[p])) {
      const int n = g.pt_prior_alt[p] ? 3 : 2;
      const int dg[3] = {3, 6, 8};
      for (int a = 0; a < n; a++) {
        const double sc = 1.0 / fmax(g.pt_prior_sigma[3 * (long)p + a], kEps);
        acc[a] += sc * sc * (d.pts[3 * (long)p + a] - g.pt_prior[3 * (long)p + a]);
        acc[dg[a]] += sc * sc;
      }
    }
    for (int j = 0; j < 3; j++) d.g_pt[3 * (long)p + j] = acc[j];
    for (int j = 0; j < 6; j++) d.Hpp[6 * (long)p + j] = acc[3 + j];
  };
  if (o1 - o0 <= kCoopObs) {
    if (tid < o1 - o0) {
      double v[9];
      products(o0 + tid, v);
#pragma unroll
      for (int q = 0; q < 9; q++) c[q][tid] = v[q];
    }
    __syncthreads();
    const int p = p0 + tid;
    if (p >= p1) return;
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!(d.point_fixed && d.point_fixed[p]))
      for (int k = (int)(d.pt_off[p] - o0); k < (int)(d.pt_off[p + 1] - o0); k++)
#pragma unroll
        for (int q = 0; q < 9; q++) acc[q] += c[q][k];
    finish(p, acc);
  } else if (tid == 0) {  // one track longer than the tile
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!(d.point_fixed && d.point_fixed[p0]))
      for (long o = o0; o < o1; o++) {
        double v[9];
        products(o, v);
#pragma unroll
        for (int q = 0; q < 9; q++) acc[q] += v[q];
      }
    finish(p0, acc);
  }
}

// points without observations (control points that nothing sees yet, or a problem without observations at all): prior only
__global__ void gen_point_grad_empty_kernel(Dev d) {
  const GenDev &g = d.g;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= d.P) return;
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (g.pt_prior_sigma && g.pt_prior_sigma[3 * (long)p] > 0 && !(d.point_fixed && d.point_fixed[p])) {
    const int n = g.pt_prior_alt[p] ? 3 : 2;
    const int dg[3] = {3, 6, 8};
    for (int a = 0; a < n; a++) {
      const double sc = 1.0 / fmax(g.pt_prior_sigma[3 * (long)p + a], kEps);
      acc[a] += sc * sc * (d.pts[3 * (long)p + a] - g.pt_prior[3 * (long)p + a]);
      acc[dg[a]] += sc * sc;
    }
  }
  for (int j = 0; j < 3; j++) d.g_pt[3 * (long)p + j] = acc[j];
  for (int j = 0; j < 6; j++) d.Hpp[6 * (long)p + j] = acc[3 + j];
}

// per instance (one wavefront): gradient and J^T J block over the observations of all its views + the prior block; per VIEW: the
// gradient and the diagonal of J^T J on the border slots (vpart[v][0 .. KW) and [KW .. 2 KW)), reduced per border column afterwards
template <int NR, int KWT, int MODEL>
__global__ void __launch_bounds__(64) gen_shot_grad_kernel(Dev d, int loss, double la) {
  const GenDev &g = d.g;
  const int s = (int)xcd_contiguous(blockIdx.x, gridDim.x), lane = threadIdx.x;
  const int KW = g.KW;
  double v[27];  // g (6), H (21)
#pragma unroll
  for (int i = 0; i < 27; i++) v[i] = 0;
  for (int vw = g.inst_view0[s]; vw < g.inst_view0[s + 1]; vw++) {
    double gb[KWT], db[KWT];
#pragma unroll
    for (int i = 0; i < KWT; i++) gb[i] = db[i] = 0.0;
    for (long k = g.view_off[vw] + lane; k < g.view_off[vw + 1]; k += 64) {
      double rw[NR], jpw[NR][3], jcw[NR][6], jbw[NR][KWT];
      d.sm_wt[k] = gen_sm_row<NR, KWT, true, MODEL>(d, vw, k, -1.0, loss, la, rw, jpw, jcw, jbw);  // (the weight: for the other per-instance kernels of this linearisation)
#pragma unroll
      for (int e = 0; e < NR; e++) {
        const double r = rw[e];
        double a[6];
#pragma unroll
        for (int j = 0; j < 6; j++) {
          a[j] = jcw[e][j];
          v[j] += a[j] * r;
        }
        int q = 6;
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
          for (int j = 0; j <= i; j++) v[q++] += a[i] * a[j];
#pragma unroll
        for (int i = 0; i < KWT; i++)
          if (i < KW) {
            const double b = jbw[e][i];
            gb[i] += b * r;
            db[i] += b * b;
          }
      }
    }
#pragma unroll
    for (int i = 0; i < KWT; i++)
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        gb[i] += __shfl_xor(gb[i], m);
        db[i] += __shfl_xor(db[i], m);
      }
    if (lane == 0)
#pragma unroll
      for (int i = 0; i < KWT; i++)
        if (i < KW) {
          g.vpart[(long)vw * 2 * KW + i] = gb[i];
          g.vpart[(long)vw * 2 * KW + KW + i] = db[i];
        }
  }
#pragma unroll
  for (int i = 0; i < 27; i++)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v[i] += __shfl_xor(v[i], m);
  if (lane == 0) {
    const bool fixed = d.shot_fixed && d.shot_fixed[s];
    const double *pi = g.PI + 36 * (long)s;
    int q = 0;
    for (int i = 0; i < 6; i++)
      for (int j = 0; j <= i; j++, q++) v[6 + q] += pi[6 * i + j];  // the preconditioners and the LM diagonal see the priors through Hcc
    const int dg[6] = {0, 2, 5, 9, 14, 20};
    for (int i = 0; i < 6; i++) {
      d.g_red[6 * s + i] = fixed ? 0.0 : v[i] + g.gpri[6 * s + i];
      d.prior_diag[6 * s + i] = 0.0;
      d.diag_red[6 * s + i] = fixed ? 0.0 : v[6 + dg[i]];
    }
    for (int i = 0; i < 21; i++) d.Hcc[21 * (long)s + i] = v[6 + i];
  }
}

// out[j] = sum over the views whose slot table holds border column j of vpart[v][off + slot]: one workgroup per border column, fixed order.
// ncomp_stride = entries per view in vpart, off = where the wanted KW-vector starts.  mode 0: zc[cam0 + j] = sum;  1: g_red = sum + gpri,
// and (second call with off = KW, mode 2) diag_red = sum + Cpri[j][j]
__global__ void __launch_bounds__(256) gen_border_reduce_kernel(Dev d, int stride, int off, int mode) {
  __shared__ double lds[8];
  const GenDev &g = d.g;
  const int j = blockIdx.x;
  double v[1] = {0.0};
  for (int vw = threadIdx.x; vw < g.NV; vw += 256) {
    const int slot = g.col_slot[(long)j * g.NV + vw];
    if (slot != 255) v[0] += g.vpart[(long)vw * stride + off + slot];
  }
  block_sum<1, 256>(v, lds);
  if (threadIdx.x == 0) {
    const int i = d.cam0 + j;
    if (mode == 0) d.zc[i] = v[0];
    else if (mode == 1) {
      d.g_red[i] = v[0] + g.gpri[i];
      d.prior_diag[i] = 0.0;
    } else
      d.diag_red[i] = v[0] + g.Cpri[(long)j * g.NB + j];
  }
}

// ---- Schur mat-vec ----------------------------------------------------------------------------------------------------------------------
// yv[v][i] = y[cam0 + col of slot i of view v] (0 for an empty slot): pass A then reads a view's border step contiguously
__global__ void gen_view_gather_kernel(Dev d, const double *y) {
  const GenDev &g = d.g;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)g.NV * g.KW) return;
  const int col = g.view_col[t];
  g.yv[t] = col < 0 ? 0.0 : y[d.cam0 + col];
}

// pass A, the generic twin of schur_point_coop_kernel (same partition, same summation orders):
// MODE 0: w_o = t_o - Jp_o Hhat sum(Jp^T t),  t_o = Jc_o y_s + Jb_o y_b     (mat-vec)
// MODE 1: w_o = -Jp_o Hhat (-g_p)                                            (right-hand side)
// MODE 2: d_pt = Hhat (-g_p - sum(Jp^T t)), partial[block] = the rows' share of the model cost change   (back-substitution)
template <int NR, int MODE, int MODEL = -1, bool COMPACT = false>
__global__ void __launch_bounds__(kCoopObs) gen_schur_point_kernel(Dev d, const double *y) {
  __shared__ double gsum[kCoopObs * 3];
  __shared__ double vpt[kCoopObs * 3];
  const GenDev &g = d.g;
  const int tid = threadIdx.x;
  const int p0 = d.wg_pt[blockIdx.x], p1 = d.wg_pt[blockIdx.x + 1];
  const long o0 = d.pt_off[p0], o1 = d.pt_off[p1];
  const int nobs = (int)(o1 - o0);
  const int KW = g.KW;
  auto row_t = [&](long o, double (&t)[NR]) {
    const int vw = g.o_view[o], s = d.o_shot[o];
    const double *ys = y + 6 * (long)s, *yb = g.yv + (long)vw * KW;
#pragma unroll
    for (int e = 0; e < NR; e++) t[e] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double yj = ys[j];
#pragma unroll
      for (int e = 0; e < NR; e++) t[e] += GA(o, g.oJc + 6 * e + j) * yj;
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {  // translation columns = -Jp (not stored): t + (-Jp) y = t - Jp y, the same bits
      const double yj = ys[3 + j];
#pragma unroll
      for (int e = 0; e < NR; e++) t[e] -= GA(o, g.oJp + 3 * e + j) * yj;
    }
    if constexpr (COMPACT) {
      double jb[2][16];
      int nkc;
      gen_compact_jb<MODEL>(d, o, vw, jb, nkc);
#pragma unroll
      for (int i = 0; i < 16; i++) {
        if (i >= nkc) continue;  // (the slots beyond the camera's parameters hold zeros in the full layout: t + 0 y = t)
        const double yi = yb[i];
#pragma unroll
        for (int e = 0; e < NR; e++) t[e] += jb[e][i] * yi;
      }
    } else {
      for (int i = 0; i < KW; i++) {
        const double yi = yb[i];
#pragma unroll
        for (int e = 0; e < NR; e++) t[e] += GA(o, g.oJb + e * KW + i) * yi;
      }
    }
  };
  if (nobs <= kCoopObs) {  // uniform per workgroup
    double t[NR], jp[NR][3];
#pragma unroll
    for (int e = 0; e < NR; e++) {
      t[e] = 0.0;
      jp[e][0] = jp[e][1] = jp[e][2] = 0.0;
    }
    int pl = 0;
    const long o = o0 + tid;
    if (tid < nobs) {
      pl = d.o_point[o] - p0;
      if (MODE != 1) row_t(o, t);
#pragma unroll
      for (int e = 0; e < NR; e++)
#pragma unroll
        for (int j = 0; j < 3; j++) jp[e][j] = GA(o, g.oJp + 3 * e + j);
      if (MODE != 1) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
          double u = 0.0;
#pragma unroll
          for (int e = 0; e < NR; e++) u += jp[e][j] * t[e];
          gsum[3 * tid + j] = u;
        }
      }
    }
    __syncthreads();
    if (tid < p1 - p0) {
      const int p = p0 + tid;
      double u[3] = {0, 0, 0};
      if (MODE != 1) {
        const int a = (int)(d.pt_off[p] - o0), b = (int)(d.pt_off[p + 1] - o0);
        for (int k = a; k < b; k++) {
          u[0] += gsum[3 * k];
          u[1] += gsum[3 * k + 1];
          u[2] += gsum[3 * k + 2];
        }
      }
      if (MODE == 1)
        for (int j = 0; j < 3; j++) u[j] = -d.g_pt[3 * (long)p + j];
      if (MODE == 2)
        for (int j = 0; j < 3; j++) u[j] = -d.g_pt[3 * (long)p + j] - u[j];
      const double *Hh = d.Hhat + 6 * (long)p;
      const double v0 = Hh[0] * u[0] + Hh[1] * u[1] + Hh[2] * u[2];
      const double v1 = Hh[1] * u[0] + Hh[3] * u[1] + Hh[4] * u[2];
      const double v2 = Hh[2] * u[0] + Hh[4] * u[1] + Hh[5] * u[2];
      if (MODE == 2) {
        d.d_pt[3 * (long)p] = v0;
        d.d_pt[3 * (long)p + 1] = v1;
        d.d_pt[3 * (long)p + 2] = v2;
      }
      vpt[3 * tid] = v0;
      vpt[3 * tid + 1] = v1;
      vpt[3 * tid + 2] = v2;
    }
    __syncthreads();
    if (MODE == 2) {
      double acc[1] = {0.0};
      if (tid < nobs) {
        const double v0 = vpt[3 * pl], v1 = vpt[3 * pl + 1], v2 = vpt[3 * pl + 2];
#pragma unroll
        for (int e = 0; e < NR; e++) {
          const double m = (jp[e][0] * v0 + jp[e][1] * v1 + jp[e][2] * v2) + t[e];
          acc[0] -= m * (GA(o, e) + 0.5 * m);
        }
      }
      __syncthreads();
      block_sum<1, kCoopObs>(acc, gsum);
      if (tid == 0) d.partial[blockIdx.x] = acc[0];
      return;
    }
    if (tid < nobs) {
      const double v0 = vpt[3 * pl], v1 = vpt[3 * pl + 1], v2 = vpt[3 * pl + 2];
#pragma unroll
      for (int e = 0; e < NR; e++) d.w[(long)NR * o + e] = t[e] - (jp[e][0] * v0 + jp[e][1] * v1 + jp[e][2] * v2);
    }
    return;
  }
  // one long track: strided over the workgroup, fixed-order tree reduction
  double u[3] = {0, 0, 0};
  if (MODE != 1) {
    for (long o = o0 + tid; o < o1; o += kCoopObs) {
      double t[NR];
      row_t(o, t);
      if (MODE == 0)
#pragma unroll
        for (int e = 0; e < NR; e++) d.w[(long)NR * o + e] = t[e];
#pragma unroll
      for (int j = 0; j < 3; j++)
#pragma unroll
        for (int e = 0; e < NR; e++) u[j] += GA(o, g.oJp + 3 * e + j) * t[e];
    }
  }
  for (int j = 0; j < 3; j++) gsum[3 * tid + j] = u[j];
  __syncthreads();
  for (int h = kCoopObs / 2; h >= 1; h >>= 1) {
    if (tid < h)
      for (int j = 0; j < 3; j++) gsum[3 * tid + j] += gsum[3 * (tid + h) + j];
    __syncthreads();
  }
  const double *Hh = d.Hhat + 6 * (long)p0;
  double u0 = gsum[0], u1 = gsum[1], u2 = gsum[2];
  if (MODE == 1) { u0 = -d.g_pt[3 * (long)p0]; u1 = -d.g_pt[3 * (long)p0 + 1]; u2 = -d.g_pt[3 * (long)p0 + 2]; }
  if (MODE == 2) { u0 = -d.g_pt[3 * (long)p0] - u0; u1 = -d.g_pt[3 * (long)p0 + 1] - u1; u2 = -d.g_pt[3 * (long)p0 + 2] - u2; }
  const double v0 = Hh[0] * u0 + Hh[1] * u1 + Hh[2] * u2;
  const double v1 = Hh[1] * u0 + Hh[3] * u1 + Hh[4] * u2;
  const double v2 = Hh[2] * u0 + Hh[4] * u1 + Hh[5] * u2;
  if (MODE == 2) {
    if (tid == 0) {
      d.d_pt[3 * (long)p0] = v0;
      d.d_pt[3 * (long)p0 + 1] = v1;
      d.d_pt[3 * (long)p0 + 2] = v2;
    }
    double acc[1] = {0.0};
    for (long o = o0 + tid; o < o1; o += kCoopObs) {
      double t[NR];
      row_t(o, t);
#pragma unroll
      for (int e = 0; e < NR; e++) {
        const double m = (GA(o, g.oJp + 3 * e) * v0 + GA(o, g.oJp + 3 * e + 1) * v1 + GA(o, g.oJp + 3 * e + 2) * v2) + t[e];
        acc[0] -= m * (GA(o, e) + 0.5 * m);
      }
    }
    __syncthreads();
    block_sum<1, kCoopObs>(acc, gsum);
    if (tid == 0) d.partial[blockIdx.x] = acc[0];
    return;
  }
  for (long o = o0 + tid; o < o1; o += kCoopObs) {
#pragma unroll
    for (int e = 0; e < NR; e++) {
      const double m = GA(o, g.oJp + 3 * e) * v0 + GA(o, g.oJp + 3 * e + 1) * v1 + GA(o, g.oJp + 3 * e + 2) * v2;
      if (MODE == 0) d.w[(long)NR * o + e] -= m;
      else d.w[(long)NR * o + e] = -m;
    }
  }
}

// pass B, wavefront per instance: zc_s = sum Jc^T w over all its views; per view the border partial vpart[v][0 .. KW) = sum Jb^T w
template <int NR, int KWT, int MODEL>
__global__ void __launch_bounds__(64) gen_schur_shot_kernel(Dev d) {
  const GenDev &g = d.g;
  const int s = (int)xcd_contiguous(blockIdx.x, gridDim.x), lane = threadIdx.x;
  const int KW = g.KW;
  double vs[6] = {0, 0, 0, 0, 0, 0};
  for (int vw = g.inst_view0[s]; vw < g.inst_view0[s + 1]; vw++) {
    double vb[KWT];
#pragma unroll
    for (int i = 0; i < KWT; i++) vb[i] = 0.0;
    for (long k = g.view_off[vw] + lane; k < g.view_off[vw + 1]; k += 64) {
      const long o = d.shot_obs[k];  // w lives in point-major order
      double rw[NR], jpw[NR][3], jcw[NR][6], jbw[NR][KWT];
      gen_sm_row<NR, KWT, true, MODEL>(d, vw, k, d.sm_wt[k], 0, 0.0, rw, jpw, jcw, jbw);
#pragma unroll
      for (int e = 0; e < NR; e++) {
        const double we = d.w[(long)NR * o + e];
#pragma unroll
        for (int j = 0; j < 6; j++) vs[j] += jcw[e][j] * we;
#pragma unroll
        for (int i = 0; i < KWT; i++)
          if (i < KW) vb[i] += jbw[e][i] * we;
      }
    }
#pragma unroll
    for (int i = 0; i < KWT; i++)
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) vb[i] += __shfl_xor(vb[i], m);
    if (lane == 0)
#pragma unroll
      for (int i = 0; i < KWT; i++)
        if (i < KW) g.vpart[(long)vw * 2 * KW + i] = vb[i];
  }
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) vs[i] += __shfl_xor(vs[i], m);
  if (lane == 0)
    for (int j = 0; j < 6; j++) d.zc[6 * s + j] = vs[j];
}

// bdot[j][c] = the share of slice c (of kBpriSlices) of Bpri[j] . y_s (the priors' instance x border coupling applied from the border's
// side); gen_schur_finish_kernel adds a row's slices in order
constexpr int kBpriSlices = 32;
__global__ void __launch_bounds__(256) gen_bpri_dot_kernel(Dev d, const double *y) {
  __shared__ double lds[8];
  const GenDev &g = d.g;
  const int j = blockIdx.x, c = blockIdx.y, n6 = d.cam0;
  const int per = (n6 + kBpriSlices - 1) / kBpriSlices, t0 = c * per, t1 = min(n6, t0 + per);
  double v[1] = {0.0};
  for (int t = t0 + threadIdx.x; t < t1; t += 256) v[0] += g.Bpri[(long)j * n6 + t] * y[t];
  block_sum<1, 256>(v, lds);
  if (threadIdx.x == 0) g.bdot[j * kBpriSlices + c] = v[0];
}

// finish: out = sc (zc + priors y) + (D / radius) x   (mode 0)   or   out = sc (-g + zc)   (mode 1, right-hand side).
// zc holds the observation rows' share for all nred unknowns (gen_schur_shot_kernel, gen_border_reduce_kernel).
__device__ __forceinline__ double gen_schur_finish_row(const Dev &d, const double *x, const double *y, double *out, double radius, int mode, int have_obs, int have_bpri, int i,
                                                       bool want_dot) {
  const GenDev &g = d.g;
  const int n6 = d.cam0;
  double zc = have_obs ? d.zc[i] : 0.0;
  if (mode == 0) {
    if (i < n6) {
      const int s = i / 6, k = i - 6 * s;
      const double *pi = g.PI + 36 * (long)s + 6 * k, *ys = y + 6 * s;
      for (int j = 0; j < 6; j++) zc += pi[j] * ys[j];
      if (have_bpri)
        for (int j = 0; j < g.NB; j++) zc += g.Bpri[(long)j * n6 + i] * y[n6 + j];
    } else {
      const int j = i - n6;
      if (have_bpri)
        for (int c = 0; c < kBpriSlices; c++) zc += g.bdot[j * kBpriSlices + c];
      for (int k = 0; k < g.NB; k++) zc += g.Cpri[(long)j * g.NB + k] * y[n6 + k];
    }
    const double o = d.sc_red[i] * zc + d.D_red[i] / radius * x[i];
    out[i] = o;
    return want_dot ? x[i] * o : 0.0;
  }
  out[i] = d.sc_red[i] * (-d.g_red[i] + zc);
  return 0.0;
}
// dot_part (mode 0, optional): the workgroup's share of x . out, PCG's p . Ap (pcg_step1_kernel adds the shares in workgroup order)
__global__ void __launch_bounds__(TPB) gen_schur_finish_kernel(Dev d, const double *x, const double *y, double *out, double radius, int mode, int have_obs, int have_bpri,
                                                               double *dot_part) {
  __shared__ double lds[8];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double dot[1] = {0.0};
  if (i < d.nred) dot[0] = gen_schur_finish_row(d, x, y, out, radius, mode, have_obs, have_bpri, i, mode == 0 && dot_part != nullptr);
  if (mode == 0 && dot_part) {
    block_sum<1, TPB>(dot, lds);
    if (threadIdx.x == 0) dot_part[blockIdx.x] = dot[0];
  }
}

// block-Jacobi fallback preconditioner, generic rows: inverse of the 6 x 6 instance blocks of the scaled Schur complement (the
// border rows: the inverse of their diagonal, gen_precond_border_kernel)
template <int NR>
__global__ void __launch_bounds__(64) gen_precond_shot_kernel(Dev d, double radius) {
  const GenDev &g = d.g;
  const int s = blockIdx.x, lane = threadIdx.x;
  double v[21];
#pragma unroll
  for (int i = 0; i < 21; i++) v[i] = 0;
  for (int vw = g.inst_view0[s]; vw < g.inst_view0[s + 1]; vw++)
  for (long k = g.view_off[vw] + lane; k < g.view_off[vw + 1]; k += 64) {  // (the instance's segment, view by view: the same order)
    const int p = d.sm_point[k];
    const double *Hh = d.Hhat + 6 * (long)p;
    const double h[9] = {Hh[0], Hh[1], Hh[2], Hh[1], Hh[3], Hh[4], Hh[2], Hh[4], Hh[5]};
    double E[6][3], EH[6][3];
    double rw[NR], jpw[NR][3], jcw[NR][6], jbw[NR][1];
    gen_sm_row<NR, 1, false>(d, vw, k, d.sm_wt[k], 0, 0.0, rw, jpw, jcw, jbw);
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double t = 0.0;
#pragma unroll
        for (int e = 0; e < NR; e++) t += jcw[e][i] * jpw[e][j];
        E[i][j] = t;
      }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) EH[i][j] = E[i][0] * h[j] + E[i][1] * h[3 + j] + E[i][2] * h[6 + j];
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int j = 0; j <= i; j++) v[q++] += EH[i][0] * E[j][0] + EH[i][1] * E[j][1] + EH[i][2] * E[j][2];
  }
#pragma unroll
  for (int i = 0; i < 21; i++)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v[i] += __shfl_xor(v[i], m);
  if (lane == 0) {
    double B[6][6];
    int q = 0;
    for (int i = 0; i < 6; i++)
      for (int j = 0; j <= i; j++, q++) {
        const double si = d.sc_red[6 * s + i], sj = d.sc_red[6 * s + j];
        double val = (d.Hcc[21 * (long)s + q] - v[q]) * si * sj;
        if (i == j) val += d.D_red[6 * s + i] / radius;
        B[i][j] = B[j][i] = val;
      }
    double L[6][6];
    bool ok = true;
    for (int i = 0; i < 6; i++)
      for (int j = 0; j <= i; j++) {
        double sum = B[i][j];
        for (int k = 0; k < j; k++) sum -= L[i][k] * L[j][k];
        if (i == j) {
          if (!(sum > 0)) { ok = false; sum = 1.0; }
          L[i][i] = sqrt(sum);
        } else {
          L[i][j] = sum / L[j][j];
        }
      }
    double Li[6][6];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) Li[i][j] = 0;
    for (int c = 0; c < 6; c++)
      for (int i = c; i < 6; i++) {
        double sum = (i == c) ? 1.0 : 0.0;
        for (int k = c; k < i; k++) sum -= L[i][k] * Li[k][c];
        Li[i][c] = sum / L[i][i];
      }
    double *o = d.Binv + 36 * (long)s;
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) {
        double sum = 0;
        for (int k = (i > j ? i : j); k < 6; k++) sum += Li[k][i] * Li[k][j];
        o[6 * i + j] = ok ? sum : ((i == j) ? 1.0 / fmax(B[i][i], 1e-300) : 0.0);
      }
  }
}
// z = M^-1 r for the block-Jacobi fallback: 6 x 6 blocks on the instances, the diagonal on the border
__global__ void gen_precond_apply_kernel(Dev d, const double *r, double *z, double radius) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < d.S) {
    const double *Bi = d.Binv + 36 * (long)b, *rr = r + 6 * b;
    for (int i = 0; i < 6; i++) {
      double s = 0;
      for (int j = 0; j < 6; j++) s += Bi[6 * i + j] * rr[j];
      z[6 * b + i] = s;
    }
  } else if (b < d.S + d.g.NB) {
    const int i = d.cam0 + (b - d.S);
    const double dg = d.diag_red[i] * d.sc_red[i] * d.sc_red[i] + d.D_red[i] / radius;
    z[i] = r[i] / fmax(dg, 1e-300);
  }
}
// the border rows of a band solve's result when there is no exact border: the diagonal (bcr_up_kernel's cam_q for the fast path)
__global__ void gen_precond_border_kernel(Dev d, const double *r, double *z, double radius) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= d.g.NB) return;
  const int i = d.cam0 + j;
  const double dg = d.diag_red[i] * d.sc_red[i] * d.sc_red[i] + d.D_red[i] / radius;
  z[i] = r[i] / fmax(dg, 1e-300);
}

// candidate x + delta of the instance / camera / rig camera / bias blocks, with the norms of the step and of x over the variable blocks
// (single block; y = the unscaled reduced step).  out[1] = step^2, out[2] = x^2; out[0] (the priors' model change) is left to
// gen_prior_kernel mode 2.
__global__ void gen_candidate_kernel(Dev d, const double *y, double *out) {
  __shared__ double lds[32];
  const GenDev &g = d.g;
  const int n6 = d.cam0;
  double v[2] = {0, 0};
  auto upd = [&](const double *cur, double *nxt, int n, int idx) {  // constant blocks are not part of the problem Ceres sees
    for (int k = 0; k < n; k++) {
      const double dl = idx < 0 ? 0.0 : y[idx + k];
      nxt[k] = cur[k] + dl;
      v[0] += dl * dl;
      if (idx >= 0) v[1] += cur[k] * cur[k];
    }
  };
  for (int s = threadIdx.x; s < d.S; s += blockDim.x) upd(d.poses + 6 * (long)s, d.poses_n + 6 * (long)s, 6, (d.shot_fixed && d.shot_fixed[s]) ? -1 : 6 * s);
  for (int c = threadIdx.x; c < d.NC; c += blockDim.x) {
    const int nk = model_num_params(d.cam_model[c]);
    upd(g.cam + 16 * c, g.cam_n + 16 * c, nk, g.cam_col[c] < 0 ? -1 : n6 + g.cam_col[c]);
    for (int k = nk; k < 16; k++) g.cam_n[16 * c + k] = g.cam[16 * c + k];
    upd(g.bias + 7 * c, g.bias_n + 7 * c, 7, g.bias_col[c] < 0 ? -1 : n6 + g.bias_col[c]);
  }
  for (int q = threadIdx.x; q < g.NRC; q += blockDim.x) upd(g.rc + 6 * q, g.rc_n + 6 * q, 6, g.rc_col[q] < 0 ? -1 : n6 + g.rc_col[q]);
  block_sum<2, 1024>(v, lds);
  if (threadIdx.x == 0) {
    out[1] = v[0];
    out[2] = v[1];
  }
}

// ---- exact border of the generic path ----------------------------------------------------------------------------------------------
// Sigma^-1 = (C - B^T W)^-1 for nb <= kGenMaxNB by Gauss-Jordan with partial pivoting in LDS, one workgroup; *status = 1 when Sigma is
// singular / not finite.  (border_sigma_kernel is the nb <= 6 version of the fast path.)
__global__ void __launch_bounds__(256) gen_border_sigma_kernel(const double *Cm, const double *dots, double *SigInv, int nb, int *status) {
  extern __shared__ __attribute__((aligned(16))) double gsig[];  // nb x 2 nb: [Sigma | I]
  __shared__ int s_piv, s_bad;
  const int W = 2 * nb, tid = threadIdx.x;
  for (int t = tid; t < nb * W; t += 256) {
    const int i = t / W, j = t - i * W;
    gsig[t] = j < nb ? Cm[i * nb + j] - dots[i * nb + j] : (j - nb == i ? 1.0 : 0.0);
  }
  if (tid == 0) s_bad = 0;
  __syncthreads();
  for (int c = 0; c < nb; c++) {
    if (tid == 0) {
      int piv = c;
      for (int r2 = c + 1; r2 < nb; r2++)
        if (fabs(gsig[r2 * W + c]) > fabs(gsig[piv * W + c])) piv = r2;
      const double pv = gsig[piv * W + c];
      if (!(fabs(pv) > 0) || !(fabs(pv) < 1.0 / 0.0)) s_bad = 1;
      s_piv = piv;
    }
    __syncthreads();
    if (s_bad) break;
    const int piv = s_piv;
    if (piv != c)
      for (int q = tid; q < W; q += 256) {
        const double t0 = gsig[c * W + q];
        gsig[c * W + q] = gsig[piv * W + q];
        gsig[piv * W + q] = t0;
      }
    __syncthreads();
    const double ip = 1.0 / gsig[c * W + c];
    __syncthreads();
    for (int q = tid; q < W; q += 256) gsig[c * W + q] *= ip;
    __syncthreads();
    for (int t = tid; t < nb * W; t += 256) {
      const int r2 = t / W, q = t - r2 * W;
      if (r2 == c || q == c) continue;  // column c is read by everyone in this step: it is cleared afterwards
      gsig[t] -= gsig[r2 * W + c] * gsig[c * W + q];
    }
    __syncthreads();
    for (int r2 = tid; r2 < nb; r2 += 256)
      if (r2 != c) gsig[r2 * W + c] = 0.0;
    __syncthreads();
  }
  if (tid == 0) *status = s_bad;
  for (int t = tid; t < nb * nb; t += 256) SigInv[t] = s_bad ? 0.0 : gsig[(t / nb) * W + nb + (t % nb)];
}
// z_c = SigInv (r_c - B^T z_s)   (single block, nb <= kGenMaxNB)
__global__ void gen_border_rhs_kernel(const double *Bc, const double *SigInv, const double *r, double *z, int nb, int n, int cam0) {
  __shared__ double lds[32];
  __shared__ double yy[kGenMaxNB];
  for (int i = 0; i < nb; i++) {
    double v[1] = {0.0};
    for (int t = threadIdx.x; t < n; t += blockDim.x) v[0] += Bc[(long)i * n + t] * z[t];
    block_sum<1, 1024>(v, lds);
    if (threadIdx.x == 0) yy[i] = r[cam0 + i] - v[0];
    __syncthreads();
  }
  if ((int)threadIdx.x < nb) {
    double acc = 0.0;
    for (int j = 0; j < nb; j++) acc += SigInv[threadIdx.x * nb + j] * yy[j];
    z[cam0 + threadIdx.x] = acc;
  }
}

// ---- exact border, every column that touches observations in ONE pass over them (the generic twin of border_point / border_shot) -----
// Column c of the reduced matrix = the mat-vec of a unit vector on border unknown c.  A unit vector has no instance part and reaches an
// observation only through the slot of its view that holds column c, so all columns are formed together: pass A reads Jp once and the
// border slots column by column (t_o is the slot's Jacobian column scaled by sc_c, u_p = sum Jp^T t, v_p = Hhat u_p, w_o = t_o - Jp v_p,
// NR values per observation and column, AoS per observation), pass B reads Jc / Jb once per chunk of columns.  Same summation orders as
// gen_schur_point_kernel<0> / gen_schur_shot_kernel column by column.  `cols` lists the border columns that some view holds (the
// bias columns, which only priors reach, are left to gen_border_finish_kernel).
constexpr int kGenBorderCB = 3;  // border columns per exchange through LDS in gen_border_point_kernel (round 6; one per exchange until round 5:
                                 // two barriers per column and workgroup, 0.78 ms for the nine columns of a Brown camera at configs[4])
template <int NR, int MODEL = -1, bool COMPACT = false>
__global__ void __launch_bounds__(kCoopObs) gen_border_point_kernel(Dev d, const int *cols, int ncols, double *wB) {
  constexpr int CB = kGenBorderCB;
  __shared__ double gsum[kCoopObs * 3 * CB];
  __shared__ double vpt[kCoopObs * 3 * CB];
  const GenDev &g = d.g;
  const int tid = threadIdx.x;
  const int p0 = d.wg_pt[blockIdx.x], p1 = d.wg_pt[blockIdx.x + 1];
  const long o0 = d.pt_off[p0], o1 = d.pt_off[p1];
  const int nobs = (int)(o1 - o0), KW = g.KW;
  if (nobs <= kCoopObs) {  // uniform per workgroup
    double jp[NR][3];
    int pl = 0, vw = 0;
    const long o = o0 + tid;
    const bool on = tid < nobs;
    if (on) {
      pl = d.o_point[o] - p0;
      vw = g.o_view[o];
#pragma unroll
      for (int e = 0; e < NR; e++)
#pragma unroll
        for (int j = 0; j < 3; j++) jp[e][j] = GA(o, g.oJp + 3 * e + j);
    }
    double jbc[2][16];  // COMPACT: the observation's border slots, rebuilt once
    if constexpr (COMPACT) {
      int nkc = 0;
      if (on) gen_compact_jb<MODEL>(d, o, vw, jbc, nkc);
    }
    const int a = tid < p1 - p0 ? (int)(d.pt_off[p0 + tid] - o0) : 0, b = tid < p1 - p0 ? (int)(d.pt_off[p0 + tid + 1] - o0) : 0;
    double hh[6] = {0, 0, 0, 0, 0, 0};
    if (tid < p1 - p0)
      for (int q = 0; q < 6; q++) hh[q] = d.Hhat[6 * (long)(p0 + tid) + q];
    for (int c0 = 0; c0 < ncols; c0 += CB) {  // CB columns per exchange; every column's sums in the order of the one-column form (the same bits)
      double t[CB][NR];
#pragma unroll
      for (int cc = 0; cc < CB; cc++)
#pragma unroll
        for (int e = 0; e < NR; e++) t[cc][e] = 0.0;
      if (on) {
#pragma unroll
        for (int cc = 0; cc < CB; cc++) {
          if (c0 + cc < ncols) {
            const int col = cols[c0 + cc];
            const int slot = g.col_slot[(long)col * g.NV + vw];
            if (slot != 255) {
              const double sc = d.sc_red[d.cam0 + col];
#pragma unroll
              for (int e = 0; e < NR; e++) {
                if constexpr (COMPACT) t[cc][e] = gen_pick16(jbc[e], slot) * sc;
                else t[cc][e] = GA(o, g.oJb + e * KW + slot) * sc;
              }
            }
          }
#pragma unroll
          for (int j = 0; j < 3; j++) {
            double u = 0.0;
#pragma unroll
            for (int e = 0; e < NR; e++) u += jp[e][j] * t[cc][e];
            gsum[(3 * tid + j) * CB + cc] = u;
          }
        }
      }
      __syncthreads();
      if (tid < p1 - p0) {
#pragma unroll
        for (int cc = 0; cc < CB; cc++) {
          double u[3] = {0, 0, 0};
          for (int k = a; k < b; k++) {
            u[0] += gsum[(3 * k) * CB + cc];
            u[1] += gsum[(3 * k + 1) * CB + cc];
            u[2] += gsum[(3 * k + 2) * CB + cc];
          }
          vpt[(3 * tid) * CB + cc] = hh[0] * u[0] + hh[1] * u[1] + hh[2] * u[2];
          vpt[(3 * tid + 1) * CB + cc] = hh[1] * u[0] + hh[3] * u[1] + hh[4] * u[2];
          vpt[(3 * tid + 2) * CB + cc] = hh[2] * u[0] + hh[4] * u[1] + hh[5] * u[2];
        }
      }
      __syncthreads();
      if (on) {
#pragma unroll
        for (int cc = 0; cc < CB; cc++)
          if (c0 + cc < ncols) {
            const double v0 = vpt[(3 * pl) * CB + cc], v1 = vpt[(3 * pl + 1) * CB + cc], v2 = vpt[(3 * pl + 2) * CB + cc];
#pragma unroll
            for (int e = 0; e < NR; e++) wB[((long)o * ncols + c0 + cc) * NR + e] = t[cc][e] - (jp[e][0] * v0 + jp[e][1] * v1 + jp[e][2] * v2);
          }
      }
    }
    return;
  }
  // one long track: strided over the workgroup, fixed-order tree reduction, column by column
  const double *Hh = d.Hhat + 6 * (long)p0;
  for (int c = 0; c < ncols; c++) {
    const int col = cols[c];
    const double sc = d.sc_red[d.cam0 + col];
    double u[3] = {0, 0, 0};
    for (long o = o0 + tid; o < o1; o += kCoopObs) {
      const int slot = g.col_slot[(long)col * g.NV + g.o_view[o]];
      double jbl[2][16];
      if constexpr (COMPACT) {
        int nkc;
        gen_compact_jb<MODEL>(d, o, g.o_view[o], jbl, nkc);
      }
#pragma unroll
      for (int e = 0; e < NR; e++) {
        double te = 0.0;
        if (slot != 255) {
          if constexpr (COMPACT) te = gen_pick16(jbl[e], slot) * sc;
          else te = GA(o, g.oJb + e * KW + slot) * sc;
        }
#pragma unroll
        for (int j = 0; j < 3; j++) u[j] += GA(o, g.oJp + 3 * e + j) * te;
      }
    }
    __syncthreads();
    for (int j = 0; j < 3; j++) gsum[3 * tid + j] = u[j];
    __syncthreads();
    for (int h = kCoopObs / 2; h >= 1; h >>= 1) {
      if (tid < h)
        for (int j = 0; j < 3; j++) gsum[3 * tid + j] += gsum[3 * (tid + h) + j];
      __syncthreads();
    }
    const double u0 = gsum[0], u1 = gsum[1], u2 = gsum[2];
    const double v0 = Hh[0] * u0 + Hh[1] * u1 + Hh[2] * u2, v1 = Hh[1] * u0 + Hh[3] * u1 + Hh[4] * u2, v2 = Hh[2] * u0 + Hh[4] * u1 + Hh[5] * u2;
    for (long o = o0 + tid; o < o1; o += kCoopObs) {
      const int slot = g.col_slot[(long)col * g.NV + g.o_view[o]];
      double jbl[2][16];
      if constexpr (COMPACT) {
        int nkc;
        gen_compact_jb<MODEL>(d, o, g.o_view[o], jbl, nkc);
      }
#pragma unroll
      for (int e = 0; e < NR; e++) {
        double te = 0.0;
        if (slot != 255) {
          if constexpr (COMPACT) te = gen_pick16(jbl[e], slot) * sc;
          else te = GA(o, g.oJb + e * KW + slot) * sc;
        }
        wB[((long)o * ncols + c) * NR + e] = te - (GA(o, g.oJp + 3 * e) * v0 + GA(o, g.oJp + 3 * e + 1) * v1 + GA(o, g.oJp + 3 * e + 2) * v2);
      }
    }
  }
}

// pass B for the columns [c0, c0 + CH) of `cols`: wavefront per instance.  Bc[col][6 s + j] = sc (sum Jc^T w_col) (the instance rows of the
// column, observation part), vpartB[v][c][0 .. KW) = sum Jb^T w_col per view (reduced per border row by gen_border_finish_kernel)
template <int NR, int KWT, int CH, int MODEL>
__global__ void __launch_bounds__(64) gen_border_shot_kernel(Dev d, const int *cols, int ncols, int c0, const double *wB, double *Bc, double *vpartB) {
  const GenDev &g = d.g;
  const int s = (int)xcd_contiguous(blockIdx.x, gridDim.x), lane = threadIdx.x;
  const int KW = g.KW, n6 = d.cam0;
  double vs[CH][6];
#pragma unroll
  for (int c = 0; c < CH; c++)
#pragma unroll
    for (int j = 0; j < 6; j++) vs[c][j] = 0.0;
  for (int vw = g.inst_view0[s]; vw < g.inst_view0[s + 1]; vw++) {
    double vb[CH][KWT];
#pragma unroll
    for (int c = 0; c < CH; c++)
#pragma unroll
      for (int i = 0; i < KWT; i++) vb[c][i] = 0.0;
    for (long k = g.view_off[vw] + lane; k < g.view_off[vw + 1]; k += 64) {
      const long o = d.shot_obs[k];
      const double *src = wB + ((long)o * ncols + c0) * NR;
      double rw[NR], jpw[NR][3], jcw[NR][6], jbw[NR][KWT];
      gen_sm_row<NR, KWT, true, MODEL>(d, vw, k, d.sm_wt[k], 0, 0.0, rw, jpw, jcw, jbw);
#pragma unroll
      for (int e = 0; e < NR; e++) {
        double jc[6], jb[KWT];
#pragma unroll
        for (int j = 0; j < 6; j++) jc[j] = jcw[e][j];
#pragma unroll
        for (int i = 0; i < KWT; i++) jb[i] = i < KW ? jbw[e][i] : 0.0;
#pragma unroll
        for (int c = 0; c < CH; c++) {
          const double we = c0 + c < ncols ? src[c * NR + e] : 0.0;
#pragma unroll
          for (int j = 0; j < 6; j++) vs[c][j] += jc[j] * we;
#pragma unroll
          for (int i = 0; i < KWT; i++) vb[c][i] += jb[i] * we;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CH; c++)
#pragma unroll
      for (int i = 0; i < KWT; i++)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) vb[c][i] += __shfl_xor(vb[c][i], m);
    if (lane == 0)
#pragma unroll
      for (int c = 0; c < CH; c++)
        if (c0 + c < ncols)
#pragma unroll
          for (int i = 0; i < KWT; i++)
            if (i < KW) vpartB[((long)vw * ncols + c0 + c) * KW + i] = vb[c][i];
  }
#pragma unroll
  for (int c = 0; c < CH; c++)
#pragma unroll
    for (int j = 0; j < 6; j++)
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) vs[c][j] += __shfl_xor(vs[c][j], m);
  if (lane == 0)
#pragma unroll
    for (int c = 0; c < CH; c++)
      if (c0 + c < ncols)
        for (int j = 0; j < 6; j++) Bc[(long)cols[c0 + c] * n6 + 6 * s + j] = d.sc_red[6 * s + j] * vs[c][j];
}

// finish of the columns: the priors' share on the instance rows (Bc[col][i] += sc_i Bpri[col][i] sc_col; a column no view holds is that
// alone), and the border rows Cm[row][col] = sc_row (sum over the views holding `row` of vpartB + Cpri[row][col] sc_col) + D / radius on the
// diagonal.  Grid: NB x NB workgroups for the border rows (fixed-order reductions over the views), then nblk(6 S) x NB for the instance rows.
__global__ void __launch_bounds__(256) gen_border_finish_kernel(Dev d, const int *col_pos, int ncols, const double *vpartB, double *Bc, double *Cm, double radius,
                                                                int have_bpri) {
  __shared__ double lds[8];
  const GenDev &g = d.g;
  const int NB = g.NB, n6 = d.cam0;
  if ((int)blockIdx.x < NB * NB) {
    const int row = blockIdx.x / NB, col = blockIdx.x - row * NB;
    const int c = col_pos[col];  // position of `col` among the observation-touching columns, -1: none
    double v[1] = {0.0};
    if (c >= 0)
      for (int vw = threadIdx.x; vw < g.NV; vw += 256) {
        const int slot = g.col_slot[(long)row * g.NV + vw];
        if (slot != 255) v[0] += vpartB[((long)vw * ncols + c) * g.KW + slot];
      }
    block_sum<1, 256>(v, lds);
    if (threadIdx.x == 0) {
      const double sr = d.sc_red[n6 + row], scol = d.sc_red[n6 + col];
      Cm[row * NB + col] = sr * (v[0] + g.Cpri[(long)row * NB + col] * scol) + (row == col ? d.D_red[n6 + row] / radius : 0.0);
    }
    return;
  }
  const long t = (long)(blockIdx.x - NB * NB) * 256 + threadIdx.x;
  if (t >= (long)NB * n6) return;
  const int col = (int)(t / n6), i = (int)(t - (long)col * n6);
  double val = col_pos[col] >= 0 ? Bc[t] : 0.0;
  if (have_bpri) val += d.sc_red[i] * g.Bpri[t] * d.sc_red[n6 + col];
  Bc[t] = val;
}
