// Leave-one-out refits of a small tPLS model, ALL FOLDS IN ONE LAUNCH: validate.get_q2y (cmtf_pls/validate.py:7-37)
// refits the model once per held-out sample (validate.py:27-33); each refit is a complete tPLS.fit
// (tpls.py:73-113) on I - 1 samples followed by predict (tpls.py:122-143) on the one left out.  For the sizes this
// helper is used at (hundreds of samples, a few thousand columns) one refit is a few hundred tiny launches, i.e. pure
// launch latency, and the I refits are independent -- so here ONE WORKGROUP owns one fold and runs the whole fit for
// it (centring, the NIPALS loop with its convergence test, rank-1 extraction, deflation, inner regression, Y
// deflation, projection of the held-out row) without leaving the kernel; the folds run side by side on the CUs.
//
// What is shared between folds instead of recomputed (SURVEY 8(f2) "down-date instead of refitting"): the column
// sums of X and Y are formed once; fold i's mean is (colsum - row_i) / (I - 1).  The held-out row is zeroed in the
// fold's centred working copy, which removes it from every sum of the fit without a row gather.
//
// Arithmetic: float64 throughout, the operation order of the reference loop; the rank-1 extraction is the product's
// (Gram matrix of the smaller side squared repeatedly with power-of-two rescaling until numerically rank one, one
// exact pass with Z, sign rule on the last mode), run inside the workgroup with G in LDS.
// Limits (the caller falls back to one refit per fold on the regular engine otherwise): X of order 2 or 3 without
// missing values, min(A, B) <= 64, M <= 64, R <= 16, and the per-workgroup vectors must fit 150 KB of LDS.
#include "common.hpp"
#include "fold_regress.hpp"

namespace cmtfpls {

constexpr int kLooMaxN = 64, kLooMaxR = 16, kLooMaxM = 64;

struct LooArgs {
  const double* X;        // (I, P) original, uncentred
  const double* Y;        // (I, M)
  const double* colsum_x; // (P)
  const double* colsum_y; // (M)
  double* ws;             // per resident fold: Xf (I*P) | Yf (I*M) | T (I*R)
  double* Ypred;          // (I, M): row i = prediction of the model fitted without sample i
  int* n_iter;            // (I, R) inner iterations executed (nullable)
  int64_t ws_per_fold;    // doubles
  int I, A, B, M, R, max_iter, fold0, nfolds;
  double tol;
  // whole != 0 (round 3, cmtfpls_fit_small_f64): ONE workgroup fits ALL I samples -- no held-out row, means over I rows
  // formed here -- and writes the fitted state instead of a prediction: the complete tPLS.fit (tpls.py:73-120) of a small
  // problem in one launch.  T goes to ws (I x R, the caller's output buffer).
  int whole;
  double* U_out;          // (I, R)  Y scores
  double* WA_out;         // (A, R)
  double* WB_out;         // (B, R)
  double* Q_out;          // (M, R)
  double* coef_out;       // (R, R)
  double* ssq_out;        // (R + 1, 2): row 0 = |X_c|^2, |Y_c|^2; row a + 1 = the same after deflating component a
  double* xmean_out;      // (P)
  double* ymean_out;      // (M)
  int* flag_out;          // set to 1 when X or Y holds a non-finite value (the caller then takes the regular engine)
  double* T_whole;        // (I, R) X scores (whole fit)
  int64_t lds_xy_offset;  // > 0: the centred X (I * P) and Y (I * M) are kept in LDS, this many doubles into the dynamic allocation
};

#include "loo_rank1.hpp"

// NT = 256 for the leave-one-out launch (one workgroup per fold, the folds side by side on the CUs); NT = 1024 for the
// whole fit, where the one workgroup is all the parallelism there is
template <int NT>
__global__ __launch_bounds__(NT) void loo_tpls_kernel(LooArgs a) {
  constexpr int kLooThreads = NT;
  extern __shared__ double sm[];
  __shared__ double red[16];
  __shared__ int ired[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int I = a.I, A = a.A, B = a.B, M = a.M, R = a.R, P = A * B;
  const int n = A < B ? A : B, k = A < B ? B : A;
  const bool whole = a.whole != 0;
  const int fold = whole ? -1 : a.fold0 + blockIdx.x;              // -1: no row is held out
  if (!whole && (blockIdx.x >= a.nfolds || fold >= I)) return;
  double* Xf = a.ws + (int64_t)blockIdx.x * a.ws_per_fold;
  double* Yf = Xf + (int64_t)I * P;
  // whole fit of a problem whose centred copies fit next to the vectors: X and Y live in LDS for the whole fit (the tail of the
  // dynamic allocation, a.lds_xy_offset doubles in) -- every sweep of an iteration is then an LDS sweep instead of an L2 one
  if (whole && a.lds_xy_offset > 0) {
    Xf = sm + a.lds_xy_offset;
    Yf = Xf + (int64_t)I * P;
  }
  double* T = whole ? a.T_whole : Yf + (int64_t)I * M;
  // LDS carve-up
  double* u = sm;
  double* t = u + I;
  double* Z = t + I;
  double* wA = Z + P;
  double* wB = wA + A;
  double* q = wB + B;
  double* qn = q + M;
  double* G0 = qn + M;
  double* G1 = G0 + n * n;
  double* xs = G1 + n * n;
  double* ys = xs + n;
  double* my = ys + k;            // mean of Y over the training rows
  double* coef = my + M;          // R x R
  double* Wa = coef + R * R;      // R x A
  double* Wb = Wa + R * A;        // R x B
  double* Qs = Wb + R * B;        // R x M
  double* Gn = Qs + R * M;        // (a+1) x (a+1) normal equations
  double* gn = Gn + R * R;
  double* bb = gn + R;
  double* dd = bb + R;
  double* part = dd + R;          // NT doubles: partial rows of the contraction when P < NT
  const int nrg = (P < kLooThreads) ? kLooThreads / P : 1;
  const double inv = 1.0 / (double)(whole ? I : I - 1);

  // ---- preprocess (tpls.py:61-71): means over the I - 1 training rows by down-dating the column sums; the
  // held-out row is zero in the working copies, i.e. absent from every sum below.  (whole fit: the column sums are
  // formed here, over all I rows; a non-finite sum = a missing value somewhere: flag it and leave)
  for (int o = tid; o < R * R; o += kLooThreads) coef[o] = 0.0;
  if (whole) {
    double bad = 0.0;
    for (int m = tid; m < M; m += kLooThreads) {
      double s = 0.0;
      for (int r = 0; r < I; ++r) s += a.Y[(int64_t)r * M + m];
      my[m] = s / (double)I;                                            // nanmean without NaNs (tpls.py:67)
      if (!isfinite(s)) bad = 1.0;
    }
    for (int c = tid; c < P; c += kLooThreads) {
      double s = 0.0;
      for (int r = 0; r < I; ++r) s += a.X[(int64_t)r * P + c];
      Z[c] = s / (double)I;                                             // tpls.py:66
      if (!isfinite(s)) bad = 1.0;
    }
    bad = loo_sum<NT>(bad, red);
    if (bad > 0.0) { if (tid == 0) *a.flag_out = 1; return; }           // uniform
    for (int c = tid; c < P; c += kLooThreads) a.xmean_out[c] = Z[c];
    for (int m = tid; m < M; m += kLooThreads) a.ymean_out[m] = my[m];
  } else {
    for (int m = tid; m < M; m += kLooThreads) my[m] = (a.colsum_y[m] - a.Y[(int64_t)fold * M + m]) * inv;
    for (int c = tid; c < P; c += kLooThreads) {
      const double mu = (a.colsum_x[c] - a.X[(int64_t)fold * P + c]) * inv;
      Z[c] = mu;                                            // kept in Z until the first iteration overwrites it
    }
  }
  __syncthreads();
  for (int64_t idx = tid; idx < (int64_t)I * P; idx += kLooThreads) {
    const int r = (int)(idx / P), c = (int)(idx % P);
    Xf[idx] = (r == fold) ? 0.0 : a.X[idx] - Z[c];
  }
  for (int64_t idx = tid; idx < (int64_t)I * M; idx += kLooThreads) {
    const int r = (int)(idx / M), m = (int)(idx % M);
    Yf[idx] = (r == fold) ? 0.0 : a.Y[idx] - my[m];
  }
  __syncthreads();
  if (whole) {                                                           // |X_c|^2, |Y_c|^2: the R2X / R2Y denominators
    double sx = 0.0, sy = 0.0;
    for (int64_t idx = tid; idx < (int64_t)I * P; idx += kLooThreads) sx = fma(Xf[idx], Xf[idx], sx);
    for (int64_t idx = tid; idx < (int64_t)I * M; idx += kLooThreads) sy = fma(Yf[idx], Yf[idx], sy);
    sx = loo_sum<NT>(sx, red);
    sy = loo_sum<NT>(sy, red);
    if (tid == 0) { a.ssq_out[0] = sx; a.ssq_out[1] = sy; }
  }

  for (int comp = 0; comp < R; ++comp) {
    for (int r = tid; r < I; r += kLooThreads) u[r] = Yf[(int64_t)r * M];             // tpls.py:78
    __syncthreads();
    int it = 0;
    for (; it < a.max_iter; ++it) {                                                    // tpls.py:79
      // Z = X x_0 u (tpls.py:83): a thread owns columns, rows stream past (coalesced across the workgroup)
      // (fewer columns than threads: nrg row groups share the rows of a column, partial rows added in index order)
      if (nrg == 1) {
        for (int c = tid; c < P; c += kLooThreads) {
          double s = 0.0;
          for (int r = 0; r < I; ++r) s = fma(Xf[(int64_t)r * P + c], u[r], s);
          Z[c] = s;
        }
      } else {
        const int rg = tid / P, c = tid % P;
        if (rg < nrg) {
          double s = 0.0;
          for (int r = rg; r < I; r += nrg) s = fma(Xf[(int64_t)r * P + c], u[r], s);
          part[rg * P + c] = s;
        }
        __syncthreads();
        for (int c2 = tid; c2 < P; c2 += kLooThreads) {
          double s = 0.0;
          for (int g = 0; g < nrg; ++g) s += part[g * P + c2];
          Z[c2] = s;
        }
      }
      __syncthreads();
      if (A == 1) {                                                                    // tpls.py:84: Z / norm(Z)
        double s = 0.0;
        for (int c = tid; c < P; c += kLooThreads) s = fma(Z[c], Z[c], s);
        const double nz = sqrt(loo_sum<NT>(s, red));
        for (int c = tid; c < P; c += kLooThreads) wB[c] = Z[c] / nz;
        if (tid == 0) wA[0] = 1.0;
        __syncthreads();
      } else {
        if (n <= 8 && k <= 64) loo_rank1_wave(Z, A, B, wA, wB);                          // tpls.py:86-88, inside one wavefront
        else loo_rank1<NT>(Z, A, B, wA, wB, G0, G1, xs, ys, red, ired);
      }
      // t = X x_1 wA x_2 wB (tpls.py:97-99): one wavefront per row
      for (int r = wv; r < I; r += kLooThreads / 64) {
        double s = 0.0;
        for (int c = lane; c < P; c += 64) s = fma(Xf[(int64_t)r * P + c], wA[c / B] * wB[c % B], s);
        s = wave_sum(s);
        if (lane == 0) t[r] = s;
      }
      __syncthreads();
      // q = Y^T t / |.| (tpls.py:100-101)
      if (tid < M) {
        double s = 0.0;
        for (int r = 0; r < I; ++r) s = fma(Yf[(int64_t)r * M + tid], t[r], s);
        q[tid] = s;
      }
      __syncthreads();
      double qs = (tid < M) ? q[tid] * q[tid] : 0.0;
      const double qnrm = sqrt(loo_sum<NT>(qs, red));
      if (tid < M) qn[tid] = q[tid] / qnrm;
      __syncthreads();
      // u = Y q and |u_old - u| (tpls.py:102-103)
      double du2 = 0.0;
      for (int r = tid; r < I; r += kLooThreads) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s = fma(Yf[(int64_t)r * M + m], qn[m], s);
        const double d0 = u[r] - s;
        du2 = fma(d0, d0, du2);
        u[r] = s;
      }
      const double du = sqrt(loo_sum<NT>(du2, red));
      if (it > 0 && du < a.tol) { ++it; break; }                                       // first pass: oldU = inf (tpls.py:77)
    }
    if (a.n_iter && tid == 0) a.n_iter[(int64_t)(whole ? 0 : fold) * R + comp] = it;
    // store the component; deflate X (tpls.py:109)
    for (int r = tid; r < I; r += kLooThreads) T[(int64_t)r * R + comp] = t[r];
    for (int j = tid; j < A; j += kLooThreads) Wa[comp * A + j] = wA[j];
    for (int j = tid; j < B; j += kLooThreads) Wb[comp * B + j] = wB[j];
    for (int m = tid; m < M; m += kLooThreads) Qs[comp * M + m] = qn[m];
    double ssx = 0.0;
    for (int64_t idx = tid; idx < (int64_t)I * P; idx += kLooThreads) {
      const int r = (int)(idx / P), c = (int)(idx % P);
      const double v = Xf[idx] - t[r] * (wA[c / B] * wB[c % B]);
      Xf[idx] = v;
      ssx = fma(v, v, ssx);
    }
    if (whole) {
      for (int r = tid; r < I; r += kLooThreads) a.U_out[(int64_t)r * R + comp] = u[r];
      ssx = loo_sum<NT>(ssx, red);                                           // R2X[comp] = 1 - |X_{comp+1}|^2 / |X_c|^2 (tpls.py:115-117)
      if (tid == 0) a.ssq_out[2 * (comp + 1)] = ssx;
    }
    __syncthreads();
    // inner regression b = lstsq(T[:, :k], u) (tpls.py:110-112), fold_regress.hpp; then Y -= T b q^T (tpls.py:113), yhat = T b in t
    fold_inner_regression<NT, false>(T, u, nullptr, I, R, comp, Gn, gn, bb, dd, coef, t);
    double ssy = 0.0;
    for (int64_t idx = tid; idx < (int64_t)I * M; idx += kLooThreads) {
      const int r = (int)(idx / M), m = (int)(idx % M);
      const double v = Yf[idx] - t[r] * qn[m];
      Yf[idx] = v;
      ssy = fma(v, v, ssy);
    }
    if (whole) {
      ssy = loo_sum<NT>(ssy, red);                                           // R2Y[comp] = 1 - |Y_{comp+1}|^2 / |Y_c|^2 (tpls.py:118-120)
      if (tid == 0) a.ssq_out[2 * (comp + 1) + 1] = ssy;
    }
    __syncthreads();
  }
  if (whole) {                                                           // the fitted state (T is already in the caller's buffer)
    for (int o = tid; o < R * A; o += kLooThreads) a.WA_out[(int64_t)(o % A) * R + o / A] = Wa[o];
    for (int o = tid; o < R * B; o += kLooThreads) a.WB_out[(int64_t)(o % B) * R + o / B] = Wb[o];
    for (int o = tid; o < R * M; o += kLooThreads) a.Q_out[(int64_t)(o % M) * R + o / M] = Qs[o];
    for (int o = tid; o < R * R; o += kLooThreads) a.coef_out[o] = coef[o];
    return;
  }

  // ---- predict the held-out sample (tpls.py:122-143): centre with the fold's means, project and deflate
  for (int c = tid; c < P; c += kLooThreads) Z[c] = a.X[(int64_t)fold * P + c] - (a.colsum_x[c] - a.X[(int64_t)fold * P + c]) * inv;
  __syncthreads();
  double* sc = u;                                                                       // scores of the held-out row (R)
  for (int comp = 0; comp < R; ++comp) {
    double s = 0.0;
    for (int c = tid; c < P; c += kLooThreads) s = fma(Z[c], Wa[comp * A + c / B] * Wb[comp * B + c % B], s);
    const double sv = loo_sum<NT>(s, red);
    if (tid == 0) sc[comp] = sv;
    for (int c = tid; c < P; c += kLooThreads) Z[c] -= sv * (Wa[comp * A + c / B] * Wb[comp * B + c % B]);
    __syncthreads();
  }
  for (int m = tid; m < M; m += kLooThreads) {
    double yv = 0.0;
    for (int b2 = 0; b2 < R; ++b2) {
      double sb = 0.0;
      for (int a2 = 0; a2 < R; ++a2) sb = fma(sc[a2], coef[a2 * R + b2], sb);        // (scores @ coef_)[b]
      yv = fma(sb, Qs[b2 * M + m], yv);                                             // @ Q^T
    }
    a.Ypred[(int64_t)fold * M + m] = yv + my[m];
  }
}

static size_t loo_lds_bytes(int I, int A, int B, int M, int R, int NT) {
  const size_t n = (size_t)(A < B ? A : B), k = (size_t)(A < B ? B : A), P = (size_t)A * B;
  const size_t dbl = 2 * (size_t)I + P + A + B + 2 * (size_t)M + 2 * n * n + n + k + M + (size_t)R * R + (size_t)R * (A + B) +
                     (size_t)R * M + (size_t)R * R + 3 * (size_t)R + (size_t)NT;
  return dbl * sizeof(double);
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {

size_t cmtfpls_loo_fold_workspace_bytes(int I, int A, int B, int M, int R) {
  if (I <= 1 || A <= 0 || B <= 0 || M <= 0 || R <= 0) return 0;
  return ((size_t)I * A * B + (size_t)I * M + (size_t)I * R) * sizeof(double);
}

int cmtfpls_loo_tpls_f64(const double* X, const double* Y, const double* colsum_x, const double* colsum_y, int I, int A, int B, int M,
                         int R, double tol, int max_iter, int fold0, int nfolds, double* Ypred, int* n_iter, void* ws,
                         size_t ws_bytes, void* stream) {
  if (!X || !Y || !colsum_x || !colsum_y || !Ypred || I <= 1 || A <= 0 || B <= 0 || M <= 0 || R <= 0 || max_iter <= 0 || fold0 < 0 ||
      nfolds <= 0 || fold0 + nfolds > I) {
    set_error("loo_tpls: bad argument");
    return CMTFPLS_EINVAL;
  }
  const int n = A < B ? A : B;
  const size_t lds = loo_lds_bytes(I, A, B, M, R, 256);
  if (n > kLooMaxN || M > kLooMaxM || R > kLooMaxR || lds > 150 * 1024) {
    set_error("loo_tpls: shape outside the one-workgroup-per-fold form; refit per fold on the regular engine");
    return CMTFPLS_EUNSUPPORTED;
  }
  const size_t per = cmtfpls_loo_fold_workspace_bytes(I, A, B, M, R);
  if (!ws || ws_bytes < per * (size_t)nfolds) { set_error("loo_tpls: workspace too small"); return CMTFPLS_EWORKSPACE; }
  LooArgs a;
  a.X = X; a.Y = Y; a.colsum_x = colsum_x; a.colsum_y = colsum_y; a.ws = static_cast<double*>(ws); a.Ypred = Ypred; a.n_iter = n_iter;
  a.ws_per_fold = (int64_t)(per / sizeof(double));
  a.I = I; a.A = A; a.B = B; a.M = M; a.R = R; a.max_iter = max_iter; a.fold0 = fold0; a.nfolds = nfolds; a.tol = tol;
  a.whole = 0;
  a.T_whole = nullptr;
  a.lds_xy_offset = 0;
  a.U_out = a.WA_out = a.WB_out = a.Q_out = a.coef_out = a.ssq_out = a.xmean_out = a.ymean_out = nullptr;
  a.flag_out = nullptr;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(loo_tpls_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(loo_tpls_kernel<256>, dim3(nfolds), dim3(256), lds, (hipStream_t)stream, a);
  return check_launch("loo_tpls");
}

size_t cmtfpls_fit_small_workspace_bytes(int I, int A, int B, int M) {
  if (I <= 1 || A <= 0 || B <= 0 || M <= 0) return 0;
  return ((size_t)I * A * B + (size_t)I * M) * sizeof(double);
}

int cmtfpls_fit_small_f64(const double* X, const double* Y, int I, int A, int B, int M, int R, double tol, int max_iter,
                          double* T, double* U, double* WA, double* WB, double* Q, double* coef, double* ssq, double* x_mean,
                          double* y_mean, int* n_iter, int* flag, void* ws, size_t ws_bytes, void* stream) {
  if (!X || !Y || !T || !U || !WA || !WB || !Q || !coef || !ssq || !x_mean || !y_mean || !n_iter || !flag || I <= 1 || A <= 0 || B <= 0 ||
      M <= 0 || R <= 0 || max_iter <= 0) {
    set_error("fit_small: bad argument");
    return CMTFPLS_EINVAL;
  }
  const int n = A < B ? A : B;
  size_t lds = loo_lds_bytes(I, A, B, M, R, 1024);
  if (n > kLooMaxN || M > kLooMaxM || R > kLooMaxR || lds > 150 * 1024) {
    set_error("fit_small: shape outside the one-workgroup form; use the regular engine");
    return CMTFPLS_EUNSUPPORTED;
  }
  // the centred copies of X and Y in LDS too when everything fits 158 KB (BASELINE configs[0]: 128 KB + 6 KB + 19 KB)
  const size_t xy = ((size_t)I * A * B + (size_t)I * M) * sizeof(double);
  const int64_t xy_off = (lds + xy <= 158 * 1024) ? (int64_t)(lds / sizeof(double)) : 0;
  if (xy_off > 0) lds += xy;
  if (!ws || ws_bytes < cmtfpls_fit_small_workspace_bytes(I, A, B, M)) { set_error("fit_small: workspace too small"); return CMTFPLS_EWORKSPACE; }
  // workspace: Xf (I * P) | Yf (I * M); the kernel's third slot (T, I x R) is the caller's output buffer
  LooArgs a;
  a.X = X; a.Y = Y; a.colsum_x = nullptr; a.colsum_y = nullptr; a.ws = static_cast<double*>(ws); a.Ypred = nullptr; a.n_iter = n_iter;
  a.ws_per_fold = 0;
  a.I = I; a.A = A; a.B = B; a.M = M; a.R = R; a.max_iter = max_iter; a.fold0 = 0; a.nfolds = 1; a.tol = tol;
  a.whole = 1;
  a.T_whole = T;
  a.lds_xy_offset = xy_off;
  a.U_out = U; a.WA_out = WA; a.WB_out = WB; a.Q_out = Q; a.coef_out = coef; a.ssq_out = ssq; a.xmean_out = x_mean; a.ymean_out = y_mean;
  a.flag_out = flag;
  // (the 256-thread instance was measured against this one in round 3, profiles/r03q_small_fit.txt; build with
  // -DCMTFPLS_FIT_SMALL_NT=256 to repeat that: a compile-time variant for tools, no run-time hook in the product path)
#if defined(CMTFPLS_FIT_SMALL_NT) && CMTFPLS_FIT_SMALL_NT == 256
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(loo_tpls_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(loo_tpls_kernel<256>, dim3(1), dim3(256), lds, (hipStream_t)stream, a);
  return check_launch("fit_small");
#endif
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(loo_tpls_kernel<1024>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(loo_tpls_kernel<1024>, dim3(1), dim3(1024), lds, (hipStream_t)stream, a);
  return check_launch("fit_small");
}

}  // extern "C"
