// Cross-validation refits of a small tPLS whose X has missing values, ALL FOLDS IN ONE LAUNCH: validate.get_q2y (leave-one-out,
// cmtf_pls/validate.py:7-37) and validate.kfold_predictions.  Fold f holds out the rows r with fold_of[r] == f and refits the
// model on the others -- the reference's tPLS.fit (tpls.py:73-113) with its missing-value arithmetic (X_hasMiss, tpls.py:61-63;
// miss_tensordot / miss_mmodedot, missingvals.py:7-38) -- then predicts the held-out rows (tpls.py:122-143) with every component
// count.  One workgroup per fold, as loo_tpls_kernel (loo.hip), whose structure this follows: the fold's centred working copy
// Xf | Yf | T in the workspace, deflated in place, with the fold's column counts and means; the vectors in LDS; the direct
// NIPALS loop without leaving the kernel.
//
// The masked arithmetic is a per-column and a per-row rescale of the zero-filled working copy (held-out rows, missing entries
// and columns without a training observation are 0 in Xf, so every masked sum is an ordinary sum):
//   c_p   = training observations of column p, down-dated from the shared counts;  mu_p = down-dated sum / c_p (NaN if c_p = 0)
//   miss  = some training entry is missing (some c_p < n_f): the reference's X_hasMiss on the training rows
//   Z_p   = (sum_r Xf[r,p] u_r) / c_p * n_f      (miss_tensordot; 0 when c_p = 0)
//   t_r   = (sum_p Xf[r,p] w_p) / o_r * P         (miss_mmodedot; o_r = observed entries of training row r; held-out rows 0)
//   deflation on the observed training entries only (missing entries stay 0).
// A fold without missing training entries takes the unmasked arithmetic, as the reference does.  The held-out batch is centred
// with the fold's means and then masked (an entry is missing when it is NaN after centring: tpls.py:128-131); if any held-out
// entry of the fold is missing the whole batch takes the masked score and deflation; a held-out row with nothing observed
// predicts NaN (0 / 0, as the reference).  A training row with nothing observed makes the reference NaN everywhere: the fold
// reports status 1 and writes nothing else.
// Limits: those of the LDS form (min(A, B) <= 64, M <= 64, R <= 16, the vectors plus the per-row counts and flags within 150 KB
// of LDS), 1 <= K <= I, at least 2 training rows per fold (status 2 otherwise).
#include "common.hpp"
#include "fold_regress.hpp"

namespace cmtfpls {

#include "loo_rank1.hpp"

constexpr int kCvMaxN = 64, kCvMaxR = 16, kCvMaxM = 64, kCvThreads = 256;

struct CvMaskedArgs {
  const double* X;        // (I, P) original, uncentred, NaN = missing
  const double* Y;        // (I, M) complete
  const int* fold_of;     // (I) fold id of every row
  const double* colsum_x; // (P) sums of the observed entries of all rows
  const double* colcnt_x; // (P) observed entries per column
  const double* colsum_y; // (M)
  double* ws;             // per resident fold: Xf (I*P) | Yf (I*M) | T (I*R) | cs (P) | mu (P)
  double* Ypred;          // (R, I, M): [r - 1, i] = prediction of row i by the r-component model of its fold
  int* n_iter;            // (K, R) (nullable)
  int* status;            // (K): 0 ok, 1 a training row without an observed entry, 2 fewer than 2 training rows
  int* info;              // (K, 2) (nullable): [f, 0] the training rows took the masked arithmetic, [f, 1] the held-out batch did
  int64_t ws_per_fold;    // doubles
  int I, A, B, M, R, K, max_iter, fold0, nfolds;
  double tol;
};

__global__ __launch_bounds__(kCvThreads) void cv_masked_kernel(CvMaskedArgs a) {
  constexpr int NT = kCvThreads;
  extern __shared__ double sm[];
  __shared__ double red[16];
  __shared__ int ired[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int I = a.I, A = a.A, B = a.B, M = a.M, R = a.R, P = A * B;
  const int n = A < B ? A : B, k = A < B ? B : A;
  const int fold = a.fold0 + blockIdx.x;
  if (blockIdx.x >= a.nfolds || fold >= a.K) return;
  double* Xf = a.ws + (int64_t)blockIdx.x * a.ws_per_fold;
  double* Yf = Xf + (int64_t)I * P;
  double* T = Yf + (int64_t)I * M;
  double* cs = T + (int64_t)I * R;  // P: training observations of each column (c_p)
  double* mu = cs + P;              // P: training means of X (NaN where c_p = 0)
  // LDS carve-up: loo_tpls_kernel's, then the per-row counts and held-out flags (the per-column ones are read once per column and
  // sweep: they stay in the workspace, which keeps min(A, B) = 64 within the LDS)
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
  double* ro = part + NT;         // I: observed entries of each row (o_r)
  double* hf = ro + I;            // I: 1 = held out by this fold
  const int nrg = (P < NT) ? NT / P : 1;

  if (tid == 0) a.status[fold] = 0;
  // ---- fold sizes
  double nh = 0.0;
  for (int r = tid; r < I; r += NT) {
    const bool h = a.fold_of[r] == fold;
    hf[r] = h ? 1.0 : 0.0;
    nh += h ? 1.0 : 0.0;
  }
  nh = loo_sum<NT>(nh, red);                                                  // (its barriers publish hf)
  const double nf = (double)I - nh;
  if (nf < 2.0) { if (tid == 0) a.status[fold] = 2; return; }                // uniform
  // ---- means (tpls.py:66-67, np.nanmean): down-date the shared sums and counts by the held-out rows
  for (int o = tid; o < R * R; o += NT) coef[o] = 0.0;
  double missing = 0.0;
  for (int c = tid; c < P; c += NT) {
    double s = 0.0, cnt = 0.0;
    for (int r = 0; r < I; ++r) {
      if (hf[r] == 0.0) continue;
      const double x = a.X[(int64_t)r * P + c];
      if (!isnan(x)) { s += x; cnt += 1.0; }
    }
    const double cp = a.colcnt_x[c] - cnt;
    cs[c] = cp;
    mu[c] = cp > 0.0 ? (a.colsum_x[c] - s) / cp : __builtin_nan("");
    if (cp < nf) missing = 1.0;
  }
  for (int m = tid; m < M; m += NT) {
    double s = 0.0;
    for (int r = 0; r < I; ++r)
      if (hf[r] != 0.0) s += a.Y[(int64_t)r * M + m];
    my[m] = (a.colsum_y[m] - s) / nf;
  }
  const bool miss = loo_sum<NT>(missing, red) > 0.0;                          // X_hasMiss of the training rows (tpls.py:61)
  // ---- working copies: centred, zero at held-out rows and missing entries
  for (int64_t idx = tid; idx < (int64_t)I * P; idx += NT) {
    const int r = (int)(idx / P), c = (int)(idx % P);
    const double x = a.X[idx];
    Xf[idx] = (hf[r] != 0.0 || isnan(x)) ? 0.0 : x - mu[c];
  }
  for (int64_t idx = tid; idx < (int64_t)I * M; idx += NT) {
    const int r = (int)(idx / M), m = (int)(idx % M);
    Yf[idx] = (hf[r] != 0.0) ? 0.0 : a.Y[idx] - my[m];
  }
  for (int64_t idx = tid; idx < (int64_t)I * R; idx += NT) T[idx] = 0.0;
  // observed entries of every training row; one without any makes the reference's score 0 / 0
  double empty = 0.0;
  for (int r = wv; r < I; r += NT / 64) {
    double cnt = 0.0;
    for (int c = lane; c < P; c += 64) cnt += isnan(a.X[(int64_t)r * P + c]) ? 0.0 : 1.0;
    cnt = wave_sum(cnt);
    if (lane == 0) ro[r] = cnt;
    if (hf[r] == 0.0 && cnt == 0.0) empty = 1.0;
  }
  if (loo_sum<NT>(empty, red) > 0.0) { if (tid == 0) a.status[fold] = 1; return; }   // uniform (its barriers publish Xf, Yf, ro)
  const double Pd = (double)P;

  for (int comp = 0; comp < R; ++comp) {
    for (int r = tid; r < I; r += NT) u[r] = Yf[(int64_t)r * M];                   // tpls.py:78
    __syncthreads();
    int it = 0;
    for (; it < a.max_iter; ++it) {                                                  // tpls.py:79
      // Z = X x_0 u (tpls.py:83), or miss_tensordot (missingvals.py:17-19): the column's sum / c_p * n_f, 0 when c_p = 0
      if (nrg == 1) {
        for (int c = tid; c < P; c += NT) {
          double s = 0.0;
          for (int r = 0; r < I; ++r) s = fma(Xf[(int64_t)r * P + c], u[r], s);
          Z[c] = miss ? (cs[c] > 0.0 ? s / cs[c] * nf : 0.0) : s;
        }
      } else {
        const int rg = tid / P, c = tid % P;
        if (rg < nrg) {
          double s = 0.0;
          for (int r = rg; r < I; r += nrg) s = fma(Xf[(int64_t)r * P + c], u[r], s);
          part[rg * P + c] = s;
        }
        __syncthreads();
        for (int c2 = tid; c2 < P; c2 += NT) {
          double s = 0.0;
          for (int g = 0; g < nrg; ++g) s += part[g * P + c2];
          Z[c2] = miss ? (cs[c2] > 0.0 ? s / cs[c2] * nf : 0.0) : s;
        }
      }
      __syncthreads();
      if (A == 1) {                                                                  // tpls.py:84: Z / norm(Z)
        double s = 0.0;
        for (int c = tid; c < P; c += NT) s = fma(Z[c], Z[c], s);
        const double nz = sqrt(loo_sum<NT>(s, red));
        for (int c = tid; c < P; c += NT) wB[c] = Z[c] / nz;
        if (tid == 0) wA[0] = 1.0;
        __syncthreads();
      } else {
        if (n <= 8 && k <= 64) loo_rank1_wave(Z, A, B, wA, wB);                        // tpls.py:86-88
        else loo_rank1<NT>(Z, A, B, wA, wB, G0, G1, xs, ys, red, ired);
      }
      // t = X x_1 wA x_2 wB (tpls.py:97-99), or miss_mmodedot (missingvals.py:37): the row's sum / o_r * P; held-out rows 0
      for (int r = wv; r < I; r += NT / 64) {
        double s = 0.0;
        for (int c = lane; c < P; c += 64) s = fma(Xf[(int64_t)r * P + c], wA[c / B] * wB[c % B], s);
        s = wave_sum(s);
        if (lane == 0) t[r] = (hf[r] != 0.0) ? 0.0 : (miss ? s / ro[r] * Pd : s);
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
      for (int r = tid; r < I; r += NT) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s = fma(Yf[(int64_t)r * M + m], qn[m], s);
        const double d0 = u[r] - s;
        du2 = fma(d0, d0, du2);
        u[r] = s;
      }
      const double du = sqrt(loo_sum<NT>(du2, red));
      if (it > 0 && du < a.tol) { ++it; break; }                                     // first pass: oldU = inf (tpls.py:77)
    }
    if (a.n_iter && tid == 0) a.n_iter[(int64_t)fold * R + comp] = it;
    // store the component; deflate the observed training entries of X (tpls.py:109: a NaN stays NaN there)
    for (int r = tid; r < I; r += NT) T[(int64_t)r * R + comp] = t[r];
    for (int j = tid; j < A; j += NT) Wa[comp * A + j] = wA[j];
    for (int j = tid; j < B; j += NT) Wb[comp * B + j] = wB[j];
    for (int m = tid; m < M; m += NT) Qs[comp * M + m] = qn[m];
    for (int64_t idx = tid; idx < (int64_t)I * P; idx += NT) {
      const int r = (int)(idx / P), c = (int)(idx % P);
      if (hf[r] != 0.0 || (miss && isnan(a.X[idx]))) continue;
      Xf[idx] = Xf[idx] - t[r] * (wA[c / B] * wB[c % B]);
    }
    __syncthreads();
    // inner regression b = lstsq(T[:, :k], u) (tpls.py:110-112), fold_regress.hpp (held-out rows of T are 0); then
    // Y -= T b q^T (tpls.py:113), yhat = T b in t
    fold_inner_regression<NT, false>(T, u, nullptr, I, R, comp, Gn, gn, bb, dd, coef, t);
    for (int64_t idx = tid; idx < (int64_t)I * M; idx += NT) {
      const int r = (int)(idx / M), m = (int)(idx % M);
      Yf[idx] = Yf[idx] - t[r] * qn[m];
    }
    __syncthreads();
  }

  // ---- predict the held-out rows (tpls.py:122-143): centre with the fold's means, THEN mask (NaN after centring, which takes in
  // the columns without a training observation); the batch is masked when any of its entries is
  double hmiss = 0.0;
  for (int r = wv; r < I; r += NT / 64) {
    if (hf[r] == 0.0) continue;                                                       // uniform in the wavefront
    double cnt = 0.0;
    for (int c = lane; c < P; c += 64) {
      const double v = a.X[(int64_t)r * P + c] - mu[c];
      const bool ob = !isnan(v);
      Xf[(int64_t)r * P + c] = ob ? v : 0.0;
      cnt += ob ? 1.0 : 0.0;
    }
    cnt = wave_sum(cnt);
    if (lane == 0) ro[r] = cnt;
    if (cnt < Pd) hmiss = 1.0;
  }
  const bool hm = loo_sum<NT>(hmiss, red) > 0.0;
  // scores and deflation per component: a wavefront owns a held-out row for all R components (no barrier between them); the
  // scores go to the row's (zero) slots of T
  for (int r = wv; r < I; r += NT / 64) {
    if (hf[r] == 0.0) continue;
    const double o_r = ro[r];
    for (int comp = 0; comp < R; ++comp) {
      double s = 0.0;
      for (int c = lane; c < P; c += 64) s = fma(Xf[(int64_t)r * P + c], Wa[comp * A + c / B] * Wb[comp * B + c % B], s);
      s = wave_sum(s);
      const double sv = hm ? s / o_r * Pd : s;                                       // o_r = 0: 0 / 0 = NaN, as the reference
      if (lane == 0) T[(int64_t)r * R + comp] = sv;
      for (int c = lane; c < P; c += 64) {
        if (hm && isnan(a.X[(int64_t)r * P + c] - mu[c])) continue;
        Xf[(int64_t)r * P + c] = Xf[(int64_t)r * P + c] - sv * (Wa[comp * A + c / B] * Wb[comp * B + c % B]);
      }
    }
  }
  __syncthreads();
  // Ypred[c - 1] = scores[:, :c] coef_[:c, :c] Q[:, :c]^T + nu for c = 1..R: coef_ is upper triangular, so h = scores coef_ is the
  // same for every c and the c-component prediction is nu + the first c terms of h Q^T
  for (int64_t o = tid; o < (int64_t)I * M; o += NT) {
    const int r = (int)(o / M), m = (int)(o % M);
    if (hf[r] == 0.0) continue;
    double acc = 0.0;
    for (int b2 = 0; b2 < R; ++b2) {
      double h = 0.0;
      for (int a2 = 0; a2 <= b2; ++a2) h = fma(T[(int64_t)r * R + a2], coef[a2 * R + b2], h);
      acc = fma(h, Qs[b2 * M + m], acc);
      a.Ypred[((int64_t)b2 * I + r) * M + m] = acc + my[m];
    }
  }
  if (a.info && tid == 0) {
    a.info[2 * (int64_t)fold] = miss ? 1 : 0;
    a.info[2 * (int64_t)fold + 1] = hm ? 1 : 0;
  }
}

static size_t cv_masked_lds_bytes(int I, int A, int B, int M, int R) {
  const size_t n = (size_t)(A < B ? A : B), k = (size_t)(A < B ? B : A), P = (size_t)A * B;
  const size_t dbl = 2 * (size_t)I + P + A + B + 2 * (size_t)M + 2 * n * n + n + k + M + (size_t)R * R + (size_t)R * (A + B) +
                     (size_t)R * M + (size_t)R * R + 3 * (size_t)R + (size_t)kCvThreads + 2 * (size_t)I;
  return dbl * sizeof(double);
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {

size_t cmtfpls_cv_masked_fold_workspace_bytes(int I, int A, int B, int M, int R) {
  if (I <= 1 || A <= 0 || B <= 0 || M <= 0 || R <= 0) return 0;
  return ((size_t)I * A * B + (size_t)I * M + (size_t)I * R + 2 * (size_t)A * B) * sizeof(double);
}

int cmtfpls_cv_masked_f64(const double* X, const double* Y, const int* fold_of, int K, const double* colsum_x, const double* colcnt_x,
                          const double* colsum_y, int I, int A, int B, int M, int R, double tol, int max_iter, int fold0, int nfolds,
                          double* Ypred, int* n_iter, int* status, int* info, void* ws, size_t ws_bytes, void* stream) {
  if (!X || !Y || !fold_of || !colsum_x || !colcnt_x || !colsum_y || !Ypred || !status || I <= 1 || A <= 0 || B <= 0 || M <= 0 ||
      R <= 0 || max_iter <= 0 || K <= 0 || fold0 < 0 || nfolds <= 0) {
    set_error("cv_masked: bad argument");
    return CMTFPLS_EINVAL;
  }
  const int n = A < B ? A : B;
  const size_t lds = cv_masked_lds_bytes(I, A, B, M, R);
  if (K > I || n > kCvMaxN || M > kCvMaxM || R > kCvMaxR || lds > 150 * 1024) {
    set_error("cv_masked: shape outside the one-workgroup-per-fold form; refit per fold on the regular engine");
    return CMTFPLS_EUNSUPPORTED;
  }
  if (fold0 + nfolds > K) { set_error("cv_masked: folds out of range"); return CMTFPLS_EINVAL; }
  const size_t per = cmtfpls_cv_masked_fold_workspace_bytes(I, A, B, M, R);
  if (!ws || ws_bytes < per * (size_t)nfolds) { set_error("cv_masked: workspace too small"); return CMTFPLS_EWORKSPACE; }
  CvMaskedArgs a;
  a.X = X; a.Y = Y; a.fold_of = fold_of; a.colsum_x = colsum_x; a.colcnt_x = colcnt_x; a.colsum_y = colsum_y;
  a.ws = static_cast<double*>(ws); a.Ypred = Ypred; a.n_iter = n_iter; a.status = status; a.info = info;
  a.ws_per_fold = (int64_t)(per / sizeof(double));
  a.I = I; a.A = A; a.B = B; a.M = M; a.R = R; a.K = K; a.max_iter = max_iter; a.fold0 = fold0; a.nfolds = nfolds; a.tol = tol;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cv_masked_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(cv_masked_kernel, dim3(nfolds), dim3(kCvThreads), lds, (hipStream_t)stream, a);
  return check_launch("cv_masked");
}

}  // extern "C"
