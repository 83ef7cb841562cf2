// Refits of a small tPLS whose X has missing values on count-weighted rows, ALL MODELS OF A CHUNK IN ONE LAUNCH: the permutation
// test (validate.permutation_test_q2y), repeated K-fold (validate.get_q2y_repeated_kfold) and the bootstrap
// (validate.bootstrap_factors) of such data.  Model m is defined by counts[m, r] >= 0 (how many times row r of X is in its training
// data; 0 = held out) and yrow[m, r] (the row of Y paired with X row r; nullable = identity): its training data is literally X[r]
// repeated c_r times with Y[yrow[r]], and its arithmetic is the reference's tPLS.fit (tpls.py:73-113) with the missing-value
// arithmetic (X_hasMiss, tpls.py:61-63; miss_tensordot / miss_mmodedot, missingvals.py:7-38) on that data, every sum over rows
// weighted by c_r.  Then the held-out rows (c_r = 0) are predicted as one batch (tpls.py:122-143) with every component count.
// One workgroup per model, as cv_masked_kernel (cv_masked.hip), whose structure this follows: the model's centred working copy
// Xf | Yf | T in the workspace, deflated in place, with the model's column counts and means; the vectors in LDS.
//
// With n = sum_r c_r and Xf zero at held-out rows and missing entries:
//   c_p   = sum_r c_r [x_rp observed];  mu_p = sum_r c_r x_rp / c_p (NaN if c_p = 0);  nu = sum_r c_r Y[yrow[r]] / n
//   miss  = some c_p < n: the reference's X_hasMiss on the resampled data
//   Z_p   = (sum_r c_r Xf[r,p] u_r) / c_p * n    (miss_tensordot; 0 when c_p = 0), sum_r c_r Xf[r,p] u_r when not masked
//   t_r   = (sum_p Xf[r,p] w_p) / o_r * P         (miss_mmodedot; o_r = observed entries of row r; held-out rows 0)
//   q     = sum_r c_r Yf[r] t_r, normalised; convergence on sqrt(sum_r c_r (u_r - u_old,r)^2)
//   lstsq = (T^T C T) b = T^T C u, Y deflated on the training rows; X deflated on the observed training entries only.
// The held-out batch: centred by mu, then masked (NaN after centring counts as missing); masked for the whole batch when any of
// its entries is missing; a held-out row with nothing observed predicts NaN (0 / 0, as the reference).  Status 1: a training row
// with nothing observed (the reference is NaN everywhere); 2: n < 2; 3: a negative count or a yrow outside 0..I-1.  A model with a
// status writes nothing else.  With 0/1 counts and identity yrow a model is a fold of cv_masked_kernel.
// Limits: those of cv_masked.hip (min(A, B) <= 64, M <= 64, R <= 16, the vectors plus the per-row counts within 150 KB of LDS).
#include "common.hpp"
#include "fold_regress.hpp"

namespace cmtfpls {

#include "loo_rank1.hpp"

constexpr int kCvmMaxN = 64, kCvmMaxR = 16, kCvmMaxM = 64, kCvmThreads = 256;

struct CvMaskedModelsArgs {
  const double* X;        // (I, P) original, uncentred, NaN = missing
  const double* Y;        // (I, M) complete
  const int* counts;      // (nm, I) multiplicity of every row in every model
  const int* yrow;        // (nm, I) row of Y paired with each X row (nullable: identity)
  double* ws;             // per resident model: Xf (I*P) | Yf (I*M) | T (I*R) | cs (P) | mu (P)
  double* Ypred;          // (nm, R, I, M): [m, r - 1, i] = prediction of held-out row i by model m's r-component fit
  double* Wa;             // (nm, R, A) (nullable)
  double* Wb;             // (nm, R, B) (nullable)
  double* coef;           // (nm, R, R) (nullable): coef_[row, component]
  double* Q;              // (nm, R, M) (nullable)
  int* n_iter;            // (nm, R) (nullable)
  int* status;            // (nm)
  int* info;              // (nm, 2) (nullable): [m, 0] the training rows took the masked arithmetic, [m, 1] the held-out batch did
  int64_t ws_per_model;   // doubles
  int I, A, B, M, R, nm, max_iter, model0, nmodels;
  double tol;
};

__global__ __launch_bounds__(kCvmThreads) void cv_masked_models_kernel(CvMaskedModelsArgs a) {
  constexpr int NT = kCvmThreads;
  extern __shared__ double sm[];
  __shared__ double red[16];
  __shared__ int ired[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int I = a.I, A = a.A, B = a.B, M = a.M, R = a.R, P = A * B;
  const int n = A < B ? A : B, k = A < B ? B : A;
  const int model = a.model0 + blockIdx.x;
  if (blockIdx.x >= a.nmodels || model >= a.nm) return;
  const int* cnt_m = a.counts + (int64_t)model * I;
  const int* yrow_m = a.yrow ? a.yrow + (int64_t)model * I : nullptr;
  double* Xf = a.ws + (int64_t)blockIdx.x * a.ws_per_model;
  double* Yf = Xf + (int64_t)I * P;
  double* T = Yf + (int64_t)I * M;
  double* cs = T + (int64_t)I * R;  // P: weighted observations of each column (c_p)
  double* mu = cs + P;              // P: weighted means of X (NaN where c_p = 0)
  // LDS carve-up: cv_masked_kernel's, with the per-row counts where it keeps its held-out flags
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
  double* my = ys + k;            // weighted mean of the paired Y rows (nu)
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
  double* cw = ro + I;            // I: c_r, 0 = held out
  const int nrg = (P < NT) ? NT / P : 1;

  if (tid == 0) a.status[model] = 0;
  // ---- counts and training size; a bad count or Y row stops the model before Y is read
  double nt = 0.0, bad = 0.0;
  for (int r = tid; r < I; r += NT) {
    const int c = cnt_m[r];
    const int yr = yrow_m ? yrow_m[r] : r;
    if (c < 0 || yr < 0 || yr >= I) bad = 1.0;
    cw[r] = c > 0 ? (double)c : 0.0;
    nt += c > 0 ? (double)c : 0.0;
  }
  const double nf = loo_sum<NT>(nt, red);                                       // (its barriers publish cw)
  if (loo_sum<NT>(bad, red) > 0.0) { if (tid == 0) a.status[model] = 3; return; }   // uniform
  if (nf < 2.0) { if (tid == 0) a.status[model] = 2; return; }                 // uniform
  // ---- means (tpls.py:66-67, np.nanmean on the resampled rows)
  for (int o = tid; o < R * R; o += NT) coef[o] = 0.0;
  double missing = 0.0;
  for (int c = tid; c < P; c += NT) {
    double s = 0.0, cp = 0.0;
    for (int r = 0; r < I; ++r) {
      const double w = cw[r];
      if (w == 0.0) continue;
      const double x = a.X[(int64_t)r * P + c];
      if (!isnan(x)) { s = fma(w, x, s); cp += w; }
    }
    cs[c] = cp;
    mu[c] = cp > 0.0 ? s / cp : __builtin_nan("");
    if (cp < nf) missing = 1.0;
  }
  for (int m = tid; m < M; m += NT) {
    double s = 0.0;
    for (int r = 0; r < I; ++r) {
      const double w = cw[r];
      if (w != 0.0) s = fma(w, a.Y[(int64_t)(yrow_m ? yrow_m[r] : r) * M + m], s);
    }
    my[m] = s / nf;
  }
  const bool miss = loo_sum<NT>(missing, red) > 0.0;                          // X_hasMiss of the training data (tpls.py:61)
  // ---- working copies: centred, zero at held-out rows and missing entries
  for (int64_t idx = tid; idx < (int64_t)I * P; idx += NT) {
    const int r = (int)(idx / P), c = (int)(idx % P);
    const double x = a.X[idx];
    Xf[idx] = (cw[r] == 0.0 || isnan(x)) ? 0.0 : x - mu[c];
  }
  for (int64_t idx = tid; idx < (int64_t)I * M; idx += NT) {
    const int r = (int)(idx / M), m = (int)(idx % M);
    Yf[idx] = (cw[r] == 0.0) ? 0.0 : a.Y[(int64_t)(yrow_m ? yrow_m[r] : r) * M + m] - my[m];
  }
  for (int64_t idx = tid; idx < (int64_t)I * R; idx += NT) T[idx] = 0.0;
  // observed entries of every row; a training row without any makes the reference's score 0 / 0
  double empty = 0.0;
  for (int r = wv; r < I; r += NT / 64) {
    double cnt = 0.0;
    for (int c = lane; c < P; c += 64) cnt += isnan(a.X[(int64_t)r * P + c]) ? 0.0 : 1.0;
    cnt = wave_sum(cnt);
    if (lane == 0) ro[r] = cnt;
    if (cw[r] != 0.0 && cnt == 0.0) empty = 1.0;
  }
  if (loo_sum<NT>(empty, red) > 0.0) { if (tid == 0) a.status[model] = 1; return; }   // uniform (its barriers publish Xf, Yf, ro)
  const double Pd = (double)P;

  for (int comp = 0; comp < R; ++comp) {
    for (int r = tid; r < I; r += NT) u[r] = Yf[(int64_t)r * M];                   // tpls.py:78
    __syncthreads();
    int it = 0;
    for (; it < a.max_iter; ++it) {                                                  // tpls.py:79
      // Z = X x_0 u over the weighted rows (tpls.py:83), or miss_tensordot: the column's sum / c_p * n, 0 when c_p = 0
      if (nrg == 1) {
        for (int c = tid; c < P; c += NT) {
          double s = 0.0;
          for (int r = 0; r < I; ++r) s = fma(Xf[(int64_t)r * P + c], cw[r] * u[r], s);
          Z[c] = miss ? (cs[c] > 0.0 ? s / cs[c] * nf : 0.0) : s;
        }
      } else {
        const int rg = tid / P, c = tid % P;
        if (rg < nrg) {
          double s = 0.0;
          for (int r = rg; r < I; r += nrg) s = fma(Xf[(int64_t)r * P + c], cw[r] * u[r], s);
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
      // t = X x_1 wA x_2 wB (tpls.py:97-99), or miss_mmodedot: the row's sum / o_r * P; held-out rows 0
      for (int r = wv; r < I; r += NT / 64) {
        double s = 0.0;
        for (int c = lane; c < P; c += 64) s = fma(Xf[(int64_t)r * P + c], wA[c / B] * wB[c % B], s);
        s = wave_sum(s);
        if (lane == 0) t[r] = (cw[r] == 0.0) ? 0.0 : (miss ? s / ro[r] * Pd : s);
      }
      __syncthreads();
      // q = Y^T C t / |.| (tpls.py:100-101)
      if (tid < M) {
        double s = 0.0;
        for (int r = 0; r < I; ++r) s = fma(Yf[(int64_t)r * M + tid], cw[r] * t[r], s);
        q[tid] = s;
      }
      __syncthreads();
      double qs = (tid < M) ? q[tid] * q[tid] : 0.0;
      const double qnrm = sqrt(loo_sum<NT>(qs, red));
      if (tid < M) qn[tid] = q[tid] / qnrm;
      __syncthreads();
      // u = Y q and the weighted |u_old - u| (tpls.py:102-103)
      double du2 = 0.0;
      for (int r = tid; r < I; r += NT) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s = fma(Yf[(int64_t)r * M + m], qn[m], s);
        const double d0 = u[r] - s;
        du2 = fma(cw[r] * d0, d0, du2);
        u[r] = s;
      }
      const double du = sqrt(loo_sum<NT>(du2, red));
      if (it > 0 && du < a.tol) { ++it; break; }                                     // first pass: oldU = inf (tpls.py:77)
    }
    if (a.n_iter && tid == 0) a.n_iter[(int64_t)model * R + comp] = it;
    // store the component; deflate the observed training entries of X (tpls.py:109: a NaN stays NaN there)
    for (int r = tid; r < I; r += NT) T[(int64_t)r * R + comp] = t[r];
    for (int j = tid; j < A; j += NT) Wa[comp * A + j] = wA[j];
    for (int j = tid; j < B; j += NT) Wb[comp * B + j] = wB[j];
    for (int m = tid; m < M; m += NT) Qs[comp * M + m] = qn[m];
    for (int64_t idx = tid; idx < (int64_t)I * P; idx += NT) {
      const int r = (int)(idx / P), c = (int)(idx % P);
      if (cw[r] == 0.0 || (miss && isnan(a.X[idx]))) continue;
      Xf[idx] = Xf[idx] - t[r] * (wA[c / B] * wB[c % B]);
    }
    __syncthreads();
    // inner regression b = lstsq(T[:, :k], u) on the weighted rows (tpls.py:110-112): (T^T C T) b = T^T C u, fold_regress.hpp; then
    // Y -= T b q^T (tpls.py:113), yhat = T b in t; held-out rows of T are 0, so their Yf stays 0
    fold_inner_regression<NT, true>(T, u, cw, I, R, comp, Gn, gn, bb, dd, coef, t);
    for (int64_t idx = tid; idx < (int64_t)I * M; idx += NT) {
      const int r = (int)(idx / M), m = (int)(idx % M);
      Yf[idx] = Yf[idx] - t[r] * qn[m];
    }
    __syncthreads();
  }

  // ---- predict the held-out rows (tpls.py:122-143): centre with the model's means, THEN mask (NaN after centring, which takes
  // in the columns without a training observation); the batch is masked when any of its entries is
  double hmiss = 0.0;
  for (int r = wv; r < I; r += NT / 64) {
    if (cw[r] != 0.0) continue;                                                       // uniform in the wavefront
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
  // scores and deflation per component: a wavefront owns a held-out row for all R components (no barrier between them)
  for (int r = wv; r < I; r += NT / 64) {
    if (cw[r] != 0.0) continue;
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
  // Ypred[m, c - 1] = scores[:, :c] coef_[:c, :c] Q[:, :c]^T + nu for c = 1..R (coef_ upper triangular: one pass over h Q^T)
  double* yp = a.Ypred + (int64_t)model * R * I * M;
  for (int64_t o = tid; o < (int64_t)I * M; o += NT) {
    const int r = (int)(o / M), m = (int)(o % M);
    if (cw[r] != 0.0) continue;
    double acc = 0.0;
    for (int b2 = 0; b2 < R; ++b2) {
      double h = 0.0;
      for (int a2 = 0; a2 <= b2; ++a2) h = fma(T[(int64_t)r * R + a2], coef[a2 * R + b2], h);
      acc = fma(h, Qs[b2 * M + m], acc);
      yp[((int64_t)b2 * I + r) * M + m] = acc + my[m];
    }
  }
  // the model's factors (the bootstrap aligns them on the host)
  if (a.Wa) for (int o = tid; o < R * A; o += NT) a.Wa[(int64_t)model * R * A + o] = Wa[o];
  if (a.Wb) for (int o = tid; o < R * B; o += NT) a.Wb[(int64_t)model * R * B + o] = Wb[o];
  if (a.coef) for (int o = tid; o < R * R; o += NT) a.coef[(int64_t)model * R * R + o] = coef[o];
  if (a.Q) for (int o = tid; o < R * M; o += NT) a.Q[(int64_t)model * R * M + o] = Qs[o];
  if (a.info && tid == 0) {
    a.info[2 * (int64_t)model] = miss ? 1 : 0;
    a.info[2 * (int64_t)model + 1] = hm ? 1 : 0;
  }
}

static size_t cv_masked_models_lds_bytes(int I, int A, int B, int M, int R) {
  const size_t n = (size_t)(A < B ? A : B), k = (size_t)(A < B ? B : A), P = (size_t)A * B;
  const size_t dbl = 2 * (size_t)I + P + A + B + 2 * (size_t)M + 2 * n * n + n + k + M + (size_t)R * R + (size_t)R * (A + B) +
                     (size_t)R * M + (size_t)R * R + 3 * (size_t)R + (size_t)kCvmThreads + 2 * (size_t)I;
  return dbl * sizeof(double);
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {

size_t cmtfpls_cv_masked_model_workspace_bytes(int I, int A, int B, int M, int R) {
  if (I <= 1 || A <= 0 || B <= 0 || M <= 0 || R <= 0) return 0;
  return ((size_t)I * A * B + (size_t)I * M + (size_t)I * R + 2 * (size_t)A * B) * sizeof(double);
}

int cmtfpls_cv_masked_models_f64(const double* X, const double* Y, const int* counts, const int* yrow, int nm, int I, int A, int B,
                                 int M, int R, double tol, int max_iter, int model0, int nmodels, double* Ypred, double* Wa,
                                 double* Wb, double* coef, double* Q, int* n_iter, int* status, int* info, void* ws, size_t ws_bytes,
                                 void* stream) {
  if (!X || !Y || !counts || !Ypred || !status || I <= 1 || A <= 0 || B <= 0 || M <= 0 || R <= 0 || max_iter <= 0 || nm <= 0 ||
      model0 < 0 || nmodels <= 0) {
    set_error("cv_masked_models: bad argument");
    return CMTFPLS_EINVAL;
  }
  const int n = A < B ? A : B;
  const size_t lds = cv_masked_models_lds_bytes(I, A, B, M, R);
  if (n > kCvmMaxN || M > kCvmMaxM || R > kCvmMaxR || lds > 150 * 1024) {
    set_error("cv_masked_models: shape outside the one-workgroup-per-model form; refit per model on the regular engine");
    return CMTFPLS_EUNSUPPORTED;
  }
  if (model0 + nmodels > nm) { set_error("cv_masked_models: models out of range"); return CMTFPLS_EINVAL; }
  const size_t per = cmtfpls_cv_masked_model_workspace_bytes(I, A, B, M, R);
  if (!ws || ws_bytes < per * (size_t)nmodels) { set_error("cv_masked_models: workspace too small"); return CMTFPLS_EWORKSPACE; }
  CvMaskedModelsArgs a;
  a.X = X; a.Y = Y; a.counts = counts; a.yrow = yrow;
  a.ws = static_cast<double*>(ws); a.Ypred = Ypred; a.Wa = Wa; a.Wb = Wb; a.coef = coef; a.Q = Q;
  a.n_iter = n_iter; a.status = status; a.info = info;
  a.ws_per_model = (int64_t)(per / sizeof(double));
  a.I = I; a.A = A; a.B = B; a.M = M; a.R = R; a.nm = nm; a.max_iter = max_iter; a.model0 = model0; a.nmodels = nmodels;
  a.tol = tol;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cv_masked_models_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
  hipLaunchKernelGGL(cv_masked_models_kernel, dim3(nmodels), dim3(kCvmThreads), lds, (hipStream_t)stream, a);
  return check_launch("cv_masked_models");
}

}  // extern "C"
