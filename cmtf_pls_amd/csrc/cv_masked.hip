// Refits of a small tPLS whose X has missing values, ALL MODELS OF A CHUNK IN ONE LAUNCH, one workgroup per model, in two forms
// of one kernel over the steps of masked_fold.hpp.
//   The fold form (cmtfpls_cv_masked_f64): validate.get_q2y (leave-one-out, cmtf_pls/validate.py:7-37) and
// validate.kfold_predictions.  Model f holds out the rows r with fold_of[r] == f; its means are down-dated from the shared column
// sums and counts, its sums over rows are unweighted, its predictions land in one (R, I, M) array.
//   The count-weighted form (cmtfpls_cv_masked_models_f64): the permutation test (validate.permutation_test_q2y), repeated K-fold
// (validate.get_q2y_repeated_kfold) and the bootstrap (validate.bootstrap_factors).  Model m is counts[m, r] >= 0 (how many times
// row r of X is in its training data; 0 = held out) and yrow[m, r] (the row of Y paired with X row r; nullable = identity): its
// training data is literally X[r] repeated c_r times with Y[yrow[r]], every sum over rows weighted by c_r; predictions (and,
// optionally, factors) per model.  With 0/1 counts and identity yrow it computes a fold of the fold form.
// Either way the model is the reference's tPLS.fit (tpls.py:73-113) with its missing-value arithmetic (X_hasMiss, tpls.py:61-63;
// miss_tensordot / miss_mmodedot, missingvals.py:7-38) on the training rows, then the held-out rows predicted as one batch
// (tpls.py:122-143) with every component count.  As loo_tpls_kernel (loo.hip): the model's centred working copy Xf | Yf | T in the
// workspace, deflated in place, with the model's column counts and means; the vectors in LDS; the NIPALS loop inside the kernel.
//
// The masked arithmetic is a per-column and a per-row rescale of the zero-filled working copy (held-out rows, missing entries and
// columns without a training observation are 0 in Xf, so every masked sum is an ordinary sum).  With n = sum_r c_r (c_r = 1 on
// the training rows of a fold):
//   c_p   = sum_r c_r [x_rp observed];  mu_p = sum_r c_r x_rp / c_p (NaN if c_p = 0);  nu = sum_r c_r Y[yrow[r]] / n
//   miss  = some c_p < n: the reference's X_hasMiss on the training data
//   Z_p   = (sum_r c_r Xf[r,p] u_r) / c_p * n    (miss_tensordot; 0 when c_p = 0)
//   t_r   = (sum_p Xf[r,p] w_p) / o_r * P         (miss_mmodedot; o_r = observed entries of training row r; held-out rows 0)
//   q     = sum_r c_r Yf[r] t_r, normalised; convergence on sqrt(sum_r c_r (u_r - u_old,r)^2)
//   lstsq = (T^T C T) b = T^T C u, Y deflated on the training rows; X deflated on the observed training entries only.
// A model without missing training entries takes the unmasked arithmetic, as the reference does.  The held-out batch is centred
// with the model's means and then masked (an entry is missing when it is NaN after centring: tpls.py:128-131); if any held-out
// entry of the model is missing the whole batch takes the masked score and deflation; a held-out row with nothing observed
// predicts NaN (0 / 0, as the reference).  Status 1: a training row with nothing observed (the reference is NaN everywhere);
// 2: n < 2; 3 (count-weighted form): a negative count or a yrow outside 0..I-1.  A model with a status writes nothing else.
// Limits: those of the LDS form (min(A, B) <= 64, M <= 64, R <= 16, the vectors plus the per-row counts and weights within 150 KB
// of LDS); the fold form 1 <= K <= I.
//
// TENSOR (cmtfpls_cv_masked_tensor_f64, cmtfpls_cv_masked_tensor_models_f64): X of order 4, I x A x B1 x B2.  The same kernel on the
// I x A x B view with B = B1 B2: Z (A x B1 x B2, in LDS, already rescaled by mf_contract when the model is masked) goes through the
// rank-1 CP of fold_loop.hpp (lx_cp3, tpls.py:86-88 on a tensor Z) in place of mf_loading, and its wA and wB = wK (x) wL feed the
// unchanged steps.  lx_cp3 is templated on the thread count; this form runs it, and the mf_* steps, at 512 threads, where a wavefront
// has 256 registers and the inlined CP spills nothing (at 1024 threads and 128 registers it does); its Zt, U, yl and vr (P doubles each)
// follow the model's means in the workspace; G0 / G1 and xs are sized for the largest short side n of the three unfoldings of Z,
// min(A, B1 B2), min(B1, A B2), min(B2, A B1).  Limits: that n <= 64, M <= 64, R <= 16, the LDS within 150 KB, 1 <= K <= I.
#include <string>

#include "common.hpp"
#include "fold_loop.hpp"
#include "fold_regress.hpp"

namespace cmtfpls {

#include "loo_rank1.hpp"
#include "masked_fold.hpp"

constexpr int kCvMaxN = 64, kCvMaxR = 16, kCvMaxM = 64, kCvThreads = 256, kCvTensorThreads = 512;

struct CvMaskedArgs {
  const double* X;        // (I, P) original, uncentred, NaN = missing
  const double* Y;        // (I, M) complete
  const int* rows;        // fold form: fold_of (I), the fold id of every row; else counts (nm, I), the multiplicity of every row
  const int* yrow;        // (nm, I) row of Y paired with each X row (nullable: identity)
  const double* colsum_x; // fold form: (P) sums of the observed entries of all rows
  const double* colcnt_x; // fold form: (P) observed entries per column
  const double* colsum_y; // fold form: (M)
  double* ws;             // per resident model: Xf (I*P) | Yf (I*M) | T (I*R) | cs (P) | mu (P)
  double* Ypred;          // (R, I, M) in the fold form, else (nm, R, I, M): [(m,) r - 1, i] = held-out row i by its model's r-component fit
  double* Wa;             // (nm, R, A) (nullable)
  double* Wb;             // (nm, R, B) (nullable)
  double* coef;           // (nm, R, R) (nullable): coef_[row, component]
  double* Q;              // (nm, R, M) (nullable)
  int* n_iter;            // (nm, R) (nullable)
  int* status;            // (nm)
  int* info;              // (nm, 2) (nullable): [m, 0] the training rows took the masked arithmetic, [m, 1] the held-out batch did
  int64_t ws_per_model;   // doubles
  int I, A, B, M, R, nm, max_iter, model0, nmodels;   // nm = K in the fold form
  double tol;
  int B1, B2;             // TENSOR: the trailing dims of X, B = B1 B2
  double* Wk;             // TENSOR: (nm, R, B1) (nullable)
  double* Wl;             // TENSOR: (nm, R, B2) (nullable)
};

// TENSOR: the largest short side of the three unfoldings of an A x B1 x B2 tensor
__host__ __device__ inline int cv_tensor_short_side(int A, int B1, int B2) {
  const int64_t P = (int64_t)A * B1 * B2;
  int64_t n = 0;
  for (const int d : {A, B1, B2}) {
    const int64_t s = d < P / d ? d : P / d;
    if (s > n) n = s;
  }
  return n > INT32_MAX ? INT32_MAX : (int)n;
}

// The reduction buffers of loo_sum and loo_rank1: one pair for both instantiations.  Declared inside the kernel every instantiation
// gets its own pair, and the compiler's LDS layout for a module with two such kernels costs each of them 2 VGPRs.
__shared__ double red[16];
__shared__ int ired[4];

template <bool MODELS, bool TENSOR = false>
__global__ __launch_bounds__(TENSOR ? kCvTensorThreads : kCvThreads) void cv_masked_kernel(CvMaskedArgs a) {
  constexpr int NT = TENSOR ? kCvTensorThreads : kCvThreads;
  extern __shared__ double sm[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int I = a.I, A = a.A, B = a.B, M = a.M, R = a.R, P = A * B;
  const int n = TENSOR ? cv_tensor_short_side(A, a.B1, a.B2) : (A < B ? A : B);
  const int k = TENSOR ? 0 : (A < B ? B : A);       // (ys: the CP keeps its long vector in the workspace)
  const int model = a.model0 + blockIdx.x;
  if (blockIdx.x >= a.nmodels || model >= a.nm) return;
  const int* rows_m = MODELS ? a.rows + (int64_t)model * I : a.rows;
  const int* yrow_m = (MODELS && a.yrow) ? a.yrow + (int64_t)model * I : nullptr;
  double* Xf = a.ws + (int64_t)blockIdx.x * a.ws_per_model;
  double* Yf = Xf + (int64_t)I * P;
  double* T = Yf + (int64_t)I * M;
  double* cs = T + (int64_t)I * R;  // P: (weighted) training observations of each column (c_p)
  double* mu = cs + P;              // P: (weighted) training means of X (NaN where c_p = 0)
  // LDS carve-up: loo_tpls_kernel's, then the per-row counts and weights (the per-column ones are read once per column and sweep:
  // they stay in the workspace, which keeps min(A, B) = 64 within the LDS)
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
  double* my = ys + k;            // (weighted) mean of the paired Y rows over the training rows (nu)
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
  double* cw = ro + I;            // I: 0 = held out, otherwise the row's weight c_r (1 in the fold form)
  LxTensor tn;                    // TENSOR: the CP's vectors after cw, its unfoldings after mu; part is shared with mf_contract
  double* bestv = nullptr;
  int* besti = nullptr;
  if constexpr (TENSOR) {
    const int dmax = A > a.B1 ? (A > a.B2 ? A : a.B2) : (a.B1 > a.B2 ? a.B1 : a.B2);
    tn.B1 = a.B1; tn.B2 = a.B2;
    tn.wK = cw + I;
    tn.wL = tn.wK + a.B1;
    tn.v = tn.wL + a.B2;
    tn.tmp = tn.v + B;
    tn.part = part;
    bestv = tn.tmp + dmax;        // NT / 64 doubles, then NT / 64 ints
    besti = reinterpret_cast<int*>(bestv + NT / 64);
    tn.U = mu + 2 * (int64_t)P;
    tn.yl = tn.U + P;
    tn.vr = tn.yl + P;
  }

  if (tid == 0) a.status[model] = 0;
  double nf, missing = 0.0;
  if constexpr (MODELS) {
    // ---- counts and training size; a bad count or Y row stops the model before Y is read
    const int st = mf_weights<NT>(rows_m, yrow_m, I, cw, &nf, red);
    if (st != 0) { if (tid == 0) a.status[model] = st; return; }                // uniform
    // ---- means (tpls.py:66-67, np.nanmean on the resampled rows)
    for (int o = tid; o < R * R; o += NT) coef[o] = 0.0;
    missing = mf_weighted_means<NT>(a.X, cw, I, P, nf, cs, mu);
    mf_weighted_mean_y<NT>(a.Y, yrow_m, cw, I, M, nf, my);
  } else {
    // ---- fold sizes
    double nh = 0.0;
    for (int r = tid; r < I; r += NT) {
      const bool h = rows_m[r] == model;
      cw[r] = h ? 0.0 : 1.0;
      nh += h ? 1.0 : 0.0;
    }
    nh = loo_sum<NT>(nh, red);                                                  // (its barriers publish cw)
    nf = (double)I - nh;
    if (nf < 2.0) { if (tid == 0) a.status[model] = 2; return; }                // uniform
    // ---- means (tpls.py:66-67, np.nanmean): down-date the shared sums and counts by the held-out rows
    for (int o = tid; o < R * R; o += NT) coef[o] = 0.0;
    for (int c = tid; c < P; c += NT) {
      double s = 0.0, cnt = 0.0;
      for (int r = 0; r < I; ++r) {
        if (cw[r] != 0.0) continue;
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
        if (cw[r] == 0.0) s += a.Y[(int64_t)r * M + m];
      my[m] = (a.colsum_y[m] - s) / nf;
    }
  }
  const bool miss = loo_sum<NT>(missing, red) > 0.0;                            // X_hasMiss of the training data (tpls.py:61)
  // ---- working copies; a training row without an observed entry makes the reference's score 0 / 0
  mf_working_copy_y<NT>(a.Y, yrow_m, cw, my, I, M, R, Yf, T);
  const double empty = mf_working_copy<NT>(a.X, cw, mu, I, P, Xf, ro);
  if (loo_sum<NT>(empty, red) > 0.0) { if (tid == 0) a.status[model] = 1; return; }   // uniform (its barriers publish Xf, Yf, ro)
  const double Pd = (double)P;

  for (int comp = 0; comp < R; ++comp) {
    for (int r = tid; r < I; r += NT) u[r] = Yf[(int64_t)r * M];                   // tpls.py:78
    __syncthreads();
    int it = 0;
    for (; it < a.max_iter; ++it) {                                                  // tpls.py:79
      mf_contract<NT, MODELS>(Xf, u, cw, cs, I, P, miss, nf, part, Z);
      if constexpr (TENSOR) lx_cp3<NT>(Z, mu + P, A, a.tol, tn, wA, wB, G0, G1, xs, red, bestv, besti);   // wB = wK (x) wL
      else mf_loading<NT>(Z, A, B, wA, wB, G0, G1, xs, ys, red, ired);
      // t = X x_1 wA x_2 wB (tpls.py:97-99), or miss_mmodedot (missingvals.py:37): the row's sum / o_r * P; held-out rows 0
      for (int r = wv; r < I; r += NT / 64) {
        const double s = mf_row_dot(Xf + (int64_t)r * P, wA, wB, P, B);
        if (lane == 0) t[r] = (cw[r] == 0.0) ? 0.0 : (miss ? s / ro[r] * Pd : s);
      }
      __syncthreads();
      const double du = mf_y_step<NT, MODELS>(Yf, t, cw, I, M, q, qn, u, red);
      if (it > 0 && du < a.tol) { ++it; break; }                                     // first pass: oldU = inf (tpls.py:77)
    }
    if (a.n_iter && tid == 0) a.n_iter[(int64_t)model * R + comp] = it;
    // store the component; deflate X, then Y after the inner regression
    for (int r = tid; r < I; r += NT) T[(int64_t)r * R + comp] = t[r];
    for (int m = tid; m < M; m += NT) Qs[comp * M + m] = qn[m];
    mf_deflate_x<NT>(a.X, cw, t, wA, wB, I, A, B, comp, miss, Wa, Wb, Xf);
    if constexpr (MODELS && TENSOR) {                                                // the modes of wB, straight to the outputs
      mf_write_factor<NT>(a.Wk, ((int64_t)model * R + comp) * a.B1, tn.wK, a.B1);
      mf_write_factor<NT>(a.Wl, ((int64_t)model * R + comp) * a.B2, tn.wL, a.B2);
    }
    __syncthreads();
    mf_regress_deflate_y<NT, MODELS>(T, u, cw, qn, I, M, R, comp, Gn, gn, bb, dd, coef, t, Yf);
  }

  // ---- predict the held-out rows (tpls.py:122-143)
  const bool hm = mf_heldout_batch<NT>(a.X, mu, cw, I, P, Xf, ro, red);
  // scores and deflation per component: a wavefront owns a held-out row for all R components (no barrier between them); the
  // scores go to the row's (zero) slots of T
  for (int r = wv; r < I; r += NT / 64) {
    if (cw[r] != 0.0) continue;
    const double o_r = ro[r];
    for (int comp = 0; comp < R; ++comp) {
      const double s = mf_row_dot(Xf + (int64_t)r * P, Wa + comp * A, Wb + comp * B, P, B);
      const double sv = hm ? s / o_r * Pd : s;                                       // o_r = 0: 0 / 0 = NaN, as the reference
      if (lane == 0) T[(int64_t)r * R + comp] = sv;
      mf_heldout_deflate(a.X + (int64_t)r * P, mu, Wa + comp * A, Wb + comp * B, P, B, sv, hm, Xf + (int64_t)r * P);
    }
  }
  __syncthreads();
  mf_predict<NT>(T, coef, Qs, my, cw, I, M, R, MODELS ? a.Ypred + (int64_t)model * R * I * M : a.Ypred);
  if constexpr (MODELS) {                                                            // the model's factors (the bootstrap aligns them on the host)
    mf_write_factor<NT>(a.Wa, (int64_t)model * R * A, Wa, R * A);
    if constexpr (!TENSOR) mf_write_factor<NT>(a.Wb, (int64_t)model * R * B, Wb, R * B);
    mf_write_factor<NT>(a.coef, (int64_t)model * R * R, coef, R * R);
    mf_write_factor<NT>(a.Q, (int64_t)model * R * M, Qs, R * M);
  }
  if (a.info && tid == 0) {
    a.info[2 * (int64_t)model] = miss ? 1 : 0;
    a.info[2 * (int64_t)model + 1] = hm ? 1 : 0;
  }
}

static size_t cv_masked_lds_bytes(int I, int A, int B, int M, int R) {
  const size_t n = (size_t)(A < B ? A : B), k = (size_t)(A < B ? B : A), P = (size_t)A * B;
  const size_t dbl = 2 * (size_t)I + P + A + B + 2 * (size_t)M + 2 * n * n + n + k + M + (size_t)R * R + (size_t)R * (A + B) +
                     (size_t)R * M + (size_t)R * R + 3 * (size_t)R + (size_t)kCvThreads + 2 * (size_t)I;
  return dbl * sizeof(double);
}

static size_t cv_masked_workspace_bytes(int I, int A, int B, int M, int R) {
  if (I <= 1 || A <= 0 || B <= 0 || M <= 0 || R <= 0) return 0;
  return ((size_t)I * A * B + (size_t)I * M + (size_t)I * R + 2 * (size_t)A * B) * sizeof(double);
}

// TENSOR: the carve-up above with B = B1 B2, n the largest short side, no ys, kCvTensorThreads partials, then wK, wL, v, the CP's unscaled
// contraction (max(A, B1, B2)) and its argmax scratch (a double and an int per wavefront)
static size_t cv_masked_tensor_lds_bytes(int I, int A, int B1, int B2, int M, int R) {
  const size_t B = (size_t)B1 * B2, P = (size_t)A * B, n = (size_t)cv_tensor_short_side(A, B1, B2);
  const size_t dmax = (size_t)(A > B1 ? (A > B2 ? A : B2) : (B1 > B2 ? B1 : B2));
  const size_t dbl = 2 * (size_t)I + P + A + B + 2 * (size_t)M + 2 * n * n + n + M + (size_t)R * R + (size_t)R * (A + B) +
                     (size_t)R * M + (size_t)R * R + 3 * (size_t)R + (size_t)kCvTensorThreads + 2 * (size_t)I + B1 + B2 + B + dmax +
                     kCvTensorThreads / 64 + kCvTensorThreads / 128;
  return dbl * sizeof(double);
}

// TENSOR: the order-3 workspace, then Zt | U | yl | vr of the CP (P doubles each)
static size_t cv_masked_tensor_workspace_bytes(int I, int A, int B1, int B2, int M, int R) {
  if (I <= 1 || A <= 0 || B1 <= 0 || B2 <= 0 || M <= 0 || R <= 0) return 0;
  const size_t P = (size_t)A * B1 * B2;
  return ((size_t)I * P + (size_t)I * M + (size_t)I * R + 6 * P) * sizeof(double);
}

// Whether the TENSOR form takes the shape (every limit in 64-bit arithmetic, before a pointer is touched)
static bool cv_masked_tensor_fits(int I, int A, int B1, int B2, int M, int R) {
  if ((int64_t)A * B1 * B2 > INT32_MAX / 2) return false;
  return cv_tensor_short_side(A, B1, B2) <= kCvMaxN && M <= kCvMaxM && R <= kCvMaxR &&
         cv_masked_tensor_lds_bytes(I, A, B1, B2, M, R) <= 150 * 1024;
}

template <bool MODELS, bool TENSOR = false>
static void cv_masked_launch(const CvMaskedArgs& a, size_t lds, void* stream) {
  const auto kernel = cv_masked_kernel<MODELS, TENSOR>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3(a.nmodels), dim3(TENSOR ? kCvTensorThreads : kCvThreads), lds, (hipStream_t)stream, a);
}

// The checks and the launch of the four entries.  `a` is the entry's call as it stands: its pointers (the fold entries' fold_of, or
// the model entries' counts, in rows), nm = K or the number of models, model0 / nmodels the first item and the count, and for
// TENSOR B1, B2 with B left 0; ws_per_model and the tensor form's B = B1 B2 are filled in here, after the checks.  The fold entries
// (MODELS = false) also need the column sums and counts and K <= I.
template <bool MODELS, bool TENSOR>
static int cv_masked_run(const std::string& who, CvMaskedArgs a, size_t ws_bytes, void* stream) {
  const std::string item = MODELS ? "model" : "fold";
  auto fail = [&](int code, const std::string& what) { set_error((who + ": " + what).c_str()); return code; };
  if (!a.X || !a.Y || !a.rows || (!MODELS && (!a.colsum_x || !a.colcnt_x || !a.colsum_y)) || !a.Ypred || !a.status || a.I <= 1 ||
      a.A <= 0 || (TENSOR ? a.B1 <= 0 || a.B2 <= 0 : a.B <= 0) || a.M <= 0 || a.R <= 0 || a.max_iter <= 0 || a.nm <= 0 ||
      a.model0 < 0 || a.nmodels <= 0)
    return fail(CMTFPLS_EINVAL, "bad argument");
  size_t lds, per;
  bool fits;
  if constexpr (TENSOR) {
    fits = cv_masked_tensor_fits(a.I, a.A, a.B1, a.B2, a.M, a.R);
    lds = cv_masked_tensor_lds_bytes(a.I, a.A, a.B1, a.B2, a.M, a.R);
    per = cv_masked_tensor_workspace_bytes(a.I, a.A, a.B1, a.B2, a.M, a.R);
  } else {
    lds = cv_masked_lds_bytes(a.I, a.A, a.B, a.M, a.R);
    fits = (a.A < a.B ? a.A : a.B) <= kCvMaxN && a.M <= kCvMaxM && a.R <= kCvMaxR && lds <= 150 * 1024;
    per = cv_masked_workspace_bytes(a.I, a.A, a.B, a.M, a.R);
  }
  if ((!MODELS && a.nm > a.I) || !fits)
    return fail(CMTFPLS_EUNSUPPORTED, "shape outside the one-workgroup-per-" + item + " form; refit per " + item + " on the regular engine");
  if (a.model0 + a.nmodels > a.nm) return fail(CMTFPLS_EINVAL, item + "s out of range");
  if (!a.ws || ws_bytes < per * (size_t)a.nmodels) return fail(CMTFPLS_EWORKSPACE, "workspace too small");
  a.ws_per_model = (int64_t)(per / sizeof(double));
  if constexpr (TENSOR) a.B = a.B1 * a.B2;
  cv_masked_launch<MODELS, TENSOR>(a, lds, stream);
  return check_launch(who.c_str());
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {

size_t cmtfpls_cv_masked_fold_workspace_bytes(int I, int A, int B, int M, int R) { return cv_masked_workspace_bytes(I, A, B, M, R); }

size_t cmtfpls_cv_masked_model_workspace_bytes(int I, int A, int B, int M, int R) { return cv_masked_workspace_bytes(I, A, B, M, R); }

// (the braces follow CvMaskedArgs' fields: X, Y, rows, yrow, the column sums and counts, ws, Ypred, Wa, Wb, coef, Q, n_iter, status,
// info, ws_per_model, I, A, B, M, R, nm, max_iter, model0, nmodels, tol, then B1, B2, Wk, Wl)
int cmtfpls_cv_masked_f64(const double* X, const double* Y, const int* fold_of, int K, const double* colsum_x, const double* colcnt_x,
                          const double* colsum_y, int I, int A, int B, int M, int R, double tol, int max_iter, int fold0, int nfolds,
                          double* Ypred, int* n_iter, int* status, int* info, void* ws, size_t ws_bytes, void* stream) {
  return cv_masked_run<false, false>("cv_masked", {X, Y, fold_of, nullptr, colsum_x, colcnt_x, colsum_y, static_cast<double*>(ws), Ypred,
                                                   nullptr, nullptr, nullptr, nullptr, n_iter, status, info, 0, I, A, B, M, R, K,
                                                   max_iter, fold0, nfolds, tol, 0, 0, nullptr, nullptr}, ws_bytes, stream);
}

int cmtfpls_cv_masked_models_f64(const double* X, const double* Y, const int* counts, const int* yrow, int nm, int I, int A, int B,
                                 int M, int R, double tol, int max_iter, int model0, int nmodels, double* Ypred, double* Wa,
                                 double* Wb, double* coef, double* Q, int* n_iter, int* status, int* info, void* ws, size_t ws_bytes,
                                 void* stream) {
  return cv_masked_run<true, false>("cv_masked_models", {X, Y, counts, yrow, nullptr, nullptr, nullptr, static_cast<double*>(ws), Ypred,
                                                         Wa, Wb, coef, Q, n_iter, status, info, 0, I, A, B, M, R, nm, max_iter, model0,
                                                         nmodels, tol, 0, 0, nullptr, nullptr}, ws_bytes, stream);
}

size_t cmtfpls_cv_masked_tensor_fold_workspace_bytes(int I, int A, int B1, int B2, int M, int R) {
  return cv_masked_tensor_workspace_bytes(I, A, B1, B2, M, R);
}

size_t cmtfpls_cv_masked_tensor_model_workspace_bytes(int I, int A, int B1, int B2, int M, int R) {
  return cv_masked_tensor_workspace_bytes(I, A, B1, B2, M, R);
}

size_t cmtfpls_cv_masked_tensor_lds_bytes(int I, int A, int B1, int B2, int M, int R) {
  if (I <= 1 || A <= 0 || B1 <= 0 || B2 <= 0 || M <= 0 || R <= 0) return 0;
  return cv_masked_tensor_lds_bytes(I, A, B1, B2, M, R);
}

int cmtfpls_cv_masked_tensor_f64(const double* X, const double* Y, const int* fold_of, int K, const double* colsum_x,
                                 const double* colcnt_x, const double* colsum_y, int I, int A, int B1, int B2, int M, int R, double tol,
                                 int max_iter, int fold0, int nfolds, double* Ypred, int* n_iter, int* status, int* info, void* ws,
                                 size_t ws_bytes, void* stream) {
  return cv_masked_run<false, true>("cv_masked_tensor", {X, Y, fold_of, nullptr, colsum_x, colcnt_x, colsum_y, static_cast<double*>(ws),
                                                         Ypred, nullptr, nullptr, nullptr, nullptr, n_iter, status, info, 0, I, A, 0, M, R,
                                                         K, max_iter, fold0, nfolds, tol, B1, B2, nullptr, nullptr}, ws_bytes, stream);
}

int cmtfpls_cv_masked_tensor_models_f64(const double* X, const double* Y, const int* counts, const int* yrow, int nm, int I, int A,
                                        int B1, int B2, int M, int R, double tol, int max_iter, int model0, int nmodels, double* Ypred,
                                        double* Wa, double* Wk, double* Wl, double* coef, double* Q, int* n_iter, int* status,
                                        int* info, void* ws, size_t ws_bytes, void* stream) {
  return cv_masked_run<true, true>("cv_masked_tensor_models", {X, Y, counts, yrow, nullptr, nullptr, nullptr, static_cast<double*>(ws),
                                                               Ypred, Wa, nullptr, coef, Q, n_iter, status, info, 0, I, A, 0, M, R, nm,
                                                               max_iter, model0, nmodels, tol, B1, B2, Wk, Wl}, ws_bytes, stream);
}

}  // extern "C"
