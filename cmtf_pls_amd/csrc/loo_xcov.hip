// Leave-one-out refits BEYOND the LDS-resident shapes of loo.hip (validate.get_q2y, cmtf_pls/validate.py:7-37; SURVEY 8(f).2
// "down-date S and the means instead of refitting"): all folds of a launch side by side, ONE 1024-thread WORKGROUP PER FOLD
// running that fold's whole tPLS.fit (tpls.py:73-113) and the prediction of its held-out sample (tpls.py:122-143), for
// trailing shapes up to min(A, B) = 256 (128 x 128, 256 x 256, ...), where loo.hip's per-fold vectors (Z, two n x n Gram
// buffers) no longer fit the LDS and the product used to refit once per fold on the regular engine.
//
// What a fold does NOT recompute or re-read:
//  * the means: (column sums of all samples - the held-out row) / (I - 1); the held-out row is zero in the fold's centred
//    working copies, which removes it from every sum (as loo.hip);
//  * the tensor inside the NIPALS loop: within a component X_f and Y_f are fixed and u = Y_f q, so
//        np.einsum(X, u) = S^T q   (tpls.py:83),   Y.T @ t = S (wA (x) wB)   (tpls.py:100),   |u_old - u|^2 = dq^T (Y_f^T Y_f) dq   (tpls.py:103)
//    with S = Y_f^T X_f (M x P) formed ONCE per component: an inner iteration reads the 2 M P doubles of S instead of the
//    2 I P of the fold's tensor (I / M times less: 32 x at 512 samples, 16 responses) -- the cross-covariance re-association of
//    the engine's algorithm="xcov", here inside one workgroup.  Per component the fold's tensor is read for S, for the final
//    score, and read + written by the deflation (tpls.py:109).
//  * the rank-1 extraction (tpls.py:86-88) is the product's: Gram matrix of the smaller side squared repeatedly with
//    power-of-two rescaling until numerically rank one, each n x n x n product on the f64 matrix cores
//    (v_mfma_f64_16x16x4_f64, operands straight from L2 in the MFMA layout, the 16 wavefronts of the workgroup dealing the
//    lower-triangular 16 x 16 tiles among themselves), one exact pass with Z, sign rule on the last mode.
// Arithmetic: float64 throughout, the reference's operation order outside the re-association above.
// The fold's steps (means and centred copies, the S build, G_y, the Y score, the deflation, the regression with the Y deflation, the
// held-out row and the prediction tail) are loo_xcov_fold.hpp's, shared with loo_xcov_coupled.hip; the inner loop is fold_loop.hpp's.
// Limits: X of order 2 or 3 without missing values, min(A, B) <= 256, M <= 128, R <= 64, the workgroup's small vectors in
// 150 KB of LDS; per resident fold a workspace of I P + M P + 3 P + 2 n^2 + I (M + R + 2) + R (A + B) doubles (cmtfpls_loo_xcov_fold_workspace_bytes).
//
// X of order 4 (I x A x B1 x B2, cmtfpls_loo_xcov_tensor_f64): the same kernel as its TENSOR instantiation.  The fold sees X as
// I x A x B with B = B1 B2; only the extraction differs: the rank-1 CP of the A x B1 x B2 cross-covariance (lx_cp3, fold_loop.hpp)
// in place of the leading singular pair, which leaves wB = wK (x) wL (C order).  The score, the deflation and the held-out
// prediction see X through wk = wA (x) wB and Wa[c / B] Wb[c % B] alone, so they are the order-3 code unchanged.  n is then the
// largest short side of the three unfoldings of A x B1 x B2 (each <= 256).  LDS: xs (n), then in place of ys (k) lx_cp3's wK (B1),
// wL (B2), v (B), tmp (max(A, B1, B2)) and part (1024); workspace: lx_cp3's U, yl, vr (P each) after wk
// (cmtfpls_loo_xcov_tensor_fold_workspace_bytes).
#include <string>

#include "loo_xcov_fold.hpp"

namespace cmtfpls {

struct LooXArgs {
  const double* X;        // (I, P) original, uncentred
  const double* Y;        // (I, M)
  const double* colsum_x; // (P)
  const double* colsum_y; // (M)
  double* ws;             // per resident fold, see carve-up in the kernel
  double* Ypred;          // (I, M): row i = prediction of the model fitted without sample i
  int* n_iter;            // (I, R), nullable
  int64_t ws_per_fold;    // doubles
  int I, A, B, M, R, max_iter, fold0, nfolds;
  double tol;
};

// the trailing dims of an order-4 X and the largest short side of the three unfoldings of A x B1 x B2 (B == B1 * B2)
struct LooXTensorArgs : LooXArgs {
  int B1, B2, nmax;
};

template <bool TENSOR>
struct LooXArgsOf { typedef LooXArgs type; };
template <>
struct LooXArgsOf<true> { typedef LooXTensorArgs type; };

// TENSOR = false: X of order 2 or 3, the code this kernel always was.  TENSOR = true: see the head of the file.
template <bool TENSOR>
__global__ __launch_bounds__(kLxNT) void loo_xcov_kernel(typename LooXArgsOf<TENSOR>::type a) {
  extern __shared__ double sm[];
  __shared__ double red[kLxWaves];
  __shared__ double bestv[kLxWaves];
  __shared__ int besti[kLxWaves];
  __shared__ double scv[kLxMaxR];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int I = a.I, A = a.A, B = a.B, M = a.M, R = a.R;
  const int64_t P = (int64_t)A * B;
  int n = A < B ? A : B, k = A < B ? B : A;
  if constexpr (TENSOR) {                                    // xs, G0, G1: the largest short side of the unfoldings; ys: lx_cp3's vectors
    n = a.nmax;
    k = a.B1 + a.B2 + B + max(A, max(a.B1, a.B2)) + kLxNT;
  }
  if ((int)blockIdx.x >= a.nfolds) return;
  const int fold = a.fold0 + blockIdx.x;
  if (fold >= I) return;
  // global carve-up of this fold's workspace
  double* Xf = a.ws + (int64_t)blockIdx.x * a.ws_per_fold;   // I x P   centred, held-out row zero, deflated in place
  double* Yf = Xf + (int64_t)I * P;                          // I x M
  double* T = Yf + (int64_t)I * M;                           // I x R
  double* S = T + (int64_t)I * R;                            // M x P   cross-covariance of the current component
  double* Z = S + (int64_t)M * P;                            // P
  double* Zt = Z + P;                                        // P       (transpose scratch of the rank-1 extraction)
  double* wk = Zt + P;                                       // P       kron(wA, wB) of the current loadings
  double* G0 = wk + (TENSOR ? 4 : 1) * P;                    // n x n   (TENSOR: after lx_cp3's U, yl, vr)
  double* G1 = G0 + (int64_t)n * n;
  double* u = G1 + (int64_t)n * n;                           // I
  double* t = u + I;                                         // I
  double* Wa = t + I;                                        // R x A   loadings of the components so far (read again by the prediction only)
  double* Wb = Wa + (int64_t)R * A;                          // R x B
  // LDS carve-up
  double* wA = sm;
  double* wB = wA + A;
  double* q = wB + B;
  double* qn = q + M;
  double* tq = qn + M;
  double* my = tq + M;
  double* Gy = my + M;            // M x M   Y_f^T Y_f of the current component
  double* xs = Gy + M * M;        // n
  double* ys = xs + n;            // k       (TENSOR: lx_cp3's wK, wL, v, tmp, part instead)
  double* coef = ys + k;          // R x R
  double* Qs = coef + R * R;      // R x M
  double* Gn = Qs + R * M;        // (a+1) x (a+1) normal equations
  double* gn = Gn + R * R;
  double* bb = gn + R;
  double* dd = bb + R;
  const double inv = 1.0 / (double)(I - 1);

  // ---- preprocess (tpls.py:61-71): the fold's means by down-dating the column sums; centred copies with the held-out row zero
  for (int o = tid; o < R * R; o += kLxNT) coef[o] = 0.0;
  lxf_mean_y<kLxNT>(a.Y, a.colsum_y, fold, M, inv, my);
  lxf_centre_block<kLxNT>(a.X, a.colsum_x, fold, I, P, inv, Z, Xf);
  lxf_centre_y<kLxNT>(a.Y, my, fold, I, M, Yf);

  for (int comp = 0; comp < R; ++comp) {
    // ---- S = Y_f^T X_f and G_y = Y_f^T Y_f of this component (X_f, Y_f as deflated so far), then the inner loop on them ----
    lxf_build_s<kLxNT>(Xf, Yf, I, P, M, S);
    lxf_gram_y<kLxNT>(Yf, I, M, Gy);
    int it;
    if constexpr (TENSOR) {
      const LxTensor lt = lx_tensor_scratch(ys, wk + P, a.B1, a.B2, B, max(A, max(a.B1, a.B2)), P, kLxNT);
      it = lx_inner_loop(S, Gy, P, M, A, B, a.tol, a.max_iter, q, qn, tq, Z, Zt, wk, wA, wB, G0, G1, xs, ys, red, bestv, besti, lt);
    } else {
      it = lx_inner_loop(S, Gy, P, M, A, B, a.tol, a.max_iter, q, qn, tq, Z, Zt, wk, wA, wB, G0, G1, xs, ys, red, bestv, besti);
    }
    if (a.n_iter && tid == 0) a.n_iter[(int64_t)fold * R + comp] = it;
    // ---- the component's score and Y score with the converged loadings (tpls.py:97-102); wk holds their Kronecker product ----
    lx_row_dots(Xf, wk, P, I, lane, wv, [t](int r, double s) { t[r] = s; });
    lxf_y_score<kLxNT>(Yf, q, I, M, u);
    __syncthreads();
    for (int r = tid; r < I; r += kLxNT) T[(int64_t)r * R + comp] = t[r];
    for (int j = tid; j < A; j += kLxNT) Wa[comp * A + j] = wA[j];
    for (int j = tid; j < B; j += kLxNT) Wb[comp * B + j] = wB[j];
    for (int m = tid; m < M; m += kLxNT) Qs[comp * M + m] = q[m];
    lxf_deflate<kLxNT>(Xf, t, wk, I, P);                                              // tpls.py:109
    __syncthreads();
    lxf_regress_deflate_y<kLxNT>(T, u, I, M, R, comp, Gn, gn, bb, dd, coef, t, q, Yf);
  }

  // ---- predict the held-out sample (tpls.py:122-143): centre with the fold's means, project and deflate ----
  lxf_heldout_row<kLxNT>(a.X, a.colsum_x, fold, P, inv, Z);
  __syncthreads();
  double* sc = scv;                                                                     // scores of the held-out row (R)
  for (int comp = 0; comp < R; ++comp) {
    double s = 0.0;
    for (int64_t c = tid; c < P; c += kLxNT) s = fma(Z[c], Wa[comp * A + c / B] * Wb[comp * B + c % B], s);
    const double sv = lx_sum(s, red);
    if (tid == 0) sc[comp] = sv;
    for (int64_t c = tid; c < P; c += kLxNT) Z[c] = fma(-sv, Wa[comp * A + c / B] * Wb[comp * B + c % B], Z[c]);
    __syncthreads();
  }
  lxf_predict<kLxNT>(sc, coef, Qs, my, R, M, a.Ypred + (int64_t)fold * M);
}

static size_t lx_lds_bytes(int A, int B, int M, int R) {
  const size_t n = (size_t)(A < B ? A : B), k = (size_t)(A < B ? B : A);
  const size_t dbl = (size_t)A + B + 4 * (size_t)M + (size_t)M * M + n + k + (size_t)R * R + (size_t)R * M + (size_t)R * R + 3 * (size_t)R;
  return dbl * sizeof(double);
}

// lx_lds_bytes with xs (nmax) and, in place of ys, lx_cp3's wK (B1), wL (B2), v (B1 B2), tmp (max dim) and part (kLxNT)
static size_t lx_tensor_lds_bytes(int A, int B1, int B2, int M, int R) {
  const size_t B = (size_t)B1 * B2, dmax = (size_t)(A > B1 ? (A > B2 ? A : B2) : (B1 > B2 ? B1 : B2));
  const size_t dbl = (size_t)A + B + 4 * (size_t)M + (size_t)M * M + lx_tensor_nmax(A, B1, B2) + B1 + B2 + B + dmax + kLxNT +
                     (size_t)R * R + (size_t)R * M + (size_t)R * R + 3 * (size_t)R;
  return dbl * sizeof(double);
}

// The checks, argument fill and launch of the two entries: cmtfpls_loo_xcov_f64 (TENSOR = false: the trailing dim B as B1, B2 = 1)
// and cmtfpls_loo_xcov_tensor_f64.  The shape checks are each entry's own, with its texts in its order.
template <bool TENSOR>
static int lx_run(const double* X, const double* Y, const double* colsum_x, const double* colsum_y, int I, int A, int B1, int B2, int M,
                  int R, double tol, int max_iter, int fold0, int nfolds, double* Ypred, int* n_iter, void* ws, size_t ws_bytes,
                  void* stream) {
  const std::string who = TENSOR ? "loo_xcov_tensor" : "loo_xcov";
  const std::string refit = "; refit per fold on the regular engine";
  auto fail = [&](int code, const std::string& what) { set_error((who + ": " + what).c_str()); return code; };
  if (!X || !Y || !colsum_x || !colsum_y || !Ypred || I <= 1 || A <= 0 || B1 <= 0 || B2 <= 0 || M <= 0 || R <= 0 || max_iter <= 0 ||
      fold0 < 0 || nfolds <= 0 || fold0 + nfolds > I)
    return fail(CMTFPLS_EINVAL, "bad argument");
  size_t lds, per;
  if constexpr (TENSOR) {
    if ((int64_t)A * B1 * B2 > (int64_t)1 << 24) return fail(CMTFPLS_EUNSUPPORTED, "A * B1 * B2 > 2^24" + refit);
    for (int m = 0; m < 3; ++m)
      if (lx_tensor_short(A, B1, B2, m) > kLxMaxN)
        return fail(CMTFPLS_EUNSUPPORTED, "an unfolding of A x B1 x B2 with its shorter side > 256" + refit);
    if (M > kLxMaxM || R > kLxMaxR)
      return fail(CMTFPLS_EUNSUPPORTED, "shape outside the workgroup-per-fold form (M <= 128, R <= 64)" + refit);
    lds = lx_tensor_lds_bytes(A, B1, B2, M, R);
    if (lds > 150 * 1024) return fail(CMTFPLS_EUNSUPPORTED, "the fold's vectors exceed 150 KB of LDS" + refit);
    per = cmtfpls_loo_xcov_tensor_fold_workspace_bytes(I, A, B1, B2, M, R);
  } else {
    lds = lx_lds_bytes(A, B1, M, R);
    if ((A < B1 ? A : B1) > kLxMaxN || M > kLxMaxM || R > kLxMaxR || lds > 150 * 1024 || (int64_t)A * B1 > (int64_t)1 << 24)
      return fail(CMTFPLS_EUNSUPPORTED, "shape outside the workgroup-per-fold form (min(A, B) <= 256, M <= 128, R <= 64, small vectors "
                                        "within 150 KB of LDS)" + refit);
    per = cmtfpls_loo_xcov_fold_workspace_bytes(I, A, B1, M, R);
  }
  if (!ws || ws_bytes < per * (size_t)nfolds) return fail(CMTFPLS_EWORKSPACE, "workspace too small");
  typename LooXArgsOf<TENSOR>::type a;
  a.X = X; a.Y = Y; a.colsum_x = colsum_x; a.colsum_y = colsum_y; a.ws = static_cast<double*>(ws); a.Ypred = Ypred; a.n_iter = n_iter;
  a.ws_per_fold = (int64_t)(per / sizeof(double));
  a.I = I; a.A = A; a.B = B1 * B2; a.M = M; a.R = R; a.max_iter = max_iter; a.fold0 = fold0; a.nfolds = nfolds; a.tol = tol;
  if constexpr (TENSOR) { a.B1 = B1; a.B2 = B2; a.nmax = lx_tensor_nmax(A, B1, B2); }
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(loo_xcov_kernel<TENSOR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(loo_xcov_kernel<TENSOR>, dim3(nfolds), dim3(kLxNT), lds, (hipStream_t)stream, a);
  return check_launch(who.c_str());
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {

size_t cmtfpls_loo_xcov_fold_workspace_bytes(int I, int A, int B, int M, int R) {
  if (I <= 1 || A <= 0 || B <= 0 || M <= 0 || R <= 0) return 0;
  const size_t P = (size_t)A * B, n = (size_t)(A < B ? A : B);
  return ((size_t)I * P + (size_t)I * M + (size_t)I * R + (size_t)M * P + 3 * P + 2 * n * n + 2 * (size_t)I + (size_t)R * ((size_t)A + B)) * sizeof(double);
}

size_t cmtfpls_loo_xcov_tensor_fold_workspace_bytes(int I, int A, int B1, int B2, int M, int R) {
  if (I <= 1 || A <= 0 || B1 <= 0 || B2 <= 0 || M <= 0 || R <= 0) return 0;
  const size_t B = (size_t)B1 * B2, P = (size_t)A * B, n = (size_t)lx_tensor_nmax(A, B1, B2);
  return ((size_t)I * P + (size_t)I * M + (size_t)I * R + (size_t)M * P + 6 * P + 2 * n * n + 2 * (size_t)I + (size_t)R * ((size_t)A + B)) * sizeof(double);
}

size_t cmtfpls_loo_xcov_tensor_lds_bytes(int A, int B1, int B2, int M, int R) {
  if (A <= 0 || B1 <= 0 || B2 <= 0 || M <= 0 || R <= 0) return 0;
  return lx_tensor_lds_bytes(A, B1, B2, M, R);
}

int cmtfpls_loo_xcov_f64(const double* X, const double* Y, const double* colsum_x, const double* colsum_y, int I, int A, int B, int M,
                         int R, double tol, int max_iter, int fold0, int nfolds, double* Ypred, int* n_iter, void* ws,
                         size_t ws_bytes, void* stream) {
  return lx_run<false>(X, Y, colsum_x, colsum_y, I, A, B, 1, M, R, tol, max_iter, fold0, nfolds, Ypred, n_iter, ws, ws_bytes, stream);
}

int cmtfpls_loo_xcov_tensor_f64(const double* X, const double* Y, const double* colsum_x, const double* colsum_y, int I, int A, int B1,
                                int B2, int M, int R, double tol, int max_iter, int fold0, int nfolds, double* Ypred, int* n_iter,
                                void* ws, size_t ws_bytes, void* stream) {
  return lx_run<true>(X, Y, colsum_x, colsum_y, I, A, B1, B2, M, R, tol, max_iter, fold0, nfolds, Ypred, n_iter, ws, ws_bytes, stream);
}

}  // extern "C"
