// K-fold cross-validation of a tPLS model with every fold served by the same reads of X (validate.kfold_predictions).
//
// The folds of a K-fold split differ only in which rows are training rows, their means and their loadings; X_0 (the caller's
// uncentred tensor) is the same for all of them.  The no-write cross-covariance fit (fitrun_xcov.FitRun._finish_xcov_nowrite)
// needs X_0 only linearly in w (scores: X_0 w - (mu^T w) 1 - T g) and in t (down-date of S: X_0^T t - (1^T t) mu), so one pass
// over X with K columns serves all K folds:
//   kfold_xcov      S_f = X[rows_f]^T Y[rows_f] and the column sums / sums of squares per fold, ONE read of X; the training
//                   cross-covariance of fold k is the all-minus-own sum_f S_f - S_k, centred by a rank-one correction
//   kfold_inner     the whole inner loop of one component for every fold (a 1024-thread workgroup per fold, fold_loop.hpp)
//   (score pass)    X_0 [w_1 .. w_K] through cmtfpls_mttkrp_*                                       ONE read of X
//   kfold_epilogue  stage 1: the scores of every row under every fold (held-out rows: the prediction's projection), the row sums
//                   of the inner regression, the Y-side deflation and G_y on a grid of row tiles x folds, the R x R solve per
//                   fold; stage 2: the down-date of S_k from r = X_c^T t
//   (contraction)   X_0^T [t_1 * train_1 .. t_K * train_K] through cmtfpls_xcov_*                    ONE read of X
// 2R reads of X for all K folds; nothing is written to X and no copy of it is made.  Arithmetic: float64 (an f32 X is widened
// on load; 16-bit storage, bf16_t / f16_t of common.hpp, likewise: every stored element goes through to_f64, which is exact, so the
// _bf16 / _f16 builds of S return the bits of the _f32 build on the upcast values).  No workgroup waits on another.  Coupled models (ctPLS): the same steps per block with the score shared, see the
// section "coupled models" below.
#include "fold_loop.hpp"
#include "fold_regress.hpp"

namespace cmtfpls {

constexpr int kKfMaxK = 32, kKfMaxM = 64, kKfMaxR = 64, kKfMaxN = 256;
constexpr int kKfCols = 256;          // columns per workgroup of the column-owner kernels (one per thread)
// which fold a model holds out and where its held-out scores go (kfold_rows_kernel, kfold_ydefl_kernel): model k = fold k
// (kKfPlain), the grouped models of the permutation test (kKfGrouped), the split-major models of repeated K-fold (kKfSplits) or
// the bootstrap models, each row weighted by its count in the model's resample (kKfWeighted)
enum KfMode : int { kKfPlain = 0, kKfGrouped = 1, kKfSplits = 2, kKfWeighted = 3 };

// ---- kfold_xcov ------------------------------------------------------------------------------------------------------------
// Row chunks per fold so that the partial-sum grid has >= ~2048 workgroups (a thread per column, rows sequential: the rows of a
// workgroup are all of one fold, in the host's fold-sorted order); <= 64.
static int kf_chunks(int64_t I, int64_t P, int K) {
  const int64_t cb = (P + kKfCols - 1) / kKfCols;
  int64_t ch = (2048 + cb * K - 1) / (cb * K);
  const int64_t per_fold = I / K;
  if (ch > per_fold / 64) ch = per_fold / 64;
  if (ch > 64) ch = 64;
  return ch < 1 ? 1 : (int)ch;
}

template <typename T, int MT>
__global__ __launch_bounds__(kKfCols) void kfold_partials_kernel(const T* __restrict__ X, int64_t P, const double* __restrict__ Y, int M,
                                                                 const int* __restrict__ order, const int* __restrict__ off, int nch,
                                                                 double* __restrict__ part) {
  const int64_t c = (int64_t)blockIdx.x * kKfCols + threadIdx.x;
  const int k = blockIdx.y, ch = blockIdx.z;
  if (c >= P) return;
  const int lo0 = off[k], n = off[k + 1] - lo0, len = (n + nch - 1) / nch;
  const int lo = lo0 + min(n, ch * len), hi = lo0 + min(n, (ch + 1) * len);
  double acc[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) acc[j] = 0.0;
  double s1 = 0.0, s2 = 0.0;
  int r = lo;
  for (; r + 4 <= hi; r += 4) {                                   // four rows in flight
    int i4[4];
    double x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) i4[u] = order[r + u];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = to_f64(X[(int64_t)i4[u] * P + c]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double* y = Y + (int64_t)i4[u] * M;
#pragma unroll
      for (int j = 0; j < MT; ++j)
        if (j < M) acc[j] = fma(y[j], x[u], acc[j]);
      s1 += x[u];
      s2 = fma(x[u], x[u], s2);
    }
  }
  for (; r < hi; ++r) {
    const int i = order[r];
    const double xv = to_f64(X[(int64_t)i * P + c]);
    const double* y = Y + (int64_t)i * M;
#pragma unroll
    for (int j = 0; j < MT; ++j)
      if (j < M) acc[j] = fma(y[j], xv, acc[j]);
    s1 += xv;
    s2 = fma(xv, xv, s2);
  }
  double* o = part + (int64_t)(k * nch + ch) * (M + 2) * P + c;
#pragma unroll
  for (int j = 0; j < MT; ++j)
    if (j < M) o[(int64_t)j * P] = acc[j];
  o[(int64_t)M * P] = s1;
  o[(int64_t)(M + 1) * P] = s2;
}

// all-minus-own: S_k = sum_f S_f - S_own(k) - n_k mu_k ydev_k^T (the centring of the training rows as a rank-one correction),
// mu_k = (colsum - colsum_own(k)) / n_k (n_k: training rows of fold k)
__global__ __launch_bounds__(kKfCols) void kfold_finish_kernel(int64_t P, int M, int K, int nch, int I, const int* __restrict__ off,
                                                               const double* __restrict__ part, const double* __restrict__ ydev,
                                                               double* __restrict__ S, double* __restrict__ mean, double* __restrict__ stats) {
  const int64_t c = (int64_t)blockIdx.x * kKfCols + threadIdx.x;
  if (c >= P) return;
  double own[kKfMaxK], mu[kKfMaxK];
  auto fold_sum = [&](int k, int j) {
    double s = 0.0;
    for (int ch = 0; ch < nch; ++ch) s += part[((int64_t)(k * nch + ch) * (M + 2) + j) * P + c];
    return s;
  };
  double tot = 0.0, totq = 0.0;
  for (int k = 0; k < K; ++k) { own[k] = fold_sum(k, M); tot += own[k]; totq += fold_sum(k, M + 1); }
  stats[c] = tot;
  stats[P + c] = totq;
  for (int k = 0; k < K; ++k) {
    const double ntr = (double)(I - (off[k + 1] - off[k]));
    mu[k] = (tot - own[k]) / ntr;
    mean[(int64_t)k * P + c] = mu[k];
  }
  for (int m = 0; m < M; ++m) {
    double t = 0.0;
    for (int k = 0; k < K; ++k) { own[k] = fold_sum(k, m); t += own[k]; }
    for (int k = 0; k < K; ++k) {
      const double ntr = (double)(I - (off[k + 1] - off[k]));
      S[((int64_t)k * M + m) * P + c] = (t - own[k]) - ntr * mu[k] * ydev[k * M + m];
    }
  }
}

// ---- row tiles of the epilogue ------------------------------------------------------------------------------------------------
// The row work of a component (scores, the training Gram row, T^T u, Y^T t, the Y deflation, Y^T Y) runs on a grid of row tiles x
// folds; each tile writes its partial sums, which are added in tile order (fixed order: the same bits on every run).
constexpr int kKfRowThreads = 256, kKfMaxTiles = 128, kKfChunk = 32;

__host__ __device__ inline int kf_tiles(int64_t I) {
  int64_t nt = (I + kKfRowThreads - 1) / kKfRowThreads;
  return (int)(nt > kKfMaxTiles ? kKfMaxTiles : (nt < 1 ? 1 : nt));
}

__device__ __forceinline__ void kf_tile_rows(int I, int NT, int tile, int* lo, int* hi) {
  const int len = (I + NT - 1) / NT;
  *lo = min(I, tile * len);
  *hi = min(I, (tile + 1) * len);
}

// vec of fold k: b (R) | c (R) | ya (M) | 1^T t (1) | g (R) | mu^T w (1)
__host__ __device__ inline int kf_vec_len(int R, int M) { return 3 * R + M + 2; }

// ---- kfold_inner ------------------------------------------------------------------------------------------------------------
static size_t kf_inner_lds_bytes(int A, int B, int M) {
  const size_t n = (size_t)(A < B ? A : B), k = (size_t)(A < B ? B : A);
  return ((size_t)A + B + 3 * (size_t)M + (size_t)M * M + n + k) * sizeof(double);
}

// X of order 4 (cmtfpls_kfold_inner_tensor_f64): the trailing dims B1 x B2 = B, the mode loadings' outputs (nullable) and the
// largest short side of the three unfoldings of Z (the Gram scratch of lx_cp3's init).  B2 == 0: order 2 or 3.
struct KfTensor {
  int B1, B2, nmax;
  double* Wk;             // K x R x B1
  double* Wl;             // K x R x B2
};

// LDS: wA (A), wB (B), q, qn, tq (M each), G_y (M x M), xs (nmax), then lx_cp3's wK (B1), wL (B2), v (B), tmp (max dim), part
static size_t kf_inner_tensor_lds_bytes(int A, int B1, int B2, int M) {
  const size_t B = (size_t)B1 * B2, dmax = (size_t)(A > B1 ? (A > B2 ? A : B2) : (B1 > B2 ? B1 : B2));
  return ((size_t)A + B + 3 * (size_t)M + (size_t)M * M + lx_tensor_nmax(A, B1, B2) + B1 + B2 + B + dmax + kLxNT) * sizeof(double);
}

// per fold: Z, Zt, wk, then lx_cp3's U, yl, vr (P each), G0, G1 (nmax x nmax each)
static int64_t kf_inner_tensor_ws_per_fold(int A, int B1, int B2) {
  const int64_t n = lx_tensor_nmax(A, B1, B2);
  return 6 * (int64_t)A * B1 * B2 + 2 * n * n;
}

// a workgroup per fold: G_y from the row tiles' partials, the inner loop, then what the row pass needs of the new loadings:
// mu_k^T w and g_j = w_j^T w_a (Gram of a Khatri-Rao product = product of the mode Grams).
// GROUPED (permutation test, see "grouped models" below): the "folds" of the state are models, model m holding out fold
// model_fold[m]; the training means are those of that fold.  Without it model k is fold k and the code is the one it always was.
// TENSOR (X of order 4, st.B = tn.B1 tn.B2): the extraction is lx_cp3, wB = wK (x) wL, and the mode loadings go to tn.Wk / tn.Wl;
// everything after the loop sees the block as I x A x B, as for order 3.
template <bool GROUPED, bool TENSOR = false>
__global__ __launch_bounds__(kLxNT) void kfold_inner_kernel(cmtfpls_kfold_state st, int a, double tol, int max_iter, double* ws,
                                                            int64_t ws_per_fold, const int* __restrict__ model_fold,
                                                            KfTensor tn = KfTensor{0, 0, 0, nullptr, nullptr}) {
  extern __shared__ double sm[];
  __shared__ double red[kLxWaves];
  __shared__ double bestv[kLxWaves];
  __shared__ int besti[kLxWaves];
  const int tid = threadIdx.x, fold = blockIdx.x;
  const int A = st.A, B = st.B, M = st.M, K = st.K, R = st.R;
  const int64_t P = (int64_t)A * B;
  const int n = TENSOR ? tn.nmax : (A < B ? A : B), NT = kf_tiles(st.I);
  double* Z = ws + (int64_t)fold * ws_per_fold;                  // P
  double* Zt = Z + P;                                             // P
  double* wk = Zt + P;                                            // P
  double* G0 = wk + (TENSOR ? 4 : 1) * P;                         // n x n (TENSOR: after U, yl, vr)
  double* G1 = G0 + (int64_t)n * n;                               // n x n
  double* wA = sm;
  double* wB = wA + A;
  double* q = wB + B;
  double* qn = q + M;
  double* tq = qn + M;
  double* Gy = tq + M;
  double* xs = Gy + M * M;
  double* ys = xs + n;
  LxTensor lt;                                                    // (ys itself is not used by lx_cp3: its long vector is lt.yl)
  if (TENSOR) lt = lx_tensor_scratch(ys, wk + P, tn.B1, tn.B2, B, max(A, max(tn.B1, tn.B2)), P, kLxNT);
  for (int o = tid; o < M * M; o += kLxNT) {
    double s = 0.0;
    for (int t = 0; t < NT; ++t) s += st.Gy[((int64_t)fold * NT + t) * M * M + o];
    Gy[o] = s;
  }
  __syncthreads();
  const int it = lx_inner_loop(st.S + (int64_t)fold * M * P, Gy, P, M, A, B, tol, max_iter, q, qn, tq, Z, Zt, wk, wA, wB, G0, G1, xs,
                               ys, red, bestv, besti, lt);
  bool bad = false;
  if (TENSOR) {
    for (int j = tid; j < tn.B1; j += kLxNT) {
      if (tn.Wk) tn.Wk[((int64_t)fold * R + a) * tn.B1 + j] = lt.wK[j];
      bad |= !isfinite(lt.wK[j]);
    }
    for (int j = tid; j < tn.B2; j += kLxNT) {
      if (tn.Wl) tn.Wl[((int64_t)fold * R + a) * tn.B2 + j] = lt.wL[j];
      bad |= !isfinite(lt.wL[j]);
    }
  }
  for (int j = tid; j < A; j += kLxNT) {
    st.WA[(int64_t)j * K + fold] = wA[j];
    st.Wa[((int64_t)fold * R + a) * A + j] = wA[j];
    bad |= !isfinite(wA[j]);
  }
  for (int j = tid; j < B; j += kLxNT) {
    st.WB[(int64_t)j * K + fold] = wB[j];
    st.Wb[((int64_t)fold * R + a) * B + j] = wB[j];
    bad |= !isfinite(wB[j]);
  }
  for (int m = tid; m < M; m += kLxNT) { st.Q[((int64_t)fold * R + a) * M + m] = q[m]; bad |= !isfinite(q[m]); }
  if (bad) atomicOr(st.status + fold, 1);
  if (tid == 0) st.n_iter[fold * R + a] = it;
  double* vec = st.vec + (int64_t)fold * kf_vec_len(R, M);
  const double* mean = st.mean + (int64_t)(GROUPED ? model_fold[fold] : fold) * P;
  double s = 0.0;
  for (int64_t c = tid; c < P; c += kLxNT) s = fma(mean[c], wk[c], s);     // (wk: the converged loadings' Kronecker product)
  s = lx_sum(s, red);
  if (tid == 0) vec[3 * R + M + 1] = s;
  for (int j = 0; j < a; ++j) {
    double sa = 0.0, sb = 0.0;
    for (int i = tid; i < A; i += kLxNT) sa = fma(st.Wa[((int64_t)fold * R + j) * A + i], wA[i], sa);
    for (int i = tid; i < B; i += kLxNT) sb = fma(st.Wb[((int64_t)fold * R + j) * B + i], wB[i], sb);
    sa = lx_sum(sa, red);
    sb = lx_sum(sb, red);
    if (tid == 0) vec[2 * R + M + 1 + j] = sa * sb;
  }
}

// ---- kfold_epilogue ---------------------------------------------------------------------------------------------------------
// stage 1a, grid (row tiles, folds): t_k = X_0 w_k - (mu_k^T w_k) 1 - T_k[:, :a] g_k for every row of the tile (held-out rows: the
// projection predict makes, tpls.py:133-142), the training-masked score, u = Y_k q, and the tile's partial sums of
// T_train^T t (the Gram row a), T_train^T u, 1^T t_train and Y_k^T t.  kKfGrouped: model k holds out fold model_fold[k] and writes
// its held-out scores to group k % groups of Tout (groups x I x R).  kKfSplits: `groups` is the folds per split; model k holds out
// fold k % groups of split k / groups, whose fold map is row k / groups of fold_of, and writes its held-out scores to that split's
// slot of Tout (splits x I x R).  kKfWeighted: fold_of is n x I counts, model k trains on the rows with c = fold_of[k I + i] > 0
// and every training-row sum is weighted by c (tm = c t); Tout is not written (the rows with c = 0 keep their projection in T)
template <int MODE>
__global__ __launch_bounds__(kKfRowThreads) void kfold_rows_kernel(cmtfpls_kfold_state st, int a, const double* __restrict__ sc,
                                                                   const int* __restrict__ model_fold, int groups) {
  constexpr int NW = kKfRowThreads / 64;
  __shared__ double acc[NW][2 * kKfMaxR + 1 + kKfMaxM];
  __shared__ double q[kKfMaxM], g[kKfMaxR];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, tile = blockIdx.x, k = blockIdx.y;
  const int I = st.I, M = st.M, K = st.K, R = st.R, kk = a + 1, NT = kf_tiles(I), nv = 2 * kk + 1 + M;
  const double* vec = st.vec + (int64_t)k * kf_vec_len(R, M);
  const double mw = vec[3 * R + M + 1];
  const int own = MODE == kKfGrouped ? model_fold[k] : MODE == kKfSplits ? k % groups : k;
  const int* fold_of = MODE == kKfSplits ? st.fold_of + (int64_t)(k / groups) * I
                       : MODE == kKfWeighted ? st.fold_of + (int64_t)k * I : st.fold_of;
  double* Tout = MODE == kKfGrouped ? st.Tout + (int64_t)(k % groups) * I * R
                 : MODE == kKfSplits ? st.Tout + (int64_t)(k / groups) * I * R : st.Tout;
  for (int m = tid; m < M; m += kKfRowThreads) q[m] = st.Q[((int64_t)k * R + a) * M + m];
  for (int j = tid; j < a; j += kKfRowThreads) g[j] = vec[2 * R + M + 1 + j];
  for (int v = tid; v < NW * (2 * kKfMaxR + 1 + kKfMaxM); v += kKfRowThreads) (&acc[0][0])[v] = 0.0;
  __syncthreads();
  double* T = st.T + (int64_t)k * I * R;
  const double* Yk = st.Yk + (int64_t)k * I * M;
  int lo, hi;
  kf_tile_rows(I, NT, tile, &lo, &hi);
  for (int i0 = lo; i0 < hi; i0 += kKfRowThreads) {
    const int i = i0 + tid;
    const bool ok = i < hi;
    bool train = false;
    double t = 0.0, u = 0.0, wt = 0.0;
    if (ok) {
      t = sc[(int64_t)i * K + k] - mw;
      for (int j = 0; j < a; ++j) t = fma(-T[(int64_t)i * R + j], g[j], t);
      T[(int64_t)i * R + a] = t;
      if (MODE == kKfWeighted) {
        const int c = fold_of[i];
        train = c > 0;
        wt = (double)c;
      } else {
        train = fold_of[i] != own;
        if (!train) Tout[(int64_t)i * R + a] = t;
      }
      st.tm[(int64_t)i * K + k] = train ? (MODE == kKfWeighted ? wt * t : t) : 0.0;
      if (train)
        for (int m = 0; m < M; ++m) u = fma(Yk[(int64_t)i * M + m], q[m], u);
      if (MODE == kKfWeighted) u *= wt;
    }
    const double tt = train ? (MODE == kKfWeighted ? wt * t : t) : 0.0;
    for (int p = 0; p < kk; ++p) {
      const double tp = train ? (p == a ? t : T[(int64_t)i * R + p]) : 0.0;
      const double s1 = wave_sum(tp * tt), s2 = wave_sum(tp * u);
      if (lane == 0) { acc[wv][p] += s1; acc[wv][kk + p] += s2; }
    }
    const double s3 = wave_sum(tt);
    if (lane == 0) acc[wv][2 * kk] += s3;
    for (int m = 0; m < M; ++m) {                                  // (held-out rows of Y_k are 0)
      const double s4 = wave_sum(ok ? Yk[(int64_t)i * M + m] * (MODE == kKfWeighted ? tt : t) : 0.0);
      if (lane == 0) acc[wv][2 * kk + 1 + m] += s4;
    }
  }
  __syncthreads();
  for (int v = tid; v < nv; v += kKfRowThreads) {
    double s = 0.0;
    for (int w = 0; w < NW; ++w) s += acc[w][v];
    st.part[((int64_t)k * NT + tile) * (2 * kKfMaxR + 1 + kKfMaxM) + v] = s;
  }
}

// stage 1b, a workgroup per fold: the tiles' sums in tile order; coef_[:a+1, a] = lstsq(T_train, u) (tpls.py:110-112: normal
// equations, equilibrated Cholesky, a column with a pivot below (a+1) eps dropped); c = T^T T b for the down-date
__global__ __launch_bounds__(64) void kfold_solve_kernel(cmtfpls_kfold_state st, int a) {
  __shared__ double tot[2 * kKfMaxR + 1 + kKfMaxM];
  __shared__ double Gn[kKfMaxR * kKfMaxR];
  __shared__ double bb[kKfMaxR], dd[kKfMaxR];
  const int tid = threadIdx.x, k = blockIdx.x;
  const int M = st.M, R = st.R, kk = a + 1, NT = kf_tiles(st.I), nv = 2 * kk + 1 + M;
  double* Gt = st.Gt + (int64_t)k * R * R;
  double* vec = st.vec + (int64_t)k * kf_vec_len(R, M);
  for (int v = tid; v < nv; v += 64) {
    double s = 0.0;
    for (int t = 0; t < NT; ++t) s += st.part[((int64_t)k * NT + t) * (2 * kKfMaxR + 1 + kKfMaxM) + v];
    tot[v] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int p = 0; p < kk; ++p) { Gt[a * R + p] = tot[p]; Gt[p * R + a] = tot[p]; }
  for (int i = 0; i < kk; ++i)
    for (int j = 0; j < kk; ++j) Gn[i * kk + j] = Gt[i * R + j];
  fold_normal_solve(Gn, tot + kk, kk, dd, bb);                      // fold_regress.hpp
  for (int r = 0; r < kk; ++r) { st.coef[((int64_t)k * R + r) * R + a] = bb[r]; vec[r] = bb[r]; }
  for (int r = 0; r < kk; ++r) {                                  // c = T^T yhat = (T^T T) b, the training Gram
    double v = 0.0;
    for (int j = 0; j < kk; ++j) v = fma(Gt[r * R + j], bb[j], v);
    vec[R + r] = v;
  }
  for (int m = 0; m < M; ++m) vec[2 * R + m] = tot[2 * kk + 1 + m];
  vec[2 * R + M] = tot[2 * kk];
  if (!isfinite(bb[a]) || !isfinite(tot[2 * kk])) st.status[k] |= 2;
}

// stage 0 / 1c, grid (row tiles, folds): (deflate: Y_k -= (T b) q^T on the training rows, tpls.py:113) and the tile's partial
// Y_k^T Y_k for the next component's convergence test, rows staged through LDS a chunk at a time.  MODE: the training rows as in
// kfold_rows_kernel (`folds`: the folds per split of kKfSplits; kKfWeighted: the rows with a count > 0 deflated, the Gram
// sum_i c_i y_i y_i^T)
template <int MODE>
__global__ __launch_bounds__(kKfRowThreads) void kfold_ydefl_kernel(cmtfpls_kfold_state st, int a, int deflate,
                                                                    const int* __restrict__ model_fold, int folds) {
  constexpr int EPT = kKfMaxM * kKfMaxM / kKfRowThreads;          // Gram entries per thread
  __shared__ double Ys[kKfChunk][kKfMaxM + 1];
  __shared__ double q[kKfMaxM], b[kKfMaxR];
  __shared__ double wr[MODE == kKfWeighted ? kKfChunk : 1];       // the staged rows' counts
  const int tid = threadIdx.x, tile = blockIdx.x, k = blockIdx.y;
  const int I = st.I, M = st.M, R = st.R, kk = a + 1, NT = kf_tiles(I);
  const double* vec = st.vec + (int64_t)k * kf_vec_len(R, M);
  const int own = MODE == kKfGrouped ? model_fold[k] : MODE == kKfSplits ? k % folds : k;
  const int* fold_of = MODE == kKfSplits ? st.fold_of + (int64_t)(k / folds) * I
                       : MODE == kKfWeighted ? st.fold_of + (int64_t)k * I : st.fold_of;
  if (deflate) {
    for (int m = tid; m < M; m += kKfRowThreads) q[m] = st.Q[((int64_t)k * R + a) * M + m];
    for (int j = tid; j < kk; j += kKfRowThreads) b[j] = vec[j];
  }
  __syncthreads();
  const double* T = st.T + (int64_t)k * I * R;
  double* Yk = st.Yk + (int64_t)k * I * M;
  double accg[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) accg[e] = 0.0;
  int lo, hi;
  kf_tile_rows(I, NT, tile, &lo, &hi);
  for (int i0 = lo; i0 < hi; i0 += kKfChunk) {
    for (int idx = tid; idx < kKfChunk * M; idx += kKfRowThreads) {
      const int r = idx / M, m = idx % M, i = i0 + r;
      double y = 0.0;
      if (i < hi) {
        y = Yk[(int64_t)i * M + m];
        if (deflate && (MODE == kKfWeighted ? fold_of[i] > 0 : fold_of[i] != own)) {
          double yh = 0.0;
          for (int j = 0; j < kk; ++j) yh = fma(T[(int64_t)i * R + j], b[j], yh);
          y = fma(-yh, q[m], y);
          Yk[(int64_t)i * M + m] = y;
        }
      }
      Ys[r][m] = y;
      if (MODE == kKfWeighted && m == 0) wr[r] = i < hi ? (double)fold_of[i] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int o = tid + e * kKfRowThreads;
      if (o < M * M) {
        const int m1 = o / M, m2 = o % M;
        double s = accg[e];
        if (MODE == kKfWeighted)
          for (int r = 0; r < kKfChunk; ++r) s = fma(Ys[r][m1] * wr[r], Ys[r][m2], s);
        else
          for (int r = 0; r < kKfChunk; ++r) s = fma(Ys[r][m1], Ys[r][m2], s);
        accg[e] = s;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int o = tid + e * kKfRowThreads;
    if (o < M * M) st.Gy[((int64_t)k * NT + tile) * M * M + o] = accg[e];
  }
}

// stage 2, a thread per column and fold: r_a = X_c^T t_a = rs - (1^T t) mu (rs = X_0^T (t * train) from the contraction pass), kept
// for later components; X_{a+1}^T yhat = sum_{j<=a} b_j r_j - sum_{j<=a} c_j w_j; S -= w ya^T + (X_{a+1}^T yhat) q^T
// (fitrun_xcov._finish_xcov_nowrite, cmtfpls_s_downdate_f64)
template <bool GROUPED>
__global__ __launch_bounds__(kKfCols) void kfold_downdate_kernel(cmtfpls_kfold_state st, int a, const double* __restrict__ rs,
                                                                 const int* __restrict__ model_fold) {
  const int64_t c = (int64_t)blockIdx.x * kKfCols + threadIdx.x;
  const int k = blockIdx.y;
  const int A = st.A, B = st.B, M = st.M, R = st.R;
  const int64_t P = (int64_t)A * B;
  if (c >= P) return;
  const double* vec = st.vec + (int64_t)k * kf_vec_len(R, M);
  const int ia = (int)(c / B), ib = (int)(c % B);
  const double r = rs[(int64_t)k * P + c] - vec[2 * R + M] * st.mean[(int64_t)(GROUPED ? model_fold[k] : k) * P + c];
  st.Rm[((int64_t)k * R + a) * P + c] = r;
  double v = 0.0;
  for (int j = 0; j < a; ++j) v = fma(vec[j], st.Rm[((int64_t)k * R + j) * P + c], v);
  v = fma(vec[a], r, v);
  for (int j = 0; j <= a; ++j) v = fma(-vec[R + j], st.Wa[((int64_t)k * R + j) * A + ia] * st.Wb[((int64_t)k * R + j) * B + ib], v);
  const double w = st.Wa[((int64_t)k * R + a) * A + ia] * st.Wb[((int64_t)k * R + a) * B + ib];
  const double* q = st.Q + ((int64_t)k * R + a) * M;
  double* S = st.S + (int64_t)k * M * P + c;
  for (int m = 0; m < M; ++m) S[(int64_t)m * P] -= fma(w, vec[2 * R + m], v * q[m]);
}

static bool kf_shape_ok(int64_t I, int A, int B, int M, int K, int R) {
  const int n = A < B ? A : B;
  return K >= 2 && K <= kKfMaxK && M >= 1 && M <= kKfMaxM && R >= 1 && R <= kKfMaxR && n <= kKfMaxN && I >= K &&
         I <= (int64_t)1 << 30 && (int64_t)A * B <= (int64_t)1 << 24 && kf_inner_lds_bytes(A, B, M) <= 150 * 1024;
}

template <typename T>
static int run_kfold_xcov(const T* X, int64_t I, int A, int B, const double* Y, int M, const int* order, const int* fold_off, int K,
                          const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!X || !Y || !order || !fold_off || !ydev || !S || !mean || !stats || I <= 0 || A <= 0 || B <= 0 || M <= 0 || K <= 0) {
    set_error("kfold_xcov: bad argument");
    return CMTFPLS_EINVAL;
  }
  if (!kf_shape_ok(I, A, B, M, K, 1)) {
    set_error("kfold_xcov: shape outside the device form (2 <= K <= 32, M <= 64, min(A, B) <= 256); refit per fold");
    return CMTFPLS_EUNSUPPORTED;
  }
  const int64_t P = (int64_t)A * B;
  const size_t need = cmtfpls_kfold_xcov_workspace_bytes(I, P, M, K);
  if (!ws || ws_bytes < need) { set_error("kfold_xcov: workspace too small"); return CMTFPLS_EWORKSPACE; }
  const int nch = kf_chunks(I, P, K);
  double* part = static_cast<double*>(ws);
  const dim3 g((unsigned)((P + kKfCols - 1) / kKfCols), (unsigned)K, (unsigned)nch);
  if (M <= 8) hipLaunchKernelGGL((kfold_partials_kernel<T, 8>), g, dim3(kKfCols), 0, st, X, P, Y, M, order, fold_off, nch, part);
  else if (M <= 16) hipLaunchKernelGGL((kfold_partials_kernel<T, 16>), g, dim3(kKfCols), 0, st, X, P, Y, M, order, fold_off, nch, part);
  else if (M <= 32) hipLaunchKernelGGL((kfold_partials_kernel<T, 32>), g, dim3(kKfCols), 0, st, X, P, Y, M, order, fold_off, nch, part);
  else hipLaunchKernelGGL((kfold_partials_kernel<T, 64>), g, dim3(kKfCols), 0, st, X, P, Y, M, order, fold_off, nch, part);
  int rc = check_launch("kfold_xcov");
  if (rc) return rc;
  hipLaunchKernelGGL(kfold_finish_kernel, dim3((unsigned)((P + kKfCols - 1) / kKfCols)), dim3(kKfCols), 0, st, P, M, K, nch, (int)I,
                     fold_off, part, ydev, S, mean, stats);
  return check_launch("kfold_xcov");
}

static bool kf_state_ok(const cmtfpls_kfold_state* s) {
  return s && s->fold_of && s->S && s->mean && s->Yk && s->Gy && s->WA && s->WB && s->Q && s->Wa && s->Wb && s->T && s->Gt && s->coef &&
         s->Rm && s->tm && s->Tout && s->vec && s->n_iter && s->status && s->part;
}

// ---- coupled models (ctPLS) -------------------------------------------------------------------------------------------------
// nb blocks share the sample mode and one score, t = (1/nb) sum_b X_b^(a) w_b (cmtf.py:95-126); each block is deflated by that t.
// Each block has a state view of its own: S, mean, WA, WB, Wa, Wb, Rm, A and B are the block's, every other field is the same
// buffer in all views (the Y side, the scores, the solve).  Per component:
//   kfold_inner_coupled  every fold's inner loop over all blocks (a workgroup per fold, the blocks in turn):
//                        Z_b = S_b^T q, rank-1 of Z_b -> w_b, q ∝ (1/nb) sum_b S_b w_b; then the block-averaged mu^T w and g
//   (score pass)         X_b [w_b,1 .. w_b,K] per block through cmtfpls_mttkrp_*                          ONE read of each block
//   kfold_combine        the average of the blocks' scores; then kfold_epilogue stage 1 on the first view (t = that average
//                        - mean(mu_b^T w_b) - T mean(g_b): the tPLS epilogue on the shared t)
//   (contraction)        X_b^T [t_1 * train_1 .. t_K * train_K] per block through cmtfpls_xcov_*          ONE read of each block
//   kfold_epilogue 2     per block on its own view: S_b -= w_b ya^T + (X_b,(a+1)^T yhat) q^T, the tPLS down-date with the
//                        block's w, r = X_b,c^T t and mean (X_b,(a+1) = X_b,c - sum_j t_j w_b,j^T)
// Sums over blocks are added in block order.
constexpr int kKfMaxBlocks = 8;

struct KfBlocks {
  cmtfpls_kfold_state b[kKfMaxBlocks];
  int nb;
};

struct KfCoupledDims {
  int64_t pmax, psum;                 // largest A * B, sum of A * B over the blocks
  int amax, bmax, nmax, kmax;         // largest A, B, min(A, B), max(A, B)
};

static KfCoupledDims kf_coupled_dims(const cmtfpls_kfold_state* v, int nb) {
  KfCoupledDims d{0, 0, 0, 0, 0, 0};
  for (int b = 0; b < nb; ++b) {
    const int64_t P = (int64_t)v[b].A * v[b].B;
    d.pmax = P > d.pmax ? P : d.pmax;
    d.psum += P;
    d.amax = v[b].A > d.amax ? v[b].A : d.amax;
    d.bmax = v[b].B > d.bmax ? v[b].B : d.bmax;
    const int n = v[b].A < v[b].B ? v[b].A : v[b].B, k = v[b].A < v[b].B ? v[b].B : v[b].A;
    d.nmax = n > d.nmax ? n : d.nmax;
    d.kmax = k > d.kmax ? k : d.kmax;
  }
  return d;
}

// LDS: wA (amax), wB (bmax), q, qn, tq (M each), G_y (M x M), xs (nmax), ys (kmax)
static size_t kf_coupled_lds_bytes(const KfCoupledDims& d, int M) {
  return ((size_t)d.amax + d.bmax + 3 * (size_t)M + (size_t)M * M + d.nmax + d.kmax) * sizeof(double);
}

// per fold: Z, Zt (pmax each), G0, G1 (nmax x nmax each), then every block's Kronecker loading wk_b (A_b * B_b), one after another
static int64_t kf_coupled_ws_per_fold(const KfCoupledDims& d) { return 2 * d.pmax + 2 * (int64_t)d.nmax * d.nmax + d.psum; }

// Blocks of order 4 (cmtfpls_kfold_inner_coupled_tensor_f64): per block the trailing dims B1 x B2 = B (B2 == 0: a matrix block, order
// 2 or 3) and where its slice of the mode loadings' outputs starts; the scratch of lx_cp3 is shared, sized over the tensor blocks.
struct KfCoupledTensor {
  int B1[kKfMaxBlocks], B2[kKfMaxBlocks];
  int64_t ok[kKfMaxBlocks], ol[kKfMaxBlocks];   // block b's K x R x B1_b / K x R x B2_b slice of Wk / Wl starts here (in doubles)
  int b1max, b2max, btmax, dmax, kmax;          // tensor blocks: largest B1, B2, B1 B2, single dim; matrix blocks: largest max(A, B)
  int64_t ptmax, psum;                          // largest A B1 B2 of a tensor block; sum of A B over every block
  double* Wk;                                   // nullable
  double* Wl;                                   // nullable
};

struct KfCoupledTensorDims {
  KfCoupledDims d;      // pmax, psum, amax, bmax over every block (B = B1 B2); nmax over the matrix blocks' min(A, B) and the short
  KfCoupledTensor tn;   // sides of every unfolding of every tensor block; kmax over the matrix blocks alone (a tensor block has no ys)
};

static KfCoupledTensorDims kf_coupled_tensor_dims(const cmtfpls_kfold_state* v, int nb, const int* dims) {
  KfCoupledTensorDims o{};
  const int64_t KR = (int64_t)v[0].K * v[0].R;
  int64_t ok = 0, ol = 0;
  for (int b = 0; b < nb; ++b) {
    const int A = v[b].A, B = v[b].B, B1 = dims[2 * b], B2 = dims[2 * b + 1];
    const int64_t P = (int64_t)A * B;
    o.d.pmax = P > o.d.pmax ? P : o.d.pmax;
    o.d.psum += P;
    o.d.amax = A > o.d.amax ? A : o.d.amax;
    o.d.bmax = B > o.d.bmax ? B : o.d.bmax;
    o.tn.B1[b] = B1;
    o.tn.B2[b] = B2;
    o.tn.ok[b] = ok;
    o.tn.ol[b] = ol;
    int n;
    if (B2 > 0) {
      n = lx_tensor_nmax(A, B1, B2);
      const int dm = A > B1 ? (A > B2 ? A : B2) : (B1 > B2 ? B1 : B2);
      o.tn.b1max = B1 > o.tn.b1max ? B1 : o.tn.b1max;
      o.tn.b2max = B2 > o.tn.b2max ? B2 : o.tn.b2max;
      o.tn.btmax = B > o.tn.btmax ? B : o.tn.btmax;
      o.tn.dmax = dm > o.tn.dmax ? dm : o.tn.dmax;
      o.tn.ptmax = P > o.tn.ptmax ? P : o.tn.ptmax;
      ok += KR * B1;
      ol += KR * B2;
    } else {
      n = A < B ? A : B;
      const int k = A < B ? B : A;
      o.d.kmax = k > o.d.kmax ? k : o.d.kmax;
    }
    o.d.nmax = n > o.d.nmax ? n : o.d.nmax;
  }
  o.tn.kmax = o.d.kmax;
  o.tn.psum = o.d.psum;
  return o;
}

// LDS: kf_coupled_lds_bytes' wA (amax), wB (bmax), q, qn, tq (M each), G_y (M x M), xs (nmax), ys (kmax), then lx_cp3's wK (b1max),
// wL (b2max), v (btmax), tmp (dmax) and part (the 1024 row-group partials).  One block of order 4: kf_inner_tensor_lds_bytes.
static size_t kf_coupled_tensor_lds_bytes(const KfCoupledTensorDims& o, int M) {
  return kf_coupled_lds_bytes(o.d, M) + ((size_t)o.tn.b1max + o.tn.b2max + o.tn.btmax + o.tn.dmax + kLxNT) * sizeof(double);
}

// per fold: kf_coupled_ws_per_fold's Z, Zt, G0, G1 and wk_b, then lx_cp3's U, yl, vr (ptmax each).  One block of order 4:
// kf_inner_tensor_ws_per_fold.
static int64_t kf_coupled_tensor_ws_per_fold(const KfCoupledTensorDims& o) { return kf_coupled_ws_per_fold(o.d) + 3 * o.tn.ptmax; }

// a workgroup per fold.  A pass is lx_inner_loop's steps (fold_loop.hpp) once per block, with tq zeroed, every block's S_b w_b added
// to it in block order and the average taken in lx_q_step; Wa / Wb and Wk / Wl are stored between a block's extraction and the
// barrier after its Kronecker product.  With one block every step is the one of kfold_inner_kernel in the same order, so the
// result is bitwise that of the tPLS kernel.  GROUPED (permutation test, see "grouped models" below): every view's mean is per
// fold (folds x P_b) and model m reads row model_fold[m] of it; S, the loadings, Q, vec, n_iter, status and Gy are per model in
// every layout.  Without it model k is fold k and the code is the one it always was.
// TENSOR (a block of order 4 among them, tn.B2[b] > 0 with B_b = tn.B1[b] tn.B2[b]): that block's extraction is lx_cp3, its
// wB = wK (x) wL, and its mode loadings go to its slice of tn.Wk / tn.Wl on every pass (the last pass's stay, as Wa / Wb);
// everything after the extraction sees the block as I x A x B.  With one such block every step is the one of
// kfold_inner_kernel<GROUPED, true> in the same order.  Without TENSOR the code is the one it always was.
template <bool GROUPED, bool TENSOR = false>
__global__ __launch_bounds__(kLxNT) void kfold_inner_coupled_kernel(KfBlocks bl, int a, double tol, int max_iter, double* ws,
                                                                    int64_t ws_per_fold, int64_t pmax, int nmax, int amax, int bmax,
                                                                    const int* __restrict__ model_fold,
                                                                    KfCoupledTensor tn = KfCoupledTensor{}) {
  extern __shared__ double sm[];
  __shared__ double red[kLxWaves];
  __shared__ double bestv[kLxWaves];
  __shared__ int besti[kLxWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fold = blockIdx.x;
  const int nb = bl.nb, M = bl.b[0].M, K = bl.b[0].K, R = bl.b[0].R, NT = kf_tiles(bl.b[0].I);
  double* Z = ws + (int64_t)fold * ws_per_fold;                  // pmax
  double* Zt = Z + pmax;                                          // pmax
  double* G0 = Zt + pmax;                                         // nmax x nmax
  double* G1 = G0 + (int64_t)nmax * nmax;                         // nmax x nmax
  double* wk0 = G1 + (int64_t)nmax * nmax;                        // sum_b A_b B_b
  double* wA = sm;
  double* wB = wA + amax;
  double* q = wB + bmax;
  double* qn = q + M;
  double* tq = qn + M;
  double* Gy = tq + M;
  double* xs = Gy + M * M;
  double* ys = xs + nmax;                                         // kmax
  LxTensor lt;                                                    // lx_cp3's scratch, shared by the tensor blocks: LDS after ys, global
  if (TENSOR)                                                     // after the blocks' wk
    lt = lx_tensor_scratch(ys + tn.kmax, wk0 + tn.psum, tn.b1max, tn.b2max, tn.btmax, tn.dmax, tn.ptmax, kLxNT);
  for (int o = tid; o < M * M; o += kLxNT) {
    double s = 0.0;
    for (int t = 0; t < NT; ++t) s += bl.b[0].Gy[((int64_t)fold * NT + t) * M * M + o];
    Gy[o] = s;
  }
  for (int m = tid; m < M; m += kLxNT) q[m] = (m == 0) ? 1.0 : 0.0;                 // u_0 = Y_f[:, 0] (cmtf.py:88)
  __syncthreads();
  int it = 0;
  for (; it < max_iter; ++it) {                                                    // cmtf.py:89
    for (int m = tid; m < M; m += kLxNT) tq[m] = 0.0;
    double* wk = wk0;
    for (int b = 0; b < nb; ++b) {                                                 // cmtf.py:90-103, block by block
      const int A = bl.b[b].A, B = bl.b[b].B;
      const int64_t P = (int64_t)A * B;
      const double* S = bl.b[b].S + (int64_t)fold * M * P;
      lx_z_from_s(S, q, Z, P, M);                                                    // Z_b = X_b x_0 u = S_b^T q
      if (TENSOR) {                                                                  // B2 > 0: order 4, the rank-1 CP of the A x B1 x B2 Z
        lt.B1 = tn.B1[b];
        lt.B2 = tn.B2[b];
      }
      lx_extract<TENSOR>(Z, Zt, A, B, P, tol, lt, wA, wB, G0, G1, xs, ys, red, bestv, besti);
      if (TENSOR && lt.B2 > 0) {
        if (tn.Wk) for (int j = tid; j < lt.B1; j += kLxNT) tn.Wk[tn.ok[b] + ((int64_t)fold * R + a) * lt.B1 + j] = lt.wK[j];
        if (tn.Wl) for (int j = tid; j < lt.B2; j += kLxNT) tn.Wl[tn.ol[b] + ((int64_t)fold * R + a) * lt.B2 + j] = lt.wL[j];
      }
      lx_kron(wk, wA, wB, P, B);
      double* oa = bl.b[b].Wa + ((int64_t)fold * R + a) * A;                         // (the last pass's loadings stay)
      double* ob = bl.b[b].Wb + ((int64_t)fold * R + a) * B;
      for (int j = tid; j < A; j += kLxNT) oa[j] = wA[j];
      for (int j = tid; j < B; j += kLxNT) ob[j] = wB[j];
      __syncthreads();
      lx_row_dots(S, wk, P, M, lane, wv, [tq](int m, double s) { tq[m] += s; });     // Y^T t_b = S_b w_b, added to 0.0 in block order
      __syncthreads();
      wk += P;
    }
    if (lx_q_step(tq, (double)nb, q, qn, Gy, M, tol, it, red)) { ++it; break; }     // t the blocks' average (cmtf.py:126-130)
  }
  bool bad = false;
  for (int m = tid; m < M; m += kLxNT) { bl.b[0].Q[((int64_t)fold * R + a) * M + m] = q[m]; bad |= !isfinite(q[m]); }
  if (tid == 0) bl.b[0].n_iter[fold * R + a] = it;
  double mw = 0.0;
  double* wk = wk0;
  for (int b = 0; b < nb; ++b) {                                                   // the MTTKRP operands and mu_b^T w_b
    const cmtfpls_kfold_state& v = bl.b[b];
    const int64_t P = (int64_t)v.A * v.B;
    const double* wa = v.Wa + ((int64_t)fold * R + a) * v.A;
    const double* wb = v.Wb + ((int64_t)fold * R + a) * v.B;
    for (int j = tid; j < v.A; j += kLxNT) { v.WA[(int64_t)j * K + fold] = wa[j]; bad |= !isfinite(wa[j]); }
    for (int j = tid; j < v.B; j += kLxNT) { v.WB[(int64_t)j * K + fold] = wb[j]; bad |= !isfinite(wb[j]); }
    const double* mean = v.mean + (int64_t)(GROUPED ? model_fold[fold] : fold) * P;
    double s = 0.0;
    for (int64_t c = tid; c < P; c += kLxNT) s = fma(mean[c], wk[c], s);
    mw += lx_sum(s, red);
    wk += P;
  }
  if (bad) atomicOr(bl.b[0].status + fold, 1);
  double* vec = bl.b[0].vec + (int64_t)fold * kf_vec_len(R, M);
  if (tid == 0) vec[3 * R + M + 1] = mw / (double)nb;
  for (int j = 0; j < a; ++j) {                                                    // g_j = mean over blocks of w_b,j^T w_b,a
    double g = 0.0;
    for (int b = 0; b < nb; ++b) {
      const cmtfpls_kfold_state& v = bl.b[b];
      const double* wa = v.Wa + (int64_t)fold * R * v.A;
      const double* wb = v.Wb + (int64_t)fold * R * v.B;
      double sa = 0.0, sb = 0.0;
      for (int i = tid; i < v.A; i += kLxNT) sa = fma(wa[(int64_t)j * v.A + i], wa[(int64_t)a * v.A + i], sa);
      for (int i = tid; i < v.B; i += kLxNT) sb = fma(wb[(int64_t)j * v.B + i], wb[(int64_t)a * v.B + i], sb);
      sa = lx_sum(sa, red);
      sb = lx_sum(sb, red);
      g += sa * sb;
    }
    if (tid == 0) vec[2 * R + M + 1 + j] = g / (double)nb;
  }
}

// out = (1/nb) sum_b sc[b] (n entries each), added in block order
__global__ __launch_bounds__(256) void kfold_combine_kernel(const double* __restrict__ sc, int nb, int64_t n, double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += sc[(int64_t)b * n + i];
    out[i] = s / (double)nb;
  }
}

// every view valid, inside the device form, and sharing every field that is not the block's own.  folds > 0 (the grouped entry):
// the K models hold out `folds` folds, so I >= folds is enough (every model of a fold shares its rows), as in kf_grouped_check
static int kf_blocks_check(const cmtfpls_kfold_state* v, int nb, const char* what, int folds = 0) {
  if (!v || nb < 1 || nb > kKfMaxBlocks) { set_error("kfold coupled: 1 <= nb <= 8 block views"); return CMTFPLS_EINVAL; }
  const cmtfpls_kfold_state& s = v[0];
  for (int b = 0; b < nb; ++b) {
    const cmtfpls_kfold_state& o = v[b];
    if (!kf_state_ok(&o) || o.I != s.I || o.M != s.M || o.K != s.K || o.R != s.R || o.fold_of != s.fold_of || o.Yk != s.Yk ||
        o.Gy != s.Gy || o.Q != s.Q || o.T != s.T || o.Gt != s.Gt || o.coef != s.coef || o.tm != s.tm || o.Tout != s.Tout ||
        o.vec != s.vec || o.n_iter != s.n_iter || o.status != s.status || o.part != s.part) {
      set_error(what);
      return CMTFPLS_EINVAL;
    }
    if ((folds && (folds < 2 || o.I < folds)) || !kf_shape_ok(folds && o.I < o.K ? o.K : o.I, o.A, o.B, o.M, o.K, o.R)) {
      set_error("kfold coupled: a block outside the device form (2 <= K <= 32, M <= 64, R <= 64, min(A, B) <= 256); refit per fold");
      return CMTFPLS_EUNSUPPORTED;
    }
  }
  return CMTFPLS_OK;
}

// ---- grouped models (permutation test, permutation.py) ---------------------------------------------------------------------
// A pass of the response-permutation test carries G permuted responses x K folds = n <= kKfMaxK models; model m = k G + p holds
// out fold k and is fitted to Y[pi_p].  X is never permuted, so every model reads the same X_0 and the models differ only in Y,
// in which rows train them and in their loadings:
//   kfold_wide      S_f = X[rows_f]^T Y' for every fold f from ONE pass over X, Y' = [Y[pi_1] - ybar, .., Y[pi_G] - ybar]
//                   (W = G M <= 1024 columns) on v_mfma_f64_16x16x4_f64; kfold_finish_kernel (the all-minus-own identity, column-
//                   block-wise) then gives model m's S as the m-th M x P block of K x W x P
//   the inner loop, the score pass, the epilogue and the contraction are those of the folds above with n columns; the grouped
//   instantiations (GROUPED = true) read which fold a model holds out from model_fold[m] and write its held-out scores to group
//   m % groups of Tout (groups x I x R)
// A coupled model (ctPLS, EngineOptions.coupled_permutations) runs the same pass on a state view per block: kfold_wide per block
// into that view's S and per-fold mean, kfold_inner_coupled_kernel<true> (model m reads row model_fold[m] of every view's mean),
// the score pass per block and kfold_combine, stage 1 on the first view, the contraction and the grouped stage 2 per view.
constexpr int kKfWideMaxW = 1024, kKfWideCols = 256, kKfWideUn = 4;


struct KfWidePlan {
  int nyb, mt, nch;                  // column blocks of Y' (16 mt columns each), row chunks per fold
};

// Y' column blocks of <= 64 columns (MT <= 4 MFMA tiles per wavefront, so the accumulators stay in registers); row chunks per
// fold so that the grid has >= ~2048 workgroups; <= 16
static KfWidePlan kf_wide_plan(int64_t I, int64_t P, int W, int K) {
  KfWidePlan p;
  p.nyb = (W + 63) / 64;
  p.mt = (W + 16 * p.nyb - 1) / (16 * p.nyb);
  const int64_t ct = (P + kKfWideCols - 1) / kKfWideCols;
  int64_t ch = (2048 + ct * p.nyb * K - 1) / (ct * p.nyb * K);
  const int64_t per_fold = I / K;
  if (ch > per_fold / 64) ch = per_fold / 64;
  if (ch > 16) ch = 16;
  p.nch = ch < 1 ? 1 : (int)ch;
  return p;
}

// grid (column tiles x Y' blocks, folds x row chunks): a wavefront owns 64 columns of X (4 consecutive per lane) and 16 MT columns
// of Y', and goes through its chunk's rows in the host's fold-sorted order, four rows per MFMA (tile mapping of xcov.hip):
//   A = Y'[row(kq)][y0 + 16 mt + nn], B of MFMA e = X[row(kq)][c + e], D tile e register g = S[y0 + 16 mt + kq + 4 g][c + e].
// The Y' blocks of one column tile are neighbours in the launch order, so X streams from HBM once and the other blocks meet it in
// the caches.  The first Y' block also sums every column and its squares (the fold's partial column sums: the training means
// and the NaN / offset statistics).  Partials (W + 2 rows per chunk) go to `part` in the layout of kfold_partials_kernel; every
// sum runs in a fixed order, so the result is the same bits on every run.
template <typename T, int MT, bool VEC>
__global__ __launch_bounds__(kKfWideCols) void kfold_wide_kernel(const T* __restrict__ X, int64_t P, const double* __restrict__ Y, int W,
                                                                 const int* __restrict__ order, const int* __restrict__ off, int nyb,
                                                                 int nch, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, kq = lane >> 4, nn = lane & 15;
  const int yb = (int)(blockIdx.x % (unsigned)nyb);
  const int64_t ct = blockIdx.x / (unsigned)nyb;
  const int k = (int)blockIdx.y / nch, ch = (int)blockIdx.y % nch;
  const int64_t cb = (ct * 4 + wv) * 64;
  if (cb >= P) return;                                         // whole wavefront past the last column
  const int64_t c = cb + 4 * nn;
  const int lo0 = off[k], n = off[k + 1] - lo0, len = (n + nch - 1) / nch;
  const int lo = lo0 + min(n, ch * len), hi = lo0 + min(n, (ch + 1) * len);
  const int y0 = yb * 16 * MT;
  using XV = Pack<T, 4>;
  lx_d4_t acc[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[mt][e] = lx_d4_t{0.0, 0.0, 0.0, 0.0};
  bool mok[MT], cok[4];
  int ycol[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    mok[mt] = y0 + 16 * mt + nn < W;
    ycol[mt] = mok[mt] ? y0 + 16 * mt + nn : W - 1;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) cok[e] = c + e < P;
  const int64_t cc = (c < P) ? c : (VEC ? P - 4 : P - 1);     // (VEC: P % 4 == 0, so c < P means c + 3 < P)
  double cs[4] = {0.0, 0.0, 0.0, 0.0}, cq[4] = {0.0, 0.0, 0.0, 0.0};
  // loads are unconditional (clamped row and column) and masked in the MFMAs
  for (int r = lo; r < hi; r += 4 * kKfWideUn) {
    XV x[kKfWideUn];
    double a[kKfWideUn][MT];
#pragma unroll
    for (int s = 0; s < kKfWideUn; ++s) {
      const int pos = r + 4 * s + kq;
      const int64_t i = order[pos < hi ? pos : hi - 1];
      if (VEC) {
        x[s] = *reinterpret_cast<const XV*>(X + i * P + cc);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[s].e[e] = X[i * P + (cok[e] ? c + e : P - 1)];
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[s][mt] = Y[i * W + ycol[mt]];
    }
#pragma unroll
    for (int s = 0; s < kKfWideUn; ++s) {
      const bool rok = r + 4 * s + kq < hi;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double b = (rok && cok[e]) ? to_f64(x[s].e[e]) : 0.0;
        cs[e] += b;
        cq[e] = fma(b, b, cq[e]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[mt][e] = __builtin_amdgcn_mfma_f64_16x16x4f64((rok && mok[mt]) ? a[s][mt] : 0.0, b, acc[mt][e], 0, 0, 0);
      }
    }
  }
  double* base = part + (int64_t)(k * nch + ch) * (W + 2) * P;
  if (yb == 0) {                                               // the four lane groups hold the same columns for different rows
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double v = cs[e], w = cq[e];
      v += __shfl_xor(v, 16, kWave);
      v += __shfl_xor(v, 32, kWave);
      w += __shfl_xor(w, 16, kWave);
      w += __shfl_xor(w, 32, kWave);
      if (kq == 0 && cok[e]) { base[(int64_t)W * P + c + e] = v; base[(int64_t)(W + 1) * P + c + e] = w; }
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int j = y0 + 16 * mt + kq + 4 * g;
      if (j < W) {
        double* dst = base + (int64_t)j * P + c;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (cok[e]) dst[e] = acc[mt][e][g];
      }
    }
}

template <typename T, int MT>
static void kf_wide_launch(dim3 g, hipStream_t st, const T* X, int64_t P, const double* Y, int W, const int* order, const int* off,
                           int nyb, int nch, double* part) {
  // VEC reads X + i P + c as a Pack<T, 4>: every row start is aligned only when P % 4 == 0 and X itself is (a view into a larger
  // buffer need not be).  16-bit storage: the lane's 4 columns are one 8-byte load, so the base must be 8-byte aligned; a base that
  // is only 2-byte aligned takes the scalar path, whose indices are clamped into the row
  if (P % 4 == 0 && reinterpret_cast<uintptr_t>(X) % sizeof(Pack<T, 4>) == 0)
    hipLaunchKernelGGL((kfold_wide_kernel<T, MT, true>), g, dim3(kKfWideCols), 0, st, X, P, Y, W, order, off, nyb, nch, part);
  else
    hipLaunchKernelGGL((kfold_wide_kernel<T, MT, false>), g, dim3(kKfWideCols), 0, st, X, P, Y, W, order, off, nyb, nch, part);
}

// the MT (MFMA tiles per wavefront) instance of the plan
template <typename T>
static void kf_wide_dispatch(const KfWidePlan& pl, dim3 g, hipStream_t st, const T* X, int64_t P, const double* Y, int W, const int* order,
                             const int* off, double* part) {
  switch (pl.mt) {
    case 1: kf_wide_launch<T, 1>(g, st, X, P, Y, W, order, off, pl.nyb, pl.nch, part); break;
    case 2: kf_wide_launch<T, 2>(g, st, X, P, Y, W, order, off, pl.nyb, pl.nch, part); break;
    case 3: kf_wide_launch<T, 3>(g, st, X, P, Y, W, order, off, pl.nyb, pl.nch, part); break;
    default: kf_wide_launch<T, 4>(g, st, X, P, Y, W, order, off, pl.nyb, pl.nch, part); break;
  }
}

template <typename T>
static int run_kfold_wide(const T* X, int64_t I, int A, int B, const double* Y, int W, const int* order, const int* fold_off, int K,
                          const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!X || !Y || !order || !fold_off || !ydev || !S || !mean || !stats || I <= 0 || A <= 0 || B <= 0 || W <= 0 || K <= 0) {
    set_error("kfold_wide_xcov: bad argument");
    return CMTFPLS_EINVAL;
  }
  const int64_t P = (int64_t)A * B;
  if (K < 2 || K > kKfMaxK || W > kKfWideMaxW || I < K || I > (int64_t)1 << 30 || P > (int64_t)1 << 24) {
    set_error("kfold_wide_xcov: shape outside the device form (2 <= K <= 32, W <= 1024, A * B <= 2^24)");
    return CMTFPLS_EUNSUPPORTED;
  }
  const size_t need = cmtfpls_kfold_wide_xcov_workspace_bytes(I, P, W, K);
  if (!ws || ws_bytes < need) { set_error("kfold_wide_xcov: workspace too small"); return CMTFPLS_EWORKSPACE; }
  const KfWidePlan pl = kf_wide_plan(I, P, W, K);
  double* part = static_cast<double*>(ws);
  const int64_t ct = (P + kKfWideCols - 1) / kKfWideCols;
  const dim3 g((unsigned)(ct * pl.nyb), (unsigned)(K * pl.nch));
  kf_wide_dispatch<T>(pl, g, st, X, P, Y, W, order, fold_off, part);
  int rc = check_launch("kfold_wide_xcov");
  if (rc) return rc;
  hipLaunchKernelGGL(kfold_finish_kernel, dim3((unsigned)((P + kKfCols - 1) / kKfCols)), dim3(kKfCols), 0, st, P, W, K, pl.nch, (int)I,
                     fold_off, part, ydev, S, mean, stats);
  return check_launch("kfold_wide_xcov");
}

// the grouped entries: n = st->K models in `groups` groups, model m holding out fold model_fold[m] < n / groups (the folds of
// st->mean); I >= the number of folds (every model of a fold shares its rows)
static int kf_grouped_check(const cmtfpls_kfold_state* st, const int* model_fold, int groups, int a, const char* what) {
  if (!kf_state_ok(st) || !model_fold || groups < 1 || st->K % groups != 0 || a < 0 || a >= st->R) {
    set_error(what);
    return CMTFPLS_EINVAL;
  }
  const int folds = st->K / groups;
  if (folds < 2 || st->I < folds || !kf_shape_ok(st->I < st->K ? st->K : st->I, st->A, st->B, st->M, st->K, st->R)) {
    set_error("kfold grouped: shape outside the device form (n <= 32 models, M <= 64, R <= 64, min(A, B) <= 256); refit");
    return CMTFPLS_EUNSUPPORTED;
  }
  return CMTFPLS_OK;
}

// the launch of the inner entries (plain, grouped, order 4), after their argument checks; tn: KfTensor{} unless TENSOR
template <bool GROUPED, bool TENSOR>
static int kf_inner_launch(const cmtfpls_kfold_state* st, const int* model_fold, const KfTensor& tn, int a, double tol, int max_iter,
                           void* ws, size_t ws_bytes, hipStream_t s) {
  const size_t need = TENSOR ? cmtfpls_kfold_inner_tensor_workspace_bytes(st->A, tn.B1, tn.B2, st->K)
                             : cmtfpls_kfold_inner_workspace_bytes(st->A, st->B, st->K);
  if (!ws || ws_bytes < need) {                                   // behaviour: the order-4 entry's texts have no grouped variant
    set_error(TENSOR ? "kfold_inner_tensor: workspace too small"
                     : GROUPED ? "kfold_inner_grouped: workspace too small" : "kfold_inner: workspace too small");
    return CMTFPLS_EWORKSPACE;
  }
  const size_t lds = TENSOR ? kf_inner_tensor_lds_bytes(st->A, tn.B1, tn.B2, st->M) : kf_inner_lds_bytes(st->A, st->B, st->M);
  const int64_t per = TENSOR ? kf_inner_tensor_ws_per_fold(st->A, tn.B1, tn.B2) : (int64_t)(need / st->K / sizeof(double));
  const auto kernel = kfold_inner_kernel<GROUPED, TENSOR>;
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3(st->K), dim3(kLxNT), lds, s, *st, a, tol, max_iter, static_cast<double*>(ws), per, model_fold, tn);
  return check_launch(TENSOR ? "kfold_inner_tensor" : GROUPED ? "kfold_inner_grouped" : "kfold_inner");
}

static KfBlocks kf_blocks_of(const cmtfpls_kfold_state* blocks, int nb) {
  KfBlocks bl;
  for (int b = 0; b < kKfMaxBlocks; ++b) bl.b[b] = blocks[b < nb ? b : 0];
  bl.nb = nb;
  return bl;
}

// the launch of the coupled inner entries (plain, grouped, blocks of order 4), after their argument checks; o: kf_coupled_dims in
// o.d and nothing else unless TENSOR (then kf_coupled_tensor_dims with the outputs Wk, Wl in o.tn)
template <bool GROUPED, bool TENSOR>
static int kf_inner_coupled_launch(const cmtfpls_kfold_state* blocks, int nb, const int* model_fold, const KfCoupledTensorDims& o, int a,
                                   double tol, int max_iter, void* ws, size_t ws_bytes, hipStream_t s) {
  const size_t lds = TENSOR ? kf_coupled_tensor_lds_bytes(o, blocks[0].M) : kf_coupled_lds_bytes(o.d, blocks[0].M);
  if (!TENSOR && lds > 150 * 1024) {                              // behaviour: the order-4 entry checks the LDS before it comes here
    set_error(GROUPED ? "kfold_inner_coupled_grouped: the blocks' vectors exceed the LDS of one workgroup; refit per fold"
                      : "kfold_inner_coupled: the blocks' vectors exceed the LDS of one workgroup; refit per fold");
    return CMTFPLS_EUNSUPPORTED;
  }
  const size_t need = TENSOR ? (size_t)blocks[0].K * (size_t)kf_coupled_tensor_ws_per_fold(o) * sizeof(double)
                             : cmtfpls_kfold_inner_coupled_workspace_bytes(blocks, nb);
  if (!ws || ws_bytes < need) {                                   // behaviour: the order-4 entry's texts have no grouped variant
    set_error(TENSOR ? "kfold_inner_coupled_tensor: workspace too small"
                     : GROUPED ? "kfold_inner_coupled_grouped: workspace too small" : "kfold_inner_coupled: workspace too small");
    return CMTFPLS_EWORKSPACE;
  }
  const auto kernel = kfold_inner_coupled_kernel<GROUPED, TENSOR>;
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3(blocks[0].K), dim3(kLxNT), lds, s, kf_blocks_of(blocks, nb), a, tol, max_iter, static_cast<double*>(ws),
                     kf_coupled_tensor_ws_per_fold(o), o.d.pmax, o.d.nmax, o.d.amax, o.d.bmax, model_fold, o.tn);   // (3 ptmax = 0 unless TENSOR)
  return check_launch(TENSOR ? "kfold_inner_coupled_tensor" : GROUPED ? "kfold_inner_coupled_grouped" : "kfold_inner_coupled");
}

// the argument test of the epilogue entries
static bool kf_epilogue_args_ok(const cmtfpls_kfold_state* st, int stage, int a, const double* in) {
  return kf_state_ok(st) && stage >= 0 && stage <= 2 && a >= 0 && a < st->R && (stage == 0 || in);
}

// the stage switch of the three epilogue entries, after their argument checks: stage 0 the Y-side Gram, stage 1 the row work, the
// solve and (but for the last component) the Y deflation, stage 2 the down-date of S.  kKfGrouped: model_fold and its `groups`;
// kKfSplits: `groups` is the folds per split; kKfPlain: model_fold null, groups 1
template <int MODE>
static int kf_epilogue_launch(const cmtfpls_kfold_state* st, const int* model_fold, int groups, int stage, int a, const double* in,
                              hipStream_t s, const char* what) {
  const dim3 rows((unsigned)kf_tiles(st->I), (unsigned)st->K);
  const int folds = MODE == kKfSplits ? groups : 1;
  if (stage == 0) {
    hipLaunchKernelGGL(kfold_ydefl_kernel<MODE>, rows, dim3(kKfRowThreads), 0, s, *st, a, 0, model_fold, folds);
  } else if (stage == 1) {
    hipLaunchKernelGGL(kfold_rows_kernel<MODE>, rows, dim3(kKfRowThreads), 0, s, *st, a, in, model_fold, groups);
    hipLaunchKernelGGL(kfold_solve_kernel, dim3(st->K), dim3(64), 0, s, *st, a);
    if (a + 1 < st->R) hipLaunchKernelGGL(kfold_ydefl_kernel<MODE>, rows, dim3(kKfRowThreads), 0, s, *st, a, 1, model_fold, folds);
  } else {
    const int64_t P = (int64_t)st->A * st->B;
    hipLaunchKernelGGL(kfold_downdate_kernel<MODE == kKfGrouped>, dim3((unsigned)((P + kKfCols - 1) / kKfCols), (unsigned)st->K),
                       dim3(kKfCols), 0, s, *st, a, in, model_fold);
  }
  return check_launch(what);
}

// ---- split-major models (repeated K-fold, repeated.py) ----------------------------------------------------------------------
// A pass of repeated K-fold carries G shuffled splits x K folds = n <= kKfMaxK models; model m = g K + k holds out fold k of split
// g.  Each split's S, mean and Y side are a contiguous K-model slice of the state, built per split by kfold_xcov; the inner loop
// (kfold_inner, or kfold_inner_coupled on block views), the score pass, the contraction and stages 0 and 2 are those of the folds
// above with n columns.  Only stage 1 differs (kKfSplits instantiations of kfold_rows_kernel / kfold_ydefl_kernel): fold_of is
// splits x I, model m reads row m / K of it, and its held-out scores go to slot m / K of Tout (splits x I x R).  The splits are
// partitions of the rows, so every row of every slot is written exactly once.

// ---- weighted models (bootstrap, bootstrap.py) -----------------------------------------------------------------------------
// A bootstrap resample differs from the fitted data only in each row's multiplicity c_i (0, 1, 2, ..): the refit on the resampled
// rows is the fit in which every sum over rows is weighted by c.  A pass carries n <= 32 resamples as models of one state; its
// fold_of is n x I counts.  Per pass:
//   kfold_weighted  every model's S_b = X_0^T (c_b * (Y - nu_b)) and mu_b = X_0^T c_b / I from ONE pass over X: kfold_wide_kernel
//                   over Y'' = [c_1 * (Y - nu_1) .. c_n * (Y - nu_n) | c_1 .. c_n] (W = n (M + 1) <= 1024 columns) with all rows
//                   as one fold, then the chunks' partials added in chunk order.  (sum_i c_i (Y_i - nu_b) = 0, so S_b is the
//                   centred cross-covariance of the resample.)  Also the column sums / sums of squares of all rows, unweighted
//   the inner loop, the score pass, the contraction and stage 2 are those of the folds above with n columns; stages 0 and 1 are
//   the kKfWeighted instantiations of kfold_ydefl_kernel / kfold_rows_kernel
// identity row order and one fold of all rows for kfold_wide_kernel
__global__ __launch_bounds__(256) void kfold_iota_kernel(int* __restrict__ order, int I, int* __restrict__ off) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < I; i += gridDim.x * 256) order[i] = i;
  if (blockIdx.x == 0 && threadIdx.x == 0) { off[0] = 0; off[1] = I; }
}

// a thread per column: S (n x M x P) = the first n M columns of Y'', mean (n x P) = the count columns / I, stats (2 P)
__global__ __launch_bounds__(kKfCols) void kfold_weighted_finish_kernel(int64_t P, int n, int M, int nch, int I,
                                                                        const double* __restrict__ part, double* __restrict__ S,
                                                                        double* __restrict__ mean, double* __restrict__ stats) {
  const int64_t c = (int64_t)blockIdx.x * kKfCols + threadIdx.x;
  if (c >= P) return;
  const int W = n * (M + 1);
  auto sum = [&](int j) {
    double s = 0.0;
    for (int ch = 0; ch < nch; ++ch) s += part[((int64_t)ch * (W + 2) + j) * P + c];
    return s;
  };
  stats[c] = sum(W);
  stats[P + c] = sum(W + 1);
  for (int b = 0; b < n; ++b) mean[(int64_t)b * P + c] = sum(n * M + b) / (double)I;
  for (int j = 0; j < n * M; ++j) S[(int64_t)j * P + c] = sum(j);
}

static size_t kf_weighted_part_bytes(int64_t I, int64_t P, int W) {
  return (size_t)kf_wide_plan(I, P, W, 1).nch * (size_t)(W + 2) * (size_t)P * sizeof(double);
}

template <typename T>
static int run_kfold_weighted(const T* X, int64_t I, int A, int B, const double* Y, int n, int M, double* S, double* mean,
                              double* stats, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!X || !Y || !S || !mean || !stats || I <= 0 || A <= 0 || B <= 0 || n <= 0 || M <= 0) {
    set_error("kfold_weighted_xcov: bad argument");
    return CMTFPLS_EINVAL;
  }
  const int64_t P = (int64_t)A * B;
  const int W = n * (M + 1);
  if (n > kKfMaxK || M > kKfMaxM || W > kKfWideMaxW || I > (int64_t)1 << 30 || P > (int64_t)1 << 24) {
    set_error("kfold_weighted_xcov: shape outside the device form (n <= 32, M <= 64, n (M + 1) <= 1024, A * B <= 2^24)");
    return CMTFPLS_EUNSUPPORTED;
  }
  const size_t need = cmtfpls_kfold_weighted_xcov_workspace_bytes(I, P, n, M);
  if (!ws || ws_bytes < need) { set_error("kfold_weighted_xcov: workspace too small"); return CMTFPLS_EWORKSPACE; }
  const KfWidePlan pl = kf_wide_plan(I, P, W, 1);
  double* part = static_cast<double*>(ws);
  int* order = reinterpret_cast<int*>(static_cast<char*>(ws) + kf_weighted_part_bytes(I, P, W));
  int* off = order + I;
  int64_t gi = (I + 255) / 256;
  if (gi > 4096) gi = 4096;
  hipLaunchKernelGGL(kfold_iota_kernel, dim3((unsigned)gi), dim3(256), 0, st, order, (int)I, off);
  int rc = check_launch("kfold_weighted_xcov");
  if (rc) return rc;
  const int64_t ct = (P + kKfWideCols - 1) / kKfWideCols;
  const dim3 g((unsigned)(ct * pl.nyb), (unsigned)pl.nch);
  kf_wide_dispatch<T>(pl, g, st, X, P, Y, W, order, off, part);
  rc = check_launch("kfold_weighted_xcov");
  if (rc) return rc;
  hipLaunchKernelGGL(kfold_weighted_finish_kernel, dim3((unsigned)((P + kKfCols - 1) / kKfCols)), dim3(kKfCols), 0, st, P, n, M,
                     pl.nch, (int)I, part, S, mean, stats);
  return check_launch("kfold_weighted_xcov");
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {

size_t cmtfpls_kfold_xcov_workspace_bytes(int64_t I, int64_t P, int M, int K) {
  if (I <= 0 || P <= 0 || M <= 0 || K <= 0) return 0;
  return (size_t)K * kf_chunks(I, P, K) * (size_t)(M + 2) * (size_t)P * sizeof(double);
}

int cmtfpls_kfold_xcov_f32(const float* X, int64_t I, int A, int B, const double* Y, int M, const int* order, const int* fold_off, int K,
                           const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream) {
  return run_kfold_xcov<float>(X, I, A, B, Y, M, order, fold_off, K, ydev, S, mean, stats, ws, ws_bytes, (hipStream_t)stream);
}

int cmtfpls_kfold_xcov_f64(const double* X, int64_t I, int A, int B, const double* Y, int M, const int* order, const int* fold_off, int K,
                           const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream) {
  return run_kfold_xcov<double>(X, I, A, B, Y, M, order, fold_off, K, ydev, S, mean, stats, ws, ws_bytes, (hipStream_t)stream);
}

int cmtfpls_kfold_xcov_bf16(const uint16_t* X, int64_t I, int A, int B, const double* Y, int M, const int* order, const int* fold_off, int K,
                            const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream) {
  return run_kfold_xcov<bf16_t>(reinterpret_cast<const bf16_t*>(X), I, A, B, Y, M, order, fold_off, K, ydev, S, mean, stats, ws, ws_bytes,
                                (hipStream_t)stream);
}

int cmtfpls_kfold_xcov_f16(const uint16_t* X, int64_t I, int A, int B, const double* Y, int M, const int* order, const int* fold_off, int K,
                           const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream) {
  return run_kfold_xcov<f16_t>(reinterpret_cast<const f16_t*>(X), I, A, B, Y, M, order, fold_off, K, ydev, S, mean, stats, ws, ws_bytes,
                               (hipStream_t)stream);
}

int cmtfpls_kfold_row_tiles(int64_t I) { return I > 0 ? kf_tiles(I) : 0; }

int cmtfpls_kfold_part_stride(void) { return 2 * kKfMaxR + 1 + kKfMaxM; }

size_t cmtfpls_kfold_inner_workspace_bytes(int A, int B, int K) {
  if (A <= 0 || B <= 0 || K <= 0) return 0;
  const size_t P = (size_t)A * B, n = (size_t)(A < B ? A : B);
  return (size_t)K * (3 * P + 2 * n * n) * sizeof(double);
}

int cmtfpls_kfold_inner_f64(const cmtfpls_kfold_state* st, int a, double tol, int max_iter, void* ws, size_t ws_bytes, void* stream) {
  if (!kf_state_ok(st) || a < 0 || a >= st->R || max_iter <= 0) { set_error("kfold_inner: bad argument"); return CMTFPLS_EINVAL; }
  if (!kf_shape_ok(st->I, st->A, st->B, st->M, st->K, st->R)) {
    set_error("kfold_inner: shape outside the device form (2 <= K <= 32, M <= 64, R <= 64, min(A, B) <= 256); refit per fold");
    return CMTFPLS_EUNSUPPORTED;
  }
  return kf_inner_launch<false, false>(st, nullptr, KfTensor{}, a, tol, max_iter, ws, ws_bytes, (hipStream_t)stream);
}

size_t cmtfpls_kfold_inner_tensor_workspace_bytes(int A, int B1, int B2, int K) {
  if (A <= 0 || B1 <= 0 || B2 <= 0 || K <= 0 || (int64_t)A * B1 * B2 > (int64_t)1 << 24) return 0;
  return (size_t)K * (size_t)kf_inner_tensor_ws_per_fold(A, B1, B2) * sizeof(double);
}

size_t cmtfpls_kfold_inner_tensor_lds_bytes(int A, int B1, int B2, int M) {
  if (A <= 0 || B1 <= 0 || B2 <= 0 || M <= 0) return 0;
  return kf_inner_tensor_lds_bytes(A, B1, B2, M);
}

int cmtfpls_kfold_inner_tensor_f64(const cmtfpls_kfold_state* st, const int* model_fold, int groups, int B1, int B2, int a, double tol,
                                   int max_iter, double* Wk, double* Wl, void* ws, size_t ws_bytes, void* stream) {
  if (!kf_state_ok(st) || B1 <= 0 || B2 <= 0 || (int64_t)B1 * B2 != st->B || a < 0 || a >= st->R || max_iter <= 0 || groups < 1 ||
      (!model_fold && groups != 1)) {
    set_error("kfold_inner_tensor: bad argument (B1 * B2 == st->B; model_fold NULL with groups == 1, or the grouped layout)");
    return CMTFPLS_EINVAL;
  }
  for (int m = 0; m < 3; ++m)
    if (lx_tensor_short(st->A, B1, B2, m) > kLxMaxN) {
      set_error("kfold_inner_tensor: an unfolding of A x B1 x B2 with its shorter side > 256; refit per fold");
      return CMTFPLS_EUNSUPPORTED;
    }
  if (model_fold) {
    const int rc = kf_grouped_check(st, model_fold, groups, a, "kfold_inner_tensor: bad argument");
    if (rc) return rc;
  } else if (!kf_shape_ok(st->I, st->A, st->B, st->M, st->K, st->R)) {
    set_error("kfold_inner_tensor: shape outside the device form (2 <= K <= 32, M <= 64, R <= 64, min(A, B1 B2) <= 256); refit per fold");
    return CMTFPLS_EUNSUPPORTED;
  }
  if (kf_inner_tensor_lds_bytes(st->A, B1, B2, st->M) > 150 * 1024) {
    set_error("kfold_inner_tensor: the fold's vectors exceed the LDS of one workgroup; refit per fold");
    return CMTFPLS_EUNSUPPORTED;
  }
  const KfTensor tn{B1, B2, lx_tensor_nmax(st->A, B1, B2), Wk, Wl};
  if (model_fold) return kf_inner_launch<true, true>(st, model_fold, tn, a, tol, max_iter, ws, ws_bytes, (hipStream_t)stream);
  return kf_inner_launch<false, true>(st, nullptr, tn, a, tol, max_iter, ws, ws_bytes, (hipStream_t)stream);
}

int cmtfpls_kfold_epilogue_f64(const cmtfpls_kfold_state* st, int stage, int a, const double* in, void* stream) {
  if (!kf_epilogue_args_ok(st, stage, a, in)) {
    set_error("kfold_epilogue: bad argument");
    return CMTFPLS_EINVAL;
  }
  if (!kf_shape_ok(st->I, st->A, st->B, st->M, st->K, st->R)) {
    set_error("kfold_epilogue: shape outside the device form; refit per fold");
    return CMTFPLS_EUNSUPPORTED;
  }
  return kf_epilogue_launch<kKfPlain>(st, nullptr, 1, stage, a, in, (hipStream_t)stream, "kfold_epilogue");
}

size_t cmtfpls_kfold_inner_coupled_workspace_bytes(const cmtfpls_kfold_state* blocks, int nb) {
  if (!blocks || nb < 1 || nb > kKfMaxBlocks || blocks[0].K <= 0) return 0;
  for (int b = 0; b < nb; ++b)
    if (blocks[b].A <= 0 || blocks[b].B <= 0) return 0;
  return (size_t)blocks[0].K * (size_t)kf_coupled_ws_per_fold(kf_coupled_dims(blocks, nb)) * sizeof(double);
}

int cmtfpls_kfold_inner_coupled_f64(const cmtfpls_kfold_state* blocks, int nb, int a, double tol, int max_iter, void* ws, size_t ws_bytes,
                                    void* stream) {
  int rc = kf_blocks_check(blocks, nb, "kfold_inner_coupled: bad block views (the shared fields must be the same in every view)");
  if (rc) return rc;
  if (a < 0 || a >= blocks[0].R || max_iter <= 0) { set_error("kfold_inner_coupled: bad argument"); return CMTFPLS_EINVAL; }
  KfCoupledTensorDims o{};
  o.d = kf_coupled_dims(blocks, nb);
  return kf_inner_coupled_launch<false, false>(blocks, nb, nullptr, o, a, tol, max_iter, ws, ws_bytes, (hipStream_t)stream);
}

// dims: (B1_b, B2_b) per block, (0, 0) for a matrix block, B_b = B1_b B2_b for a tensor block
static bool kf_coupled_tensor_dims_ok(const cmtfpls_kfold_state* blocks, int nb, const int* dims) {
  if (!blocks || nb < 1 || nb > kKfMaxBlocks || !dims) return false;
  for (int b = 0; b < nb; ++b) {
    const int B1 = dims[2 * b], B2 = dims[2 * b + 1];
    if (B1 == 0 && B2 == 0) continue;
    if (B1 <= 0 || B2 <= 0 || (int64_t)B1 * B2 != blocks[b].B) return false;
  }
  return true;
}

size_t cmtfpls_kfold_inner_coupled_tensor_workspace_bytes(const cmtfpls_kfold_state* blocks, int nb, const int* dims) {
  if (!kf_coupled_tensor_dims_ok(blocks, nb, dims) || blocks[0].K <= 0 || blocks[0].R <= 0) return 0;
  for (int b = 0; b < nb; ++b)
    if (blocks[b].A <= 0 || blocks[b].B <= 0 || (int64_t)blocks[b].A * blocks[b].B > (int64_t)1 << 24) return 0;
  return (size_t)blocks[0].K * (size_t)kf_coupled_tensor_ws_per_fold(kf_coupled_tensor_dims(blocks, nb, dims)) * sizeof(double);
}

size_t cmtfpls_kfold_inner_coupled_tensor_lds_bytes(const cmtfpls_kfold_state* blocks, int nb, const int* dims) {
  if (!kf_coupled_tensor_dims_ok(blocks, nb, dims) || blocks[0].M <= 0) return 0;
  for (int b = 0; b < nb; ++b)
    if (blocks[b].A <= 0 || blocks[b].B <= 0) return 0;
  return kf_coupled_tensor_lds_bytes(kf_coupled_tensor_dims(blocks, nb, dims), blocks[0].M);
}

int cmtfpls_kfold_inner_coupled_tensor_f64(const cmtfpls_kfold_state* blocks, int nb, const int* dims, const int* model_fold, int groups,
                                           int a, double tol, int max_iter, double* Wk, double* Wl, void* ws, size_t ws_bytes,
                                           void* stream) {
  if (!kf_coupled_tensor_dims_ok(blocks, nb, dims) || groups < 1 || (!model_fold && groups != 1)) {   // before any pointer is looked at
    set_error("kfold_inner_coupled_tensor: bad argument (1 <= nb <= 8 block views; dims (B1, B2) per block with B1 * B2 == B, or "
              "(0, 0) for a matrix block; model_fold NULL with groups == 1, or the grouped layout)");
    return CMTFPLS_EINVAL;
  }
  if ((model_fold && blocks[0].K % groups != 0) || a < 0 || a >= blocks[0].R || max_iter <= 0) {
    set_error("kfold_inner_coupled_tensor: bad argument");
    return CMTFPLS_EINVAL;
  }
  int rc = kf_blocks_check(blocks, nb, "kfold_inner_coupled_tensor: bad block views (the shared fields must be the same in every view)",
                           model_fold ? blocks[0].K / groups : 0);
  if (rc) return rc;
  for (int b = 0; b < nb; ++b)
    for (int m = 0; m < 3 && dims[2 * b + 1] > 0; ++m)
      if (lx_tensor_short(blocks[b].A, dims[2 * b], dims[2 * b + 1], m) > kLxMaxN) {
        set_error("kfold_inner_coupled_tensor: an unfolding of a block's A x B1 x B2 with its shorter side > 256; refit per fold");
        return CMTFPLS_EUNSUPPORTED;
      }
  KfCoupledTensorDims o = kf_coupled_tensor_dims(blocks, nb, dims);
  if (kf_coupled_tensor_lds_bytes(o, blocks[0].M) > 150 * 1024) {         // behaviour: checked here, ahead of the launch helper
    set_error("kfold_inner_coupled_tensor: the blocks' vectors exceed the LDS of one workgroup; refit per fold");
    return CMTFPLS_EUNSUPPORTED;
  }
  o.tn.Wk = Wk;
  o.tn.Wl = Wl;
  if (model_fold) return kf_inner_coupled_launch<true, true>(blocks, nb, model_fold, o, a, tol, max_iter, ws, ws_bytes, (hipStream_t)stream);
  return kf_inner_coupled_launch<false, true>(blocks, nb, nullptr, o, a, tol, max_iter, ws, ws_bytes, (hipStream_t)stream);
}

int cmtfpls_kfold_combine_scores_f64(const double* sc, int nb, int64_t n, double* out, void* stream) {
  if (!sc || !out || nb < 1 || nb > kKfMaxBlocks || n <= 0) { set_error("kfold_combine_scores: bad argument"); return CMTFPLS_EINVAL; }
  int64_t g = (n + 255) / 256;
  if (g > 65536) g = 65536;
  hipLaunchKernelGGL(kfold_combine_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, sc, nb, n, out);
  return check_launch("kfold_combine_scores");
}

size_t cmtfpls_kfold_wide_xcov_workspace_bytes(int64_t I, int64_t P, int W, int K) {
  if (I <= 0 || P <= 0 || W <= 0 || K <= 0) return 0;
  return (size_t)K * kf_wide_plan(I, P, W, K).nch * (size_t)(W + 2) * (size_t)P * sizeof(double);
}

int cmtfpls_kfold_wide_xcov_f32(const float* X, int64_t I, int A, int B, const double* Y, int W, const int* order, const int* fold_off,
                                int K, const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream) {
  return run_kfold_wide<float>(X, I, A, B, Y, W, order, fold_off, K, ydev, S, mean, stats, ws, ws_bytes, (hipStream_t)stream);
}

int cmtfpls_kfold_wide_xcov_f64(const double* X, int64_t I, int A, int B, const double* Y, int W, const int* order, const int* fold_off,
                                int K, const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream) {
  return run_kfold_wide<double>(X, I, A, B, Y, W, order, fold_off, K, ydev, S, mean, stats, ws, ws_bytes, (hipStream_t)stream);
}

int cmtfpls_kfold_wide_xcov_bf16(const uint16_t* X, int64_t I, int A, int B, const double* Y, int W, const int* order, const int* fold_off,
                                 int K, const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream) {
  return run_kfold_wide<bf16_t>(reinterpret_cast<const bf16_t*>(X), I, A, B, Y, W, order, fold_off, K, ydev, S, mean, stats, ws, ws_bytes,
                                (hipStream_t)stream);
}

int cmtfpls_kfold_wide_xcov_f16(const uint16_t* X, int64_t I, int A, int B, const double* Y, int W, const int* order, const int* fold_off,
                                int K, const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream) {
  return run_kfold_wide<f16_t>(reinterpret_cast<const f16_t*>(X), I, A, B, Y, W, order, fold_off, K, ydev, S, mean, stats, ws, ws_bytes,
                               (hipStream_t)stream);
}

int cmtfpls_kfold_inner_grouped_f64(const cmtfpls_kfold_state* st, const int* model_fold, int groups, int a, double tol, int max_iter,
                                    void* ws, size_t ws_bytes, void* stream) {
  int rc = kf_grouped_check(st, model_fold, groups, a, "kfold_inner_grouped: bad argument");
  if (rc) return rc;
  if (max_iter <= 0) { set_error("kfold_inner_grouped: bad argument"); return CMTFPLS_EINVAL; }
  return kf_inner_launch<true, false>(st, model_fold, KfTensor{}, a, tol, max_iter, ws, ws_bytes, (hipStream_t)stream);
}

int cmtfpls_kfold_inner_coupled_grouped_f64(const cmtfpls_kfold_state* blocks, int nb, const int* model_fold, int groups, int a, double tol,
                                            int max_iter, void* ws, size_t ws_bytes, void* stream) {
  if (!blocks || nb < 1 || nb > kKfMaxBlocks || !model_fold || groups < 1) {             // before any pointer is looked at
    set_error("kfold_inner_coupled_grouped: bad argument (1 <= nb <= 8 block views, model_fold, groups >= 1)");
    return CMTFPLS_EINVAL;
  }
  if (blocks[0].K % groups != 0 || a < 0 || a >= blocks[0].R || max_iter <= 0) {
    set_error("kfold_inner_coupled_grouped: bad argument");
    return CMTFPLS_EINVAL;
  }
  int rc = kf_blocks_check(blocks, nb, "kfold_inner_coupled_grouped: bad block views (the shared fields must be the same in every view)",
                           blocks[0].K / groups);
  if (rc) return rc;
  KfCoupledTensorDims o{};
  o.d = kf_coupled_dims(blocks, nb);
  return kf_inner_coupled_launch<true, false>(blocks, nb, model_fold, o, a, tol, max_iter, ws, ws_bytes, (hipStream_t)stream);
}

int cmtfpls_kfold_epilogue_grouped_f64(const cmtfpls_kfold_state* st, const int* model_fold, int groups, int stage, int a, const double* in,
                                       void* stream) {
  int rc = kf_grouped_check(st, model_fold, groups, a, "kfold_epilogue_grouped: bad argument");
  if (rc) return rc;
  if (stage < 0 || stage > 2 || (stage > 0 && !in)) { set_error("kfold_epilogue_grouped: bad argument"); return CMTFPLS_EINVAL; }
  return kf_epilogue_launch<kKfGrouped>(st, model_fold, groups, stage, a, in, (hipStream_t)stream, "kfold_epilogue_grouped");
}

int cmtfpls_kfold_epilogue_splits_f64(const cmtfpls_kfold_state* st, int splits, int stage, int a, const double* in, void* stream) {
  if (!kf_epilogue_args_ok(st, stage, a, in) || splits < 1 || st->K % splits != 0) {
    set_error("kfold_epilogue_splits: bad argument");
    return CMTFPLS_EINVAL;
  }
  const int folds = st->K / splits;
  if (folds < 2 || !kf_shape_ok(st->I, st->A, st->B, st->M, st->K, st->R)) {
    set_error("kfold_epilogue_splits: shape outside the device form (2 <= folds, n <= 32 models <= I, M <= 64, R <= 64); refit");
    return CMTFPLS_EUNSUPPORTED;
  }
  return kf_epilogue_launch<kKfSplits>(st, nullptr, folds, stage, a, in, (hipStream_t)stream, "kfold_epilogue_splits");
}

size_t cmtfpls_kfold_weighted_xcov_workspace_bytes(int64_t I, int64_t P, int n, int M) {
  if (I <= 0 || P <= 0 || n <= 0 || M <= 0) return 0;
  return kf_weighted_part_bytes(I, P, n * (M + 1)) + (size_t)(I + 2) * sizeof(int);
}

int cmtfpls_kfold_weighted_xcov_f32(const float* X, int64_t I, int A, int B, const double* Y, int n, int M, double* S, double* mean,
                                    double* stats, void* ws, size_t ws_bytes, void* stream) {
  return run_kfold_weighted<float>(X, I, A, B, Y, n, M, S, mean, stats, ws, ws_bytes, (hipStream_t)stream);
}

int cmtfpls_kfold_weighted_xcov_f64(const double* X, int64_t I, int A, int B, const double* Y, int n, int M, double* S, double* mean,
                                    double* stats, void* ws, size_t ws_bytes, void* stream) {
  return run_kfold_weighted<double>(X, I, A, B, Y, n, M, S, mean, stats, ws, ws_bytes, (hipStream_t)stream);
}

int cmtfpls_kfold_weighted_xcov_bf16(const uint16_t* X, int64_t I, int A, int B, const double* Y, int n, int M, double* S, double* mean,
                                     double* stats, void* ws, size_t ws_bytes, void* stream) {
  return run_kfold_weighted<bf16_t>(reinterpret_cast<const bf16_t*>(X), I, A, B, Y, n, M, S, mean, stats, ws, ws_bytes, (hipStream_t)stream);
}

int cmtfpls_kfold_weighted_xcov_f16(const uint16_t* X, int64_t I, int A, int B, const double* Y, int n, int M, double* S, double* mean,
                                    double* stats, void* ws, size_t ws_bytes, void* stream) {
  return run_kfold_weighted<f16_t>(reinterpret_cast<const f16_t*>(X), I, A, B, Y, n, M, S, mean, stats, ws, ws_bytes, (hipStream_t)stream);
}

int cmtfpls_kfold_epilogue_weighted_f64(const cmtfpls_kfold_state* st, int stage, int a, const double* in, void* stream) {
  if (!kf_epilogue_args_ok(st, stage, a, in)) {
    set_error("kfold_epilogue_weighted: bad argument");
    return CMTFPLS_EINVAL;
  }
  if (!kf_shape_ok(st->I, st->A, st->B, st->M, st->K, st->R)) {
    set_error("kfold_epilogue_weighted: shape outside the device form (2 <= n <= 32 models <= I, M <= 64, R <= 64); refit");
    return CMTFPLS_EUNSUPPORTED;
  }
  return kf_epilogue_launch<kKfWeighted>(st, nullptr, 1, stage, a, in, (hipStream_t)stream, "kfold_epilogue_weighted");
}

}  // extern "C"
