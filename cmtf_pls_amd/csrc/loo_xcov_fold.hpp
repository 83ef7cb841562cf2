// The steps of one leave-one-out fold on its cross-covariance that loo_xcov.hip (a tPLS) and loo_xcov_coupled.hip (a ctPLS, once per
// block) share, by the fold's workgroup of NT threads; the inner loop's steps are fold_loop.hpp's.  Float64, the order of operations
// of the kernels these were cut from.  Each comment says which barrier a step ends on.
#pragma once
#include "fold_loop.hpp"
#include "fold_regress.hpp"

namespace cmtfpls {

// my = the fold's mean of Y by down-dating the column sums (tpls.py:61-71).  No barrier.
template <int NT>
__device__ __forceinline__ void lxf_mean_y(const double* Y, const double* colsum_y, int fold, int M, double inv, double* my) {
  const int tid = threadIdx.x;
  for (int m = tid; m < M; m += NT) my[m] = (colsum_y[m] - Y[(int64_t)fold * M + m]) * inv;
}

// One block: its down-dated mean into `mean` (P, global), a barrier, then Xf = X - mean with the held-out row zero (which removes it
// from every sum).  No barrier after the copy: a thread reads back only the columns it wrote.
template <int NT>
__device__ __forceinline__ void lxf_centre_block(const double* X, const double* colsum, int fold, int I, int64_t P, double inv, double* mean,
                                                 double* Xf) {
  const int tid = threadIdx.x;
  for (int64_t c = tid; c < P; c += NT) mean[c] = (colsum[c] - X[(int64_t)fold * P + c]) * inv;
  __syncthreads();
  for (int r = 0; r < I; ++r) {
    const double* xr = X + (int64_t)r * P;
    double* xo = Xf + (int64_t)r * P;
    if (r == fold) { for (int64_t c = tid; c < P; c += NT) xo[c] = 0.0; }
    else { for (int64_t c = tid; c < P; c += NT) xo[c] = xr[c] - mean[c]; }
  }
}

// Yf = Y - my with the held-out row zero, from a published my.  Ends on a barrier: Xf and Yf are published.
template <int NT>
__device__ __forceinline__ void lxf_centre_y(const double* Y, const double* my, int fold, int I, int M, double* Yf) {
  const int tid = threadIdx.x;
  for (int64_t idx = tid; idx < (int64_t)I * M; idx += NT) {
    const int r = (int)(idx / M), m = (int)(idx % M);
    Yf[idx] = (r == fold) ? 0.0 : Y[idx] - my[m];
  }
  __syncthreads();
}

// S = Yf^T Xf (M x P) of one block, a thread per column with 16 responses' sums in registers.  Four rows of the column are in flight
// at a time (one row per trip leaves a single load per lane outstanding: the pass is then bound by memory latency, 16 ms per
// component and fold at 512 x 16384 instead of 2).  No barrier.
template <int NT>
__device__ __forceinline__ void lxf_build_s(const double* Xf, const double* Yf, int I, int64_t P, int M, double* S) {
  const int tid = threadIdx.x;
  for (int64_t c = tid; c < P; c += NT) {
    for (int mc = 0; mc < M; mc += 16) {
      double acc[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[j] = 0.0;
      int r = 0;
      for (; r + 4 <= I; r += 4) {
        double x[4];
#pragma unroll
        for (int u4 = 0; u4 < 4; ++u4) x[u4] = Xf[(int64_t)(r + u4) * P + c];
#pragma unroll
        for (int u4 = 0; u4 < 4; ++u4) {
          const double* yr = Yf + (int64_t)(r + u4) * M + mc;
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (mc + j < M) acc[j] = fma(yr[j], x[u4], acc[j]);
        }
      }
      for (; r < I; ++r) {
        const double x = Xf[(int64_t)r * P + c];
        const double* yr = Yf + (int64_t)r * M + mc;
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (mc + j < M) acc[j] = fma(yr[j], x, acc[j]);
      }
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (mc + j < M) S[(int64_t)(mc + j) * P + c] = acc[j];
    }
  }
}

// G_y = Yf^T Yf (M x M, LDS).  No barrier (the inner loop's first barrier publishes S and G_y).
template <int NT>
__device__ __forceinline__ void lxf_gram_y(const double* Yf, int I, int M, double* Gy) {
  const int tid = threadIdx.x;
  for (int o = tid; o < M * M; o += NT) {
    const int m1 = o / M, m2 = o % M;
    double s = 0.0;
    for (int r = 0; r < I; ++r) s = fma(Yf[(int64_t)r * M + m1], Yf[(int64_t)r * M + m2], s);
    Gy[o] = s;
  }
}

// the Y score u = Yf q (tpls.py:102).  No barrier.
template <int NT>
__device__ __forceinline__ void lxf_y_score(const double* Yf, const double* q, int I, int M, double* u) {
  const int tid = threadIdx.x;
  for (int r = tid; r < I; r += NT) {
    double s = 0.0;
    for (int m = 0; m < M; ++m) s = fma(Yf[(int64_t)r * M + m], q[m], s);
    u[r] = s;
  }
}

// Xf -= t (x) wk (tpls.py:109), every thread on its own columns.  No barrier.
template <int NT>
__device__ __forceinline__ void lxf_deflate(double* Xf, const double* t, const double* wk, int I, int64_t P) {
  const int tid = threadIdx.x;
  for (int r = 0; r < I; ++r) {
    const double tr = t[r];
    double* xr = Xf + (int64_t)r * P;
    for (int64_t c = tid; c < P; c += NT) xr[c] = fma(-tr, wk[c], xr[c]);
  }
}

// coef[:, comp] = lstsq(T[:, :comp + 1], u) (tpls.py:110-112, fold_regress.hpp), yhat = T b in t, then Yf -= yhat q^T (tpls.py:113).
// Starts from a published T and u, ends on a barrier: Yf is published.
template <int NT>
__device__ __forceinline__ void lxf_regress_deflate_y(const double* T, const double* u, int I, int M, int R, int comp, double* Gn, double* gn,
                                                      double* bb, double* dd, double* coef, double* t, const double* q, double* Yf) {
  const int tid = threadIdx.x;
  fold_inner_regression<NT, false>(T, u, nullptr, I, R, comp, Gn, gn, bb, dd, coef, t);
  for (int64_t idx = tid; idx < (int64_t)I * M; idx += NT) {
    const int r = (int)(idx / M), m = (int)(idx % M);
    Yf[idx] = fma(-t[r], q[m], Yf[idx]);
  }
  __syncthreads();
}

// the held-out row of one block centred with the fold's means (tpls.py:122-126) into h (P).  No barrier.
template <int NT>
__device__ __forceinline__ void lxf_heldout_row(const double* X, const double* colsum, int fold, int64_t P, double inv, double* h) {
  const int tid = threadIdx.x;
  for (int64_t c = tid; c < P; c += NT) {
    const double xv = X[(int64_t)fold * P + c];
    h[c] = xv - (colsum[c] - xv) * inv;
  }
}

// Ypred[fold] = (sc @ coef) @ Qs + my from the held-out row's published scores sc (R) (tpls.py:143).
template <int NT>
__device__ __forceinline__ void lxf_predict(const double* sc, const double* coef, const double* Qs, const double* my, int R, int M,
                                            double* ypred) {
  const int tid = threadIdx.x;
  for (int m = tid; m < M; m += NT) {
    double yv = 0.0;
    for (int b2 = 0; b2 < R; ++b2) {
      double sb = 0.0;
      for (int a2 = 0; a2 < R; ++a2) sb = fma(sc[a2], coef[a2 * R + b2], sb);        // (scores @ coef_)[b]
      yv = fma(sb, Qs[b2 * M + m], yv);                                             // @ Q^T
    }
    ypred[m] = yv + my[m];
  }
}

}  // namespace cmtfpls
