// The steps of one masked refit, shared by the one-workgroup-per-model kernels for X with missing values (cv_masked.hip: folds and
// count-weighted models of a tPLS; cv_masked_coupled.hip: count-weighted models of a ctPLS, one call per block).  Include after
// common.hpp, fold_regress.hpp and loo_rank1.hpp, inside namespace cmtfpls.  Every function is called by all NT threads of the
// workgroup.  The row weights cw (I, LDS): 0.0 = held out, otherwise the row's weight c_r (1.0 in a fold).  WEIGHTED = false is the
// fold form: its sums over rows carry no factor cw[r] (held-out rows are 0 in Xf, Yf and t).  A block is I x P, P = A B, row-major:
// Xo the original (NaN = missing), Xf the centred working copy (0 at held-out rows and missing entries), cs (P) the training
// observations c_p of each column, mu (P) the training means, ro (I) the observed entries o_r of each row.
#pragma once

// ---- the count-weighted preamble
// counts / yrow (nullable = identity) of one model into cw, the training size n = sum_r c_r into *nf.  Returns the model's status:
// 3 a negative count or a Y row outside 0..I-1, 2 n < 2, else 0 (uniform).  Ends on a barrier; publishes cw.
template <int NT>
__device__ __forceinline__ int mf_weights(const int* cnt_m, const int* yrow_m, int I, double* cw, double* nf, double* red) {
  double nt = 0.0, bad = 0.0;
  for (int r = threadIdx.x; r < I; r += NT) {
    const int c = cnt_m[r];
    const int yr = yrow_m ? yrow_m[r] : r;
    if (c < 0 || yr < 0 || yr >= I) bad = 1.0;
    cw[r] = c > 0 ? (double)c : 0.0;
    nt += c > 0 ? (double)c : 0.0;
  }
  *nf = loo_sum<NT>(nt, red);
  if (loo_sum<NT>(bad, red) > 0.0) return 3;
  return *nf < 2.0 ? 2 : 0;
}

// Weighted column counts and means of one block (np.nanmean on the resampled rows) into cs, mu (NaN where c_p = 0).  Returns this
// thread's flag "some c_p < n" for the caller's loo_sum.  No barrier: that loo_sum publishes cs and mu.
template <int NT>
__device__ __forceinline__ double mf_weighted_means(const double* Xo, const double* cw, int I, int P, double nf, double* cs,
                                                    double* mu) {
  double missing = 0.0;
  for (int c = threadIdx.x; c < P; c += NT) {
    double s = 0.0, cp = 0.0;
    for (int r = 0; r < I; ++r) {
      const double w = cw[r];
      if (w == 0.0) continue;
      const double x = Xo[(int64_t)r * P + c];
      if (!isnan(x)) { s = fma(w, x, s); cp += w; }
    }
    cs[c] = cp;
    mu[c] = cp > 0.0 ? s / cp : __builtin_nan("");
    if (cp < nf) missing = 1.0;
  }
  return missing;
}

// Weighted mean of the paired Y rows into my (M).  No barrier: the caller's next one publishes my.
template <int NT>
__device__ __forceinline__ void mf_weighted_mean_y(const double* Y, const int* yrow_m, const double* cw, int I, int M, double nf,
                                                   double* my) {
  for (int m = threadIdx.x; m < M; m += NT) {
    double s = 0.0;
    for (int r = 0; r < I; ++r) {
      const double w = cw[r];
      if (w != 0.0) s = fma(w, Y[(int64_t)(yrow_m ? yrow_m[r] : r) * M + m], s);
    }
    my[m] = s / nf;
  }
}

// ---- working copies
// Xf of one block: centred, zero at held-out rows and missing entries; ro = observed entries of every row.  Returns this thread's
// flag "a training row without an observed entry" (its score would be 0 / 0) for the caller's loo_sum.  No barrier: that loo_sum
// publishes Xf and ro.
template <int NT>
__device__ __forceinline__ double mf_working_copy(const double* Xo, const double* cw, const double* mu, int I, int P, double* Xf,
                                                  double* ro) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int64_t idx = tid; idx < (int64_t)I * P; idx += NT) {
    const int r = (int)(idx / P), c = (int)(idx % P);
    const double x = Xo[idx];
    Xf[idx] = (cw[r] == 0.0 || isnan(x)) ? 0.0 : x - mu[c];
  }
  double empty = 0.0;
  for (int r = wv; r < I; r += NT / 64) {
    double cnt = 0.0;
    for (int c = lane; c < P; c += 64) cnt += isnan(Xo[(int64_t)r * P + c]) ? 0.0 : 1.0;
    cnt = wave_sum(cnt);
    if (lane == 0) ro[r] = cnt;
    if (cw[r] != 0.0 && cnt == 0.0) empty = 1.0;
  }
  return empty;
}

// Yf = the paired Y rows (yrow_m nullable = identity) minus my, zero at held-out rows; T (I x R) = 0.  No barrier.
template <int NT>
__device__ __forceinline__ void mf_working_copy_y(const double* Y, const int* yrow_m, const double* cw, const double* my, int I,
                                                  int M, int R, double* Yf, double* T) {
  for (int64_t idx = threadIdx.x; idx < (int64_t)I * M; idx += NT) {
    const int r = (int)(idx / M), m = (int)(idx % M);
    Yf[idx] = (cw[r] == 0.0) ? 0.0 : Y[(int64_t)(yrow_m ? yrow_m[r] : r) * M + m] - my[m];
  }
  for (int64_t idx = threadIdx.x; idx < (int64_t)I * R; idx += NT) T[idx] = 0.0;
}

// ---- the component loop
// Z = X x_0 u over the (weighted) rows (tpls.py:83, cmtf.py:93), or miss_tensordot (missingvals.py:17-19): the column's sum
// / c_p * n, 0 when c_p = 0.  P >= NT: a thread per column; P < NT: NT / P partial rows through part (NT doubles), with a barrier
// between the two halves.  Ends on a barrier; publishes Z (P).
template <int NT, bool WEIGHTED>
__device__ __forceinline__ void mf_contract(const double* Xf, const double* u, const double* cw, const double* cs, int I, int P,
                                            bool miss, double nf, double* part, double* Z) {
  const int tid = threadIdx.x;
  const int nrg = (P < NT) ? NT / P : 1;
  auto wu = [&](int r) {                                                             // (weighted) entry of u
    if constexpr (WEIGHTED) return cw[r] * u[r];
    else return u[r];
  };
  if (nrg == 1) {
    for (int c = tid; c < P; c += NT) {
      double s = 0.0;
      for (int r = 0; r < I; ++r) s = fma(Xf[(int64_t)r * P + c], wu(r), s);
      Z[c] = miss ? (cs[c] > 0.0 ? s / cs[c] * nf : 0.0) : s;
    }
  } else {
    const int rg = tid / P, c = tid % P;
    if (rg < nrg) {
      double s = 0.0;
      for (int r = rg; r < I; r += nrg) s = fma(Xf[(int64_t)r * P + c], wu(r), s);
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
}

// The block's loading from Z (A x B): Z / |Z| for a matrix block (tpls.py:84, cmtf.py:97), else the rank-1 pair of
// loo_rank1.hpp (tpls.py:86-88, cmtf.py:98-103), in one wavefront when min(A, B) <= 8 and max(A, B) <= 64.  Ends on a barrier;
// publishes wA (A), wB (B).
template <int NT>
__device__ __forceinline__ void mf_loading(const double* Z, int A, int B, double* wA, double* wB, double* G0, double* G1,
                                           double* xs, double* ys, double* red, int* ired) {
  const int tid = threadIdx.x, P = A * B;
  const int n = A < B ? A : B, k = A < B ? B : A;
  if (A == 1) {
    double s = 0.0;
    for (int c = tid; c < P; c += NT) s = fma(Z[c], Z[c], s);
    const double nz = sqrt(loo_sum<NT>(s, red));
    for (int c = tid; c < P; c += NT) wB[c] = Z[c] / nz;
    if (tid == 0) wA[0] = 1.0;
    __syncthreads();
  } else {
    if (n <= 8 && k <= 64) loo_rank1_wave(Z, A, B, wA, wB);
    else loo_rank1<NT>(Z, A, B, wA, wB, G0, G1, xs, ys, red, ired);
  }
}

// One wavefront's sum_p x[p] wa[p / B] wb[p % B] over a row x (P) of a block: every lane gets the sum.  t = X x_1 wA x_2 wB
// (tpls.py:97-99, cmtf.py:106-110) before the masked rescale / o_r * P of miss_mmodedot (missingvals.py:37).
__device__ __forceinline__ double mf_row_dot(const double* x, const double* wa, const double* wb, int P, int B) {
  double s = 0.0;
  for (int c = threadIdx.x & 63; c < P; c += 64) s = fma(x[c], wa[c / B] * wb[c % B], s);
  return wave_sum(s);
}

// q = Y^T C t / |.|, u = Y q and the (weighted) |u_old - u|, which is returned (tpls.py:100-103, cmtf.py:120-123).  The caller's
// barrier has published t.  Ends on a barrier; publishes q, qn (M) and u (I).
template <int NT, bool WEIGHTED>
__device__ __forceinline__ double mf_y_step(const double* Yf, const double* t, const double* cw, int I, int M, double* q, double* qn,
                                            double* u, double* red) {
  const int tid = threadIdx.x;
  if (tid < M) {
    double s = 0.0;
    for (int r = 0; r < I; ++r) {
      if constexpr (WEIGHTED) s = fma(Yf[(int64_t)r * M + tid], cw[r] * t[r], s);
      else s = fma(Yf[(int64_t)r * M + tid], t[r], s);
    }
    q[tid] = s;
  }
  __syncthreads();
  double qs = (tid < M) ? q[tid] * q[tid] : 0.0;
  const double qnrm = sqrt(loo_sum<NT>(qs, red));
  if (tid < M) qn[tid] = q[tid] / qnrm;
  __syncthreads();
  double du2 = 0.0;
  for (int r = tid; r < I; r += NT) {
    double s = 0.0;
    for (int m = 0; m < M; ++m) s = fma(Yf[(int64_t)r * M + m], qn[m], s);
    const double d0 = u[r] - s;
    if constexpr (WEIGHTED) du2 = fma(cw[r] * d0, d0, du2);
    else du2 = fma(d0, d0, du2);
    u[r] = s;
  }
  return sqrt(loo_sum<NT>(du2, red));
}

// Store the block's loading as component comp of Wa (R x A), Wb (R x B) and deflate the observed training entries of Xf by t
// (tpls.py:109, cmtf.py:130-131: a NaN stays NaN there).  No barrier: the caller's, after its last block, publishes them.
template <int NT>
__device__ __forceinline__ void mf_deflate_x(const double* Xo, const double* cw, const double* t, const double* wA, const double* wB,
                                             int I, int A, int B, int comp, bool miss, double* Wa, double* Wb, double* Xf) {
  const int tid = threadIdx.x, P = A * B;
  for (int j = tid; j < A; j += NT) Wa[comp * A + j] = wA[j];
  for (int j = tid; j < B; j += NT) Wb[comp * B + j] = wB[j];
  for (int64_t idx = tid; idx < (int64_t)I * P; idx += NT) {
    const int r = (int)(idx / P), c = (int)(idx % P);
    if (cw[r] == 0.0 || (miss && isnan(Xo[idx]))) continue;
    Xf[idx] = Xf[idx] - t[r] * (wA[c / B] * wB[c % B]);
  }
}

// The inner regression b = lstsq(T[:, :comp + 1], u) on the (weighted) rows (tpls.py:110-112, cmtf.py:136-138; fold_regress.hpp),
// then Y -= T b q^T (tpls.py:113, cmtf.py:139) with yhat = T b in t; held-out rows of T are 0, so their Yf stays 0.  Ends on a
// barrier; publishes coef[:, comp], t and Yf.
template <int NT, bool WEIGHTED>
__device__ __forceinline__ void mf_regress_deflate_y(const double* T, const double* u, const double* cw, const double* qn, int I,
                                                     int M, int R, int comp, double* Gn, double* gn, double* bb, double* dd,
                                                     double* coef, double* t, double* Yf) {
  fold_inner_regression<NT, WEIGHTED>(T, u, cw, I, R, comp, Gn, gn, bb, dd, coef, t);
  for (int64_t idx = threadIdx.x; idx < (int64_t)I * M; idx += NT) {
    const int r = (int)(idx / M), m = (int)(idx % M);
    Yf[idx] = Yf[idx] - t[r] * qn[m];
  }
  __syncthreads();
}

// ---- the held-out rows (tpls.py:122-143, cmtf.py:141-175)
// The held-out batch of one block: centred with the training means, THEN masked (NaN after centring, which takes in the columns
// without a training observation) into the rows' slots of Xf, their observed counts into ro.  Returns whether any entry of the batch
// is missing: the whole batch of the block then takes the masked score and deflation (uniform).  Ends on a barrier; publishes ro.
template <int NT>
__device__ __forceinline__ bool mf_heldout_batch(const double* Xo, const double* mu, const double* cw, int I, int P, double* Xf,
                                                 double* ro, double* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double Pd = (double)P;
  double hmiss = 0.0;
  for (int r = wv; r < I; r += NT / 64) {
    if (cw[r] != 0.0) continue;                                                       // uniform in the wavefront
    double cnt = 0.0;
    for (int c = lane; c < P; c += 64) {
      const double v = Xo[(int64_t)r * P + c] - mu[c];
      const bool ob = !isnan(v);
      Xf[(int64_t)r * P + c] = ob ? v : 0.0;
      cnt += ob ? 1.0 : 0.0;
    }
    cnt = wave_sum(cnt);
    if (lane == 0) ro[r] = cnt;
    if (cnt < Pd) hmiss = 1.0;
  }
  return loo_sum<NT>(hmiss, red) > 0.0;
}

// One wavefront deflates its held-out row x (P) of a block by the score sv of one component, wa (A), wb (B); xo is the original
// row: on the observed entries only when the batch is masked (hm).  Every lane rereads only the entries it wrote: no barrier.
__device__ __forceinline__ void mf_heldout_deflate(const double* xo, const double* mu, const double* wa, const double* wb, int P,
                                                   int B, double sv, bool hm, double* x) {
  for (int c = threadIdx.x & 63; c < P; c += 64) {
    if (hm && isnan(xo[c] - mu[c])) continue;
    x[c] = x[c] - sv * (wa[c / B] * wb[c % B]);
  }
}

// yp[c - 1] = scores[:, :c] coef_[:c, :c] Q[:, :c]^T + nu on the held-out rows for c = 1..R, yp (R, I, M), the scores in T: coef_
// is upper triangular, so h = scores coef_ is the same for every c and the c-component prediction is nu + the first c terms of
// h Q^T.  The caller's barrier has published T.  No barrier.
template <int NT>
__device__ __forceinline__ void mf_predict(const double* T, const double* coef, const double* Qs, const double* my, const double* cw,
                                           int I, int M, int R, double* yp) {
  for (int64_t o = threadIdx.x; o < (int64_t)I * M; o += NT) {
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
}

// An optional factor output: src (n, LDS) to dst + off when dst is given.  No barrier.
template <int NT>
__device__ __forceinline__ void mf_write_factor(double* dst, int64_t off, const double* src, int n) {
  if (dst) for (int o = threadIdx.x; o < n; o += NT) dst[off + o] = src[o];
}
