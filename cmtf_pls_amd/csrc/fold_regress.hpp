// The inner regression of one component, coef_[:a+1, a] = lstsq(T[:, :a+1], u) (tpls.py:110-112, cmtf.py:135), as the
// one-workgroup-per-fold kernels run it (loo.hip, loo_xcov.hip, loo_xcov_coupled.hip, and through masked_fold.hpp cv_masked.hip
// and cv_masked_coupled.hip) and the serial solve inside it, which kfold.hip's kfold_solve_kernel shares.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace cmtfpls {

// Solve Gn b = gn for symmetric positive semi-definite Gn (kk x kk, row-major, kk <= 64) on ONE thread; Gn is overwritten by
// the factor, dd (kk) receives the equilibration and bb (kk) the solution.
//
// The pivot rule.  The scores' columns differ in scale by orders of magnitude (late components of a well-explained X), which the
// reference's lstsq on T itself tolerates; the raw normal equations would square that spread.  So the matrix is EQUILIBRATED
// first, D Gn D with D = diag(Gn)^(-1/2) (dd[i] = 0 for a diagonal that is not positive and finite), and the Cholesky
// factorisation runs on that.  A column whose pivot is then not above kk * eps is linearly dependent on the earlier ones to
// working precision (or identically zero, or not finite: the test is !(piv > tiny), so a NaN pivot drops too): it is taken out of
// the system (diagonal 1, the column below it 0) and its coefficient is 0, which is what a truncated least-squares solve does
// with it.  Dropped columns are the set bits of one 64-bit mask.
//
// Host and device compile the same text (tests/test_fold_regress_cpu.py runs it on the host against a restatement in Python).
__host__ __device__ inline void fold_normal_solve(double* Gn, const double* gn, int kk, double* dd, double* bb) {
  const double tiny = (double)kk * 2.220446049250313e-16;
  for (int i = 0; i < kk; ++i) { const double g = Gn[i * kk + i]; dd[i] = (g > 0.0 && std::isfinite(g)) ? 1.0 / sqrt(g) : 0.0; }
  for (int i = 0; i < kk; ++i) {
    for (int j = 0; j < kk; ++j) Gn[i * kk + j] *= dd[i] * dd[j];
    bb[i] = gn[i] * dd[i];
  }
  uint64_t dep = 0;                                                                  // bit c: column c dropped
  for (int c = 0; c < kk; ++c) {
    const double piv = Gn[c * kk + c];
    if (!(piv > tiny)) {
      dep |= (uint64_t)1 << c;
      Gn[c * kk + c] = 1.0;
      for (int i = c + 1; i < kk; ++i) Gn[i * kk + c] = 0.0;
      continue;
    }
    const double l = sqrt(piv);
    Gn[c * kk + c] = l;
    for (int i = c + 1; i < kk; ++i) Gn[i * kk + c] /= l;
    for (int i = c + 1; i < kk; ++i)
      for (int j = c + 1; j <= i; ++j) Gn[i * kk + j] -= Gn[i * kk + c] * Gn[j * kk + c];
  }
  for (int r = 0; r < kk; ++r) {                                                     // forward L z = y
    double s = bb[r];
    for (int j = 0; j < r; ++j) s -= Gn[r * kk + j] * bb[j];
    bb[r] = ((dep >> r) & 1) ? 0.0 : s / Gn[r * kk + r];
  }
  for (int r = kk - 1; r >= 0; --r) {                                                // backward L^T x = z
    double s = bb[r];
    for (int j = r + 1; j < kk; ++j) s -= Gn[j * kk + r] * bb[j];
    bb[r] = ((dep >> r) & 1) ? 0.0 : s / Gn[r * kk + r];
  }
  for (int r = 0; r < kk; ++r) bb[r] *= dd[r];
}

// One component's regression step of a fold's workgroup of NT threads, kk = comp + 1: the normal equations of the scores
// T[:, :kk] (I x R, row-major) against u (I) into Gn (kk x kk), gn (kk), WEIGHTED: with the row weights cw, (T^T C T) b = T^T C u;
// the solve on thread 0 into bb, stored as coef[:kk, comp] (R x R); yhat = T b into t (I).  Ends on a barrier; the caller
// deflates Y by t.
template <int NT, bool WEIGHTED>
__device__ __forceinline__ void fold_inner_regression(const double* T, const double* u, const double* cw, int I, int R, int comp,
                                                      double* Gn, double* gn, double* bb, double* dd, double* coef, double* t) {
  const int tid = threadIdx.x, kk = comp + 1;
  auto wT = [&](int r, int p) {                                                      // (weighted) entry of the left factor
    if constexpr (WEIGHTED) return cw[r] * T[(int64_t)r * R + p];
    else return T[(int64_t)r * R + p];
  };
  for (int o = tid; o < kk * kk + kk; o += NT) {
    double s = 0.0;
    if (o < kk * kk) {
      const int p = o / kk, s2 = o % kk;
      for (int r = 0; r < I; ++r) s = fma(wT(r, p), T[(int64_t)r * R + s2], s);
      Gn[o] = s;
    } else {
      const int p = o - kk * kk;
      for (int r = 0; r < I; ++r) s = fma(wT(r, p), u[r], s);
      gn[p] = s;
    }
  }
  __syncthreads();
  if (tid == 0) {
    fold_normal_solve(Gn, gn, kk, dd, bb);
    for (int r = 0; r < kk; ++r) coef[r * R + comp] = bb[r];
  }
  __syncthreads();
  for (int r = tid; r < I; r += NT) {
    double s = 0.0;
    for (int j = 0; j < kk; ++j) s = fma(T[(int64_t)r * R + j], bb[j], s);
    t[r] = s;
  }
  __syncthreads();
}

}  // namespace cmtfpls
