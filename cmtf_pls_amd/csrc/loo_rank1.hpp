// Workgroup helpers of the one-workgroup-per-fold kernels (loo.hip: leave-one-out and the whole small fit; masked_fold.hpp: the
// steps of cv_masked.hip and cv_masked_coupled.hip, models of X with missing values): a workgroup sum and the rank-1 extraction
// of a fold's A x B contraction, block and one-wavefront forms.  Include after common.hpp, inside namespace cmtfpls.
#pragma once

// sum over the workgroup; every thread gets the same value; two barriers, so back-to-back calls may share `red`
template <int NT>
__device__ __forceinline__ double loo_sum(double v, double* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) s += red[w];
  __syncthreads();
  return s;
}

// Leading singular pair of Z (A x B row-major in LDS): wA (A), wB (B) unit norm, largest-|.| entry of wB positive.
// G0/G1: n*n doubles each; xs: n; ys: k (n = min(A,B), k = max(A,B)).  All threads must call it.
template <int NT>
__device__ void loo_rank1(const double* Z, int A, int B, double* wA, double* wB, double* G0, double* G1, double* xs, double* ys,
                          double* red, int* ired) {
  constexpr int kLooThreads = NT;
  const int tid = threadIdx.x;
  const bool rowsA = A <= B;                        // M = Z (n = A) or Z^T (n = B)
  const int n = rowsA ? A : B, k = rowsA ? B : A;
#define LOO_M(i, l) (rowsA ? Z[(i) * B + (l)] : Z[(l) * B + (i)])
  for (int o = tid; o < n * n; o += kLooThreads) {
    const int i = o / n, j = o % n;
    double s = 0.0;
    for (int l = 0; l < k; ++l) s = fma(LOO_M(i, l), LOO_M(j, l), s);
    G0[o] = s;
  }
  __syncthreads();
  double* G = G0;
  double* Gn = G1;
  for (int step = 0; step < 64; ++step) {
    double trp = 0.0, frp = 0.0;
    for (int o = tid; o < n * n; o += kLooThreads) {
      const double g = G[o];
      frp = fma(g, g, frp);
      if (o / n == o % n) trp += g;
    }
    const double tr = loo_sum<NT>(trp, red), fro = loo_sum<NT>(frp, red);
    if (!(tr > 0.0) || !isfinite(tr) || fro / (tr * tr) >= 1.0 - 1e-13) break;      // uniform
    int e;
    frexp(tr, &e);
    const double sc = ldexp(1.0, -e), sc2 = sc * sc;                              // exact power of two
    for (int o = tid; o < n * n; o += kLooThreads) {
      const int i = o / n, j = o % n;
      double s = 0.0;
      for (int l = 0; l < n; ++l) s = fma(G[i * n + l], G[j * n + l], s);          // G symmetric: row j = column j
      Gn[o] = s * sc2;
    }
    __syncthreads();
    double* tmp = G; G = Gn; Gn = tmp;
  }
  // seed = dominant column of G (first index on ties), normalised
  if (tid == 0) {
    double bv = -1.0;
    int bi = 0;
    for (int i = 0; i < n; ++i) { const double dd = G[i * n + i]; if (dd > bv) { bv = dd; bi = i; } }
    ired[0] = bi;
  }
  __syncthreads();
  const int bi = ired[0];
  double ss = 0.0;
  for (int i = tid; i < n; i += kLooThreads) { const double g = G[bi * n + i]; ss = fma(g, g, ss); }
  const double snrm = sqrt(loo_sum<NT>(ss, red));
  for (int i = tid; i < n; i += kLooThreads) xs[i] = G[bi * n + i] / snrm;          // xs = seed for now
  __syncthreads();
  for (int l = tid; l < k; l += kLooThreads) {                                       // y = M^T seed
    double s = 0.0;
    for (int i = 0; i < n; ++i) s = fma(LOO_M(i, l), xs[i], s);
    ys[l] = s;
  }
  __syncthreads();
  double xv = 0.0;                                                                   // x = M y (n <= 64 <= threads)
  if (tid < n) { for (int l = 0; l < k; ++l) xv = fma(LOO_M(tid, l), ys[l], xv); }
  __syncthreads();
  if (tid < n) xs[tid] = xv;
  __syncthreads();
#undef LOO_M
  double sx = 0.0, sy = 0.0;
  for (int i = tid; i < n; i += kLooThreads) sx = fma(xs[i], xs[i], sx);
  for (int l = tid; l < k; l += kLooThreads) sy = fma(ys[l], ys[l], sy);
  const double nx = sqrt(loo_sum<NT>(sx, red)), ny = sqrt(loo_sum<NT>(sy, red));
  // sign rule on the LAST mode's vector wB: its largest-|.| entry is positive (first index on ties)
  const double* vb = rowsA ? ys : xs;
  const int nb = rowsA ? k : n;
  if (tid == 0) {
    double bv = -1.0;
    int b2 = 0;
    for (int i = 0; i < nb; ++i) { const double dd = fabs(vb[i]); if (dd > bv) { bv = dd; b2 = i; } }
    ired[1] = (vb[b2] < 0.0) ? -1 : 1;
  }
  __syncthreads();
  const double sgn = (double)ired[1];
  double* ox = rowsA ? wA : wB;
  double* oy = rowsA ? wB : wA;
  for (int i = tid; i < n; i += kLooThreads) ox[i] = sgn * (xs[i] / nx);
  for (int l = tid; l < k; l += kLooThreads) oy[l] = sgn * (ys[l] / ny);
  __syncthreads();
}

// The same extraction for n = min(A, B) <= 8 and k = max(A, B) <= 64 (BASELINE configs[0]: 10 x 8), entirely inside ONE
// wavefront: the n x n Gram matrix is one entry per lane (lane = 8 i + j), a squaring is 16 lane permutes and 8 FMAs per lane,
// trace and Frobenius norm are butterfly sums -- no workgroup barrier anywhere (the block form above spends ~5 barriers of a
// 16-wavefront workgroup per squaring: 25 of the 46 us of a one-workgroup iteration).  Same seed rule (dominant diagonal entry,
// first index on ties), same exact pass with Z, same sign rule.  All threads call it; wavefront 0 works.
__device__ void loo_rank1_wave(const double* Z, int A, int B, double* wA, double* wB) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const bool rowsA = A <= B;
    const int n = rowsA ? A : B, k = rowsA ? B : A;
#define LOO_M(i, l) (rowsA ? Z[(i) * B + (l)] : Z[(l) * B + (i)])
    const int i = tid >> 3, j = tid & 7;
    const bool in = (i < n && j < n);
    double g = 0.0;
    if (in)
      for (int l = 0; l < k; ++l) g = fma(LOO_M(i, l), LOO_M(j, l), g);
    for (int step = 0; step < 64; ++step) {
      const double tr = wave_sum((in && i == j) ? g : 0.0), fro = wave_sum(g * g);
      if (!(tr > 0.0) || !isfinite(tr) || fro / (tr * tr) >= 1.0 - 1e-13) break;     // uniform: wave_sum gives every lane the same bits
      int e;
      frexp(tr, &e);
      const double sc = ldexp(1.0, -e), sc2 = sc * sc;
      double s2 = 0.0;
#pragma unroll
      for (int l = 0; l < 8; ++l) s2 = fma(__shfl(g, 8 * i + l, kWave), __shfl(g, 8 * j + l, kWave), s2);   // G symmetric: row j = column j
      g = in ? s2 * sc2 : 0.0;
    }
    // dominant diagonal entry (first index on ties)
    double bv = (in && i == j) ? g : -1.0;
    int bi = i;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      const double ov = __shfl_xor(bv, m, kWave);
      const int oi = __shfl_xor(bi, m, kWave);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    // seed = row bi of G, normalised: lane l < n holds seed[l]
    double seed = __shfl(g, 8 * bi + (tid & 7), kWave);
    if (tid >= n) seed = 0.0;
    const double snrm = sqrt(wave_sum(seed * seed));
    seed = seed / snrm;
    // y = M^T seed (lane l < k holds y[l]);  x = M y (lane i < n holds x[i])
    double y = 0.0;
    for (int ii = 0; ii < n; ++ii) {
      const double sv = __shfl(seed, ii, kWave);
      if (tid < k) y = fma(LOO_M(ii, tid), sv, y);
    }
    double x = 0.0;
    for (int l = 0; l < k; ++l) {
      const double yv = __shfl(y, l, kWave);
      if (tid < n) x = fma(LOO_M(tid, l), yv, x);
    }
#undef LOO_M
    const double nx = sqrt(wave_sum(tid < n ? x * x : 0.0)), ny = sqrt(wave_sum(tid < k ? y * y : 0.0));
    // sign rule on the LAST mode's vector wB: its largest-|.| entry is positive (first index on ties)
    const double vb = rowsA ? y : x;
    const int nb = rowsA ? k : n;
    double av = (tid < nb) ? fabs(vb) : -1.0;
    int ai = tid;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      const double ov = __shfl_xor(av, m, kWave);
      const int oi = __shfl_xor(ai, m, kWave);
      if (ov > av || (ov == av && oi < ai)) { av = ov; ai = oi; }
    }
    const double sgn = (__shfl(vb, ai, kWave) < 0.0) ? -1.0 : 1.0;
    double* ox = rowsA ? wA : wB;
    double* oy = rowsA ? wB : wA;
    if (tid < n) ox[tid] = sgn * (x / nx);
    if (tid < k) oy[tid] = sgn * (y / ny);
  }
  __syncthreads();
}
