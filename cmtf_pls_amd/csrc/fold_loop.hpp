// The NIPALS inner loop of one component on a cross-covariance, run by ONE 1024-thread workgroup (tpls.py:78-107 re-associated:
// np.einsum(X, u) = S^T q, Y.T @ t = S (wA (x) wB), |u_old - u|^2 = dq^T G_y dq with S = Y^T X (M x P) and G_y = Y^T Y), with the
// product's rank-1 extraction (Gram squarings on the f64 matrix cores, sign rule on the last mode).  One workgroup per fold, no
// workgroup waits on another.  A pass is five steps, each written once: lx_z_from_s, lx_extract, lx_kron, lx_row_dots, lx_q_step.
// lx_inner_loop is the loop over them for one block (loo_xcov.hip, kfold.hip's kfold_inner_kernel); the coupled kernels
// (loo_xcov_coupled.hip, kfold.hip's kfold_inner_coupled_kernel) call the first four once per block and keep what is their own: how
// a block's sum enters tq, and their stores between the Kronecker product and its barrier.  cv_masked.hip takes lx_cp3 alone.
#pragma once
#include "common.hpp"

namespace cmtfpls {

constexpr int kLxNT = 1024, kLxWaves = kLxNT / 64;    // the workgroup of the helpers below unless they are given another (NT)
constexpr int kLxMaxN = 256, kLxMaxM = 128, kLxMaxR = 64;     // (M: as far as the M x M Gram of the responses fits the LDS next to the rest)

typedef double lx_d4_t __attribute__((ext_vector_type(4)));

// sum over the workgroup; every thread gets the same value; two barriers, so back-to-back calls may share `red`
template <int NT = kLxNT>
__device__ __forceinline__ double lx_sum(double v, double* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < (NT / 64); ++w) s += red[w];
  __syncthreads();
  return s;
}

// C (n x n) = scale2 * Mx Mx^T for row-major Mx (n x k, leading dimension ld), C_keep (nullable) a second copy.
// Lower-triangular 16 x 16 tiles dealt round-robin to the 16 wavefronts, each on the f64 matrix cores:
//   v_mfma_f64_16x16x4_f64: lane l supplies A[i = l & 15][kq = l >> 4] and B[kq][j = l & 15] and holds D[(l >> 4) + 4 e][l & 15];
//   lane group kq takes the 8 consecutive columns c0 + 8 kq + (0..7) of a 32-column chunk, MFMA s multiplies column
//   c0 + 8 kq + s of row i0 + (l & 15) with the same column of row j0 + (l & 15) (B = Mx^T).
// The mirrored tile is written from the same registers (C is bitwise symmetric).  Returns tr(C) and |C|_F^2 to every thread.
template <int NT = kLxNT>
__device__ void lx_syrk(const double* Mx, int n, int k, int ld, double* C, double* C_keep, double scale2, double* red,
                        double* tr_out, double* fro_out) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ri = lane & 15, kq = lane >> 4;
  const int nt = (n + 15) / 16;
  double trp = 0.0, frp = 0.0;
  int idx = 0;
  for (int ti = 0; ti < nt; ++ti)
    for (int tj = 0; tj <= ti; ++tj, ++idx) {
      if ((idx % (NT / 64)) != wv) continue;
      const int i0 = ti * 16, j0 = tj * 16;
      const bool ra = (i0 + ri) < n, rb = (j0 + ri) < n;
      const double* rowa = Mx + (int64_t)(ra ? i0 + ri : 0) * ld;
      const double* rowb = Mx + (int64_t)(rb ? j0 + ri : 0) * ld;
      lx_d4_t acc = lx_d4_t{0.0, 0.0, 0.0, 0.0};
      for (int kk = 0; kk < k; kk += 32) {
        double a[8], b[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int c = kk + 8 * kq + s;
          const int cc = (c < k) ? c : 0;
          a[s] = rowa[cc];
          b[s] = rowb[cc];
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const bool cok = (kk + 8 * kq + s) < k;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64((ra && cok) ? a[s] : 0.0, (rb && cok) ? b[s] : 0.0, acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = i0 + kq + 4 * e, c = j0 + ri;
        if (r < n && c < n) {
          const double v = acc[e] * scale2;
          C[(int64_t)r * n + c] = v;
          if (C_keep) C_keep[(int64_t)r * n + c] = v;
          if (ti != tj) {
            C[(int64_t)c * n + r] = v;
            if (C_keep) C_keep[(int64_t)c * n + r] = v;
            frp = fma(2.0 * v, v, frp);
          } else {
            frp = fma(v, v, frp);
            if (r == c) trp += v;
          }
        }
      }
    }
  *tr_out = lx_sum<NT>(trp, red);        // (the barriers inside also publish C to the whole workgroup)
  *fro_out = lx_sum<NT>(frp, red);
}

// index of the largest key(i), i < n (keys >= 0), first index on ties, to every thread; ends on a barrier, so bestv / besti may be
// reused at once
template <int NT = kLxNT, typename Key>
__device__ __forceinline__ int lx_argmax(int n, Key key, double* bestv, int* besti) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double bv = -1.0;
  int bi = 0;
  for (int i = tid; i < n; i += NT) { const double d = key(i); if (d > bv) { bv = d; bi = i; } }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const double ov = __shfl_xor(bv, m, 64);
    const int oi = __shfl_xor(bi, m, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) { bestv[wv] = bv; besti[wv] = bi; }
  __syncthreads();
  bv = bestv[0];
  bi = besti[0];
  for (int w = 1; w < (NT / 64); ++w)
    if (bestv[w] > bv || (bestv[w] == bv && besti[w] < bi)) { bv = bestv[w]; bi = besti[w]; }
  __syncthreads();
  return bi;
}

// index of the largest |v[i]|, first index on ties, to every thread
template <int NT = kLxNT>
__device__ int lx_argmax_abs(const double* v, int n, double* bestv, int* besti) {
  return lx_argmax<NT>(n, [v](int i) { return fabs(v[i]); }, bestv, besti);
}

// Leading singular pair of Z (A x B row-major, global): wA (A), wB (B) unit norm, largest-|.| entry of wB positive.
// Zt: P doubles of scratch (the transpose when B < A); G0 / G1: n x n each (ping-pong); xs (n), ys (k) in LDS.
// LONG_GLOBAL (lx_cp3's unfoldings): the same code as an instantiation of its own, whose ys and wB are global scratch, so that the
// callers with everything in LDS keep the code they had.
template <bool LONG_GLOBAL = false, int NT = kLxNT>
__device__ void lx_rank1(const double* Z, double* Zt, int A, int B, double* wA, double* wB, double* G0, double* G1,
                         double* xs, double* ys, double* red, double* bestv, int* besti) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool rowsA = A <= B;                        // Mx = Z (n = A) or Z^T (n = B)
  const int n = rowsA ? A : B, k = rowsA ? B : A;
  const double* Mx = Z;
  if (!rowsA) {
    for (int idx = tid; idx < A * B; idx += NT) { const int b = idx / A, a = idx % A; Zt[idx] = Z[(int64_t)a * B + b]; }
    __syncthreads();
    Mx = Zt;
  }
  double tr, fro;
  lx_syrk<NT>(Mx, n, k, k, G0, nullptr, 1.0, red, &tr, &fro);                              // G_0 = Mx Mx^T
  double* G = G0;
  double* Gn = G1;
  for (int step = 0; step < 64; ++step) {
    if (!(tr > 0.0) || !isfinite(tr) || fro / (tr * tr) >= 1.0 - 1e-13) break;         // uniform: numerically rank one
    int e;
    frexp(tr, &e);
    const double sc = ldexp(1.0, -e);                                                 // exact power of two
    lx_syrk<NT>(G, n, n, n, Gn, nullptr, sc * sc, red, &tr, &fro);                         // G <- (sc G)^2   (G symmetric: G G = G G^T)
    double* tmp = G; G = Gn; Gn = tmp;
  }
  // seed = dominant column of G (first index on ties), normalised
  const int bi = lx_argmax<NT>(n, [G, n](int i) { return G[(int64_t)i * n + i]; }, bestv, besti);
  double ss = 0.0;
  for (int i = tid; i < n; i += NT) { const double g = G[(int64_t)bi * n + i]; ss = fma(g, g, ss); }
  const double snrm = sqrt(lx_sum<NT>(ss, red));
  for (int i = tid; i < n; i += NT) xs[i] = G[(int64_t)bi * n + i] / snrm;
  __syncthreads();
  for (int l = tid; l < k; l += NT) {                                               // y = Mx^T seed
    double s = 0.0;
    for (int i = 0; i < n; ++i) s = fma(Mx[(int64_t)i * k + l], xs[i], s);
    ys[l] = s;
  }
  __syncthreads();
  for (int i = wv; i < n; i += (NT / 64)) {                                             // x = Mx y: a wavefront per row
    double s = 0.0;
    for (int l = lane; l < k; l += 64) s = fma(Mx[(int64_t)i * k + l], ys[l], s);
    s = wave_sum(s);
    if (lane == 0) xs[i] = s;                 // (the seed is dead: every wavefront finished y before the barrier above)
  }
  __syncthreads();
  double sx = 0.0, sy = 0.0;
  for (int i = tid; i < n; i += NT) sx = fma(xs[i], xs[i], sx);
  for (int l = tid; l < k; l += NT) sy = fma(ys[l], ys[l], sy);
  const double nx = sqrt(lx_sum<NT>(sx, red)), ny = sqrt(lx_sum<NT>(sy, red));
  // sign rule on the LAST mode's vector wB: its largest-|.| entry is positive (first index on ties)
  const double* vb = rowsA ? ys : xs;
  const int nb = rowsA ? k : n;
  const double sgn = (vb[lx_argmax_abs<NT>(vb, nb, bestv, besti)] < 0.0) ? -1.0 : 1.0;
  double* ox = rowsA ? wA : wB;
  double* oy = rowsA ? wB : wA;
  for (int i = tid; i < n; i += NT) ox[i] = sgn * (xs[i] / nx);
  for (int l = tid; l < k; l += NT) oy[l] = sgn * (ys[l] / ny);
  __syncthreads();
}

// sum_c row[c] * wk[c] over one wavefront's columns c = lane, lane + 64, ...: one fma chain per lane in column order (the order of the
// plain loop), eight loads of each operand in flight per trip
__device__ __forceinline__ double lx_wave_dot(const double* row, const double* wk, int64_t P, int lane) {
  double s = 0.0;
  int64_t c = lane;
  for (; c + 7 * 64 < P; c += 8 * 64) {
    double xv[8], wv8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { xv[j] = row[c + 64 * j]; wv8[j] = wk[c + 64 * j]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) s = fma(xv[j], wv8[j], s);
  }
  for (; c < P; c += 64) s = fma(row[c], wk[c], s);
  return wave_sum(s);
}

// ---- rank-1 CP of an order-3 cross-covariance (X of order 4) ---------------------------------------------------------------------
// The trailing dims of an order-4 block and the scratch of its extraction.  B2 == 0: X of order 2 or 3, Z a matrix (lx_rank1).
struct LxTensor {
  int B1 = 0, B2 = 0;
  double* wK = nullptr;    // LDS: B1, the loading of mode 2 of X
  double* wL = nullptr;    // LDS: B2, the loading of mode 3 of X
  double* v = nullptr;     // LDS: B1 * B2, Z x_0 f_A (shared by the contractions of modes 1 and 2)
  double* tmp = nullptr;   // LDS: max(A, B1, B2), a contraction before its scaling
  double* part = nullptr;  // LDS: NT (the caller's thread count), the row groups' partial sums of v
  double* U = nullptr;     // global: A * B1 * B2, the unfolding of mode 1 or 2
  double* yl = nullptr;    // global: A * B1 * B2, the long vector of lx_rank1 on an unfolding
  double* vr = nullptr;    // global: A * B1 * B2, the right singular vector of an unfolding (not used)
};

template <int NT = kLxNT>
__device__ __forceinline__ double lx_dot(const double* a, const double* b, int n, double* red) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += NT) s = fma(a[i], b[i], s);
  return lx_sum<NT>(s, red);
}

// host: the shorter side of the mode-`mode` unfolding of A x B1 x B2 (what lx_rank1 squares), and the largest of the three, which
// sizes xs, G0 and G1 of an order-4 block
inline int lx_tensor_short(int A, int B1, int B2, int mode) {
  const int64_t d = mode == 0 ? A : mode == 1 ? B1 : B2, rest = (int64_t)A * B1 * B2 / d;
  return (int)(d < rest ? d : rest);
}

inline int lx_tensor_nmax(int A, int B1, int B2) {
  int n = 0;
  for (int m = 0; m < 3; ++m) n = lx_tensor_short(A, B1, B2, m) > n ? lx_tensor_short(A, B1, B2, m) : n;
  return n;
}

// Rank-1 CP factors of Z (A x B1 x B2 row-major, global): parafac(Z, 1, tol=tol, init="svd", normalize_factors=True) as
// rank1_tensor.hip:1-9 and oracle/nipals_oracle.rank1_factors state it, by the fold's workgroup.
//   init    f_m = the leading left singular vector of the mode-m unfolding (lx_rank1: mode 0 is Z as A x B1 B2, modes 1 and 2 are
//           unfolded into t.U in the C order of the other modes), largest-|.| entry positive.  The unfolding's long vector and
//           its right singular vector live in global scratch (t.yl, t.vr): only the short side is bounded (kLxMaxN).
//   sweep   cp_rank1_als_kernel's, in its order of operations, with two reads of Z instead of three: mode 0 is a dot of every
//           row of Z with f_K (x) f_L (kl, a wavefront per row); v = Z x_0 f_A with the new f_A then serves mode 1 (v f_L) and
//           mode 2 (v^T f_K), since f_A does not change between them.  v is built by floor(1024 / B) row groups of B threads
//           (coalesced over the columns), the groups' partial sums added in group order.
// fA (A), t.wK (B1), t.wL (B2): the factors as the sweeps leave them (the regular engine applies nothing further to
// cmtfpls_rank1_tensor_f64's output).  kl: B doubles of LDS, on return f_K (x) f_L.  G0 / G1: n x n for the largest short side n of
// the three unfoldings; xs: that n.
template <int NT = kLxNT>
__device__ void lx_cp3(const double* Z, double* Zt, int A, double tol, const LxTensor& t, double* fA, double* kl, double* G0, double* G1,
                       double* xs, double* red, double* bestv, int* besti) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int B1 = t.B1, B2 = t.B2, B = B1 * B2, P = A * B;
  double* f[3] = {fA, t.wK, t.wL};
  const int d[3] = {A, B1, B2};
  lx_rank1<true, NT>(Z, Zt, A, B, fA, t.vr, G0, G1, xs, t.yl, red, bestv, besti);
  for (int e = tid; e < P; e += NT) {                                             // mode 1: U[k][a B2 + l] = Z[a][k][l]
    const int k = e / (A * B2), c = e % (A * B2);
    t.U[e] = Z[(int64_t)(c / B2) * B + k * B2 + c % B2];
  }
  __syncthreads();
  lx_rank1<true, NT>(t.U, Zt, B1, A * B2, t.wK, t.vr, G0, G1, xs, t.yl, red, bestv, besti);
  for (int e = tid; e < P; e += NT) {                                             // mode 2: U[l][a B1 + k] = Z[a][k][l]
    const int l = e / (A * B1), c = e % (A * B1);
    t.U[e] = Z[(int64_t)c * B2 + l];
  }
  __syncthreads();
  lx_rank1<true, NT>(t.U, Zt, B2, A * B1, t.wL, t.vr, G0, G1, xs, t.yl, red, bestv, besti);
  for (int m = 0; m < 3; ++m) {                                                      // sign rule (cp_rank1_als_kernel:90-103)
    const int arg = lx_argmax_abs<NT>(f[m], d[m], bestv, besti);
    const bool flip = f[m][arg] < 0.0;
    __syncthreads();
    if (flip) for (int i = tid; i < d[m]; i += NT) f[m][i] = -f[m][i];
    __syncthreads();
  }
  double zz = 0.0;
  for (int e = tid; e < P; e += NT) zz = fma(Z[e], Z[e], zz);
  const double norm_z = sqrt(lx_sum<NT>(zz, red));
  const int G = B >= NT ? 1 : NT / B;                                         // row groups of v
  double weight = 1.0, prev_err = 0.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double iprod = 0.0;
    for (int m = 0; m < 3; ++m) {
      double gram = weight * weight;
      for (int i = 0; i < 3; ++i)
        if (i != m) gram *= lx_dot<NT>(f[i], f[i], d[i], red);
      if (m == 0) {                                                                  // tmp[a] = Z[a, :, :] . (f_K (x) f_L)
        for (int c = tid; c < B; c += NT) kl[c] = t.wK[c / B2] * t.wL[c % B2];
        __syncthreads();
        for (int a = wv; a < A; a += (NT / 64)) {
          const double s = lx_wave_dot(Z + (int64_t)a * B, kl, B, lane);
          if (lane == 0) t.tmp[a] = s;
        }
      } else if (m == 1) {                                                           // v = Z x_0 f_A, tmp[k] = v[k, :] . f_L
        if (G == 1) {
          for (int c = tid; c < B; c += NT) {
            double s = 0.0;
            for (int a = 0; a < A; ++a) s = fma(fA[a], Z[(int64_t)a * B + c], s);
            t.v[c] = s;
          }
        } else {
          if (tid < G * B) {
            const int g = tid / B, c = tid % B;
            double s = 0.0;
            for (int a = g; a < A; a += G) s = fma(fA[a], Z[(int64_t)a * B + c], s);
            t.part[tid] = s;
          }
          __syncthreads();
          for (int c = tid; c < B; c += NT) {
            double s = 0.0;
            for (int g = 0; g < G; ++g) s += t.part[g * B + c];
            t.v[c] = s;
          }
        }
        __syncthreads();
        for (int k = wv; k < B1; k += (NT / 64)) {
          double s = 0.0;
          for (int l = lane; l < B2; l += 64) s = fma(t.v[k * B2 + l], t.wL[l], s);
          s = wave_sum(s);
          if (lane == 0) t.tmp[k] = s;
        }
      } else {                                                                       // tmp[l] = v[:, l] . f_K
        for (int l = wv; l < B2; l += (NT / 64)) {
          double s = 0.0;
          for (int k = lane; k < B1; k += 64) s = fma(t.v[k * B2 + l], t.wK[k], s);
          s = wave_sum(s);
          if (lane == 0) t.tmp[l] = s;
        }
      }
      __syncthreads();
      if (m == 2) iprod = (weight * weight * lx_dot<NT>(t.tmp, t.tmp, d[m], red) / gram) * weight;
      for (int i = tid; i < d[m]; i += NT) f[m][i] = t.tmp[i] * weight / gram;
      __syncthreads();
    }
    double fn2 = weight * weight;
    for (int i = 0; i < 3; ++i) fn2 *= lx_dot<NT>(f[i], f[i], d[i], red);
    const double err = sqrt(fabs(norm_z * norm_z + fn2 - 2.0 * iprod)) / norm_z;
    if (sweep >= 1 && fabs(prev_err - err) < tol) break;                             // (uniform: every thread holds the same sums)
    prev_err = err;
    for (int i = 0; i < 3; ++i) {
      const double nrm = sqrt(lx_dot<NT>(f[i], f[i], d[i], red));
      weight *= nrm;
      for (int j = tid; j < d[i]; j += NT) f[i][j] = f[i][j] / nrm;
      __syncthreads();
    }
  }
  for (int c = tid; c < B; c += NT) kl[c] = t.wK[c / B2] * t.wL[c % B2];           // w_B = w_K (x) w_L (C order)
  __syncthreads();
}

// lx_cp3's scratch as an LxTensor: wK (b1), wL (b2), v (bt), tmp (dmax) and part (NT, the caller's thread count) from `lds` on, U,
// yl and vr (pt each) from `glb` on.  A single block gives its own B1, B2, B1 B2, max(A, B1, B2) and A B1 B2; a coupled kernel the
// maxima over its tensor blocks, and sets B1 / B2 per block.
__device__ __forceinline__ LxTensor lx_tensor_scratch(double* lds, double* glb, int b1, int b2, int bt, int dmax, int64_t pt, int NT) {
  LxTensor t;
  t.B1 = b1;
  t.B2 = b2;
  t.wK = lds;
  t.wL = t.wK + b1;
  t.v = t.wL + b2;
  t.tmp = t.v + bt;
  t.part = t.tmp + dmax;
  t.U = glb;
  t.yl = t.U + pt;
  t.vr = t.yl + pt;
  return t;
}

// ---- the steps of one pass of the inner loop (tpls.py:79-107, cmtf.py:91-128), by the fold's workgroup of NT threads ---------------
// Z = X x_0 u = S^T q (tpls.py:83) for S (M x P, global), four rows of S in flight in the order of the plain sum.  Ends on a
// barrier: Z is published.
template <int NT = kLxNT>
__device__ __forceinline__ void lx_z_from_s(const double* S, const double* q, double* Z, int64_t P, int M) {
  const int tid = threadIdx.x;
  for (int64_t c = tid; c < P; c += NT) {
    double s = 0.0;
    int m = 0;
    for (; m + 4 <= M; m += 4) {
      const double s0 = S[(int64_t)m * P + c], s1 = S[(int64_t)(m + 1) * P + c], s2 = S[(int64_t)(m + 2) * P + c], s3 = S[(int64_t)(m + 3) * P + c];
      s = fma(q[m], s0, s);
      s = fma(q[m + 1], s1, s);
      s = fma(q[m + 2], s2, s);
      s = fma(q[m + 3], s3, s);
    }
    for (; m < M; ++m) s = fma(q[m], S[(int64_t)m * P + c], s);
    Z[c] = s;
  }
  __syncthreads();
}

// The loadings wA (A), wB (B) of Z (A x B, P = A B; tpls.py:84-88): t.B2 > 0 (TENSOR callers only: the others never instantiate
// lx_cp3): the rank-1 CP of the A x B1 x B2 Z, wB = wK (x) wL; A == 1: Z / |Z|; else lx_rank1.  Ends on a barrier: wA and wB (and
// t.wK, t.wL) are published.
template <bool TENSOR, int NT = kLxNT>
__device__ __forceinline__ void lx_extract(const double* Z, double* Zt, int A, int B, int64_t P, double tol, const LxTensor& t, double* wA,
                                           double* wB, double* G0, double* G1, double* xs, double* ys, double* red, double* bestv,
                                           int* besti) {
  const int tid = threadIdx.x;
  bool cp = false;
  if constexpr (TENSOR) cp = t.B2 > 0;
  if (cp) {
    if constexpr (TENSOR) lx_cp3<NT>(Z, Zt, A, tol, t, wA, wB, G0, G1, xs, red, bestv, besti);
  } else if (A == 1) {
    double s = 0.0;
    for (int64_t c = tid; c < P; c += NT) s = fma(Z[c], Z[c], s);
    const double nz = sqrt(lx_sum<NT>(s, red));
    for (int64_t c = tid; c < P; c += NT) wB[c] = Z[c] / nz;
    if (tid == 0) wA[0] = 1.0;
    __syncthreads();
  } else {
    lx_rank1<false, NT>(Z, Zt, A, B, wA, wB, G0, G1, xs, ys, red, bestv, besti);
  }
}

// wk = wA (x) wB (P = A B), the Kronecker loading.  No barrier: every thread writes the entries c = tid, tid + NT, ..., and may read
// those back at once; the caller's barrier publishes wk.
template <int NT = kLxNT>
__device__ __forceinline__ void lx_kron(double* wk, const double* wA, const double* wB, int64_t P, int B) {
  const int tid = threadIdx.x;
  for (int64_t c = tid; c < P; c += NT) wk[c] = wA[c / B] * wB[c % B];
}

// put(r, Mx[r, :] . wk) for the rows r < rows of Mx (rows x P, global), a wavefront per row and its lane 0 calling put: Y^T t = S wk
// (tpls.py:97-100) on the rows of S, the score X wk on the rows of the fold's X.  Row r is always the same wavefront's, so put may add
// to what an earlier call left in its slot.  lane, wv: the caller's tid & 63 and tid >> 6, handed in as lx_wave_dot's lane is
// (computed in here, kfold_inner_kernel spills 16 bytes more).  No barrier.
template <int NT = kLxNT, typename Put>
__device__ __forceinline__ void lx_row_dots(const double* Mx, const double* wk, int64_t P, int rows, int lane, int wv, Put put) {
  for (int r = wv; r < rows; r += NT / 64) {
    const double s = lx_wave_dot(Mx + (int64_t)r * P, wk, P, lane);
    if (lane == 0) put(r, s);
  }
}

// q <- (tq / nb) / |tq / nb| (tpls.py:101; nb: the blocks whose S wk were added into tq, np.average of cmtf.py:120, 1.0 for a
// tPLS: x / 1.0 is x) and whether the loop stops: sqrt(dq^T G_y dq) = |u_old - u| < tol (tpls.py:102-103), never on the first pass
// (oldU = inf, tpls.py:77).  Starts from a published tq, ends on a barrier: q is published.
template <int NT = kLxNT>
__device__ __forceinline__ bool lx_q_step(const double* tq, double nb, double* q, double* qn, const double* Gy, int M, double tol, int it,
                                          double* red) {
  const int tid = threadIdx.x;
  double qs = 0.0;
  for (int m = tid; m < M; m += NT) { const double v = tq[m] / nb; qs = fma(v, v, qs); }
  const double qnrm = sqrt(lx_sum<NT>(qs, red));
  for (int m = tid; m < M; m += NT) qn[m] = (tq[m] / nb) / qnrm;
  __syncthreads();
  double d2 = 0.0;
  for (int o = tid; o < M * M; o += NT) d2 = fma((qn[o / M] - q[o / M]) * Gy[o], qn[o % M] - q[o % M], d2);
  d2 = lx_sum<NT>(d2, red);
  for (int m = tid; m < M; m += NT) q[m] = qn[m];
  __syncthreads();
  return it > 0 && sqrt(d2 > 0.0 ? d2 : 0.0) < tol;
}

// The whole inner loop of one component (tpls.py:78-107) on S (M x P, global) from q = e_0 (u = Y[:, 0], tpls.py:78) until
// lx_q_step stops it or max_iter passes.  On return q holds the converged q, wA / wB the loadings and wk (P) their Kronecker product;
// returns the passes executed.  Z, Zt, wk: P doubles each (global); G0, G1: n x n (global); q, qn, tq (M), xs (n), ys (k), red,
// bestv, besti: workgroup scratch; Gy: M x M.
// tn.B2 > 0: X of order 4, Z an A x B1 x B2 tensor (B = B1 B2) whose extraction is lx_cp3; wB is then w_K (x) w_L and ys is unused.
// (A caller without a tensor passes none, and the constant B2 = 0 removes lx_cp3 from its code.)
__device__ __forceinline__ int lx_inner_loop(const double* S, const double* Gy, int64_t P, int M, int A, int B, double tol, int max_iter,
                                             double* q, double* qn, double* tq, double* Z, double* Zt, double* wk, double* wA, double* wB,
                                             double* G0, double* G1, double* xs, double* ys, double* red, double* bestv, int* besti,
                                             const LxTensor tn = LxTensor()) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int m = tid; m < M; m += kLxNT) q[m] = (m == 0) ? 1.0 : 0.0;                 // u_0 = Y_f[:, 0] = Y_f e_0 (tpls.py:78)
  __syncthreads();
  int it = 0;
  for (; it < max_iter; ++it) {                                                    // tpls.py:79
    lx_z_from_s(S, q, Z, P, M);
    lx_extract<true>(Z, Zt, A, B, P, tol, tn, wA, wB, G0, G1, xs, ys, red, bestv, besti);
    lx_kron(wk, wA, wB, P, B);                                                     // once per extraction
    __syncthreads();
    lx_row_dots(S, wk, P, M, lane, wv, [tq](int m, double s) { tq[m] = s; });
    __syncthreads();
    if (lx_q_step(tq, 1.0, q, qn, Gy, M, tol, it, red)) { ++it; break; }
  }
  return it;
}

}  // namespace cmtfpls
