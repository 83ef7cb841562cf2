// Leave-one-out refits of a COUPLED model (ctPLS) on complete data: the coupled sibling of loo_xcov.hip's loo_xcov_kernel<false>.
// All folds of a launch side by side, ONE 1024-thread WORKGROUP PER FOLD running that fold's whole ctPLS.fit (cmtf.py:85-139) and the
// prediction of its held-out sample (cmtf.py:142-177) on up to 8 blocks, each of order 2 (a matrix: A = 1) or 3, float64 throughout.
//
// What a fold does NOT recompute or re-read (as loo_xcov.hip, block by block):
//  * the means of every block and of Y: (column sums of all samples - the held-out row) / (I - 1); the held-out row is zero in the
//    fold's centred working copies X_{b,f} and Y_f, which removes it from every sum.  The original blocks are only read.
//  * the blocks inside the NIPALS loop: within a component every X_{b,f} and Y_f are fixed, the blocks share ONE score t and u = Y_f q, so
//        np.einsum(X_b, u) = S_b^T q  (cmtf.py:94),   Y.T @ t = (1 / nb) sum_b S_b (wA_b (x) wB_b)  (cmtf.py:106-121),
//        |u_old - u|^2 = dq^T (Y_f^T Y_f) dq  (cmtf.py:124)
//    with S_b = Y_f^T X_{b,f} (M x P_b) and G_y = Y_f^T Y_f formed ONCE per component (four rows of a column in flight, loo_xcov.hip).
//    An inner pass reads the 2 M P_b doubles of every S_b instead of the 2 I P_b of the fold's blocks.  Per component and fold a block's
//    working copy is read for S_b, for the score t = mean_b X_{b,f} (wA_b (x) wB_b) (cmtf.py:120), and read + written by its deflation
//    with its own t (x) wA_b (x) wB_b (cmtf.py:130-131): three reads and one write.
//  * the inner loop starts from q = e_0 (u = Y_f[:, 0], cmtf.py:90), visits the blocks in list order, and never stops on its first
//    pass (oldU = inf, cmtf.py:89).  The extraction of a block (cmtf.py:98-104) is Z_b / |Z_b| for a matrix block and lx_rank1
//    (fold_loop.hpp: Gram squarings on the f64 matrix cores, sign rule on the last mode) for an order-3 block.
//  * coef[:, a] from the normal equations of T (equilibrated Cholesky, as loo_xcov.hip), then Y_f -= T b q^T (cmtf.py:135-138).
// Held-out prediction: the sequential form of cmtf.py:154-177 on the held-out rows of all blocks -- per component the block average
// of the projections, then each block's row deflated with its own loadings -- written to row `fold` of Ypred.
//
// LDS (doubles): every block's current wA_b and wB_b stay resident (the Y^T t sum needs all of them): sum_b A_b + sum_b B_b; then
// q, qn, tq, my (M each), G_y (M x M), the extraction's xs (nmax) and ys (kmax) shared by the blocks and sized for the largest
// (nmax = max_b min(A_b, B_b), kmax = max_b max(A_b, B_b)), coef (R x R), Qs (R x M), the normal equations Gn (R x R), gn, bb, dd (R):
//     sum A_b + sum B_b + 4 M + M^2 + nmax + kmax + 2 R^2 + R M + 3 R      (one block: loo_xcov's formula)
// Workspace per resident fold (doubles), sumP = sum_b P_b, Pmax = max_b P_b:
//     (I + M) sumP  [X_{b,f} | S_b]  +  3 Pmax  [Z | Zt | wk, shared]  +  2 nmax^2  [G0 | G1]  +  I (M + R + 2)  [Y_f | T | u | t]
//     +  R (sum A_b + sum B_b)  [the loadings of the components so far]       (one block: loo_xcov's formula)
// The held-out rows of the prediction (sumP doubles) reuse the head of the S_b region, which is dead by then.
// Limits: at most 8 blocks, order 2 or 3, min(A_b, B_b) <= 256, M <= 128, R <= 64, P_b <= 2^24, LDS <= 150 KB; no missing values (the
// caller's to detect: this is the complete-data form).
//
// Blocks of order 4 (I x A_b x B1_b x B2_b, cmtfpls_loo_xcov_coupled_tensor_f64): the same kernel as its TENSOR instantiation, at 512
// threads (lx_cp3 inlined at 1024 threads and 128 registers a lane would spill).  A block with B2_b > 0 is seen as I x A_b x B_b with
// B_b = B1_b B2_b (B2_b = 1 is still a tensor); only its extraction differs: the rank-1 CP of the A_b x B1_b x B2_b Z_b (lx_cp3,
// fold_loop.hpp) in place of the leading singular pair, which leaves wB_b = wK_b (x) wL_b (C order) in the block's resident wB slot.
// The Kronecker loading, the Y^T t sum, the score, the deflation, Wa / Wb and the held-out prediction see a block through wA_b and
// wB_b alone, so they are the code above unchanged; blocks of order 2 and 3 in the same model keep Z / |Z| and lx_rank1, and the
// blocks are visited in list order.  lx_cp3's scratch is shared by the tensor blocks and sized over them.
// LDS (doubles): the formula above with nmax = the largest of min(A_b, B_b) over the blocks of order 2 or 3 and of the shorter side of
// each of the three unfoldings of every tensor block, kmax over the blocks of order 2 or 3 alone (0 without one), then after ys
// lx_cp3's wK (max B1), wL (max B2), v (max B1 B2), tmp (max over A, B1, B2) and part (512), the maxima over the tensor blocks:
//     sum A_b + sum B_b + 4 M + M^2 + nmax + kmax + 2 R^2 + R M + 3 R + max B1 + max B2 + max B1 B2 + max dim + 512
// Workspace per resident fold (doubles): the formula above with that nmax, and lx_cp3's U, yl, vr (Ptmax each, Ptmax = the largest
// P_b of a tensor block) after wk:
//     (I + M) sumP + 3 Pmax + 3 Ptmax + 2 nmax^2 + I (M + R + 2) + R (sum A_b + sum B_b)
// Limits: at most 8 blocks, min(A_b, B_b) <= 256 in a block of order 2 or 3, the shorter side of every unfolding of a tensor block
// <= 256, M <= 128, R <= 64, P_b <= 2^24, LDS <= 150 KB.  A description without a block of order 4 is a bad argument (EINVAL): that
// call is cmtfpls_loo_xcov_coupled_f64's.
#include "fold_loop.hpp"
#include "fold_regress.hpp"

namespace cmtfpls {

constexpr int kLxcMaxBlocks = 8;

struct LooXCoupledArgs {
  const double* X[kLxcMaxBlocks];    // (I, P_b) original, uncentred; null past nb
  const double* cs[kLxcMaxBlocks];   // (P_b) column sums of all samples
  int A[kLxcMaxBlocks], B[kLxcMaxBlocks];
  const double* Y;        // (I, M)
  const double* colsum_y; // (M)
  double* ws;             // per resident fold, see carve-up in the kernel
  double* Ypred;          // (I, M): row i = prediction of the model fitted without sample i
  int* n_iter;            // (I, R), nullable
  int64_t ws_per_fold;    // doubles
  int64_t sumP;
  int nb, I, M, R, max_iter, fold0, nfolds, sumA, sumB, maxP, maxn, maxk;
  double tol;
};

// the trailing dims of the blocks of order 4 (B_b == B1_b * B2_b; B2_b == 0: a block of order 2 or 3) and what lx_cp3's shared
// scratch is sized by: the largest B1, B2, B1 B2, single dim and A B1 B2 over the tensor blocks
struct LooXCoupledTensorArgs : LooXCoupledArgs {
  int B1[kLxcMaxBlocks], B2[kLxcMaxBlocks];
  int b1max, b2max, btmax, dmax, ptmax;
};

template <bool TENSOR>
struct LooXCoupledArgsOf { typedef LooXCoupledArgs type; };
template <>
struct LooXCoupledArgsOf<true> { typedef LooXCoupledTensorArgs type; };

// the TENSOR instantiation runs 512 threads: at 1024 (128 VGPRs a lane) the kernel with lx_cp3 inlined spills, at 512 it does not
constexpr int kLxcTensorNT = 512;

// TENSOR = false: blocks of order 2 or 3, the code this kernel always was.  TENSOR = true: see the head of the file.
template <bool TENSOR>
__global__ __launch_bounds__(TENSOR ? kLxcTensorNT : kLxNT) void loo_xcov_coupled_kernel(typename LooXCoupledArgsOf<TENSOR>::type a) {
  constexpr int NT = TENSOR ? kLxcTensorNT : kLxNT, NW = NT / 64;
  extern __shared__ double sm[];
  __shared__ double red[NW];
  __shared__ double bestv[NW];
  __shared__ int besti[NW];
  __shared__ int sB1[TENSOR ? kLxcMaxBlocks : 1], sB2[TENSOR ? kLxcMaxBlocks : 1];   // (TENSOR only)
  __shared__ double scv[kLxMaxR];
  // the block descriptors in LDS (copied with static indices: a dynamic index into the kernel argument would go through scratch)
  __shared__ const double* sX[kLxcMaxBlocks];
  __shared__ const double* sCs[kLxcMaxBlocks];
  __shared__ long long sOp[kLxcMaxBlocks];                        // P_0 + .. + P_(b-1)
  __shared__ int sA[kLxcMaxBlocks], sB[kLxcMaxBlocks], sOa[kLxcMaxBlocks], sOb[kLxcMaxBlocks];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int I = a.I, M = a.M, R = a.R, nb = a.nb;
  if ((int)blockIdx.x >= a.nfolds) return;
  const int fold = a.fold0 + blockIdx.x;
  if (fold >= I) return;
  if (tid == 0) {
    long long op = 0;
    int oa = 0, ob = 0;
#pragma unroll
    for (int b = 0; b < kLxcMaxBlocks; ++b) {
      sX[b] = a.X[b];
      sCs[b] = a.cs[b];
      sA[b] = a.A[b];
      sB[b] = a.B[b];
      sOp[b] = op;
      sOa[b] = oa;
      sOb[b] = ob;
      if constexpr (TENSOR) {
        sB1[b] = a.B1[b];
        sB2[b] = a.B2[b];
      }
      op += (long long)a.A[b] * a.B[b];
      oa += a.A[b];
      ob += a.B[b];
    }
  }
  const int64_t sumP = a.sumP;
  const int n = a.maxn;
  // global carve-up of this fold's workspace
  double* Xf = a.ws + (int64_t)blockIdx.x * a.ws_per_fold;   // per block I x P_b at I * sOp[b]: centred, held-out row zero, deflated in place
  double* S = Xf + (int64_t)I * sumP;                        // per block M x P_b at M * sOp[b]: cross-covariance of the current component
  double* Z = S + (int64_t)M * sumP;                         // Pmax
  double* Zt = Z + a.maxP;                                   // Pmax    (transpose scratch of the rank-1 extraction)
  double* wk = Zt + a.maxP;                                  // Pmax    kron(wA_b, wB_b) of the block in hand
  double* G0 = wk + a.maxP;                                  // nmax x nmax   (TENSOR: after lx_cp3's U, yl, vr)
  if constexpr (TENSOR) G0 += 3 * (int64_t)a.ptmax;
  double* G1 = G0 + (int64_t)n * n;
  double* Yf = G1 + (int64_t)n * n;                          // I x M
  double* T = Yf + (int64_t)I * M;                           // I x R
  double* u = T + (int64_t)I * R;                            // I
  double* t = u + I;                                         // I
  double* Wa = t + I;                                        // per block R x A_b at R * sOa[b]: loadings of the components so far
  double* Wb = Wa + (int64_t)R * a.sumA;                     // per block R x B_b at R * sOb[b]
  double* H = S;                                             // sumP: the held-out rows of the prediction (S is dead by then)
  // LDS carve-up
  double* wA = sm;                // block b's at sOa[b]
  double* wB = wA + a.sumA;       // block b's at sOb[b]
  double* q = wB + a.sumB;
  double* qn = q + M;
  double* tq = qn + M;
  double* my = tq + M;
  double* Gy = my + M;            // M x M   Y_f^T Y_f of the current component
  double* xs = Gy + M * M;        // nmax
  double* ys = xs + n;            // kmax
  double* coef = ys + a.maxk;     // R x R   (TENSOR: after lx_cp3's wK, wL, v, tmp, part)
  LxTensor lt;
  if constexpr (TENSOR) {         // lx_cp3's scratch, shared by the tensor blocks
    lt.wK = ys + a.maxk;          // b1max
    lt.wL = lt.wK + a.b1max;      // b2max
    lt.v = lt.wL + a.b2max;       // btmax
    lt.tmp = lt.v + a.btmax;      // dmax
    lt.part = lt.tmp + a.dmax;    // NT
    coef = lt.part + NT;
    lt.U = wk + a.maxP;           // ptmax each
    lt.yl = lt.U + a.ptmax;
    lt.vr = lt.yl + a.ptmax;
  }
  double* Qs = coef + R * R;      // R x M
  double* Gn = Qs + R * M;        // (a+1) x (a+1) normal equations
  double* gn = Gn + R * R;
  double* bb = gn + R;
  double* dd = bb + R;
  const double inv = 1.0 / (double)(I - 1);
  const double nbd = (double)nb;

  // ---- preprocess (cmtf.py:44-83): the fold's means by down-dating the column sums; centred copies with the held-out row zero
  for (int o = tid; o < R * R; o += NT) coef[o] = 0.0;
  for (int m = tid; m < M; m += NT) my[m] = (a.colsum_y[m] - a.Y[(int64_t)fold * M + m]) * inv;
  __syncthreads();
  for (int b = 0; b < nb; ++b) {
    const int64_t P = (int64_t)sA[b] * sB[b];
    const double* Xb = sX[b];
    const double* csb = sCs[b];
    double* Xfb = Xf + (int64_t)I * sOp[b];
    for (int64_t c = tid; c < P; c += NT) Z[c] = (csb[c] - Xb[(int64_t)fold * P + c]) * inv;
    __syncthreads();
    for (int r = 0; r < I; ++r) {
      const double* xr = Xb + (int64_t)r * P;
      double* xo = Xfb + (int64_t)r * P;
      if (r == fold) { for (int64_t c = tid; c < P; c += NT) xo[c] = 0.0; }
      else { for (int64_t c = tid; c < P; c += NT) xo[c] = xr[c] - Z[c]; }
    }
    __syncthreads();
  }
  for (int64_t idx = tid; idx < (int64_t)I * M; idx += NT) {
    const int r = (int)(idx / M), m = (int)(idx % M);
    Yf[idx] = (r == fold) ? 0.0 : a.Y[idx] - my[m];
  }
  __syncthreads();

  for (int comp = 0; comp < R; ++comp) {
    // ---- S_b = Y_f^T X_{b,f} of every block and G_y = Y_f^T Y_f of this component (X_{b,f}, Y_f as deflated so far) ----
    for (int b = 0; b < nb; ++b) {
      const int64_t P = (int64_t)sA[b] * sB[b];
      const double* Xfb = Xf + (int64_t)I * sOp[b];
      double* Sb = S + (int64_t)M * sOp[b];
      for (int64_t c = tid; c < P; c += NT) {
        for (int mc = 0; mc < M; mc += 16) {
          double acc[16];
#pragma unroll
          for (int j = 0; j < 16; ++j) acc[j] = 0.0;
          // four rows of the column in flight at a time (loo_xcov.hip: one row per trip leaves the pass bound by memory latency)
          int r = 0;
          for (; r + 4 <= I; r += 4) {
            double x[4];
#pragma unroll
            for (int u4 = 0; u4 < 4; ++u4) x[u4] = Xfb[(int64_t)(r + u4) * P + c];
#pragma unroll
            for (int u4 = 0; u4 < 4; ++u4) {
              const double* yr = Yf + (int64_t)(r + u4) * M + mc;
#pragma unroll
              for (int j = 0; j < 16; ++j)
                if (mc + j < M) acc[j] = fma(yr[j], x[u4], acc[j]);
            }
          }
          for (; r < I; ++r) {
            const double x = Xfb[(int64_t)r * P + c];
            const double* yr = Yf + (int64_t)r * M + mc;
#pragma unroll
            for (int j = 0; j < 16; ++j)
              if (mc + j < M) acc[j] = fma(yr[j], x, acc[j]);
          }
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (mc + j < M) Sb[(int64_t)(mc + j) * P + c] = acc[j];
        }
      }
    }
    for (int o = tid; o < M * M; o += NT) {
      const int m1 = o / M, m2 = o % M;
      double s = 0.0;
      for (int r = 0; r < I; ++r) s = fma(Yf[(int64_t)r * M + m1], Yf[(int64_t)r * M + m2], s);
      Gy[o] = s;
    }
    // ---- the inner loop on the S_b (cmtf.py:89-128) ----
    for (int m = tid; m < M; m += NT) q[m] = (m == 0) ? 1.0 : 0.0;                 // u_0 = Y_f[:, 0] = Y_f e_0 (cmtf.py:90)
    __syncthreads();
    int it = 0;
    for (; it < a.max_iter; ++it) {                                                    // cmtf.py:91
      for (int b = 0; b < nb; ++b) {                                                   // cmtf.py:92, list order
        const int A = sA[b], B = sB[b];
        const int64_t P = (int64_t)A * B;
        const double* Sb = S + (int64_t)M * sOp[b];
        double* wAb = wA + sOa[b];
        double* wBb = wB + sOb[b];
        for (int64_t c = tid; c < P; c += NT) {                                     // Z_b = X_b x_0 u = S_b^T q (cmtf.py:94)
          double s = 0.0;
          int m = 0;
          for (; m + 4 <= M; m += 4) {                                                 // (four rows of S_b in flight; same order of the sum)
            const double s0 = Sb[(int64_t)m * P + c], s1 = Sb[(int64_t)(m + 1) * P + c], s2 = Sb[(int64_t)(m + 2) * P + c], s3 = Sb[(int64_t)(m + 3) * P + c];
            s = fma(q[m], s0, s);
            s = fma(q[m + 1], s1, s);
            s = fma(q[m + 2], s2, s);
            s = fma(q[m + 3], s3, s);
          }
          for (; m < M; ++m) s = fma(q[m], Sb[(int64_t)m * P + c], s);
          Z[c] = s;
        }
        __syncthreads();
        bool cp = false;
        if constexpr (TENSOR) cp = sB2[b] > 0;
        if (cp) {                                                                      // order 4: the rank-1 CP of the A x B1 x B2 Z_b
          if constexpr (TENSOR) {
            lt.B1 = sB1[b];
            lt.B2 = sB2[b];
            lx_cp3<NT>(Z, Zt, A, a.tol, lt, wAb, wBb, G0, G1, xs, red, bestv, besti);   // leaves wB_b = wK_b (x) wL_b
          }
        } else if (A == 1) {                                                           // cmtf.py:98: Z / norm(Z)
          double s = 0.0;
          for (int64_t c = tid; c < P; c += NT) s = fma(Z[c], Z[c], s);
          const double nz = sqrt(lx_sum<NT>(s, red));
          for (int64_t c = tid; c < P; c += NT) wBb[c] = Z[c] / nz;
          if (tid == 0) wAb[0] = 1.0;
          __syncthreads();
        } else {
          lx_rank1<false, NT>(Z, Zt, A, B, wAb, wBb, G0, G1, xs, ys, red, bestv, besti);   // cmtf.py:100-102
        }
        for (int64_t c = tid; c < P; c += NT) wk[c] = wAb[c / B] * wBb[c % B];      // the Kronecker loading, once per extraction
        __syncthreads();
        for (int m = wv; m < M; m += NW) {                                       // Y^T t: + S_b (wA_b (x) wB_b) (cmtf.py:106-121)
          const double s = lx_wave_dot(Sb + (int64_t)m * P, wk, P, lane);
          if (lane == 0) tq[m] = (b == 0) ? s : tq[m] + s;                             // (row m is always this wavefront's)
        }
        __syncthreads();
      }
      double qs = 0.0;
      for (int m = tid; m < M; m += NT) { const double v = tq[m] / nbd; qs = fma(v, v, qs); }   // np.average over the blocks (cmtf.py:120)
      const double qnrm = sqrt(lx_sum<NT>(qs, red));
      for (int m = tid; m < M; m += NT) qn[m] = (tq[m] / nbd) / qnrm;               // cmtf.py:122
      __syncthreads();
      double d2 = 0.0;                                                                 // |u_old - u|^2 = dq^T G_y dq (cmtf.py:123-124)
      for (int o = tid; o < M * M; o += NT) d2 = fma((qn[o / M] - q[o / M]) * Gy[o], qn[o % M] - q[o % M], d2);
      d2 = lx_sum<NT>(d2, red);
      for (int m = tid; m < M; m += NT) q[m] = qn[m];
      __syncthreads();
      if (it > 0 && sqrt(d2 > 0.0 ? d2 : 0.0) < a.tol) { ++it; break; }               // first pass: oldU = inf (cmtf.py:89)
    }
    if (a.n_iter && tid == 0) a.n_iter[(int64_t)fold * R + comp] = it;
    // ---- the component's score t = mean_b X_{b,f} (wA_b (x) wB_b) (cmtf.py:106-120) and Y score with the converged loadings ----
    for (int b = 0; b < nb; ++b) {
      const int B = sB[b];
      const int64_t P = (int64_t)sA[b] * B;
      const double* Xfb = Xf + (int64_t)I * sOp[b];
      const double* wAb = wA + sOa[b];
      const double* wBb = wB + sOb[b];
      for (int64_t c = tid; c < P; c += NT) wk[c] = wAb[c / B] * wBb[c % B];
      __syncthreads();
      for (int r = wv; r < I; r += NW) {
        const double s = lx_wave_dot(Xfb + (int64_t)r * P, wk, P, lane);
        if (lane == 0) t[r] = (b == 0) ? s : t[r] + s;                                 // (row r is always this wavefront's)
      }
      __syncthreads();
    }
    for (int r = tid; r < I; r += NT) {
      const double tr = t[r] / nbd;
      t[r] = tr;
      T[(int64_t)r * R + comp] = tr;
      double s = 0.0;
      for (int m = 0; m < M; ++m) s = fma(Yf[(int64_t)r * M + m], q[m], s);
      u[r] = s;
    }
    for (int b = 0; b < nb; ++b) {
      const int A = sA[b], B = sB[b];
      for (int j = tid; j < A; j += NT) Wa[(int64_t)R * sOa[b] + comp * A + j] = wA[sOa[b] + j];
      for (int j = tid; j < B; j += NT) Wb[(int64_t)R * sOb[b] + comp * B + j] = wB[sOb[b] + j];
    }
    for (int m = tid; m < M; m += NT) Qs[comp * M + m] = q[m];
    __syncthreads();
    // ---- deflate every block by its own t (x) wA_b (x) wB_b (cmtf.py:130-131) ----
    for (int b = 0; b < nb; ++b) {
      const int B = sB[b];
      const int64_t P = (int64_t)sA[b] * B;
      double* Xfb = Xf + (int64_t)I * sOp[b];
      const double* wAb = wA + sOa[b];
      const double* wBb = wB + sOb[b];
      for (int64_t c = tid; c < P; c += NT) wk[c] = wAb[c / B] * wBb[c % B];   // (each thread reads back only what it wrote)
      for (int r = 0; r < I; ++r) {
        const double tr = t[r];
        double* xr = Xfb + (int64_t)r * P;
        for (int64_t c = tid; c < P; c += NT) xr[c] = fma(-tr, wk[c], xr[c]);
      }
    }
    __syncthreads();
    // ---- inner regression b = lstsq(T[:, :k], u) (cmtf.py:135), fold_regress.hpp; then Y -= T b q^T (cmtf.py:138), yhat = T b in t ----
    fold_inner_regression<NT, false>(T, u, nullptr, I, R, comp, Gn, gn, bb, dd, coef, t);
    for (int64_t idx = tid; idx < (int64_t)I * M; idx += NT) {
      const int r = (int)(idx / M), m = (int)(idx % M);
      Yf[idx] = fma(-t[r], q[m], Yf[idx]);
    }
    __syncthreads();
  }

  // ---- predict the held-out sample (cmtf.py:142-177): centre every block's row with the fold's means, project and deflate ----
  for (int b = 0; b < nb; ++b) {
    const int64_t P = (int64_t)sA[b] * sB[b];
    const double* Xb = sX[b];
    const double* csb = sCs[b];
    double* Hb = H + sOp[b];
    for (int64_t c = tid; c < P; c += NT) {
      const double xv = Xb[(int64_t)fold * P + c];
      Hb[c] = xv - (csb[c] - xv) * inv;
    }
  }
  __syncthreads();
  double* sc = scv;                                                                     // scores of the held-out row (R)
  for (int comp = 0; comp < R; ++comp) {
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) {                                                      // cmtf.py:155-171: the block average of the projections
      const int A = sA[b], B = sB[b];
      const int64_t P = (int64_t)A * B;
      const double* Hb = H + sOp[b];
      const double* Wab = Wa + (int64_t)R * sOa[b] + comp * A;
      const double* Wbb = Wb + (int64_t)R * sOb[b] + comp * B;
      double s = 0.0;
      for (int64_t c = tid; c < P; c += NT) s = fma(Hb[c], Wab[c / B] * Wbb[c % B], s);
      acc += lx_sum<NT>(s, red);
    }
    const double sv = acc / nbd;
    if (tid == 0) sc[comp] = sv;
    for (int b = 0; b < nb; ++b) {                                                      // cmtf.py:172-176: each row with its own loadings
      const int A = sA[b], B = sB[b];
      const int64_t P = (int64_t)A * B;
      double* Hb = H + sOp[b];
      const double* Wab = Wa + (int64_t)R * sOa[b] + comp * A;
      const double* Wbb = Wb + (int64_t)R * sOb[b] + comp * B;
      for (int64_t c = tid; c < P; c += NT) Hb[c] = fma(-sv, Wab[c / B] * Wbb[c % B], Hb[c]);
    }
    __syncthreads();
  }
  for (int m = tid; m < M; m += NT) {
    double yv = 0.0;
    for (int b2 = 0; b2 < R; ++b2) {
      double sb = 0.0;
      for (int a2 = 0; a2 < R; ++a2) sb = fma(sc[a2], coef[a2 * R + b2], sb);        // (scores @ coef_)[b]
      yv = fma(sb, Qs[b2 * M + m], yv);                                             // @ Q^T
    }
    a.Ypred[(int64_t)fold * M + m] = yv + my[m];
  }
}

struct LxcShape {
  size_t sumA, sumB, sumP, maxP, maxn, maxk;
};

static LxcShape lxc_shape(const cmtfpls_loo_coupled_block* blocks, int nb) {
  LxcShape s = {0, 0, 0, 0, 0, 0};
  for (int b = 0; b < nb; ++b) {
    const size_t A = (size_t)blocks[b].A, B = (size_t)blocks[b].B, n = A < B ? A : B, k = A < B ? B : A;
    s.sumA += A;
    s.sumB += B;
    s.sumP += A * B;
    s.maxP = A * B > s.maxP ? A * B : s.maxP;
    s.maxn = n > s.maxn ? n : s.maxn;
    s.maxk = k > s.maxk ? k : s.maxk;
  }
  return s;
}

static size_t lxc_lds_bytes(const LxcShape& s, int M, int R) {
  const size_t dbl = s.sumA + s.sumB + 4 * (size_t)M + (size_t)M * M + s.maxn + s.maxk + 2 * (size_t)R * R + (size_t)R * M + 3 * (size_t)R;
  return dbl * sizeof(double);
}

static bool lxc_sizes_ok(const cmtfpls_loo_coupled_block* blocks, int nb, int I, int M, int R) {
  if (!blocks || nb <= 0 || nb > kLxcMaxBlocks || I <= 1 || M <= 0 || R <= 0) return false;
  for (int b = 0; b < nb; ++b)
    if (blocks[b].A <= 0 || blocks[b].B <= 0) return false;
  return true;
}

// ---- blocks of order 4 (cmtfpls_loo_xcov_coupled_tensor_f64) ---------------------------------------------------------------------
static int lxc_tensor_short(int A, int B1, int B2, int mode) {
  const int64_t d = mode == 0 ? A : mode == 1 ? B1 : B2, rest = (int64_t)A * B1 * B2 / d;
  return (int)(d < rest ? d : rest);
}

// LxcShape with maxn over the order-2/3 blocks' min(A, B) and the shorter side of every unfolding of every tensor block, maxk over
// the order-2/3 blocks alone (a tensor block has no ys), and what lx_cp3's shared scratch is sized by
struct LxcTensorShape {
  LxcShape s;
  size_t b1max, b2max, btmax, dmax, ptmax;
  int tensors;
};

static LxcTensorShape lxc_tensor_shape(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims) {
  LxcTensorShape o = {{0, 0, 0, 0, 0, 0}, 0, 0, 0, 0, 0, 0};
  for (int b = 0; b < nb; ++b) {
    const size_t A = (size_t)blocks[b].A, B = (size_t)blocks[b].B, B1 = (size_t)dims[2 * b], B2 = (size_t)dims[2 * b + 1];
    size_t n;
    o.s.sumA += A;
    o.s.sumB += B;
    o.s.sumP += A * B;
    o.s.maxP = A * B > o.s.maxP ? A * B : o.s.maxP;
    if (B2 > 0) {
      n = 0;
      for (int m = 0; m < 3; ++m) {
        const size_t sh = (size_t)lxc_tensor_short((int)A, (int)B1, (int)B2, m);
        n = sh > n ? sh : n;
      }
      const size_t dm = A > B1 ? (A > B2 ? A : B2) : (B1 > B2 ? B1 : B2);
      o.b1max = B1 > o.b1max ? B1 : o.b1max;
      o.b2max = B2 > o.b2max ? B2 : o.b2max;
      o.btmax = B > o.btmax ? B : o.btmax;
      o.dmax = dm > o.dmax ? dm : o.dmax;
      o.ptmax = A * B > o.ptmax ? A * B : o.ptmax;
      ++o.tensors;
    } else {
      n = A < B ? A : B;
      const size_t k = A < B ? B : A;
      o.s.maxk = k > o.s.maxk ? k : o.s.maxk;
    }
    o.s.maxn = n > o.s.maxn ? n : o.s.maxn;
  }
  return o;
}

// lxc_lds_bytes, then lx_cp3's wK (b1max), wL (b2max), v (btmax), tmp (dmax) and part (the workgroup's 512 threads)
static size_t lxc_tensor_lds_bytes(const LxcTensorShape& o, int M, int R) {
  return lxc_lds_bytes(o.s, M, R) + (o.b1max + o.b2max + o.btmax + o.dmax + kLxcTensorNT) * sizeof(double);
}

// what the size functions and the entry call a well-formed description: lxc_sizes_ok, dims without a negative entry, order 4 exactly
// where B2 > 0 (then B1 B2 == B), no order above 4 and at least one block of order 4; P_b <= 2^24 keeps the sums in range
static bool lxc_tensor_dims_ok(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims) {
  if (!dims) return false;
  int tensors = 0;
  for (int b = 0; b < nb; ++b) {
    const int B1 = dims[2 * b], B2 = dims[2 * b + 1], order = blocks[b].order;
    if (B1 < 0 || B2 < 0 || order > 4 || (order == 4) != (B2 > 0)) return false;
    if (B2 > 0 && (int64_t)B1 * B2 != (int64_t)blocks[b].B) return false;
    tensors += B2 > 0;
  }
  return tensors > 0;
}

static bool lxc_cells_ok(const cmtfpls_loo_coupled_block* blocks, int nb) {
  for (int b = 0; b < nb; ++b)
    if ((int64_t)blocks[b].A * blocks[b].B > (int64_t)1 << 24) return false;
  return true;
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {

size_t cmtfpls_loo_xcov_coupled_fold_workspace_bytes(const cmtfpls_loo_coupled_block* blocks, int nb, int I, int M, int R) {
  if (!lxc_sizes_ok(blocks, nb, I, M, R)) return 0;
  const LxcShape s = lxc_shape(blocks, nb);
  return (((size_t)I + M) * s.sumP + 3 * s.maxP + 2 * s.maxn * s.maxn + (size_t)I * ((size_t)M + R + 2) + (size_t)R * (s.sumA + s.sumB)) *
         sizeof(double);
}

size_t cmtfpls_loo_xcov_coupled_lds_bytes(const cmtfpls_loo_coupled_block* blocks, int nb, int I, int M, int R) {
  if (!lxc_sizes_ok(blocks, nb, I, M, R)) return 0;
  return lxc_lds_bytes(lxc_shape(blocks, nb), M, R);
}

int cmtfpls_loo_xcov_coupled_f64(const cmtfpls_loo_coupled_block* blocks, int nb, const double* Y, const double* colsum_y, int I, int M,
                                 int R, double tol, int max_iter, int fold0, int nfolds, double* Ypred, int* n_iter, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (!blocks || !Y || !colsum_y || !Ypred || nb <= 0 || I <= 1 || M <= 0 || R <= 0 || max_iter <= 0 || fold0 < 0 || nfolds <= 0 ||
      fold0 + nfolds > I) {
    set_error("loo_xcov_coupled: bad argument");
    return CMTFPLS_EINVAL;
  }
  if (nb > kLxcMaxBlocks) {
    set_error("loo_xcov_coupled: more than 8 blocks; refit per fold on the regular engine");
    return CMTFPLS_EUNSUPPORTED;
  }
  for (int b = 0; b < nb; ++b) {
    const cmtfpls_loo_coupled_block& k = blocks[b];
    if (!k.X || !k.colsum || k.A <= 0 || k.B <= 0 || k.order < 2 || (k.order == 2 && k.A != 1)) {
      set_error("loo_xcov_coupled: bad block");
      return CMTFPLS_EINVAL;
    }
  }
  for (int b = 0; b < nb; ++b)
    if (blocks[b].order > 3) {
      set_error("loo_xcov_coupled: a block of order > 3; refit per fold on the regular engine");
      return CMTFPLS_EUNSUPPORTED;
    }
  for (int b = 0; b < nb; ++b)
    if ((blocks[b].A < blocks[b].B ? blocks[b].A : blocks[b].B) > kLxMaxN) {
      set_error("loo_xcov_coupled: min(A, B) > 256 in a block; refit per fold on the regular engine");
      return CMTFPLS_EUNSUPPORTED;
    }
  if (M > kLxMaxM) { set_error("loo_xcov_coupled: M > 128; refit per fold on the regular engine"); return CMTFPLS_EUNSUPPORTED; }
  if (R > kLxMaxR) { set_error("loo_xcov_coupled: R > 64; refit per fold on the regular engine"); return CMTFPLS_EUNSUPPORTED; }
  for (int b = 0; b < nb; ++b)
    if ((int64_t)blocks[b].A * blocks[b].B > (int64_t)1 << 24) {
      set_error("loo_xcov_coupled: A * B > 2^24 in a block; refit per fold on the regular engine");
      return CMTFPLS_EUNSUPPORTED;
    }
  const LxcShape s = lxc_shape(blocks, nb);
  const size_t lds = lxc_lds_bytes(s, M, R);
  if (lds > 150 * 1024) {
    set_error("loo_xcov_coupled: the fold's vectors exceed 150 KB of LDS; refit per fold on the regular engine");
    return CMTFPLS_EUNSUPPORTED;
  }
  const size_t per = cmtfpls_loo_xcov_coupled_fold_workspace_bytes(blocks, nb, I, M, R);
  if (!ws || ws_bytes < per * (size_t)nfolds) { set_error("loo_xcov_coupled: workspace too small"); return CMTFPLS_EWORKSPACE; }
  LooXCoupledArgs a;
  for (int b = 0; b < kLxcMaxBlocks; ++b) {
    a.X[b] = b < nb ? blocks[b].X : nullptr;
    a.cs[b] = b < nb ? blocks[b].colsum : nullptr;
    a.A[b] = b < nb ? blocks[b].A : 0;
    a.B[b] = b < nb ? blocks[b].B : 0;
  }
  a.Y = Y; a.colsum_y = colsum_y; a.ws = static_cast<double*>(ws); a.Ypred = Ypred; a.n_iter = n_iter;
  a.ws_per_fold = (int64_t)(per / sizeof(double));
  a.sumP = (int64_t)s.sumP;
  a.nb = nb; a.I = I; a.M = M; a.R = R; a.max_iter = max_iter; a.fold0 = fold0; a.nfolds = nfolds;
  a.sumA = (int)s.sumA; a.sumB = (int)s.sumB; a.maxP = (int)s.maxP; a.maxn = (int)s.maxn; a.maxk = (int)s.maxk;
  a.tol = tol;
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(loo_xcov_coupled_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  hipLaunchKernelGGL(loo_xcov_coupled_kernel<false>, dim3(nfolds), dim3(kLxNT), lds, (hipStream_t)stream, a);
  return check_launch("loo_xcov_coupled");
}

size_t cmtfpls_loo_xcov_coupled_tensor_fold_workspace_bytes(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims, int I, int M,
                                                            int R) {
  if (!lxc_sizes_ok(blocks, nb, I, M, R) || !lxc_tensor_dims_ok(blocks, nb, dims) || !lxc_cells_ok(blocks, nb)) return 0;
  const LxcTensorShape o = lxc_tensor_shape(blocks, nb, dims);
  return (((size_t)I + M) * o.s.sumP + 3 * o.s.maxP + 3 * o.ptmax + 2 * o.s.maxn * o.s.maxn + (size_t)I * ((size_t)M + R + 2) +
          (size_t)R * (o.s.sumA + o.s.sumB)) * sizeof(double);
}

size_t cmtfpls_loo_xcov_coupled_tensor_lds_bytes(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims, int I, int M, int R) {
  if (!lxc_sizes_ok(blocks, nb, I, M, R) || !lxc_tensor_dims_ok(blocks, nb, dims) || !lxc_cells_ok(blocks, nb)) return 0;
  return lxc_tensor_lds_bytes(lxc_tensor_shape(blocks, nb, dims), M, R);
}

int cmtfpls_loo_xcov_coupled_tensor_f64(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims, const double* Y,
                                        const double* colsum_y, int I, int M, int R, double tol, int max_iter, int fold0, int nfolds,
                                        double* Ypred, int* n_iter, void* ws, size_t ws_bytes, void* stream) {
  if (!blocks || !dims || !Y || !colsum_y || !Ypred || nb <= 0 || I <= 1 || M <= 0 || R <= 0 || max_iter <= 0 || fold0 < 0 ||
      nfolds <= 0 || fold0 + nfolds > I) {
    set_error("loo_xcov_coupled_tensor: bad argument");
    return CMTFPLS_EINVAL;
  }
  for (int b = 0; b < nb; ++b) {
    const cmtfpls_loo_coupled_block& k = blocks[b];
    if (!k.X || !k.colsum || k.A <= 0 || k.B <= 0 || k.order < 2 || (k.order == 2 && k.A != 1)) {
      set_error("loo_xcov_coupled_tensor: bad block");
      return CMTFPLS_EINVAL;
    }
  }
  if (!lxc_tensor_dims_ok(blocks, nb, dims)) {
    set_error("loo_xcov_coupled_tensor: bad dims ((B1, B2) with B1 * B2 == B for every block of order 4 and at least one such block, "
              "(0, 0) for a block of order 2 or 3; no order above 4)");
    return CMTFPLS_EINVAL;
  }
  if (nb > kLxcMaxBlocks) {
    set_error("loo_xcov_coupled_tensor: more than 8 blocks; refit per fold on the regular engine");
    return CMTFPLS_EUNSUPPORTED;
  }
  for (int b = 0; b < nb; ++b)
    if (dims[2 * b + 1] == 0 && (blocks[b].A < blocks[b].B ? blocks[b].A : blocks[b].B) > kLxMaxN) {
      set_error("loo_xcov_coupled_tensor: min(A, B) > 256 in a block of order 2 or 3; refit per fold on the regular engine");
      return CMTFPLS_EUNSUPPORTED;
    }
  for (int b = 0; b < nb; ++b)
    for (int m = 0; m < 3 && dims[2 * b + 1] > 0; ++m)
      if (lxc_tensor_short(blocks[b].A, dims[2 * b], dims[2 * b + 1], m) > kLxMaxN) {
        set_error("loo_xcov_coupled_tensor: an unfolding of a block's A x B1 x B2 with its shorter side > 256; refit per fold on the "
                  "regular engine");
        return CMTFPLS_EUNSUPPORTED;
      }
  if (M > kLxMaxM) { set_error("loo_xcov_coupled_tensor: M > 128; refit per fold on the regular engine"); return CMTFPLS_EUNSUPPORTED; }
  if (R > kLxMaxR) { set_error("loo_xcov_coupled_tensor: R > 64; refit per fold on the regular engine"); return CMTFPLS_EUNSUPPORTED; }
  if (!lxc_cells_ok(blocks, nb)) {
    set_error("loo_xcov_coupled_tensor: A * B > 2^24 in a block; refit per fold on the regular engine");
    return CMTFPLS_EUNSUPPORTED;
  }
  const LxcTensorShape o = lxc_tensor_shape(blocks, nb, dims);
  const size_t lds = lxc_tensor_lds_bytes(o, M, R);
  if (lds > 150 * 1024) {
    set_error("loo_xcov_coupled_tensor: the fold's vectors exceed 150 KB of LDS; refit per fold on the regular engine");
    return CMTFPLS_EUNSUPPORTED;
  }
  const size_t per = cmtfpls_loo_xcov_coupled_tensor_fold_workspace_bytes(blocks, nb, dims, I, M, R);
  if (!ws || ws_bytes < per * (size_t)nfolds) { set_error("loo_xcov_coupled_tensor: workspace too small"); return CMTFPLS_EWORKSPACE; }
  LooXCoupledTensorArgs a;
  for (int b = 0; b < kLxcMaxBlocks; ++b) {
    a.X[b] = b < nb ? blocks[b].X : nullptr;
    a.cs[b] = b < nb ? blocks[b].colsum : nullptr;
    a.A[b] = b < nb ? blocks[b].A : 0;
    a.B[b] = b < nb ? blocks[b].B : 0;
    a.B1[b] = b < nb ? dims[2 * b] : 0;
    a.B2[b] = b < nb ? dims[2 * b + 1] : 0;
  }
  a.Y = Y; a.colsum_y = colsum_y; a.ws = static_cast<double*>(ws); a.Ypred = Ypred; a.n_iter = n_iter;
  a.ws_per_fold = (int64_t)(per / sizeof(double));
  a.sumP = (int64_t)o.s.sumP;
  a.nb = nb; a.I = I; a.M = M; a.R = R; a.max_iter = max_iter; a.fold0 = fold0; a.nfolds = nfolds;
  a.sumA = (int)o.s.sumA; a.sumB = (int)o.s.sumB; a.maxP = (int)o.s.maxP; a.maxn = (int)o.s.maxn; a.maxk = (int)o.s.maxk;
  a.b1max = (int)o.b1max; a.b2max = (int)o.b2max; a.btmax = (int)o.btmax; a.dmax = (int)o.dmax; a.ptmax = (int)o.ptmax;
  a.tol = tol;
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(loo_xcov_coupled_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  hipLaunchKernelGGL(loo_xcov_coupled_kernel<true>, dim3(nfolds), dim3(kLxcTensorNT), lds, (hipStream_t)stream, a);
  return check_launch("loo_xcov_coupled_tensor");
}

}  // extern "C"
