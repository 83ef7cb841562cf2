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
// The steps are loo_xcov.hip's, called once per block: loo_xcov_fold.hpp for the fold's own, fold_loop.hpp for a pass of the inner
// loop.  This kernel keeps the block descriptors in LDS, the block-order sums into tq and t with their / nb, the Kronecker loading
// recomputed per block (one wk buffer serves all blocks), and the 512-thread TENSOR instantiation.
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
#include <string>
#include "loo_xcov_fold.hpp"

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
  if constexpr (TENSOR) {         // lx_cp3's scratch, shared by the tensor blocks: LDS after ys, global after wk
    lt = lx_tensor_scratch(ys + a.maxk, wk + a.maxP, a.b1max, a.b2max, a.btmax, a.dmax, a.ptmax, NT);
    coef = lt.part + NT;
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
  lxf_mean_y<NT>(a.Y, a.colsum_y, fold, M, inv, my);
  __syncthreads();
  for (int b = 0; b < nb; ++b) {
    lxf_centre_block<NT>(sX[b], sCs[b], fold, I, (int64_t)sA[b] * sB[b], inv, Z, Xf + (int64_t)I * sOp[b]);
    __syncthreads();
  }
  lxf_centre_y<NT>(a.Y, my, fold, I, M, Yf);

  for (int comp = 0; comp < R; ++comp) {
    // ---- S_b = Y_f^T X_{b,f} of every block and G_y = Y_f^T Y_f of this component (X_{b,f}, Y_f as deflated so far) ----
    for (int b = 0; b < nb; ++b)
      lxf_build_s<NT>(Xf + (int64_t)I * sOp[b], Yf, I, (int64_t)sA[b] * sB[b], M, S + (int64_t)M * sOp[b]);
    lxf_gram_y<NT>(Yf, I, M, Gy);
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
        lx_z_from_s<NT>(Sb, q, Z, P, M);                                               // cmtf.py:94
        if constexpr (TENSOR) {                                                        // B2 > 0: order 4, lx_cp3 leaves wB_b = wK_b (x) wL_b
          lt.B1 = sB1[b];
          lt.B2 = sB2[b];
        }
        lx_extract<TENSOR, NT>(Z, Zt, A, B, P, a.tol, lt, wAb, wBb, G0, G1, xs, ys, red, bestv, besti);   // cmtf.py:98-104
        lx_kron<NT>(wk, wAb, wBb, P, B);                                               // once per extraction
        __syncthreads();
        // Y^T t: + S_b (wA_b (x) wB_b) (cmtf.py:106-121), assigned by block 0 and added in block order; / nb in lx_q_step
        lx_row_dots<NT>(Sb, wk, P, M, lane, wv, [tq, b](int m, double s) { tq[m] = (b == 0) ? s : tq[m] + s; });
        __syncthreads();
      }
      if (lx_q_step<NT>(tq, nbd, q, qn, Gy, M, a.tol, it, red)) { ++it; break; }     // np.average over the blocks (cmtf.py:120-124)
    }
    if (a.n_iter && tid == 0) a.n_iter[(int64_t)fold * R + comp] = it;
    // ---- the component's score t = mean_b X_{b,f} (wA_b (x) wB_b) (cmtf.py:106-120) and Y score with the converged loadings ----
    for (int b = 0; b < nb; ++b) {
      const int64_t P = (int64_t)sA[b] * sB[b];
      lx_kron<NT>(wk, wA + sOa[b], wB + sOb[b], P, sB[b]);
      __syncthreads();
      lx_row_dots<NT>(Xf + (int64_t)I * sOp[b], wk, P, I, lane, wv, [t, b](int r, double s) { t[r] = (b == 0) ? s : t[r] + s; });
      __syncthreads();
    }
    for (int r = tid; r < I; r += NT) {                // (the Y score stays in this loop: as lxf_y_score in a loop of its own it spills)
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
      const int64_t P = (int64_t)sA[b] * sB[b];
      lx_kron<NT>(wk, wA + sOa[b], wB + sOb[b], P, sB[b]);                             // (each thread reads back only what it wrote)
      lxf_deflate<NT>(Xf + (int64_t)I * sOp[b], t, wk, I, P);
    }
    __syncthreads();
    lxf_regress_deflate_y<NT>(T, u, I, M, R, comp, Gn, gn, bb, dd, coef, t, q, Yf);   // cmtf.py:135-138
  }

  // ---- predict the held-out sample (cmtf.py:142-177): centre every block's row with the fold's means, project and deflate ----
  for (int b = 0; b < nb; ++b) lxf_heldout_row<NT>(sX[b], sCs[b], fold, (int64_t)sA[b] * sB[b], inv, H + sOp[b]);
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
  lxf_predict<NT>(sc, coef, Qs, my, R, M, a.Ypred + (int64_t)fold * M);
}

// what the kernel's LDS and workspace are sized by: sums and maxima over the blocks; maxn over the order-2/3 blocks' min(A, B) and
// the shorter side of every unfolding of every tensor block, maxk over the order-2/3 blocks' max(A, B) alone (a tensor block has no
// ys); lx_cp3's shared scratch by the largest B1, B2, B1 B2, single dim and A B1 B2 over the tensor blocks
struct LxcShape {
  size_t sumA, sumB, sumP, maxP, maxn, maxk;
  size_t b1max, b2max, btmax, dmax, ptmax;
};

// dims: (B1, B2) per block, B2 > 0 a block of order 4; null: no such block (cmtfpls_loo_xcov_coupled_f64)
static LxcShape lxc_shape(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims) {
  LxcShape o = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = 0; b < nb; ++b) {
    const size_t A = (size_t)blocks[b].A, B = (size_t)blocks[b].B, B1 = dims ? (size_t)dims[2 * b] : 0, B2 = dims ? (size_t)dims[2 * b + 1] : 0;
    size_t n;
    o.sumA += A;
    o.sumB += B;
    o.sumP += A * B;
    o.maxP = A * B > o.maxP ? A * B : o.maxP;
    if (B2 > 0) {
      n = (size_t)lx_tensor_nmax((int)A, (int)B1, (int)B2);
      const size_t dm = A > B1 ? (A > B2 ? A : B2) : (B1 > B2 ? B1 : B2);
      o.b1max = B1 > o.b1max ? B1 : o.b1max;
      o.b2max = B2 > o.b2max ? B2 : o.b2max;
      o.btmax = B > o.btmax ? B : o.btmax;
      o.dmax = dm > o.dmax ? dm : o.dmax;
      o.ptmax = A * B > o.ptmax ? A * B : o.ptmax;
    } else {
      n = A < B ? A : B;
      const size_t k = A < B ? B : A;
      o.maxk = k > o.maxk ? k : o.maxk;
    }
    o.maxn = n > o.maxn ? n : o.maxn;
  }
  return o;
}

// the kernel's LDS carve-up; TENSOR: then lx_cp3's wK (b1max), wL (b2max), v (btmax), tmp (dmax) and part (the workgroup's 512 threads)
template <bool TENSOR>
static size_t lxc_lds_bytes(const LxcShape& s, int M, int R) {
  const size_t dbl = s.sumA + s.sumB + 4 * (size_t)M + (size_t)M * M + s.maxn + s.maxk + 2 * (size_t)R * R + (size_t)R * M + 3 * (size_t)R;
  return (dbl + (TENSOR ? s.b1max + s.b2max + s.btmax + s.dmax + kLxcTensorNT : 0)) * sizeof(double);
}

// the kernel's global carve-up per resident fold; TENSOR: with lx_cp3's U, yl, vr (ptmax each)
template <bool TENSOR>
static size_t lxc_ws_bytes(const LxcShape& s, int I, int M, int R) {
  return (((size_t)I + M) * s.sumP + 3 * s.maxP + (TENSOR ? 3 * s.ptmax : 0) + 2 * s.maxn * s.maxn + (size_t)I * ((size_t)M + R + 2) +
          (size_t)R * (s.sumA + s.sumB)) * sizeof(double);
}

static bool lxc_sizes_ok(const cmtfpls_loo_coupled_block* blocks, int nb, int I, int M, int R) {
  if (!blocks || nb <= 0 || nb > kLxcMaxBlocks || I <= 1 || M <= 0 || R <= 0) return false;
  for (int b = 0; b < nb; ++b)
    if (blocks[b].A <= 0 || blocks[b].B <= 0) return false;
  return true;
}

// what the tensor size functions and entry call a well-formed description: lxc_sizes_ok, dims without a negative entry, order 4
// exactly where B2 > 0 (then B1 B2 == B), no order above 4 and at least one block of order 4; P_b <= 2^24 keeps the sums in range
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

// The checks, argument fill and launch of the two entries: cmtfpls_loo_xcov_coupled_f64 (TENSOR = false, dims null) and
// cmtfpls_loo_xcov_coupled_tensor_f64.  Each keeps the order of its checks: only where "more than 8 blocks" is tested differs, and
// what a block's short side is.
template <bool TENSOR>
static int lxc_run(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims, const double* Y, const double* colsum_y, int I, int M,
                   int R, double tol, int max_iter, int fold0, int nfolds, double* Ypred, int* n_iter, void* ws, size_t ws_bytes,
                   void* stream) {
  const std::string who = TENSOR ? "loo_xcov_coupled_tensor" : "loo_xcov_coupled";
  const std::string refit = "; refit per fold on the regular engine";
  auto fail = [&](int code, const std::string& what) { set_error((who + ": " + what).c_str()); return code; };
  if (!blocks || (TENSOR && !dims) || !Y || !colsum_y || !Ypred || nb <= 0 || I <= 1 || M <= 0 || R <= 0 || max_iter <= 0 || fold0 < 0 ||
      nfolds <= 0 || fold0 + nfolds > I)
    return fail(CMTFPLS_EINVAL, "bad argument");
  if (!TENSOR && nb > kLxcMaxBlocks) return fail(CMTFPLS_EUNSUPPORTED, "more than 8 blocks" + refit);
  for (int b = 0; b < nb; ++b) {
    const cmtfpls_loo_coupled_block& k = blocks[b];
    if (!k.X || !k.colsum || k.A <= 0 || k.B <= 0 || k.order < 2 || (k.order == 2 && k.A != 1)) return fail(CMTFPLS_EINVAL, "bad block");
  }
  if constexpr (TENSOR) {
    if (!lxc_tensor_dims_ok(blocks, nb, dims))
      return fail(CMTFPLS_EINVAL, "bad dims ((B1, B2) with B1 * B2 == B for every block of order 4 and at least one such block, "
                                  "(0, 0) for a block of order 2 or 3; no order above 4)");
    if (nb > kLxcMaxBlocks) return fail(CMTFPLS_EUNSUPPORTED, "more than 8 blocks" + refit);
  } else {
    for (int b = 0; b < nb; ++b)
      if (blocks[b].order > 3) return fail(CMTFPLS_EUNSUPPORTED, "a block of order > 3" + refit);
  }
  for (int b = 0; b < nb; ++b)
    if (!(TENSOR && dims[2 * b + 1] > 0) && (blocks[b].A < blocks[b].B ? blocks[b].A : blocks[b].B) > kLxMaxN)
      return fail(CMTFPLS_EUNSUPPORTED, (TENSOR ? "min(A, B) > 256 in a block of order 2 or 3" : "min(A, B) > 256 in a block") + refit);
  if constexpr (TENSOR)
    for (int b = 0; b < nb; ++b)
      for (int m = 0; m < 3 && dims[2 * b + 1] > 0; ++m)
        if (lx_tensor_short(blocks[b].A, dims[2 * b], dims[2 * b + 1], m) > kLxMaxN)
          return fail(CMTFPLS_EUNSUPPORTED, "an unfolding of a block's A x B1 x B2 with its shorter side > 256" + refit);
  if (M > kLxMaxM) return fail(CMTFPLS_EUNSUPPORTED, "M > 128" + refit);
  if (R > kLxMaxR) return fail(CMTFPLS_EUNSUPPORTED, "R > 64" + refit);
  if (!lxc_cells_ok(blocks, nb)) return fail(CMTFPLS_EUNSUPPORTED, "A * B > 2^24 in a block" + refit);
  const LxcShape s = lxc_shape(blocks, nb, dims);
  const size_t lds = lxc_lds_bytes<TENSOR>(s, M, R);
  if (lds > 150 * 1024) return fail(CMTFPLS_EUNSUPPORTED, "the fold's vectors exceed 150 KB of LDS" + refit);
  const size_t per = lxc_ws_bytes<TENSOR>(s, I, M, R);
  if (!ws || ws_bytes < per * (size_t)nfolds) return fail(CMTFPLS_EWORKSPACE, "workspace too small");
  typename LooXCoupledArgsOf<TENSOR>::type a;
  for (int b = 0; b < kLxcMaxBlocks; ++b) {
    a.X[b] = b < nb ? blocks[b].X : nullptr;
    a.cs[b] = b < nb ? blocks[b].colsum : nullptr;
    a.A[b] = b < nb ? blocks[b].A : 0;
    a.B[b] = b < nb ? blocks[b].B : 0;
    if constexpr (TENSOR) {
      a.B1[b] = b < nb ? dims[2 * b] : 0;
      a.B2[b] = b < nb ? dims[2 * b + 1] : 0;
    }
  }
  a.Y = Y; a.colsum_y = colsum_y; a.ws = static_cast<double*>(ws); a.Ypred = Ypred; a.n_iter = n_iter;
  a.ws_per_fold = (int64_t)(per / sizeof(double));
  a.sumP = (int64_t)s.sumP;
  a.nb = nb; a.I = I; a.M = M; a.R = R; a.max_iter = max_iter; a.fold0 = fold0; a.nfolds = nfolds;
  a.sumA = (int)s.sumA; a.sumB = (int)s.sumB; a.maxP = (int)s.maxP; a.maxn = (int)s.maxn; a.maxk = (int)s.maxk;
  if constexpr (TENSOR) {
    a.b1max = (int)s.b1max; a.b2max = (int)s.b2max; a.btmax = (int)s.btmax; a.dmax = (int)s.dmax; a.ptmax = (int)s.ptmax;
  }
  a.tol = tol;
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(loo_xcov_coupled_kernel<TENSOR>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  hipLaunchKernelGGL(loo_xcov_coupled_kernel<TENSOR>, dim3(nfolds), dim3(TENSOR ? kLxcTensorNT : kLxNT), lds, (hipStream_t)stream, a);
  return check_launch(who.c_str());
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {

size_t cmtfpls_loo_xcov_coupled_fold_workspace_bytes(const cmtfpls_loo_coupled_block* blocks, int nb, int I, int M, int R) {
  if (!lxc_sizes_ok(blocks, nb, I, M, R)) return 0;
  return lxc_ws_bytes<false>(lxc_shape(blocks, nb, nullptr), I, M, R);
}

size_t cmtfpls_loo_xcov_coupled_lds_bytes(const cmtfpls_loo_coupled_block* blocks, int nb, int I, int M, int R) {
  if (!lxc_sizes_ok(blocks, nb, I, M, R)) return 0;
  return lxc_lds_bytes<false>(lxc_shape(blocks, nb, nullptr), M, R);
}

int cmtfpls_loo_xcov_coupled_f64(const cmtfpls_loo_coupled_block* blocks, int nb, const double* Y, const double* colsum_y, int I, int M,
                                 int R, double tol, int max_iter, int fold0, int nfolds, double* Ypred, int* n_iter, void* ws,
                                 size_t ws_bytes, void* stream) {
  return lxc_run<false>(blocks, nb, nullptr, Y, colsum_y, I, M, R, tol, max_iter, fold0, nfolds, Ypred, n_iter, ws, ws_bytes, stream);
}

size_t cmtfpls_loo_xcov_coupled_tensor_fold_workspace_bytes(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims, int I, int M,
                                                            int R) {
  if (!lxc_sizes_ok(blocks, nb, I, M, R) || !lxc_tensor_dims_ok(blocks, nb, dims) || !lxc_cells_ok(blocks, nb)) return 0;
  return lxc_ws_bytes<true>(lxc_shape(blocks, nb, dims), I, M, R);
}

size_t cmtfpls_loo_xcov_coupled_tensor_lds_bytes(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims, int I, int M, int R) {
  if (!lxc_sizes_ok(blocks, nb, I, M, R) || !lxc_tensor_dims_ok(blocks, nb, dims) || !lxc_cells_ok(blocks, nb)) return 0;
  return lxc_lds_bytes<true>(lxc_shape(blocks, nb, dims), M, R);
}

int cmtfpls_loo_xcov_coupled_tensor_f64(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims, const double* Y,
                                        const double* colsum_y, int I, int M, int R, double tol, int max_iter, int fold0, int nfolds,
                                        double* Ypred, int* n_iter, void* ws, size_t ws_bytes, void* stream) {
  return lxc_run<true>(blocks, nb, dims, Y, colsum_y, I, M, R, tol, max_iter, fold0, nfolds, Ypred, n_iter, ws, ws_bytes, stream);
}

}  // extern "C"
