// Refits of a small coupled model (ctPLS: nb blocks sharing the sample mode and ONE score) whose blocks have missing values, on
// count-weighted rows, ALL MODELS OF A CHUNK IN ONE LAUNCH: K-fold and leave-one-out Q2Y, the permutation test, repeated K-fold and
// the bootstrap of such data (validate.py with EngineOptions.masked_folds_coupled).  The count-weighted model of cv_masked.hip
// for 1 <= nb <= 8 blocks, the steps of masked_fold.hpp once per block: model m is counts[m, r] >= 0 copies of row r of EVERY block
// paired with Y[yrow[m, r]] (yrow nullable = identity); the reference's ctPLS.fit (cmtf.py:87-139) on that literal data, the
// missing-value arithmetic switched on BLOCK BY BLOCK (Xs_hasMiss[ti], cmtf.py:77-82, 92-121), every sum over rows weighted by c_r.
// Then the rows with c_r = 0 are predicted as one batch (cmtf.py:141-175) with every component count.  One 256-thread workgroup per
// model; the model's centred working copies in the workspace, deflated in place; the vectors in LDS.
//
// With n = sum_r c_r and, per block b (I x A_b x B_b, a matrix block A_b = 1, P_b = A_b B_b), Xf^b zero at held-out rows and
// missing entries:
//   c_p^b  = sum_r c_r [x^b_rp observed];  mu^b_p = sum_r c_r x^b_rp / c_p^b (NaN if 0);  nu = sum_r c_r Y[yrow r] / n   (cmtf.py:74-75)
//   miss_b = some c_p^b < n: the reference's Xs_hasMiss[b] on the resampled data; a complete block takes the unmasked sums
//   Z^b_p  = sum_r c_r Xf^b_rp u_r, and when miss_b: / c_p^b * n, 0 where c_p^b = 0                              (cmtf.py:92-95)
//   w^b    = rank-1 of Z^b (A_b = 1: Z / |Z|), loo_rank1.hpp's sign rule                                         (cmtf.py:97-103)
//   t^b_r  = sum_p Xf^b_rp w^b_p, and when miss_b: / o^b_r * P_b (o^b_r = observed entries of row r of block b)  (cmtf.py:105-118)
//   t      = (t^0 + .. + t^(nb-1)) / nb, the blocks added in order; held-out rows 0                              (cmtf.py:119)
//   q      = sum_r c_r Yf_r t_r normalised, u = Yf q, stop on sqrt(sum_r c_r (u_r - u_old,r)^2) < tol            (cmtf.py:120-128)
//   every block deflated by the shared t on its observed training entries; (T^T C T) b = T^T C u; Y deflated     (cmtf.py:130-139)
// The held-out batch, per block: centred by mu^b, THEN masked (NaN after centring, columns with c_p^b = 0 included); block b of
// the batch takes the masked score when any of its entries is missing; the blocks' scores averaged, every block deflated by the
// average.  A held-out row with nothing observed in some block has a NaN score there (0 / 0), so a NaN average, and the deflation
// by it makes every later score of the row NaN: NaN from that component on, as the reference (and projection.py) give.
// Status 1: a training row with nothing observed in some block (the reference is NaN everywhere); 2: n < 2; 3: a negative count or
// a yrow outside 0..I-1.  A model with a status writes nothing else.  info[m] = (bit b: block b's training rows took the masked
// arithmetic, bit b: block b's held-out batch did).  With nb = 1 a model is a count-weighted model of cv_masked_kernel.
//
// Workspace per resident model (doubles): for each block Xf^b (I P_b) | c^b (P_b) | mu^b (P_b); then Yf (I M) | T (I R).
// LDS (doubles): 3 I (u, t, c) + 3 M (q, q normalised, nu) + 2 R^2 + R M + 3 R (coef, Q, the normal equations) + 256 (partial rows)
//   + Pmax + 2 nmax^2 + nmax + kmax   (Z, the two Gram buffers, xs, ys: used by one block at a time, sized for the largest:
//                                      Pmax = max P_b, nmax = max min(A_b, B_b), kmax = max max(A_b, B_b))
//   + sum_b [(R + 1)(A_b + B_b) + I]  (the current and the R stored loadings, the per-row observed counts o^b)
// Limits: every block min(A_b, B_b) <= 64 and order 2 or 3, M <= 64, R <= 16, nb <= 8, the LDS above <= 150 KB.
//
// TENSOR (cmtfpls_cv_masked_coupled_tensor_f64): blocks of order 4, I x A x B1 x B2, next to blocks of order 2 and 3.  The same kernel
// with such a block on its I x A x B view, B = B1 B2: every mf_* step runs on the view unchanged, and the block's Z (A x B1 x B2, in
// LDS, already / c_p * n when the block is masked) goes through the rank-1 CP of fold_loop.hpp (lx_cp3) in place of mf_loading; its wA
// and wB = wK (x) wL (C order) feed the unchanged steps, wK and wL go straight to the outputs Wk, Wl.  A matrix block keeps
// mf_loading.  This instantiation runs at 512 threads, where a wavefront has 256 registers for the inlined CP (cv_masked.hip's
// TENSOR form, loo_xcov_coupled.hip's).  LDS: the carve-up above with 512 partial rows (shared by mf_contract and the CP), nmax the
// largest short side over the matrix blocks and every unfolding of every tensor block, kmax over the matrix blocks alone (the CP keeps
// its long vector in the workspace), and after ys the CP's wK (max B1), wL (max B2), v (max B1 B2), tmp (max single dim) over the
// tensor blocks and 8 + 4 doubles of argmax scratch.  Workspace: the above, then the CP's Zt | U | yl | vr, each max P_b over the tensor
// blocks.  Limits: the short side of every unfolding of a tensor block <= 64, the others as above.
#include "common.hpp"
#include "fold_loop.hpp"
#include "fold_regress.hpp"

namespace cmtfpls {

#include "loo_rank1.hpp"
#include "masked_fold.hpp"

constexpr int kCvcMaxN = 64, kCvcMaxR = 16, kCvcMaxM = 64, kCvcThreads = 256, kCvcTensorThreads = 512, kCvcMaxBlocks = 8;

struct CvMaskedCoupledArgs {
  const double* X[kCvcMaxBlocks];   // (I, P_b) original, uncentred, NaN = missing; null past nb
  int A[kCvcMaxBlocks], B[kCvcMaxBlocks];
  const double* Y;        // (I, M) complete
  const int* counts;      // (nm, I) multiplicity of every row in every model
  const int* yrow;        // (nm, I) row of Y paired with each X row (nullable: identity)
  double* ws;             // per resident model: per block Xf | cs | mu; then Yf (I*M) | T (I*R)
  double* Ypred;          // (nm, R, I, M): [m, r - 1, i] = prediction of held-out row i by model m's r-component fit
  double* Wa;             // (nm, R sumA) (nullable): per model block b's R x A_b at R * (A_0 + .. + A_(b-1))
  double* Wb;             // (nm, R sumB) (nullable): likewise
  double* coef;           // (nm, R, R) (nullable): coef_[row, component]
  double* Q;              // (nm, R, M) (nullable)
  int* n_iter;            // (nm, R) (nullable)
  int* status;            // (nm)
  int* info;              // (nm, 2) (nullable): bit masks over the blocks: training rows masked, held-out batch masked
  int64_t ws_per_model;   // doubles
  int nb, I, M, R, nm, max_iter, model0, nmodels, sumA, sumB, maxP, maxn, maxk;
  double tol;
};

// TENSOR: the trailing dims of the blocks of order 4 ((0, 0): a block of order 2 or 3), the outputs of their modes and what sizes
// lx_cp3's scratch, shared by the tensor blocks.  An argument type of its own: the matrix form keeps the argument it had.
struct CvMaskedCoupledTensorArgs : CvMaskedCoupledArgs {
  int B1[kCvcMaxBlocks], B2[kCvcMaxBlocks];
  double* Wk;             // (nm, R sumB1) (nullable): per model tensor block b's R x B1_b at R * (the B1 of the tensor blocks before it)
  double* Wl;             // (nm, R sumB2) (nullable): likewise
  int sumB1, sumB2, b1max, b2max, btmax, dmax, ptmax;
};

template <bool TENSOR> struct CvcArgsOf { typedef CvMaskedCoupledArgs type; };
template <> struct CvcArgsOf<true> { typedef CvMaskedCoupledTensorArgs type; };

// TENSOR: the tensor half of the block descriptor in LDS.  In a function that the matrix form never calls: declared in the kernel, even
// as arrays of one int, it moves that form's dynamic LDS by 8 bytes.
__device__ __forceinline__ int* cvc_tensor_descriptor() {
  __shared__ int s[4 * kCvcMaxBlocks];
  return s;
}

template <bool TENSOR>
__global__ __launch_bounds__(TENSOR ? kCvcTensorThreads : kCvcThreads) void cv_masked_coupled_kernel(typename CvcArgsOf<TENSOR>::type a) {
  constexpr int NT = TENSOR ? kCvcTensorThreads : kCvcThreads;
  extern __shared__ double sm[];
  __shared__ double red[16];
  __shared__ int ired[4];
  // the block descriptor in LDS (copied with static indices: a dynamic index into the kernel argument would go through scratch)
  __shared__ const double* sX[kCvcMaxBlocks];
  __shared__ long long sWs[kCvcMaxBlocks];                       // offset of the block's Xf in the model's workspace
  __shared__ int sA[kCvcMaxBlocks], sB[kCvcMaxBlocks], sLds[kCvcMaxBlocks], sOa[kCvcMaxBlocks], sOb[kCvcMaxBlocks];
  int *sB1 = nullptr, *sB2 = nullptr, *sOk = nullptr, *sOl = nullptr;   // TENSOR: the trailing dims, the blocks' offsets in Wk / Wl
  if constexpr (TENSOR) {
    sB1 = cvc_tensor_descriptor();
    sB2 = sB1 + kCvcMaxBlocks;
    sOk = sB2 + kCvcMaxBlocks;
    sOl = sOk + kCvcMaxBlocks;
  }
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int I = a.I, M = a.M, R = a.R, nb = a.nb;
  const int model = a.model0 + blockIdx.x;
  if (blockIdx.x >= a.nmodels || model >= a.nm) return;
  const int* yrow_m = a.yrow ? a.yrow + (int64_t)model * I : nullptr;
  double* wsm = a.ws + (int64_t)blockIdx.x * a.ws_per_model;
  // LDS carve-up: the shared part, the per-block scratch sized for the largest block, then each block's own vectors
  double* u = sm;
  double* t = u + I;
  double* cw = t + I;             // I: c_r, 0 = held out
  double* q = cw + I;
  double* qn = q + M;
  double* my = qn + M;            // weighted mean of the paired Y rows (nu)
  double* coef = my + M;          // R x R
  double* Qs = coef + R * R;      // R x M
  double* Gn = Qs + R * M;        // (a+1) x (a+1) normal equations
  double* gn = Gn + R * R;
  double* bb = gn + R;
  double* dd = bb + R;
  double* part = dd + R;          // NT doubles: partial rows of the contraction when P_b < NT
  double* Z = part + NT;          // maxP
  double* G0 = Z + a.maxP;
  double* G1 = G0 + a.maxn * a.maxn;
  double* xs = G1 + a.maxn * a.maxn;
  double* ys = xs + a.maxn;
  int own0 = (int)(ys + a.maxk - sm);
  if constexpr (TENSOR) own0 += a.b1max + a.b2max + a.btmax + a.dmax + NT / 64 + NT / 128;   // lx_cp3's wK, wL, v, tmp, the argmax scratch
  if (tid == 0) {
#pragma unroll
    for (int b = 0; b < kCvcMaxBlocks; ++b) { sX[b] = a.X[b]; sA[b] = a.A[b]; sB[b] = a.B[b]; }
    if constexpr (TENSOR) {
#pragma unroll
      for (int b = 0; b < kCvcMaxBlocks; ++b) { sB1[b] = a.B1[b]; sB2[b] = a.B2[b]; }
    }
    long long w = 0;
    int l = own0, oa = 0, ob = 0;
    for (int b = 0; b < nb; ++b) {
      const int A = sA[b], B = sB[b];
      sWs[b] = w; sLds[b] = l; sOa[b] = oa; sOb[b] = ob;
      w += (long long)I * A * B + 2LL * A * B;
      l += (R + 1) * (A + B) + I;
      oa += A; ob += B;
    }
    if constexpr (TENSOR) {
      int ok = 0, ol = 0;
      for (int b = 0; b < nb; ++b) { sOk[b] = ok; sOl[b] = ol; ok += sB1[b]; ol += sB2[b]; }   // (a matrix block: (0, 0))
    }
  }
  __syncthreads();
  int64_t wtot = 0;
  for (int b = 0; b < nb; ++b) wtot += (int64_t)(I + 2) * sA[b] * sB[b];
  double* Yf = wsm + wtot;
  double* T = Yf + (int64_t)I * M;
  LxTensor lt;                    // TENSOR: lx_cp3's scratch, shared by the tensor blocks: LDS after ys, global after T (Zt, then U, yl, vr)
  double* Zt = nullptr;
  double* bestv = nullptr;
  int* besti = nullptr;
  if constexpr (TENSOR) {
    Zt = T + (int64_t)I * R;
    lt = lx_tensor_scratch(ys + a.maxk, Zt + a.ptmax, a.b1max, a.b2max, a.btmax, a.dmax, a.ptmax, NT);
    bestv = lt.part;              // NT / 64 doubles, then NT / 64 ints; the CP's partial sums share mf_contract's `part`
    besti = reinterpret_cast<int*>(bestv + NT / 64);
    lt.part = part;
  }
  // a block's pieces: Xf, cs (c_p), mu in the workspace; wA, wB (current), Wa, Wb (stored), ro (o_r) in LDS
#define CVC_BLOCK(b)                                                                                                   \
  const int A = sA[b], B = sB[b], P = A * B;                                                                           \
  const double* Xo = sX[b];                                                                                            \
  double* Xf = wsm + sWs[b];                                                                                           \
  double* cs = Xf + (int64_t)I * P;                                                                                    \
  double* mu = cs + P;                                                                                                 \
  double* wA = sm + sLds[b];                                                                                           \
  double* wB = wA + A;                                                                                                 \
  double* Wa = wB + B;                                                                                                 \
  double* Wb = Wa + R * A;                                                                                             \
  double* ro = Wb + R * B;                                                                                             \
  (void)Xo, (void)Xf, (void)cs, (void)mu, (void)wA, (void)Wa, (void)ro, (void)P

  if (tid == 0) a.status[model] = 0;
  // ---- counts and training size; a bad count or Y row stops the model before Y is read
  double nf;
  const int st = mf_weights<NT>(a.counts + (int64_t)model * I, yrow_m, I, cw, &nf, red);
  if (st != 0) { if (tid == 0) a.status[model] = st; return; }                  // uniform
  for (int o = tid; o < R * R; o += NT) coef[o] = 0.0;
  // ---- means (cmtf.py:74-75, np.nanmean on the resampled rows), the masked flag per block (cmtf.py:77)
  unsigned missmask = 0u;
  for (int b = 0; b < nb; ++b) {
    CVC_BLOCK(b);
    const double missing = mf_weighted_means<NT>(Xo, cw, I, P, nf, cs, mu);
    if (loo_sum<NT>(missing, red) > 0.0) missmask |= 1u << b;                  // (its barriers publish cs, mu)
  }
  mf_weighted_mean_y<NT>(a.Y, yrow_m, cw, I, M, nf, my);
  __syncthreads();
  // ---- working copies; a training row without an observed entry in some block makes the reference's block score 0 / 0
  double empty = 0.0;
  for (int b = 0; b < nb; ++b) {
    CVC_BLOCK(b);
    if (mf_working_copy<NT>(Xo, cw, mu, I, P, Xf, ro) != 0.0) empty = 1.0;
  }
  mf_working_copy_y<NT>(a.Y, yrow_m, cw, my, I, M, R, Yf, T);
  if (loo_sum<NT>(empty, red) > 0.0) { if (tid == 0) a.status[model] = 1; return; }   // uniform (its barriers publish Xf, Yf, ro)
  const double inv_nb = 1.0 / (double)nb;

  for (int comp = 0; comp < R; ++comp) {
    for (int r = tid; r < I; r += NT) u[r] = Yf[(int64_t)r * M];                   // cmtf.py:89
    __syncthreads();
    int it = 0;
    for (; it < a.max_iter; ++it) {                                                  // cmtf.py:90
      for (int b = 0; b < nb; ++b) {                                                 // cmtf.py:91-118, the blocks in turn
        CVC_BLOCK(b);
        const bool miss = (missmask >> b) & 1u;
        mf_contract<NT, true>(Xf, u, cw, cs, I, P, miss, nf, part, Z);
        bool cp = false;
        if constexpr (TENSOR) cp = sB2[b] > 0;
        if (cp) {
          if constexpr (TENSOR) {                                                    // wB = wK (x) wL; the modes straight to the outputs
            lt.B1 = sB1[b];
            lt.B2 = sB2[b];
            lx_cp3<NT>(Z, Zt, A, a.tol, lt, wA, wB, G0, G1, xs, red, bestv, besti);
            mf_write_factor<NT>(a.Wk, ((int64_t)model * a.sumB1 + sOk[b]) * R + (int64_t)comp * lt.B1, lt.wK, lt.B1);
            mf_write_factor<NT>(a.Wl, ((int64_t)model * a.sumB2 + sOl[b]) * R + (int64_t)comp * lt.B2, lt.wL, lt.B2);
          }
        } else {
          mf_loading<NT>(Z, A, B, wA, wB, G0, G1, xs, ys, red, ired);
        }
        // t^b = X x_1 wA x_2 wB (cmtf.py:106-110), or miss_mmodedot: the row's sum / o_r * P_b; added to the blocks before it
        // by the row's own wavefront; after the last block the average (cmtf.py:119); held-out rows 0
        const double Pd = (double)P;
        for (int r = wv; r < I; r += NT / 64) {
          const double s = mf_row_dot(Xf + (int64_t)r * P, wA, wB, P, B);
          if (lane == 0) {
            double v = (b == 0 ? 0.0 : t[r]) + (miss ? s / ro[r] * Pd : s);
            if (b == nb - 1) v *= inv_nb;
            t[r] = (cw[r] == 0.0) ? 0.0 : v;
          }
        }
      }
      __syncthreads();
      const double du = mf_y_step<NT, true>(Yf, t, cw, I, M, q, qn, u, red);
      if (it > 0 && du < a.tol) { ++it; break; }                                     // first pass: oldU = inf (cmtf.py:88)
    }
    if (a.n_iter && tid == 0) a.n_iter[(int64_t)model * R + comp] = it;
    // store the component; deflate every block by the shared t, then Y after the inner regression
    for (int r = tid; r < I; r += NT) T[(int64_t)r * R + comp] = t[r];
    for (int m = tid; m < M; m += NT) Qs[comp * M + m] = qn[m];
    for (int b = 0; b < nb; ++b) {
      CVC_BLOCK(b);
      mf_deflate_x<NT>(Xo, cw, t, wA, wB, I, A, B, comp, (missmask >> b) & 1u, Wa, Wb, Xf);
    }
    __syncthreads();
    mf_regress_deflate_y<NT, true>(T, u, cw, qn, I, M, R, comp, Gn, gn, bb, dd, coef, t, Yf);
  }

  // ---- predict the held-out rows (cmtf.py:141-175): a block of the batch is masked when any of its entries is missing
  unsigned hmask = 0u;
  for (int b = 0; b < nb; ++b) {
    CVC_BLOCK(b);
    if (mf_heldout_batch<NT>(Xo, mu, cw, I, P, Xf, ro, red)) hmask |= 1u << b;
  }
  // scores and deflation per component: a wavefront owns a held-out row of every block for all R components (no barrier between
  // them: every lane rereads only the entries it wrote)
  for (int r = wv; r < I; r += NT / 64) {
    if (cw[r] != 0.0) continue;
    for (int comp = 0; comp < R; ++comp) {
      double sv = 0.0;
      for (int b = 0; b < nb; ++b) {
        CVC_BLOCK(b);
        const double s = mf_row_dot(Xf + (int64_t)r * P, Wa + comp * A, Wb + comp * B, P, B);
        sv += ((hmask >> b) & 1u) ? s / ro[r] * (double)P : s;                     // o_r = 0: 0 / 0 = NaN, as the reference
      }
      sv *= inv_nb;
      if (lane == 0) T[(int64_t)r * R + comp] = sv;
      for (int b = 0; b < nb; ++b) {
        CVC_BLOCK(b);
        mf_heldout_deflate(Xo + (int64_t)r * P, mu, Wa + comp * A, Wb + comp * B, P, B, sv, (hmask >> b) & 1u, Xf + (int64_t)r * P);
      }
    }
  }
  __syncthreads();
  mf_predict<NT>(T, coef, Qs, my, cw, I, M, R, a.Ypred + (int64_t)model * R * I * M);
  // the model's factors (the bootstrap aligns them on the host)
  for (int b = 0; b < nb; ++b) {
    CVC_BLOCK(b);
    mf_write_factor<NT>(a.Wa, (int64_t)model * R * a.sumA + (int64_t)R * sOa[b], Wa, R * A);
    mf_write_factor<NT>(a.Wb, (int64_t)model * R * a.sumB + (int64_t)R * sOb[b], Wb, R * B);
  }
  mf_write_factor<NT>(a.coef, (int64_t)model * R * R, coef, R * R);
  mf_write_factor<NT>(a.Q, (int64_t)model * R * M, Qs, R * M);
  if (a.info && tid == 0) {
    a.info[2 * (int64_t)model] = (int)missmask;
    a.info[2 * (int64_t)model + 1] = (int)hmask;
  }
#undef CVC_BLOCK
}

static size_t cv_masked_coupled_lds_bytes(const cmtfpls_cv_coupled_block* blocks, int nb, int I, int M, int R) {
  size_t Pmax = 0, nmax = 0, kmax = 0, own = 0;
  for (int b = 0; b < nb; ++b) {
    const size_t A = (size_t)blocks[b].A, B = (size_t)blocks[b].B;
    const size_t n = A < B ? A : B, k = A < B ? B : A;
    Pmax = A * B > Pmax ? A * B : Pmax;
    nmax = n > nmax ? n : nmax;
    kmax = k > kmax ? k : kmax;
    own += ((size_t)R + 1) * (A + B) + (size_t)I;
  }
  const size_t dbl = 3 * (size_t)I + 3 * (size_t)M + 2 * (size_t)R * R + (size_t)R * M + 3 * (size_t)R + (size_t)kCvcThreads + Pmax +
                     2 * nmax * nmax + nmax + kmax + own;
  return dbl * sizeof(double);
}

// TENSOR: what sizes the kernel's LDS and workspace.  dims: (B1, B2) per block, B2 > 0 a block of order 4.  Pmax and sumB1 / sumB2 as
// they stand; nmax over the matrix blocks' min(A, B) and the shorter side of every unfolding of every tensor block, kmax over the
// matrix blocks' max(A, B) alone; lx_cp3's shared scratch by the largest B1, B2, B1 B2, single dim and A B1 B2 over the tensor blocks
struct CvcTensorShape {
  size_t Pmax, nmax, kmax, own, sumB1, sumB2, b1max, b2max, btmax, dmax, ptmax;
};

static CvcTensorShape cvc_tensor_shape(const cmtfpls_cv_coupled_block* blocks, int nb, const int* dims, int I, int R) {
  CvcTensorShape o = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  auto up = [](size_t& m, size_t v) { if (v > m) m = v; };
  for (int b = 0; b < nb; ++b) {
    const size_t A = (size_t)blocks[b].A, B = (size_t)blocks[b].B, B1 = (size_t)dims[2 * b], B2 = (size_t)dims[2 * b + 1];
    up(o.Pmax, A * B);
    o.own += ((size_t)R + 1) * (A + B) + (size_t)I;
    if (B2 > 0) {
      for (const size_t d : {A, B1, B2}) up(o.nmax, d < A * B / d ? d : A * B / d);
      for (const size_t d : {A, B1, B2}) up(o.dmax, d);
      o.sumB1 += B1; o.sumB2 += B2;
      up(o.b1max, B1); up(o.b2max, B2); up(o.btmax, B); up(o.ptmax, A * B);
    } else {
      up(o.nmax, A < B ? A : B);
      up(o.kmax, A < B ? B : A);
    }
  }
  return o;
}

// the carve-up of cv_masked_coupled_lds_bytes with 512 partial rows, then lx_cp3's wK, wL, v, tmp and the argmax scratch (a double
// and an int per wavefront)
static size_t cvc_tensor_lds_bytes(const CvcTensorShape& s, int I, int M, int R) {
  const size_t dbl = 3 * (size_t)I + 3 * (size_t)M + 2 * (size_t)R * R + (size_t)R * M + 3 * (size_t)R + (size_t)kCvcTensorThreads + s.Pmax +
                     2 * s.nmax * s.nmax + s.nmax + s.kmax + s.b1max + s.b2max + s.btmax + s.dmax + kCvcTensorThreads / 64 +
                     kCvcTensorThreads / 128 + s.own;
  return dbl * sizeof(double);
}

// what the tensor size functions and entry call a well-formed description: sizes as the matrix form's, dims without a negative entry,
// order 4 exactly where B2 > 0 (then B1 B2 == B), no order above 4 and at least one block of order 4
static bool cvc_tensor_dims_ok(const cmtfpls_cv_coupled_block* blocks, int nb, const int* dims) {
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

static bool cvc_sizes_ok(const cmtfpls_cv_coupled_block* blocks, int nb, int I, int M, int R) {
  if (!blocks || nb <= 0 || nb > kCvcMaxBlocks || I <= 1 || M <= 0 || R <= 0) return false;
  for (int b = 0; b < nb; ++b)
    if (blocks[b].A <= 0 || blocks[b].B <= 0) return false;
  return true;
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {

size_t cmtfpls_cv_masked_coupled_workspace_bytes(const cmtfpls_cv_coupled_block* blocks, int nb, int I, int M, int R) {
  if (!blocks || nb <= 0 || nb > kCvcMaxBlocks || I <= 1 || M <= 0 || R <= 0) return 0;
  size_t dbl = (size_t)I * M + (size_t)I * R;
  for (int b = 0; b < nb; ++b) {
    if (blocks[b].A <= 0 || blocks[b].B <= 0) return 0;
    dbl += ((size_t)I + 2) * (size_t)blocks[b].A * (size_t)blocks[b].B;
  }
  return dbl * sizeof(double);
}

size_t cmtfpls_cv_masked_coupled_lds_bytes(const cmtfpls_cv_coupled_block* blocks, int nb, int I, int M, int R) {
  if (!blocks || nb <= 0 || nb > kCvcMaxBlocks || I <= 1 || M <= 0 || R <= 0) return 0;
  for (int b = 0; b < nb; ++b)
    if (blocks[b].A <= 0 || blocks[b].B <= 0) return 0;
  return cv_masked_coupled_lds_bytes(blocks, nb, I, M, R);
}

int cmtfpls_cv_masked_coupled_f64(const cmtfpls_cv_coupled_block* blocks, int nb, const double* Y, const int* counts,
                                  const int* yrow, int nm, int I, int M, int R, double tol, int max_iter, int model0, int nmodels,
                                  double* Ypred, double* Wa, double* Wb, double* coef, double* Q, int* n_iter, int* status,
                                  int* info, void* ws, size_t ws_bytes, void* stream) {
  if (!blocks || !Y || !counts || !Ypred || !status || nb <= 0 || I <= 1 || M <= 0 || R <= 0 || max_iter <= 0 || nm <= 0 ||
      model0 < 0 || nmodels <= 0) {
    set_error("cv_masked_coupled: bad argument");
    return CMTFPLS_EINVAL;
  }
  const char* outside = "cv_masked_coupled: shape outside the one-workgroup-per-model form; refit per model on the regular engine";
  if (nb > kCvcMaxBlocks || M > kCvcMaxM || R > kCvcMaxR) { set_error(outside); return CMTFPLS_EUNSUPPORTED; }
  for (int b = 0; b < nb; ++b) {
    const cmtfpls_cv_coupled_block& k = blocks[b];
    if (!k.X || k.A <= 0 || k.B <= 0 || (k.order == 2 && k.A != 1)) { set_error("cv_masked_coupled: bad block"); return CMTFPLS_EINVAL; }
    if ((k.order != 2 && k.order != 3) || (k.A < k.B ? k.A : k.B) > kCvcMaxN) { set_error(outside); return CMTFPLS_EUNSUPPORTED; }
  }
  const size_t lds = cv_masked_coupled_lds_bytes(blocks, nb, I, M, R);
  if (lds > 150 * 1024) { set_error(outside); return CMTFPLS_EUNSUPPORTED; }
  if (model0 + nmodels > nm) { set_error("cv_masked_coupled: models out of range"); return CMTFPLS_EINVAL; }
  const size_t per = cmtfpls_cv_masked_coupled_workspace_bytes(blocks, nb, I, M, R);
  if (!ws || ws_bytes < per * (size_t)nmodels) { set_error("cv_masked_coupled: workspace too small"); return CMTFPLS_EWORKSPACE; }
  CvMaskedCoupledArgs a;
  a.sumA = a.sumB = a.maxP = a.maxn = a.maxk = 0;
  for (int b = 0; b < kCvcMaxBlocks; ++b) {
    a.X[b] = b < nb ? blocks[b].X : nullptr;
    a.A[b] = b < nb ? blocks[b].A : 0;
    a.B[b] = b < nb ? blocks[b].B : 0;
    const int n = a.A[b] < a.B[b] ? a.A[b] : a.B[b], k = a.A[b] < a.B[b] ? a.B[b] : a.A[b];
    a.sumA += a.A[b]; a.sumB += a.B[b];
    a.maxP = a.A[b] * a.B[b] > a.maxP ? a.A[b] * a.B[b] : a.maxP;
    a.maxn = n > a.maxn ? n : a.maxn;
    a.maxk = k > a.maxk ? k : a.maxk;
  }
  a.Y = Y; a.counts = counts; a.yrow = yrow;
  a.ws = static_cast<double*>(ws); a.Ypred = Ypred; a.Wa = Wa; a.Wb = Wb; a.coef = coef; a.Q = Q;
  a.n_iter = n_iter; a.status = status; a.info = info;
  a.ws_per_model = (int64_t)(per / sizeof(double));
  a.nb = nb; a.I = I; a.M = M; a.R = R; a.nm = nm; a.max_iter = max_iter; a.model0 = model0; a.nmodels = nmodels;
  a.tol = tol;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cv_masked_coupled_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
  hipLaunchKernelGGL(cv_masked_coupled_kernel<false>, dim3(nmodels), dim3(kCvcThreads), lds, (hipStream_t)stream, a);
  return check_launch("cv_masked_coupled");
}

size_t cmtfpls_cv_masked_coupled_tensor_workspace_bytes(const cmtfpls_cv_coupled_block* blocks, int nb, const int* dims, int I, int M,
                                                        int R) {
  if (!cvc_sizes_ok(blocks, nb, I, M, R) || !cvc_tensor_dims_ok(blocks, nb, dims)) return 0;
  return cmtfpls_cv_masked_coupled_workspace_bytes(blocks, nb, I, M, R) + 4 * cvc_tensor_shape(blocks, nb, dims, I, R).ptmax * sizeof(double);
}

size_t cmtfpls_cv_masked_coupled_tensor_lds_bytes(const cmtfpls_cv_coupled_block* blocks, int nb, const int* dims, int I, int M, int R) {
  if (!cvc_sizes_ok(blocks, nb, I, M, R) || !cvc_tensor_dims_ok(blocks, nb, dims)) return 0;
  return cvc_tensor_lds_bytes(cvc_tensor_shape(blocks, nb, dims, I, R), I, M, R);
}

int cmtfpls_cv_masked_coupled_tensor_f64(const cmtfpls_cv_coupled_block* blocks, int nb, const int* dims, const double* Y,
                                         const int* counts, const int* yrow, int nm, int I, int M, int R, double tol, int max_iter,
                                         int model0, int nmodels, double* Ypred, double* Wa, double* Wb, double* Wk, double* Wl,
                                         double* coef, double* Q, int* n_iter, int* status, int* info, void* ws, size_t ws_bytes,
                                         void* stream) {
  auto fail = [](int code, const char* what) { set_error(what); return code; };
  if (!blocks || !dims || !Y || !counts || !Ypred || !status || nb <= 0 || I <= 1 || M <= 0 || R <= 0 || max_iter <= 0 || nm <= 0 ||
      model0 < 0 || nmodels <= 0)
    return fail(CMTFPLS_EINVAL, "cv_masked_coupled_tensor: bad argument");
  const char* outside = "cv_masked_coupled_tensor: shape outside the one-workgroup-per-model form; refit per model on the regular engine";
  if (nb > kCvcMaxBlocks || M > kCvcMaxM || R > kCvcMaxR) return fail(CMTFPLS_EUNSUPPORTED, outside);
  for (int b = 0; b < nb; ++b) {
    const cmtfpls_cv_coupled_block& k = blocks[b];
    if (!k.X || k.A <= 0 || k.B <= 0 || k.order < 2 || (k.order == 2 && k.A != 1)) return fail(CMTFPLS_EINVAL, "cv_masked_coupled_tensor: bad block");
  }
  if (!cvc_tensor_dims_ok(blocks, nb, dims))
    return fail(CMTFPLS_EINVAL, "cv_masked_coupled_tensor: bad dims ((B1, B2) with B1 * B2 == B for every block of order 4 and at least one "
                                "such block, (0, 0) for a block of order 2 or 3; no order above 4)");
  const CvcTensorShape s = cvc_tensor_shape(blocks, nb, dims, I, R);
  if (s.nmax > (size_t)kCvcMaxN) return fail(CMTFPLS_EUNSUPPORTED, outside);   // a matrix block's min(A, B), a tensor block's unfoldings
  const size_t lds = cvc_tensor_lds_bytes(s, I, M, R);
  if (lds > 150 * 1024) return fail(CMTFPLS_EUNSUPPORTED, outside);
  if (model0 + nmodels > nm) return fail(CMTFPLS_EINVAL, "cv_masked_coupled_tensor: models out of range");
  const size_t per = cmtfpls_cv_masked_coupled_tensor_workspace_bytes(blocks, nb, dims, I, M, R);
  if (!ws || ws_bytes < per * (size_t)nmodels) return fail(CMTFPLS_EWORKSPACE, "cv_masked_coupled_tensor: workspace too small");
  CvMaskedCoupledTensorArgs a;
  a.sumA = a.sumB = 0;
  for (int b = 0; b < kCvcMaxBlocks; ++b) {
    a.X[b] = b < nb ? blocks[b].X : nullptr;
    a.A[b] = b < nb ? blocks[b].A : 0;
    a.B[b] = b < nb ? blocks[b].B : 0;
    a.B1[b] = b < nb ? dims[2 * b] : 0;
    a.B2[b] = b < nb ? dims[2 * b + 1] : 0;
    a.sumA += a.A[b]; a.sumB += a.B[b];
  }
  a.maxP = (int)s.Pmax; a.maxn = (int)s.nmax; a.maxk = (int)s.kmax;
  a.sumB1 = (int)s.sumB1; a.sumB2 = (int)s.sumB2;
  a.b1max = (int)s.b1max; a.b2max = (int)s.b2max; a.btmax = (int)s.btmax; a.dmax = (int)s.dmax; a.ptmax = (int)s.ptmax;
  a.Y = Y; a.counts = counts; a.yrow = yrow;
  a.ws = static_cast<double*>(ws); a.Ypred = Ypred; a.Wa = Wa; a.Wb = Wb; a.Wk = Wk; a.Wl = Wl; a.coef = coef; a.Q = Q;
  a.n_iter = n_iter; a.status = status; a.info = info;
  a.ws_per_model = (int64_t)(per / sizeof(double));
  a.nb = nb; a.I = I; a.M = M; a.R = R; a.nm = nm; a.max_iter = max_iter; a.model0 = model0; a.nmodels = nmodels;
  a.tol = tol;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cv_masked_coupled_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
  hipLaunchKernelGGL(cv_masked_coupled_kernel<true>, dim3(nmodels), dim3(kCvcTensorThreads), lds, (hipStream_t)stream, a);
  return check_launch("cv_masked_coupled_tensor");
}

}  // extern "C"
