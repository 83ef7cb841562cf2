// Refits of a small coupled model (ctPLS: nb blocks sharing the sample mode and ONE score) whose blocks have missing values, on
// count-weighted rows, ALL MODELS OF A CHUNK IN ONE LAUNCH: K-fold and leave-one-out Q2Y, the permutation test, repeated K-fold and
// the bootstrap of such data (validate.py with EngineOptions.masked_folds_coupled).  The count-weighted model of
// cv_masked_models.hip generalised to 1 <= nb <= 8 blocks: model m is counts[m, r] >= 0 copies of row r of EVERY block paired with
// Y[yrow[m, r]] (yrow nullable = identity); its arithmetic is the reference's ctPLS.fit (cmtf.py:87-139) on that literal data, the
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
// arithmetic, bit b: block b's held-out batch did).  With nb = 1 a model is a model of cv_masked_models_kernel.
//
// Workspace per resident model (doubles): for each block Xf^b (I P_b) | c^b (P_b) | mu^b (P_b); then Yf (I M) | T (I R).
// LDS (doubles): 3 I (u, t, c) + 3 M (q, q normalised, nu) + 2 R^2 + R M + 3 R (coef, Q, the normal equations) + 256 (partial rows)
//   + Pmax + 2 nmax^2 + nmax + kmax   (Z, the two Gram buffers, xs, ys: used by one block at a time, sized for the largest:
//                                      Pmax = max P_b, nmax = max min(A_b, B_b), kmax = max max(A_b, B_b))
//   + sum_b [(R + 1)(A_b + B_b) + I]  (the current and the R stored loadings, the per-row observed counts o^b)
// Limits: every block min(A_b, B_b) <= 64 and order 2 or 3, M <= 64, R <= 16, nb <= 8, the LDS above <= 150 KB.
#include "common.hpp"
#include "fold_regress.hpp"

namespace cmtfpls {

#include "loo_rank1.hpp"

constexpr int kCvcMaxN = 64, kCvcMaxR = 16, kCvcMaxM = 64, kCvcThreads = 256, kCvcMaxBlocks = 8;

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

__global__ __launch_bounds__(kCvcThreads) void cv_masked_coupled_kernel(CvMaskedCoupledArgs a) {
  constexpr int NT = kCvcThreads;
  extern __shared__ double sm[];
  __shared__ double red[16];
  __shared__ int ired[4];
  // the block descriptor in LDS (copied with static indices: a dynamic index into the kernel argument would go through scratch)
  __shared__ const double* sX[kCvcMaxBlocks];
  __shared__ long long sWs[kCvcMaxBlocks];                       // offset of the block's Xf in the model's workspace
  __shared__ int sA[kCvcMaxBlocks], sB[kCvcMaxBlocks], sLds[kCvcMaxBlocks], sOa[kCvcMaxBlocks], sOb[kCvcMaxBlocks];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int I = a.I, M = a.M, R = a.R, nb = a.nb;
  const int model = a.model0 + blockIdx.x;
  if (blockIdx.x >= a.nmodels || model >= a.nm) return;
  const int* cnt_m = a.counts + (int64_t)model * I;
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
  const int own0 = (int)(ys + a.maxk - sm);
  if (tid == 0) {
#pragma unroll
    for (int b = 0; b < kCvcMaxBlocks; ++b) { sX[b] = a.X[b]; sA[b] = a.A[b]; sB[b] = a.B[b]; }
    long long w = 0;
    int l = own0, oa = 0, ob = 0;
    for (int b = 0; b < nb; ++b) {
      const int A = sA[b], B = sB[b];
      sWs[b] = w; sLds[b] = l; sOa[b] = oa; sOb[b] = ob;
      w += (long long)I * A * B + 2LL * A * B;
      l += (R + 1) * (A + B) + I;
      oa += A; ob += B;
    }
  }
  __syncthreads();
  int64_t wtot = 0;
  for (int b = 0; b < nb; ++b) wtot += (int64_t)(I + 2) * sA[b] * sB[b];
  double* Yf = wsm + wtot;
  double* T = Yf + (int64_t)I * M;
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
  double nt = 0.0, bad = 0.0;
  for (int r = tid; r < I; r += NT) {
    const int c = cnt_m[r];
    const int yr = yrow_m ? yrow_m[r] : r;
    if (c < 0 || yr < 0 || yr >= I) bad = 1.0;
    cw[r] = c > 0 ? (double)c : 0.0;
    nt += c > 0 ? (double)c : 0.0;
  }
  const double nf = loo_sum<NT>(nt, red);                                       // (its barriers publish cw)
  if (loo_sum<NT>(bad, red) > 0.0) { if (tid == 0) a.status[model] = 3; return; }   // uniform
  if (nf < 2.0) { if (tid == 0) a.status[model] = 2; return; }                 // uniform
  for (int o = tid; o < R * R; o += NT) coef[o] = 0.0;
  // ---- means (cmtf.py:74-75, np.nanmean on the resampled rows), the masked flag per block (cmtf.py:77)
  unsigned missmask = 0u;
  for (int b = 0; b < nb; ++b) {
    CVC_BLOCK(b);
    double missing = 0.0;
    for (int c = tid; c < P; c += NT) {
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
    if (loo_sum<NT>(missing, red) > 0.0) missmask |= 1u << b;                  // (its barriers publish cs, mu)
  }
  for (int m = tid; m < M; m += NT) {
    double s = 0.0;
    for (int r = 0; r < I; ++r) {
      const double w = cw[r];
      if (w != 0.0) s = fma(w, a.Y[(int64_t)(yrow_m ? yrow_m[r] : r) * M + m], s);
    }
    my[m] = s / nf;
  }
  __syncthreads();
  // ---- working copies: centred, zero at held-out rows and missing entries; observed entries of every row (a training row
  // without any in some block makes the reference's block score 0 / 0)
  double empty = 0.0;
  for (int b = 0; b < nb; ++b) {
    CVC_BLOCK(b);
    for (int64_t idx = tid; idx < (int64_t)I * P; idx += NT) {
      const int r = (int)(idx / P), c = (int)(idx % P);
      const double x = Xo[idx];
      Xf[idx] = (cw[r] == 0.0 || isnan(x)) ? 0.0 : x - mu[c];
    }
    for (int r = wv; r < I; r += NT / 64) {
      double cnt = 0.0;
      for (int c = lane; c < P; c += 64) cnt += isnan(Xo[(int64_t)r * P + c]) ? 0.0 : 1.0;
      cnt = wave_sum(cnt);
      if (lane == 0) ro[r] = cnt;
      if (cw[r] != 0.0 && cnt == 0.0) empty = 1.0;
    }
  }
  for (int64_t idx = tid; idx < (int64_t)I * M; idx += NT) {
    const int r = (int)(idx / M), m = (int)(idx % M);
    Yf[idx] = (cw[r] == 0.0) ? 0.0 : a.Y[(int64_t)(yrow_m ? yrow_m[r] : r) * M + m] - my[m];
  }
  for (int64_t idx = tid; idx < (int64_t)I * R; idx += NT) T[idx] = 0.0;
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
        const int n = A < B ? A : B, k = A < B ? B : A;
        const int nrg = (P < NT) ? NT / P : 1;
        // Z = X x_0 u over the weighted rows (cmtf.py:93), or miss_tensordot: the column's sum / c_p * n, 0 when c_p = 0
        if (nrg == 1) {
          for (int c = tid; c < P; c += NT) {
            double s = 0.0;
            for (int r = 0; r < I; ++r) s = fma(Xf[(int64_t)r * P + c], cw[r] * u[r], s);
            Z[c] = miss ? (cs[c] > 0.0 ? s / cs[c] * nf : 0.0) : s;
          }
        } else {
          const int rg = tid / P, c = tid % P;
          if (rg < nrg) {
            double s = 0.0;
            for (int r = rg; r < I; r += nrg) s = fma(Xf[(int64_t)r * P + c], cw[r] * u[r], s);
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
        if (A == 1) {                                                                // cmtf.py:97: Z / norm(Z)
          double s = 0.0;
          for (int c = tid; c < P; c += NT) s = fma(Z[c], Z[c], s);
          const double nz = sqrt(loo_sum<NT>(s, red));
          for (int c = tid; c < P; c += NT) wB[c] = Z[c] / nz;
          if (tid == 0) wA[0] = 1.0;
          __syncthreads();
        } else {
          if (n <= 8 && k <= 64) loo_rank1_wave(Z, A, B, wA, wB);                      // cmtf.py:98-103
          else loo_rank1<NT>(Z, A, B, wA, wB, G0, G1, xs, ys, red, ired);
        }
        // t^b = X x_1 wA x_2 wB (cmtf.py:106-110), or miss_mmodedot: the row's sum / o_r * P_b; added to the blocks before it
        // by the row's own wavefront; after the last block the average (cmtf.py:119); held-out rows 0
        const double Pd = (double)P;
        for (int r = wv; r < I; r += NT / 64) {
          double s = 0.0;
          for (int c = lane; c < P; c += 64) s = fma(Xf[(int64_t)r * P + c], wA[c / B] * wB[c % B], s);
          s = wave_sum(s);
          if (lane == 0) {
            double v = (b == 0 ? 0.0 : t[r]) + (miss ? s / ro[r] * Pd : s);
            if (b == nb - 1) v *= inv_nb;
            t[r] = (cw[r] == 0.0) ? 0.0 : v;
          }
        }
      }
      __syncthreads();
      // q = Y^T C t / |.| (cmtf.py:120-121)
      if (tid < M) {
        double s = 0.0;
        for (int r = 0; r < I; ++r) s = fma(Yf[(int64_t)r * M + tid], cw[r] * t[r], s);
        q[tid] = s;
      }
      __syncthreads();
      double qs = (tid < M) ? q[tid] * q[tid] : 0.0;
      const double qnrm = sqrt(loo_sum<NT>(qs, red));
      if (tid < M) qn[tid] = q[tid] / qnrm;
      __syncthreads();
      // u = Y q and the weighted |u_old - u| (cmtf.py:122-123)
      double du2 = 0.0;
      for (int r = tid; r < I; r += NT) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s = fma(Yf[(int64_t)r * M + m], qn[m], s);
        const double d0 = u[r] - s;
        du2 = fma(cw[r] * d0, d0, du2);
        u[r] = s;
      }
      const double du = sqrt(loo_sum<NT>(du2, red));
      if (it > 0 && du < a.tol) { ++it; break; }                                     // first pass: oldU = inf (cmtf.py:88)
    }
    if (a.n_iter && tid == 0) a.n_iter[(int64_t)model * R + comp] = it;
    // store the component; deflate the observed training entries of every block by the shared t (cmtf.py:130-131)
    for (int r = tid; r < I; r += NT) T[(int64_t)r * R + comp] = t[r];
    for (int m = tid; m < M; m += NT) Qs[comp * M + m] = qn[m];
    for (int b = 0; b < nb; ++b) {
      CVC_BLOCK(b);
      const bool miss = (missmask >> b) & 1u;
      for (int j = tid; j < A; j += NT) Wa[comp * A + j] = wA[j];
      for (int j = tid; j < B; j += NT) Wb[comp * B + j] = wB[j];
      for (int64_t idx = tid; idx < (int64_t)I * P; idx += NT) {
        const int r = (int)(idx / P), c = (int)(idx % P);
        if (cw[r] == 0.0 || (miss && isnan(Xo[idx]))) continue;
        Xf[idx] = Xf[idx] - t[r] * (wA[c / B] * wB[c % B]);
      }
    }
    __syncthreads();
    // inner regression b = lstsq(T[:, :k], u) on the weighted rows (cmtf.py:136-138): (T^T C T) b = T^T C u, fold_regress.hpp; then
    // Y -= T b q^T (cmtf.py:139), yhat = T b in t; held-out rows of T are 0, so their Yf stays 0
    fold_inner_regression<NT, true>(T, u, cw, I, R, comp, Gn, gn, bb, dd, coef, t);
    for (int64_t idx = tid; idx < (int64_t)I * M; idx += NT) {
      const int r = (int)(idx / M), m = (int)(idx % M);
      Yf[idx] = Yf[idx] - t[r] * qn[m];
    }
    __syncthreads();
  }

  // ---- predict the held-out rows (cmtf.py:141-175): per block centre with the model's means, THEN mask (NaN after centring,
  // which takes in the columns without a training observation); a block of the batch is masked when any of its entries is
  unsigned hmask = 0u;
  for (int b = 0; b < nb; ++b) {
    CVC_BLOCK(b);
    const double Pd = (double)P;
    double hmiss = 0.0;
    for (int r = wv; r < I; r += NT / 64) {
      if (cw[r] != 0.0) continue;                                                     // uniform in the wavefront
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
    if (loo_sum<NT>(hmiss, red) > 0.0) hmask |= 1u << b;                        // (its barriers publish ro)
  }
  // scores and deflation per component: a wavefront owns a held-out row of every block for all R components (no barrier between
  // them: every lane rereads only the entries it wrote)
  for (int r = wv; r < I; r += NT / 64) {
    if (cw[r] != 0.0) continue;
    for (int comp = 0; comp < R; ++comp) {
      double sv = 0.0;
      for (int b = 0; b < nb; ++b) {
        CVC_BLOCK(b);
        double s = 0.0;
        for (int c = lane; c < P; c += 64) s = fma(Xf[(int64_t)r * P + c], Wa[comp * A + c / B] * Wb[comp * B + c % B], s);
        s = wave_sum(s);
        sv += ((hmask >> b) & 1u) ? s / ro[r] * (double)P : s;                     // o_r = 0: 0 / 0 = NaN, as the reference
      }
      sv *= inv_nb;
      if (lane == 0) T[(int64_t)r * R + comp] = sv;
      for (int b = 0; b < nb; ++b) {
        CVC_BLOCK(b);
        const bool hm = (hmask >> b) & 1u;
        for (int c = lane; c < P; c += 64) {
          if (hm && isnan(Xo[(int64_t)r * P + c] - mu[c])) continue;
          Xf[(int64_t)r * P + c] = Xf[(int64_t)r * P + c] - sv * (Wa[comp * A + c / B] * Wb[comp * B + c % B]);
        }
      }
    }
  }
  __syncthreads();
  // Ypred[m, c - 1] = scores[:, :c] coef_[:c, :c] Q[:, :c]^T + nu for c = 1..R (coef_ upper triangular: one pass over h Q^T)
  double* yp = a.Ypred + (int64_t)model * R * I * M;
  for (int64_t o = tid; o < (int64_t)I * M; o += NT) {
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
  // the model's factors (the bootstrap aligns them on the host)
  for (int b = 0; b < nb; ++b) {
    CVC_BLOCK(b);
    if (a.Wa) for (int o = tid; o < R * A; o += NT) a.Wa[(int64_t)model * R * a.sumA + (int64_t)R * sOa[b] + o] = Wa[o];
    if (a.Wb) for (int o = tid; o < R * B; o += NT) a.Wb[(int64_t)model * R * a.sumB + (int64_t)R * sOb[b] + o] = Wb[o];
  }
  if (a.coef) for (int o = tid; o < R * R; o += NT) a.coef[(int64_t)model * R * R + o] = coef[o];
  if (a.Q) for (int o = tid; o < R * M; o += NT) a.Q[(int64_t)model * R * M + o] = Qs[o];
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
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cv_masked_coupled_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
  hipLaunchKernelGGL(cv_masked_coupled_kernel, dim3(nmodels), dim3(kCvcThreads), lds, (hipStream_t)stream, a);
  return check_launch("cv_masked_coupled");
}

}  // extern "C"
