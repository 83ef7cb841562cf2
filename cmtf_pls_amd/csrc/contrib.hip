// Per-mode contributions of a sample to its Q residual (SPE) and to its Hotelling T^2 (validate.sample_contributions):
//   x = X[src, c] - mean[c],  c = j B + k,  W[c, r] = WA[j, r] WB[k, r]
//   e = x - sum_r T[i, r] W[c, r]     d = x sum_r H[i, r] W[c, r]            (both 0 where x is not finite)
//   speA[i, j] = sum_k e^2   speB[i, k] = sum_j e^2   t2A[i, j] = sum_k d   t2B[i, k] = sum_j d
// in ONE read of the uncentred X, nothing of the size of X written.  A workgroup owns whole rows (G of them), so both mode sums
// close inside it: no partials in global memory, no second kernel, no atomics, the same bits on every call.
//
// Layout.  A thread keeps V consecutive k (one 16-byte vector, for 16-bit storage 4 k in one 8-byte vector as f32: DiagVec; V = 1
// on the one-element path) for the whole row, so their R
// loadings WB[k.., :] stay in registers over every j and every row of the group, and walks j in steps of JP = 256 / LK, LK = the
// lanes along k (a power of two <= 64, so a j slice never leaves a wavefront).  The row's t and h are folded into the A side once
// per row, TH[j][r] = (t_r WA[j, r], h_r WA[j, r]) in LDS, read as a broadcast: per cell rec and dir are 2 R multiply-adds
// TH[j][r] x WB[k, r] and nothing per row lives in scalar registers.
//   sums over j (speB, t2B): in the thread's registers, closed over the JP threads of a k through an LDS slab in a fixed order;
//   sums over k (speA, t2A): a butterfly over the LK lanes of the slice (DPP inside 16 lanes, lane shuffles beyond), then one
//                            owner lane adds into the row's LDS accumulator -- the same lane for every chunk of k.
// B beyond LK V columns is walked in chunks (chunk outermost: the loadings are reloaded once per chunk and row group).  A matrix
// block (A = 1) has no j: all 256 threads lie along k, nothing is reduced, and the A outputs are skipped.
#include "model_cols.hpp"                        // the component cap (here: of WB held in registers), its dispatch and dpp_mov

namespace cmtfpls {

constexpr int kContribUnroll = 4;                // j steps whose loads are issued together
constexpr int kContribMaxRows = 8;               // rows of a workgroup (their A-side accumulators share the LDS)
constexpr size_t kContribLdsMax = 160 * 1024;    // TH (2 A R) + accumulators (2 G A) + slab (512 V) doubles must fit

// total over the aligned group of 2^lg lanes (lg uniform, <= 6); every lane of the group ends with the same bits
__device__ __forceinline__ double slice_total(double v, int lg) {
  if (lg > 0) v += dpp_mov<0xB1>(v);             // lane ^ 1
  if (lg > 1) v += dpp_mov<0x4E>(v);             // lane ^ 2
  if (lg > 2) v += dpp_mov<0x141>(v);            // the other quad of the 8
  if (lg > 3) v += dpp_mov<0x140>(v);            // the other half of the 16
  if (lg > 4) v += __shfl_xor(v, 16, kWave);
  if (lg > 5) v += __shfl_xor(v, 32, kWave);
  return v;
}

template <int V>
__device__ __forceinline__ void load_mean(const double* __restrict__ mean, int64_t off, double* mu) {
  if (!mean) {
#pragma unroll
    for (int e = 0; e < V; ++e) mu[e] = 0.0;
  } else if (V == 1) {
    mu[0] = mean[off];
  } else {                                       // off % V == 0 and the base is 16-byte aligned (checked on the host)
#pragma unroll
    for (int e = 0; e < V; e += 2) {
      const Pack<double, 2> p = *reinterpret_cast<const Pack<double, 2>*>(mean + off + e);
      mu[e] = p.e[0];
      mu[e + 1] = p.e[1];
    }
  }
}

template <typename T, int RC, bool VEC>
__global__ __launch_bounds__(kSweepThreads) void contrib_rows_kernel(const T* __restrict__ X, int64_t I, const double* __restrict__ Tm, int ldt,
                                                                    const double* __restrict__ Hm, int ldh, int R,
                                                                    const double* __restrict__ WA, const double* __restrict__ WB, int A, int B,
                                                                    const double* __restrict__ mean, const int64_t* __restrict__ rows, int64_t n,
                                                                    int G, int lgLK, double* __restrict__ speA, double* __restrict__ speB,
                                                                    double* __restrict__ t2A, double* __restrict__ t2B) {
  extern __shared__ double lds[];
  constexpr int V = VEC ? DiagVec<T>::N : 1;
  constexpr int U = kContribUnroll;
  using VT = Pack<T, V>;
  const int tid = threadIdx.x;
  const int LK = 1 << lgLK, JP = kSweepThreads >> lgLK;
  const int kvl = tid & (LK - 1), jp = tid >> lgLK;
  const bool asum = speA != nullptr;             // false for a matrix block: A = 1, LK = 256, JP = 1
  double* __restrict__ sTH = lds;
  double* __restrict__ accA = sTH + (size_t)A * R * 2;
  double* __restrict__ slab = accA + (asum ? (size_t)G * A * 2 : 0);
  const int64_t P = (int64_t)A * B;
  const int64_t g0 = (int64_t)blockIdx.x * G;
  const int gn = (int)((n - g0 < G) ? n - g0 : G);
  if (asum)
    for (int q = tid; q < gn * A * 2; q += kSweepThreads) accA[q] = 0.0;
  const int span = LK * V;                       // columns of a chunk
  const int steps = (A + JP - 1) / JP;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  for (int k0 = 0; k0 < B; k0 += span) {
    const int k = k0 + kvl * V;
    const bool klive = k < B;                    // B % V == 0: a vector is live or dead as a whole
    const int ks = klive ? k : 0;
    double wb[RC][V];
#pragma unroll
    for (int r = 0; r < RC; ++r)
#pragma unroll
      for (int e = 0; e < V; ++e) wb[r][e] = (r < R) ? WB[(int64_t)(ks + e) * R + r] : 0.0;
    for (int g = 0; g < gn; ++g) {
      const int64_t i = g0 + g;
      const int64_t src = rows ? rows[i] : i;
      const bool ok = src >= 0 && src < I;       // a row index outside X: NaN outputs, nothing read out of bounds
      const T* __restrict__ xrow = X + (ok ? src : 0) * P;
      const double* __restrict__ trow = Tm + i * ldt;
      const double* __restrict__ hrow = Hm + i * ldh;
      for (int q = tid; q < A * R; q += kSweepThreads) {   // fold the row's t and h into the A side
        const double w = WA[q];
        const int r = q % R;
        sTH[2 * q] = trow[r] * w;
        sTH[2 * q + 1] = hrow[r] * w;
      }
      __syncthreads();                           // also orders the zeroed accumulators and the previous row's slab reads
      double be[V], bd[V];
#pragma unroll
      for (int e = 0; e < V; ++e) be[e] = bd[e] = 0.0;
      for (int s0 = 0; s0 < steps; s0 += U) {
        VT xs[U];
        double mu[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (s0 + u < steps) {                  // uniform
            const int j = (s0 + u) * JP + jp;
            const int64_t off = (int64_t)(j < A ? j : 0) * B + ks;
            xs[u] = ld_stream(reinterpret_cast<const VT*>(xrow + off));
            load_mean<V>(mean, off, mu[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (s0 + u < steps) {
            const int j = (s0 + u) * JP + jp;
            const bool jlive = j < A;
            const double* __restrict__ th = sTH + (size_t)(jlive ? j : 0) * R * 2;
            double rec[V], dir[V];
#pragma unroll
            for (int e = 0; e < V; ++e) rec[e] = dir[e] = 0.0;
#pragma unroll
            for (int r = 0; r < RC; ++r) {
              if (r < R) {                       // uniform
                const double ta = th[2 * r], ha = th[2 * r + 1];
#pragma unroll
                for (int e = 0; e < V; ++e) {
                  rec[e] = fma(ta, wb[r][e], rec[e]);
                  dir[e] = fma(ha, wb[r][e], dir[e]);
                }
              }
            }
            double se = 0.0, sd = 0.0;
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const double xc = to_f64(xs[u].e[e]) - mu[u][e];
              const bool fin = jlive && klive && isfinite(xc);   // the np.isfinite mask of calcR2X (util.py:7-15)
              const double ev = fin ? xc - rec[e] : 0.0;         // a NaN score row stays NaN
              const double dv = fin ? xc * dir[e] : 0.0;
              be[e] = fma(ev, ev, be[e]);
              bd[e] += dv;
              se = fma(ev, ev, se);
              sd += dv;
            }
            if (asum) {
              const double te = slice_total(se, lgLK), td = slice_total(sd, lgLK);
              if (kvl == 0 && jlive) {           // the slice's owner: the same thread for every chunk of k
                double* __restrict__ a = accA + ((size_t)g * A + j) * 2;
                a[0] += te;
                a[1] += td;
              }
            }
          }
        }
      }
      if (JP == 1) {                             // every thread holds finished sums over j
        if (klive) {
#pragma unroll
          for (int e = 0; e < V; ++e) {
            speB[i * B + k + e] = ok ? be[e] : qnan;
            t2B[i * B + k + e] = ok ? bd[e] : qnan;
          }
        }
        __syncthreads();                         // TH is rewritten for the next row
      } else {                                   // close the sums over j: slab[jp][column of the chunk][2], added in the order of jp
#pragma unroll
        for (int e = 0; e < V; ++e) {
          double* __restrict__ s = slab + ((size_t)jp * span + kvl * V + e) * 2;
          s[0] = be[e];
          s[1] = bd[e];
        }
        __syncthreads();
        for (int q = tid; q < span; q += kSweepThreads) {
          if (k0 + q < B) {
            double s0v = slab[(size_t)q * 2], s1v = slab[(size_t)q * 2 + 1];
            for (int p = 1; p < JP; ++p) {
              s0v += slab[((size_t)p * span + q) * 2];
              s1v += slab[((size_t)p * span + q) * 2 + 1];
            }
            speB[i * B + k0 + q] = ok ? s0v : qnan;
            t2B[i * B + k0 + q] = ok ? s1v : qnan;
          }
        }
        __syncthreads();
      }
    }
  }
  if (asum) {
    __syncthreads();
    for (int q = tid; q < gn * A; q += kSweepThreads) {
      const int64_t i = g0 + q / A;
      const int64_t src = rows ? rows[i] : i;
      const bool ok = src >= 0 && src < I;
      speA[g0 * A + q] = ok ? accA[(size_t)q * 2] : qnan;
      t2A[g0 * A + q] = ok ? accA[(size_t)q * 2 + 1] : qnan;
    }
  }
}

struct ContribPlan {
  int V, lgLK, G;
  size_t lds;
};

// false: the loadings and accumulators do not fit the LDS
static bool contrib_plan(int64_t n, int R, int A, int B, bool vec, int vecN, bool asum, ContribPlan* p) {
  p->V = vec ? vecN : 1;
  if (!asum) {
    p->lgLK = 8;
  } else {
    const int kv = B / p->V;
    int lg = 0;
    while (lg < 6 && (1 << lg) < kv) ++lg;
    p->lgLK = lg;
  }
  const size_t slab = asum ? (size_t)kSweepThreads * p->V * 2 : 0;
  const size_t th = (size_t)A * R * 2;
  int64_t G = (n + 2047) / 2048;                 // ~2048 workgroups, as resid_rows; at least one row each
  if (G > kContribMaxRows) G = kContribMaxRows;
  if (G < 1) G = 1;
  for (;; G /= 2) {
    p->lds = (th + (asum ? (size_t)G * A * 2 : 0) + slab) * sizeof(double);
    if (p->lds <= kContribLdsMax || G == 1) break;
  }
  p->G = (int)G;
  return p->lds <= kContribLdsMax;
}

template <typename T>
static int run_contrib_rows(const T* X, int64_t I, const double* Tm, int ldt, const double* Hm, int ldh, int R, const double* WA,
                            const double* WB, int A, int B, const double* mean, const int64_t* rows, int64_t n, double* speA, double* speB,
                            double* t2A, double* t2B, hipStream_t st) {
  if (!X || !Tm || !Hm || !WA || !WB || !speB || !t2B || I <= 0 || n <= 0 || R <= 0 || A <= 0 || B <= 0 || ldt < R || ldh < R ||
      (!speA) != (!t2A) || (!speA && A != 1)) {
    set_error("contrib_rows: bad argument");
    return CMTFPLS_EINVAL;
  }
  if (R > kModelMaxR) { set_error("contrib_rows: more than 16 components"); return CMTFPLS_EUNSUPPORTED; }
  const bool vec = (B % DiagVec<T>::N) == 0 && (reinterpret_cast<uintptr_t>(X) & DiagVec<T>::kAlignMask) == 0 &&
                   (reinterpret_cast<uintptr_t>(mean) & 15) == 0;
  ContribPlan p;
  if (!contrib_plan(n, R, A, B, vec, DiagVec<T>::N, speA != nullptr, &p)) {
    set_error("contrib_rows: the first mode's loadings and accumulators (2 A (R + 1) doubles) do not fit the LDS");
    return CMTFPLS_EUNSUPPORTED;
  }
  const dim3 grid((unsigned)((n + p.G - 1) / p.G)), block(kSweepThreads);
  dispatch_model(R, vec, [&](auto rcb, auto vb) {
    auto kernel = contrib_rows_kernel<T, decltype(rcb)::value, decltype(vb)::value>;
    if (p.lds + 1024 > 64 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
    hipLaunchKernelGGL(kernel, grid, block, p.lds, st, X, I, Tm, ldt, Hm, ldh, R, WA, WB, A, B, mean, rows, n, p.G, p.lgLK, speA, speB, t2A,
                       t2B);
  });
  return check_launch("contrib_rows");
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {
int cmtfpls_contrib_rows_f32(const float* X, int64_t I, const double* T, int ldt, const double* H, int ldh, int R, const double* WA,
                             const double* WB, int A, int B, const double* mean, const int64_t* rows, int64_t n, double* speA, double* speB,
                             double* t2A, double* t2B, void* stream) {
  return run_contrib_rows<float>(X, I, T, ldt, H, ldh, R, WA, WB, A, B, mean, rows, n, speA, speB, t2A, t2B, (hipStream_t)stream);
}
int cmtfpls_contrib_rows_f64(const double* X, int64_t I, const double* T, int ldt, const double* H, int ldh, int R, const double* WA,
                             const double* WB, int A, int B, const double* mean, const int64_t* rows, int64_t n, double* speA, double* speB,
                             double* t2A, double* t2B, void* stream) {
  return run_contrib_rows<double>(X, I, T, ldt, H, ldh, R, WA, WB, A, B, mean, rows, n, speA, speB, t2A, t2B, (hipStream_t)stream);
}
// 16-bit X, read in place: 4 k per thread as one 8-byte load, so LK, JP, G and the LDS size are those of the f32 call and the
// outputs have its bits on the upcast values
int cmtfpls_contrib_rows_bf16(const uint16_t* X, int64_t I, const double* T, int ldt, const double* H, int ldh, int R, const double* WA,
                              const double* WB, int A, int B, const double* mean, const int64_t* rows, int64_t n, double* speA, double* speB,
                              double* t2A, double* t2B, void* stream) {
  return run_contrib_rows<bf16_t>(reinterpret_cast<const bf16_t*>(X), I, T, ldt, H, ldh, R, WA, WB, A, B, mean, rows, n, speA, speB, t2A, t2B,
                                  (hipStream_t)stream);
}
int cmtfpls_contrib_rows_f16(const uint16_t* X, int64_t I, const double* T, int ldt, const double* H, int ldh, int R, const double* WA,
                             const double* WB, int A, int B, const double* mean, const int64_t* rows, int64_t n, double* speA, double* speB,
                             double* t2A, double* t2B, void* stream) {
  return run_contrib_rows<f16_t>(reinterpret_cast<const f16_t*>(X), I, T, ldt, H, ldh, R, WA, WB, A, B, mean, rows, n, speA, speB, t2A, t2B,
                                 (hipStream_t)stream);
}
}
