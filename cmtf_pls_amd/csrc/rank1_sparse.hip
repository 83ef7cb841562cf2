// Sparse rank-1 extraction: the soft-thresholded alternating sweeps that turn the dense leading pair of the A x B
// cross-covariance Z (rank1.hip; tpls.py:84-90) into a sparse one, and the soft-thresholded normalisation of a vector Z.
// Not a reference call site: the reference's loadings are dense (DESIGN 8y states the rule).
//
//   soft(v, lam): theta = lam * max_j |v_j|, out_j = sign(v_j) * max(|v_j| - theta, 0)            0 <= lam < 1
//   sweep:        a = soft(Z wB, lamA); a /= |a|_2;  b = soft(Z^T a, lamB); b /= |b|_2;
//                 d = max(|a - wA|_inf, |b - wB|_inf); (wA, wB) = (a, b); stop when d < tol_s
//
// ONE launch of ONE workgroup of 1024 threads runs every sweep: nothing but __syncthreads between the steps, no other
// workgroup to wait for.  Two forms of the same arithmetic (cmtfpls_rank1_sparse_form):
//   1  Z is staged in LDS once (Z, the four vectors and the partial sums within 150 KB: 128 x 128 is inside);
//   2  Z is read from L2 / global memory on every half-sweep.
// Both read Z 16 bytes at a time when B is even and Z is 16-byte aligned, one double at a time otherwise.  Every sum runs in an
// order fixed by the thread index alone (no atomics), and both forms use the same thread-to-element map: the same input gives
// the same bits on every call and in either form.
#include "common.hpp"

namespace cmtfpls {
namespace {

constexpr int kSpThreads = 1024;
constexpr int kSpWaves = kSpThreads / kWave;
constexpr int kSpPartials = 2048;                 // doubles of column partial sums: slices * B <= 2048 (see col_matvec)
constexpr int kSpSlots = 32;
constexpr size_t kSpLdsBudget = 150 * 1024;
constexpr int kSpMaxSide = 4096;
constexpr int64_t kSpMaxElements = 65536;

// max that keeps a NaN once it has seen one (numpy's max: a NaN vector has a NaN threshold and a NaN distance)
__device__ __forceinline__ double nanmax(double m, double x) { return (x > m || x != x) ? x : m; }

__device__ __forceinline__ double block_nanmax(double v, double* slot) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = nanmax(v, __shfl_xor(v, m, kWave));
  __syncthreads();                                // (the previous reduction's readers are done with the slots)
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = slot[0];
  for (int w = 1; w < kSpWaves; ++w) s = nanmax(s, slot[w]);
  return s;
}

__device__ __forceinline__ double block_total(double v, double* slot) {
  __syncthreads();
  return block_sum(v, slot);
}

// v <- soft(v, lam) / |soft(v, lam)|_2 on n doubles (LDS or global); returns the norm.  The caller has synchronised v.
__device__ double soft_normalize_block(double* v, int64_t n, double lam, double* slot) {
  const int tid = threadIdx.x;
  double m = 0.0;
  for (int64_t j = tid; j < n; j += kSpThreads) m = nanmax(m, fabs(v[j]));
  const double theta = lam * block_nanmax(m, slot);
  double ssq = 0.0;
  for (int64_t j = tid; j < n; j += kSpThreads) {
    const double x = v[j], r = fabs(x) - theta;
    const double o = r > 0.0 ? copysign(r, x) : (r != r ? r : 0.0);      // thresholded entries are exactly +0.0
    v[j] = o;
    ssq += o * o;
  }
  const double nrm = sqrt(block_total(ssq, slot));
  for (int64_t j = tid; j < n; j += kSpThreads) v[j] = v[j] / nrm;       // (a zero vector: 0 / 0 = NaN, as normalize gives it)
  __syncthreads();
  return nrm;
}

// out[r] = sum_c Z[r, c] x[c]: a group of G lanes (a power of two <= 64) per row, 1024 / G rows per pass; the lanes of a
// group take the columns E at a time, strided, and the group closes with a butterfly.  E = 2: one 16-byte load per step.
template <int E>
__device__ __forceinline__ void row_matvec(const double* Z, int A, int B, const double* x, double* out) {
  const int U = B / E;
  int G = 1;
  while (G < U && G < kWave) G <<= 1;
  const int g = threadIdx.x / G, l = threadIdx.x % G, rows = kSpThreads / G;
  for (int base = 0; base < A; base += rows) {
    const int r = base + g;
    double acc = 0.0;
    if (r < A) {
      const double* row = Z + (size_t)r * B;
      for (int u = l; u < U; u += G) {
        if (E == 2) {
          const Pack<double, 2> z = *reinterpret_cast<const Pack<double, 2>*>(row + 2 * u);
          acc += z.e[0] * x[2 * u];
          acc += z.e[1] * x[2 * u + 1];
        } else {
          acc += row[u] * x[u];
        }
      }
    }
    for (int m = G >> 1; m > 0; m >>= 1) acc += __shfl_xor(acc, m, kWave);
    if (r < A && l == 0) out[r] = acc;
  }
}

// out[c] = sum_r Z[r, c] x[r]: thread (unit u, slice s) sums rows s, s + S, ... of its E columns; S = 1024 / U slices leave
// S * B <= 2048 partial sums in LDS, added per column in slice order.  U >= 1024 units: one slice, units strided, no partials.
template <int E>
__device__ __forceinline__ void col_matvec(const double* Z, int A, int B, const double* x, double* out, double* part) {
  const int U = B / E, tid = threadIdx.x;
  if (U >= kSpThreads) {
    for (int u = tid; u < U; u += kSpThreads) {
      double a0 = 0.0, a1 = 0.0;
      for (int r = 0; r < A; ++r) {
        const double* p = Z + (size_t)r * B + E * u;
        if (E == 2) {
          const Pack<double, 2> z = *reinterpret_cast<const Pack<double, 2>*>(p);
          a0 += z.e[0] * x[r];
          a1 += z.e[1] * x[r];
        } else {
          a0 += p[0] * x[r];
        }
      }
      out[E * u] = a0;
      if (E == 2) out[E * u + 1] = a1;
    }
    return;
  }
  const int S = kSpThreads / U, u = tid % U, s = tid / U;
  if (s < S) {
    double a0 = 0.0, a1 = 0.0;
    for (int r = s; r < A; r += S) {
      const double* p = Z + (size_t)r * B + E * u;
      if (E == 2) {
        const Pack<double, 2> z = *reinterpret_cast<const Pack<double, 2>*>(p);
        a0 += z.e[0] * x[r];
        a1 += z.e[1] * x[r];
      } else {
        a0 += p[0] * x[r];
      }
    }
    part[s * B + E * u] = a0;
    if (E == 2) part[s * B + E * u + 1] = a1;
  }
  __syncthreads();
  for (int c = tid; c < B; c += kSpThreads) {
    double acc = 0.0;
    for (int k = 0; k < S; ++k) acc += part[k * B + c];
    out[c] = acc;
  }
}

// LDS: [Z (A * B, form 1 only)] [cur A] [cur B] [new A] [new B] [partials 2048] [slots 32]
template <bool STAGED, int E>
__global__ __launch_bounds__(kSpThreads) void rank1_sparse_kernel(const double* __restrict__ Zg, int A, int B, double* __restrict__ wA,
                                                                  double* __restrict__ wB, double lamA, double lamB, double tol_s,
                                                                  int max_sweeps, double* __restrict__ info) {
  extern __shared__ __align__(16) double sp_lds[];
  const int tid = threadIdx.x;
  const int P = A * B;
  double* zs = sp_lds;
  double* ca = sp_lds + (STAGED ? P : 0);
  double* cb = ca + A;
  double* na = cb + B;
  double* nb = na + A;
  double* part = nb + B + ((A + B) & 1);          // (16-byte aligned again)
  double* slot = part + kSpPartials;
  if (STAGED) {
    if (E == 2) {
      for (int i = tid; i < P / 2; i += kSpThreads)
        reinterpret_cast<Pack<double, 2>*>(zs)[i] = reinterpret_cast<const Pack<double, 2>*>(Zg)[i];
    } else {
      for (int i = tid; i < P; i += kSpThreads) zs[i] = Zg[i];
    }
  }
  const double* Z = STAGED ? zs : Zg;
  for (int i = tid; i < A; i += kSpThreads) ca[i] = wA[i];
  for (int i = tid; i < B; i += kSpThreads) cb[i] = wB[i];
  __syncthreads();
  int sweeps = 0, converged = 0;
  for (int s = 0; s < max_sweeps; ++s) {
    row_matvec<E>(Z, A, B, cb, na);                                      // a = Z wB
    __syncthreads();
    soft_normalize_block(na, A, lamA, slot);
    col_matvec<E>(Z, A, B, na, nb, part);                                // b = Z^T a
    __syncthreads();
    soft_normalize_block(nb, B, lamB, slot);
    double d = 0.0;
    for (int i = tid; i < A; i += kSpThreads) d = nanmax(d, fabs(na[i] - ca[i]));
    for (int i = tid; i < B; i += kSpThreads) d = nanmax(d, fabs(nb[i] - cb[i]));
    d = block_nanmax(d, slot);
    for (int i = tid; i < A; i += kSpThreads) ca[i] = na[i];
    for (int i = tid; i < B; i += kSpThreads) cb[i] = nb[i];
    __syncthreads();
    sweeps = s + 1;
    if (d < tol_s) {                                                     // (d is the same in every thread; tol_s = 0 never stops)
      converged = 1;
      break;
    }
  }
  for (int i = tid; i < A; i += kSpThreads) wA[i] = ca[i];
  for (int i = tid; i < B; i += kSpThreads) wB[i] = cb[i];
  if (info && tid == 0) {
    info[0] = (double)converged;
    info[1] = (double)sweeps;
  }
}

__global__ __launch_bounds__(kSpThreads) void soft_normalize_kernel(double* __restrict__ v, int64_t n, double lam, double* __restrict__ nrm) {
  __shared__ double slot[kSpSlots];
  const double r = soft_normalize_block(v, n, lam, slot);
  if (nrm && threadIdx.x == 0) nrm[0] = r;
}

size_t sparse_lds_bytes(int A, int B, bool staged) {
  const size_t vec = 2 * (size_t)(A + B) + ((A + B) & 1);
  return ((staged ? (size_t)A * B : 0) + vec + kSpPartials + kSpSlots) * sizeof(double);
}

bool sparse_shape_ok(int A, int B) {
  return A >= 2 && B >= 2 && A <= kSpMaxSide && B <= kSpMaxSide && (int64_t)A * B <= kSpMaxElements;
}

template <bool STAGED, int E>
int launch_sparse(const double* Z, int A, int B, double* wA, double* wB, double lamA, double lamB, double tol_s, int max_sweeps,
                  double* info, hipStream_t st) {
  const size_t lds = sparse_lds_bytes(A, B, STAGED);
  auto kernel = rank1_sparse_kernel<STAGED, E>;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3(1), dim3(kSpThreads), lds, st, Z, A, B, wA, wB, lamA, lamB, tol_s, max_sweeps, info);
  return check_launch("rank1_sparse");
}

}  // namespace
}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {

int cmtfpls_rank1_sparse_form(int A, int B) {
  if (!sparse_shape_ok(A, B)) return 0;
  return sparse_lds_bytes(A, B, true) <= kSpLdsBudget ? 1 : 2;
}

size_t cmtfpls_rank1_sparse_workspace_bytes(int A, int B) {
  (void)A;
  (void)B;
  return 0;                                       // every intermediate lives in LDS; kept for the ABI's (ws, ws_bytes) convention
}

int cmtfpls_rank1_sparse_f64(const double* Z, int A, int B, double* wA, double* wB, double lamA, double lamB, double tol_s,
                             int max_sweeps, double* info, void* ws, size_t ws_bytes, void* stream) {
  (void)ws;
  (void)ws_bytes;
  // shape and arguments first: nothing below reads a pointer before they are accepted
  if (!sparse_shape_ok(A, B)) {
    set_error("rank1_sparse: needs 2 <= A, B <= 4096 and A * B <= 65536");
    return CMTFPLS_EUNSUPPORTED;
  }
  if (!(lamA >= 0.0 && lamA < 1.0) || !(lamB >= 0.0 && lamB < 1.0)) { set_error("rank1_sparse: lambda outside [0, 1)"); return CMTFPLS_EINVAL; }
  if (max_sweeps < 1) { set_error("rank1_sparse: max_sweeps < 1"); return CMTFPLS_EINVAL; }
  if (!(tol_s >= 0.0)) { set_error("rank1_sparse: negative tolerance"); return CMTFPLS_EINVAL; }
  if (!Z || !wA || !wB) { set_error("rank1_sparse: bad argument"); return CMTFPLS_EINVAL; }
  hipStream_t st = (hipStream_t)stream;
  const bool staged = cmtfpls_rank1_sparse_form(A, B) == 1;
  const bool vec = (B % 2) == 0 && (reinterpret_cast<uintptr_t>(Z) & 15) == 0;
  if (staged) {
    return vec ? launch_sparse<true, 2>(Z, A, B, wA, wB, lamA, lamB, tol_s, max_sweeps, info, st)
               : launch_sparse<true, 1>(Z, A, B, wA, wB, lamA, lamB, tol_s, max_sweeps, info, st);
  }
  return vec ? launch_sparse<false, 2>(Z, A, B, wA, wB, lamA, lamB, tol_s, max_sweeps, info, st)
             : launch_sparse<false, 1>(Z, A, B, wA, wB, lamA, lamB, tol_s, max_sweeps, info, st);
}

int cmtfpls_soft_normalize_f64(double* v, int64_t n, double lam, double* nrm, void* stream) {
  if (n <= 0 || n > ((int64_t)1 << 24)) { set_error("soft_normalize: needs 1 <= n <= 2^24"); return CMTFPLS_EUNSUPPORTED; }
  if (!(lam >= 0.0 && lam < 1.0)) { set_error("soft_normalize: lambda outside [0, 1)"); return CMTFPLS_EINVAL; }
  if (!v) { set_error("soft_normalize: bad argument"); return CMTFPLS_EINVAL; }
  hipLaunchKernelGGL(soft_normalize_kernel, dim3(1), dim3(kSpThreads), 0, (hipStream_t)stream, v, n, lam, nrm);
  return check_launch("soft_normalize");
}

}  // extern "C"
