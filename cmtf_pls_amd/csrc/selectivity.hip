// Target-projection sums for the selectivity ratio (validate.selectivity_ratio), one read of the caller's UNCENTRED X:
//   a[m, c] = sum_i o x tau[i, m]     d[m, c] = sum_i o tau[i, m]^2     s[c] = sum_i o x^2     n[c] = sum_i o
// with x = X[i, c] - mean[c] formed in registers and o = isfinite(x) (the calcR2X mask of resid_rows); the complete form takes
// o = 1 and leaves d to the caller (d_m = sum_i tau[i, m]^2 for every column).
//
// The tiling is xcov_kernel's (xcov.hip): v_mfma_f64_16x16x4_f64, lane l holds row kq = l >> 4 of the 4-row step and the 4
// columns cb + 4 (l & 15) .. + 3 as ONE 16-byte vector; MFMA e of a lane takes element e, so its output column l & 15 is X column
// cb + 4 (l & 15) + e.  A operand = tau[r + kq][16 mt + (l & 15)], B operand = o ? x - mean[c] : 0; the masked form issues a
// second MFMA per element with A = tau^2 and B = o (0 / 1) into a second accumulator set, which is why it holds 32 responses per
// pass (2 tiles of 16, 2 x 64 accumulator doubles per lane) where the complete form holds 64.  s and n are a per-lane fma / add on
// values the MFMA needs anyway, closed over the four lane groups (the same columns, different rows) by two shuffles.  Rows are
// split over gridDim.y row blocks; every block writes its own partial rows, summed in block order by reduce_rows_kernel: no
// atomics, no waiting between workgroups, the same bits on every call.
#include "common.hpp"

namespace cmtfpls {

typedef double d4_t __attribute__((ext_vector_type(4)));

void launch_reduce_rows(const double* part, int nrows, int64_t P, double* out, hipStream_t st);

constexpr int kSelUN = 4;                                // 4-row steps per register stage, as xcov_kernel
constexpr int kSelMaxComplete = kXcovMaxResponses;       // responses per pass: 4 tiles of 16
constexpr int kSelMaxMasked = 32;                        // masked: two accumulator sets, 2 tiles of 16

// FAST: every tile is interior (P % 256 == 0, M % 16 == 0, every row block a whole number of 32-row trips): no clamps, no selects
// on the row / column / response index (the mask o of the masked form stays).  One response tile of f32 X in vector loads without a mask (M <= 16,
// the flagship shape) is held to 3 waves per SIMD, xcov_kernel's residency there: the allocator otherwise lands 3 registers above it.
// The 16-bit instances take no hint: their X stages are half the registers, and the compiler's report puts that instance at
// 96 + 32 (bf16) / 88 + 32 (f16) registers = 4 waves per SIMD on its own, every other vector instance at or above f32's residency.
template <typename T, bool MASKED, bool VEC, int MT, bool FAST>
__global__ __launch_bounds__(256, (MT == 1 && !MASKED && VEC && sizeof(T) == 4) ? 3 : 1) void selectivity_kernel(const T* __restrict__ X, int64_t I, int64_t P,
                                                         const double* __restrict__ Tau, int ldtau, int M,
                                                         const double* __restrict__ mean, double* __restrict__ part_a,
                                                         double* __restrict__ part_d, double* __restrict__ part_s,
                                                         double* __restrict__ part_n, int rows_per_block) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int kq = lane >> 4, nn = lane & 15;
  const int64_t cb = ((int64_t)blockIdx.x * 4 + wv) * 64;
  if (cb >= P) return;                                   // whole wavefront past the last column: it owns no partial entry
  const int64_t c = cb + 4 * nn;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = (r0 + rows_per_block < I) ? r0 + rows_per_block : I;
  using XV = Pack<T, 4>;
  constexpr int UN = kSelUN;
  d4_t acc[MT][4], accd[MASKED ? MT : 1][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[mt][e] = d4_t{0.0, 0.0, 0.0, 0.0};
      if (MASKED) accd[mt][e] = d4_t{0.0, 0.0, 0.0, 0.0};
    }
  bool mok[MT];
  int tcol[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    mok[mt] = (mt * 16 + nn) < M;
    tcol[mt] = mok[mt] ? mt * 16 + nn : M - 1;
  }
  // every load is unconditional (clamped address) and masked afterwards, in two register stages (see xcov_kernel)
  const int64_t cc = (c < P) ? c : (VEC ? P - 4 : P - 1);
  double mu[4], cs[4] = {}, cn[MASKED ? 4 : 1] = {};          // (complete: every column of the block has r1 - r0 rows)
#pragma unroll
  for (int e = 0; e < 4; ++e) mu[e] = mean ? mean[(c + e < P) ? c + e : P - 1] : 0.0;

  auto load_stage = [&](XV (&x)[UN], double (&a)[UN][MT], int64_t r) {
#pragma unroll
    for (int s = 0; s < UN; ++s) {
      const int64_t row = r + 4 * s + kq;
      const int64_t rowc = (FAST || row < r1) ? row : r1 - 1;
      if (VEC) {
        x[s] = ld_stream(reinterpret_cast<const XV*>(X + rowc * P + cc));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[s].e[e] = X[rowc * P + ((cc + e < P) ? cc + e : P - 1)];
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[s][mt] = Tau[rowc * ldtau + tcol[mt]];
    }
  };
  auto mma_stage = [&](const XV (&x)[UN], const double (&a)[UN][MT], int64_t r) {
#pragma unroll
    for (int s = 0; s < UN; ++s) {
      const bool rok = FAST || (r + 4 * s + kq) < r1;
      double am[MT], ad[MASKED ? MT : 1];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        am[mt] = (FAST || (rok && mok[mt])) ? a[s][mt] : 0.0;
        if (MASKED) ad[mt] = am[mt] * am[mt];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double dv = to_f64(x[s].e[e]) - mu[e];
        bool o = FAST || (rok && c + e < P);
        if (MASKED) o = o && __builtin_isfinite(dv);
        const double b = o ? dv : 0.0;
        const double ob = o ? 1.0 : 0.0;
        cs[e] = fma(b, b, cs[e]);
        if (MASKED) cn[e] += ob;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          acc[mt][e] = __builtin_amdgcn_mfma_f64_16x16x4f64(am[mt], b, acc[mt][e], 0, 0, 0);
          if (MASKED) accd[mt][e] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[mt], ob, accd[mt][e], 0, 0, 0);
        }
      }
    }
  };

  XV xa[UN], xb[UN];
  double aa[UN][MT], ab[UN][MT];
  load_stage(xa, aa, r0);
  for (int64_t r = r0; r < r1; r += 8 * UN) {
    load_stage(xb, ab, r + 4 * UN);       // rows past r1 are clamped on load and masked in the MFMAs
    mma_stage(xa, aa, r);
    // FAST has no clamp: the look-ahead of the last trip must stay inside this block's rows
    load_stage(xa, aa, (FAST && r + 8 * UN >= r1) ? r : r + 8 * UN);
    mma_stage(xb, ab, r + 4 * UN);
  }
  if (part_s) {                                          // the four lane groups hold the same columns for different rows
    double* srow = part_s + (int64_t)blockIdx.y * P;
    double* nrow = part_n + (int64_t)blockIdx.y * P;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double v = cs[e], w = MASKED ? cn[e] : 0.0;
      v += __shfl_xor(v, 16, kWave);
      v += __shfl_xor(v, 32, kWave);
      if (MASKED) {
        w += __shfl_xor(w, 16, kWave);
        w += __shfl_xor(w, 32, kWave);
      } else {
        w = (double)(r1 - r0);
      }
      if (kq == 0 && c + e < P) { srow[c + e] = v; nrow[c + e] = w; }
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int m = mt * 16 + kq + 4 * g;
      if (m < M) {
        const int64_t at = ((int64_t)blockIdx.y * M + m) * P + c;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c + e < P) {
            part_a[at + e] = acc[mt][e][g];
            if (MASKED) part_d[at + e] = accd[mt][e][g];
          }
      }
    }
}

static size_t selectivity_ws(int64_t I, int64_t P, int M) {
  const XcovPlan p = plan_xcov(I, P);
  const size_t mc = (size_t)(M < kSelMaxComplete ? M : kSelMaxComplete);       // complete: one set of <= 64 responses
  const size_t mm = (size_t)(M < kSelMaxMasked ? M : kSelMaxMasked);           // masked: two sets of <= 32
  const size_t per = (mc > 2 * mm ? mc : 2 * mm) + 2;                          // + the s and n partial rows
  return (size_t)p.row_blocks * per * (size_t)P * sizeof(double);
}

// One pass: responses [0, M) of Tau (M <= 64 complete, <= 32 masked) into the partials of a (and d), and of s and n when part_s.
template <typename T, bool MASKED>
static void launch_selectivity(const T* X, int64_t I, int64_t P, const double* Tau, int ldtau, int M, const double* mean,
                               double* part_a, double* part_d, double* part_s, double* part_n, const XcovPlan& p, hipStream_t st) {
  const bool vec = (P % 4 == 0) && ((reinterpret_cast<uintptr_t>(X) & (4 * sizeof(T) - 1)) == 0);
  const int mt = (M + 15) / 16;                          // 1, 2, 3 -> 4, 4
  const bool fast = vec && (P % 256 == 0) && (M % 16 == 0) && (M / 16 != 3) && (I % p.rows_per_block == 0) &&
                    (p.rows_per_block % (8 * kSelUN) == 0);
  const dim3 grid(p.col_tiles, p.row_blocks), block(256);
#define SL(VC, MTT, FS) hipLaunchKernelGGL((selectivity_kernel<T, MASKED, VC, MTT, FS>), grid, block, 0, st, X, I, P, Tau, ldtau, M, mean, \
                                           part_a, part_d, part_s, part_n, p.rows_per_block)
#define SM(VC, FS) do { if (mt == 1) SL(VC, 1, FS); else if (mt == 2) SL(VC, 2, FS); else if constexpr (!MASKED) SL(VC, 4, FS); } while (0)
  if (fast) SM(true, true); else if (vec) SM(true, false); else SM(false, false);
#undef SM
#undef SL
}

template <typename T>
static int run_selectivity(const T* X, int64_t I, int64_t P, const double* Tau, int ldtau, int M, const double* mean, int masked,
                           double* a, double* d, double* s, double* n, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!X || !Tau || !a || !s || !n || (masked && !d) || I <= 0 || P <= 0 || M <= 0 || ldtau < M) {
    set_error("selectivity_cols: bad argument");
    return CMTFPLS_EINVAL;
  }
  if (!ws || ws_bytes < selectivity_ws(I, P, M)) { set_error("selectivity_cols: workspace too small"); return CMTFPLS_EWORKSPACE; }
  const XcovPlan p = plan_xcov(I, P);
  const int step = masked ? kSelMaxMasked : kSelMaxComplete;
  const size_t mfirst = (size_t)(M < step ? M : step);
  double* part_a = static_cast<double*>(ws);
  double* part_s = part_a + (size_t)p.row_blocks * (masked ? 2 : 1) * mfirst * P;
  double* part_n = part_s + (size_t)p.row_blocks * P;
  // more responses than one pass holds: further passes over X through the same workspace, ordered on the stream; s and n come
  // out of the first pass
  for (int lo = 0; lo < M; lo += step) {
    const int mc = (M - lo < step) ? M - lo : step;
    double* pd = masked ? part_a + (size_t)p.row_blocks * mc * P : nullptr;
    double* ps = lo == 0 ? part_s : nullptr;
    if (masked) launch_selectivity<T, true>(X, I, P, Tau + lo, ldtau, mc, mean, part_a, pd, ps, part_n, p, st);
    else        launch_selectivity<T, false>(X, I, P, Tau + lo, ldtau, mc, mean, part_a, pd, ps, part_n, p, st);
    launch_reduce_rows(part_a, p.row_blocks, (int64_t)mc * P, a + (int64_t)lo * P, st);
    if (masked) launch_reduce_rows(pd, p.row_blocks, (int64_t)mc * P, d + (int64_t)lo * P, st);
    if (lo == 0) {
      launch_reduce_rows(part_s, p.row_blocks, P, s, st);
      launch_reduce_rows(part_n, p.row_blocks, P, n, st);
    }
  }
  return check_launch("selectivity_cols");
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {

size_t cmtfpls_selectivity_cols_workspace_bytes(int64_t I, int64_t P, int M) {
  if (I <= 0 || P <= 0 || M <= 0) return 0;
  return selectivity_ws(I, P, M);
}
int cmtfpls_selectivity_cols_f32(const float* X, int64_t I, int64_t P, const double* Tau, int ldtau, int M, const double* mean,
                                 int masked, double* a, double* d, double* s, double* n, void* ws, size_t ws_bytes, void* stream) {
  return run_selectivity<float>(X, I, P, Tau, ldtau, M, mean, masked, a, d, s, n, ws, ws_bytes, (hipStream_t)stream);
}
int cmtfpls_selectivity_cols_f64(const double* X, int64_t I, int64_t P, const double* Tau, int ldtau, int M, const double* mean,
                                 int masked, double* a, double* d, double* s, double* n, void* ws, size_t ws_bytes, void* stream) {
  return run_selectivity<double>(X, I, P, Tau, ldtau, M, mean, masked, a, d, s, n, ws, ws_bytes, (hipStream_t)stream);
}
// 16-bit X, read in place: the lane's 4 columns are one 8-byte load, every MFMA operand the f32 entry's on the upcast values
int cmtfpls_selectivity_cols_bf16(const uint16_t* X, int64_t I, int64_t P, const double* Tau, int ldtau, int M, const double* mean,
                                  int masked, double* a, double* d, double* s, double* n, void* ws, size_t ws_bytes, void* stream) {
  return run_selectivity<bf16_t>(reinterpret_cast<const bf16_t*>(X), I, P, Tau, ldtau, M, mean, masked, a, d, s, n, ws, ws_bytes, (hipStream_t)stream);
}
int cmtfpls_selectivity_cols_f16(const uint16_t* X, int64_t I, int64_t P, const double* Tau, int ldtau, int M, const double* mean,
                                 int masked, double* a, double* d, double* s, double* n, void* ws, size_t ws_bytes, void* stream) {
  return run_selectivity<f16_t>(reinterpret_cast<const f16_t*>(X), I, P, Tau, ldtau, M, mean, masked, a, d, s, n, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
