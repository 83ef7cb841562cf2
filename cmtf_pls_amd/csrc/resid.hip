// Per-row and per-column residual sums of the model reconstruction, for the sample diagnostics (validate.sample_diagnostics):
//   e[i, c] = x - xhat,  x = X[i, c] - mean[c],  xhat = sum_r T[i, r] WA[c / B, r] WB[c % B, r]
//   rows[i] = (sum_c e^2, sum_c x^2, #finite x)      cols[c] = (sum_i e^2, sum_i x^2)       (entries with x not finite skipped)
// in ONE read of the uncentred X, the reconstruction never materialised.  The column-tile layout of model_cols.hpp; V is DiagVec's
// (16-bit storage: 4 columns, one 8-byte load, f32's mapping).  The thread's loading products and their fma loop are ModelCols'
// written out in the kernel: through the struct the f64 vector forms without column sums took more registers (R <= 8: 82 for 75,
// R <= 12: 102 for 91) and each lost a wave per SIMD.  The column sums stay in the thread's registers; a row sum is a wavefront total (DPP within the
// 16-lane rows, four lane reads across them), parked in the lane numbered after the row and combined over the four
// wavefronts every 64 rows through LDS into one partial per (column tile, row).  Two small fixed-order reduces close the
// partials: no atomics, no waiting between workgroups, the same bits on every call.
#include "model_cols.hpp"

namespace cmtfpls {

constexpr int kResidWaves = kSweepThreads / kWave;
constexpr int kResidUnroll = 4;     // rows whose loads are issued together (divides 64)

void launch_reduce_rows(const double* part, int nrows, int64_t P, double* out, hipStream_t st);

__device__ __forceinline__ double lane_read(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// Total over the 64 lanes, wave-uniform; a fixed sequence of operations (the same bits on every call).  Needs every lane active.
__device__ __forceinline__ double wave_total(double v) {
  v += dpp_mov<0xB1>(v);     // quad_perm [1, 0, 3, 2]: lane ^ 1
  v += dpp_mov<0x4E>(v);     // quad_perm [2, 3, 0, 1]: lane ^ 2
  v += dpp_mov<0x141>(v);    // row_half_mirror: the other quad of the 8
  v += dpp_mov<0x140>(v);    // row_mirror: the other half of the 16
  return (lane_read(v, 0) + lane_read(v, 16)) + (lane_read(v, 32) + lane_read(v, 48));
}

// rpart[ct][i][3]: the workgroup's row sums over its columns; cpart[rb][c][2] (COLS): the thread's column sums over its rows
template <typename T, int RC, bool VEC, bool COLS>
__global__ __launch_bounds__(kSweepThreads) void resid_rows_kernel(const T* __restrict__ X, const double* __restrict__ Tm, int ldt, int R,
                                                                  const double* __restrict__ WA, const double* __restrict__ WB, int B,
                                                                  const double* __restrict__ mean, int64_t I, int64_t P, int rows_per_block,
                                                                  double* __restrict__ rpart, double* __restrict__ cpart) {
  __shared__ double red[3][kResidWaves][kWave];
  constexpr int V = VEC ? DiagVec<T>::N : 1;
  using VT = Pack<T, V>;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int64_t c = ((int64_t)blockIdx.x * kSweepThreads + threadIdx.x) * V;
  const bool live = c < P;
  const int64_t cs = live ? c : 0;                       // dead lanes read column 0 and add nothing: every lane joins the row totals
  const int64_t i0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t i1 = (i0 + rows_per_block < I) ? i0 + rows_per_block : I;
  double w[RC][V], mu[V];                                // ModelCols, written out (see the head of the file)
  const int j = (int)(cs / B), k = (int)(cs % B);        // B % V == 0: one j for the whole vector
#pragma unroll
  for (int r = 0; r < RC; ++r)
#pragma unroll
    for (int e = 0; e < V; ++e) w[r][e] = (r < R) ? WA[(int64_t)j * R + r] * WB[(int64_t)(k + e) * R + r] : 0.0;
#pragma unroll
  for (int e = 0; e < V; ++e) mu[e] = mean ? mean[cs + e] : 0.0;
  double ce[V], cx[V];
#pragma unroll
  for (int e = 0; e < V; ++e) ce[e] = cx[e] = 0.0;
  for (int64_t ib = i0; ib < i1; ib += kWave) {
    const int n = (int)((i1 - ib < kWave) ? i1 - ib : kWave);
    double pe = 0.0, px = 0.0, pn = 0.0;                 // lane l: the wavefront's sums of row ib + l
    for (int l0 = 0; l0 < n; l0 += kResidUnroll) {
      VT xs[kResidUnroll];                               // kResidUnroll rows in flight; past the block's end: its last row again, unused
#pragma unroll
      for (int u = 0; u < kResidUnroll; ++u) {
        const int64_t i = (ib + l0 + u < i1) ? ib + l0 + u : i1 - 1;
        xs[u] = ld_stream(reinterpret_cast<const VT*>(X + i * P + cs));
      }
#pragma unroll
      for (int u = 0; u < kResidUnroll; ++u) {
        const int l = l0 + u;
        const bool use = l < n;                          // uniform
        const double* __restrict__ trow = Tm + (use ? ib + l : i1 - 1) * ldt;
        double acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.0;
#pragma unroll
        for (int r = 0; r < RC; ++r) {
          const double tr = (r < R) ? trow[r] : 0.0;     // uniform across the workgroup
#pragma unroll
          for (int e = 0; e < V; ++e) acc[e] = fma(tr, w[r][e], acc[e]);
        }
        double se = 0.0, sx = 0.0;
        int cnt = 0;
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const double xc = to_f64(xs[u].e[e]) - mu[e];
          const bool fin = use && live && isfinite(xc);  // np.isfinite mask of calcR2X (util.py:7-15)
          const double d = fin ? xc - acc[e] : 0.0;      // a NaN score row stays NaN
          const double xo = fin ? xc : 0.0;
          se = fma(d, d, se);
          sx = fma(xo, xo, sx);
          if (COLS) {
            ce[e] = fma(d, d, ce[e]);
            cx[e] = fma(xo, xo, cx[e]);
          }
          cnt += __popcll(__ballot(fin));
        }
        const double te = wave_total(se), tx = wave_total(sx);
        if (lane == l) { pe = te; px = tx; pn = (double)cnt; }
      }
    }
    red[0][wv][lane] = pe;
    red[1][wv][lane] = px;
    red[2][wv][lane] = pn;
    __syncthreads();
    if (threadIdx.x < 3 * kWave) {
      const int q = threadIdx.x / kWave, l = lane;
      if (l < n) {
        double s = red[q][0][l];
#pragma unroll
        for (int g = 1; g < kResidWaves; ++g) s += red[q][g][l];
        rpart[((int64_t)blockIdx.x * I + ib + l) * 3 + q] = s;
      }
    }
    __syncthreads();
  }
  if (COLS && live) {
    double* __restrict__ cp = cpart + ((int64_t)blockIdx.y * P + c) * 2;
#pragma unroll
    for (int e = 0; e < V; ++e) { cp[2 * e] = ce[e]; cp[2 * e + 1] = cx[e]; }
  }
}

static size_t resid_ws(int64_t I, int64_t P, const ColTilePlan& pl) {
  return ((size_t)pl.col_tiles * I * 3 + (size_t)pl.row_blocks * P * 2) * sizeof(double);
}

template <typename T>
static int run_resid_rows(const T* X, const double* Tm, int64_t I, int ldt, int R, const double* WA, const double* WB, int A, int B,
                          const double* mean, double* rows, double* cols, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!X || !Tm || !WA || !WB || !rows || I <= 0 || R <= 0 || A <= 0 || B <= 0 || ldt < R) { set_error("resid_rows: bad argument"); return CMTFPLS_EINVAL; }
  if (R > kModelMaxR) { set_error("resid_rows: more than 16 components"); return CMTFPLS_EUNSUPPORTED; }
  const bool vec = (B % DiagVec<T>::N) == 0 && (reinterpret_cast<uintptr_t>(X) & DiagVec<T>::kAlignMask) == 0;
  const int V = vec ? DiagVec<T>::N : 1;
  const int64_t P = (int64_t)A * B;
  const ColTilePlan pl = col_tile_plan(I, P, V);
  if (!ws || ws_bytes < resid_ws(I, P, pl)) { set_error("resid_rows: workspace too small"); return CMTFPLS_EWORKSPACE; }
  double* rpart = static_cast<double*>(ws);
  double* cpart = rpart + (size_t)pl.col_tiles * I * 3;
  const dim3 grid(pl.col_tiles, pl.row_blocks), block(kSweepThreads);
  dispatch_model(R, vec, [&](auto rcb, auto vb) {
    constexpr int RC = decltype(rcb)::value;
    constexpr bool VEC = decltype(vb)::value;
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, st, X, Tm, ldt, R, WA, WB, B, mean, I, P, (int)pl.rpb, rpart, cpart); };
    if (cols) launch(resid_rows_kernel<T, RC, VEC, true>);
    else      launch(resid_rows_kernel<T, RC, VEC, false>);
  });
  launch_reduce_rows(rpart, pl.col_tiles, I * 3, rows, st);
  if (cols) launch_reduce_rows(cpart, pl.row_blocks, P * 2, cols, st);
  return check_launch("resid_rows");
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {
size_t cmtfpls_resid_rows_workspace_bytes(int64_t I, int64_t P) {
  if (I <= 0 || P <= 0) return 0;
  return most_over_vector_widths(I, P, [&](const ColTilePlan& pl) { return resid_ws(I, P, pl); });
}
int cmtfpls_resid_rows_f32(const float* X, const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB, int A, int B,
                           const double* mean, double* rows, double* cols, void* ws, size_t ws_bytes, void* stream) {
  return run_resid_rows<float>(X, T, I, ldt, R, WA, WB, A, B, mean, rows, cols, ws, ws_bytes, (hipStream_t)stream);
}
int cmtfpls_resid_rows_f64(const double* X, const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB, int A, int B,
                           const double* mean, double* rows, double* cols, void* ws, size_t ws_bytes, void* stream) {
  return run_resid_rows<double>(X, T, I, ldt, R, WA, WB, A, B, mean, rows, cols, ws, ws_bytes, (hipStream_t)stream);
}
// 16-bit X, read in place: 4 columns per thread as one 8-byte load, f32's mapping and so its bits on the upcast values
int cmtfpls_resid_rows_bf16(const uint16_t* X, const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB, int A, int B,
                            const double* mean, double* rows, double* cols, void* ws, size_t ws_bytes, void* stream) {
  return run_resid_rows<bf16_t>(reinterpret_cast<const bf16_t*>(X), T, I, ldt, R, WA, WB, A, B, mean, rows, cols, ws, ws_bytes, (hipStream_t)stream);
}
int cmtfpls_resid_rows_f16(const uint16_t* X, const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB, int A, int B,
                           const double* mean, double* rows, double* cols, void* ws, size_t ws_bytes, void* stream) {
  return run_resid_rows<f16_t>(reinterpret_cast<const f16_t*>(X), T, I, ldt, R, WA, WB, A, B, mean, rows, cols, ws, ws_bytes, (hipStream_t)stream);
}
}
