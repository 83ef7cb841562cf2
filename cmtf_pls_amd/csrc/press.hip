// Squared prediction errors of the models of one cross-validation pass, scored where their state lies (nested.py):
//   h = T[j, i, :] coef[j]   (coef upper triangular: only k <= c is read)
//   pred_r[j, i, m] = nu[j, m] + sum_{c < r} h_c Q[j, c, m]
//   press[j, r - 1] = sum over the rows with eval[j, i] > 0 and over m of (pred_r - Y[i, m])^2;  eval == 2 also stores pred_r.
// A workgroup takes 1024 consecutive rows of ONE model: it reads their eval words, packs the rows to score into an LDS list in
// row order (ballot + prefix: nothing of a skipped row is read beyond that word) and leaves at once when the list is empty.
// Otherwise coef[j], Q[j] and nu[j] go to LDS and every 16-lane group takes a row of the list at a time: lane s builds
// h_c for c = s, s + 16, .. (a column of coef per lane: consecutive LDS words), then the group walks c = 0 .. R - 1 with h_c
// passed round by a lane read, lane s carrying the running prediction of the responses m = s, s + 16, .. and one squared-error
// accumulator per component.  A row per lane would carry 2 R + M doubles per lane (384 registers at the limits) where this
// carries R + R / 16 + 2 M / 16, and its loads of T would be 64 scattered rows per instruction instead of 4.
// The accumulators close with a wavefront butterfly and an in-order sum of the four wavefronts into one partial row per
// (row tile, model); launch_reduce_rows adds the row tiles in order: no atomics, the same bits on every call.
#include "common.hpp"

namespace cmtfpls {

constexpr int kPressMaxR = 64, kPressMaxM = 64;        // the K-fold state's own limits (kfold.py MAX_COMPONENTS, MAX_RESPONSES)
constexpr int kPressThreads = 256;
constexpr int kPressTile = 1024;                       // rows of a workgroup
constexpr int kPressGroup = 16;                        // lanes of a row
constexpr int kPressWaves = kPressThreads / kWave;

void launch_reduce_rows(const double* part, int nrows, int64_t P, double* out, hipStream_t st);

static size_t press_lds_bytes(int R, int M) {
  return ((size_t)R * R + (size_t)R * M + M + (size_t)kPressWaves * kPressMaxR) * sizeof(double) + (kPressTile + 16) * sizeof(int);
}

// RC >= R components and MQ * 16 >= M responses held in registers
template <int RC, int MQ>
__global__ __launch_bounds__(kPressThreads) void press_rows_kernel(const double* __restrict__ T, const double* __restrict__ coef,
                                                                  const double* __restrict__ Q, const double* __restrict__ nu,
                                                                  const double* __restrict__ Y, const int* __restrict__ eval, int64_t I,
                                                                  int R, int M, double* __restrict__ part, double* __restrict__ pred) {
  extern __shared__ __attribute__((aligned(16))) unsigned char press_smem[];
  double* sC = reinterpret_cast<double*>(press_smem);  // R x R
  double* sQ = sC + R * R;                             // R x M
  double* sNu = sQ + R * M;                            // M
  double* red = sNu + M;                               // kPressWaves x kPressMaxR
  int* list = reinterpret_cast<int*>(red + kPressWaves * kPressMaxR);   // kPressTile: row - i0, bit 30 set when eval == 2
  int* wcnt = list + kPressTile;                       // kPressWaves + 1: the wavefronts' counts of a chunk, then the running total
  constexpr int HQ = RC / kPressGroup;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const int j = blockIdx.y, n = gridDim.y;
  const int64_t i0 = (int64_t)blockIdx.x * kPressTile;
  const int rows = (int)((I - i0 < kPressTile) ? I - i0 : kPressTile);
  const int* __restrict__ ev = eval + (int64_t)j * I + i0;

  if (tid == 0) wcnt[kPressWaves] = 0;
  __syncthreads();
  for (int b = 0; b < rows; b += kPressThreads) {      // the rows to score, in row order
    const int r = b + tid;
    const int e = (r < rows) ? ev[r] : 0;
    const unsigned long long mask = __ballot(e > 0);
    if (lane == 0) wcnt[wv] = __popcll(mask);
    __syncthreads();
    int at = wcnt[kPressWaves];
    for (int w = 0; w < wv; ++w) at += wcnt[w];
    if (e > 0) list[at + __popcll(mask & ((1ull << lane) - 1ull))] = r | (e == 2 ? (1 << 30) : 0);
    __syncthreads();
    if (tid == 0) {
      int s = wcnt[kPressWaves];
      for (int w = 0; w < kPressWaves; ++w) s += wcnt[w];
      wcnt[kPressWaves] = s;
    }
    __syncthreads();
  }
  const int cnt = wcnt[kPressWaves];
  double* __restrict__ prow = part + ((int64_t)blockIdx.x * n + j) * R;
  if (cnt == 0) {                                      // nothing of this model in the tile: T, coef and Q stay unread
    if (tid < R) prow[tid] = 0.0;
    return;
  }
  for (int e = tid; e < R * R; e += kPressThreads) sC[e] = coef[(int64_t)j * R * R + e];
  for (int e = tid; e < R * M; e += kPressThreads) sQ[e] = Q[(int64_t)j * R * M + e];
  if (tid < M) sNu[tid] = nu[(int64_t)j * M + tid];
  __syncthreads();

  const int sub = lane & (kPressGroup - 1), gbase = lane - sub;
  const int grp = tid / kPressGroup;
  double acc[RC];
#pragma unroll
  for (int c = 0; c < RC; ++c) acc[c] = 0.0;
  for (int li = grp; li < cnt; li += kPressThreads / kPressGroup) {
    const int word = list[li];
    const bool store = (word >> 30) != 0 && pred != nullptr;
    const int64_t i = i0 + (word & ((1 << 30) - 1));
    const double* __restrict__ trow = T + ((int64_t)j * I + i) * R;
    double hv[HQ];
#pragma unroll
    for (int q = 0; q < HQ; ++q) hv[q] = 0.0;
    for (int k = 0; k < R; ++k) {                      // h_c = sum_{k <= c} t_k coef[k, c], k ascending
      const double t = trow[k];
#pragma unroll
      for (int q = 0; q < HQ; ++q) {
        const int c = sub + kPressGroup * q;
        if (c < R && k <= c) hv[q] = fma(t, sC[k * R + c], hv[q]);
      }
    }
    double pr[MQ], yv[MQ];
#pragma unroll
    for (int q = 0; q < MQ; ++q) {
      const int m = sub + kPressGroup * q;
      pr[q] = (m < M) ? sNu[m] : 0.0;
      yv[q] = (m < M) ? Y[i * M + m] : 0.0;
    }
#pragma unroll
    for (int c = 0; c < RC; ++c) {
      if (c < R) {                                     // uniform
        const double hc = __shfl(hv[c / kPressGroup], gbase + (c % kPressGroup), kWave);
#pragma unroll
        for (int q = 0; q < MQ; ++q) {
          const int m = sub + kPressGroup * q;
          if (m < M) {
            pr[q] = fma(hc, sQ[c * M + m], pr[q]);
            const double d = pr[q] - yv[q];
            acc[c] = fma(d, d, acc[c]);
            if (store) pred[((int64_t)c * I + i) * M + m] = pr[q];
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < RC; ++c) {
    const double s = wave_sum(acc[c]);
    if (lane == 0) red[wv * kPressMaxR + c] = s;
  }
  __syncthreads();
  if (tid < R) {
    double s = red[tid];
#pragma unroll
    for (int w = 1; w < kPressWaves; ++w) s += red[w * kPressMaxR + tid];
    prow[tid] = s;
  }
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {
size_t cmtfpls_press_rows_workspace_bytes(int n, int64_t I, int R, int M) {
  if (n <= 0 || I <= 0 || R <= 0 || M <= 0) return 0;
  return (size_t)((I + kPressTile - 1) / kPressTile) * n * R * sizeof(double);
}

int cmtfpls_press_rows_f64(const double* T, const double* coef, const double* Q, const double* nu, const double* Y, const int* eval,
                           int n, int64_t I, int R, int M, double* press, double* pred, void* ws, size_t ws_bytes, void* stream) {
  if (!T || !coef || !Q || !nu || !Y || !eval || !press || n <= 0 || I <= 0 || R <= 0 || M <= 0) {
    set_error("press_rows: bad argument");
    return CMTFPLS_EINVAL;
  }
  if (R > kPressMaxR || M > kPressMaxM || n > 65535) {
    set_error("press_rows: more than 64 components, 64 responses or 65535 models");
    return CMTFPLS_EUNSUPPORTED;
  }
  if (!ws || ws_bytes < cmtfpls_press_rows_workspace_bytes(n, I, R, M)) { set_error("press_rows: workspace too small"); return CMTFPLS_EWORKSPACE; }
  const int tiles = (int)((I + kPressTile - 1) / kPressTile);
  const size_t lds = press_lds_bytes(R, M);
  const dim3 grid(tiles, n), block(kPressThreads);
  hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(ws);
#define PRK(RCC, MQQ) do { \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(press_rows_kernel<RCC, MQQ>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    hipLaunchKernelGGL((press_rows_kernel<RCC, MQQ>), grid, block, lds, st, T, coef, Q, nu, Y, eval, I, R, M, part, pred); } while (0)
#define PRM(RCC) do { if (M <= 16) PRK(RCC, 1); else if (M <= 32) PRK(RCC, 2); else PRK(RCC, 4); } while (0)
  if (R <= 16) PRM(16); else if (R <= 32) PRM(32); else PRM(64);
#undef PRM
#undef PRK
  launch_reduce_rows(part, tiles, (int64_t)n * R, press, st);
  return check_launch("press_rows");
}
}
