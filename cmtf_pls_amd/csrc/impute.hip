// Imputation and entry-wise validation of the X model (validate.impute / validate.get_q2x_heldout), three streaming kernels:
//   holdout_mask   out = X with a counter-defined random share of its entries replaced by NaN (the private copy a masked refit
//                  needs anyway): one read, one write, no mask tensor
//   heldout_resid  sum over the held-out observed entries of (x - xhat_r)^2 for EVERY prefix model r = 1..R, of (x - mean)^2 and
//                  their number, from ONE read of the original X: the mask is regenerated from the counter, the reconstruction
//                  is never materialised, and the running sum over components is squared after each component
//   impute         non-finite entries replaced by xhat_R rounded once to the storage type, finite entries passed through bit for
//                  bit; in place only the 16-byte vectors that held a non-finite entry are stored
// The hold-out rule: element e of a block (C order) is held out iff
//   unit_open(philox4x32_10(counter = (offset + e) / 4, stream, key = seed).v[(offset + e) % 4]) < fraction,
// stream = 2 + block index (streams 0 and 1 belong to add_noise, synth.hip), offset = global index of the block's first element.
// heldout_resid and impute use the column-tile layout of model_cols.hpp with V = 16 bytes of the storage type (VecOf, not DiagVec:
// the mask and the stores are defined on 16-byte vectors, and neither entry reads 16-bit X).
// Every sum is two-stage in a fixed order (per-workgroup partials, then reduce_rows_kernel): the same bits on every call.
#include "model_cols.hpp"
#include "philox.hpp"

namespace cmtfpls {

constexpr int kMaskMaxBlocks = 4096;     // workgroups of holdout_mask (grid stride beyond): its partial rows

void launch_reduce_rows(const double* part, int nrows, int64_t P, double* out, hipStream_t st);

__device__ __forceinline__ uint32_t philox_word(const Philox4& p, uint32_t l) {
  return l == 0u ? p.v[0] : l == 1u ? p.v[1] : l == 2u ? p.v[2] : p.v[3];      // selects: no dynamically indexed register array
}

// held[e] for the V consecutive global elements g0 .. g0 + V - 1 (V <= 4: they lie in at most two Philox blocks)
template <int V>
__device__ __forceinline__ void holdout_draw(uint64_t g0, uint32_t stream, uint64_t seed, double fraction, bool held[V]) {
  const uint32_t first = (uint32_t)(g0 & 3u);
  const Philox4 p = philox4x32_10(g0 >> 2, stream, seed);
  Philox4 q = p;
  if (V > 1 && first + V > 4u) q = philox4x32_10((g0 >> 2) + 1u, stream, seed);
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const uint32_t l = first + (uint32_t)e;
    const uint32_t word = l < 4u ? philox_word(p, l) : philox_word(q, l - 4u);
    held[e] = unit_open(word) < fraction;
  }
}

// [a, a + n) and [b, b + n) share an element (compared as addresses: the buffers need not belong to one allocation)
template <typename T>
static bool ranges_overlap(const T* a, const T* b, int64_t n) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b), len = (uintptr_t)n * sizeof(T);
  return pa < pb + len && pb < pa + len;
}

// (a) ------------------------------------------------------------------------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void holdout_mask_kernel(const T* __restrict__ X, T* __restrict__ out, int64_t n, double fraction,
                                                           uint64_t seed, uint32_t stream, uint64_t offset, double* __restrict__ part) {
  __shared__ double red[16];
  constexpr int V = VEC ? VecOf<T>::N : 1;
  using VT = Pack<T, V>;
  const int64_t nvec = n / V;
  double hid = 0.0, left = 0.0;
  for (int64_t vi = (int64_t)blockIdx.x * 256 + threadIdx.x; vi < nvec; vi += (int64_t)gridDim.x * 256) {
    const int64_t e0 = vi * V;
    const VT x = ld_stream(reinterpret_cast<const VT*>(X + e0));
    bool held[V];
    holdout_draw<V>(offset + (uint64_t)e0, stream, seed, fraction, held);
    VT o;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const bool fin = isfinite(x.e[e]);
      o.e[e] = held[e] ? (T)NAN : x.e[e];
      hid += (held[e] && fin) ? 1.0 : 0.0;
      left += (!held[e] && fin) ? 1.0 : 0.0;
    }
    st_stream(reinterpret_cast<VT*>(out + e0), o);
  }
  if (VEC && blockIdx.x == 0 && threadIdx.x == 0) {          // the < V elements after the last whole vector
    for (int64_t e = nvec * V; e < n; ++e) {
      bool held[1];
      holdout_draw<1>(offset + (uint64_t)e, stream, seed, fraction, held);
      const T x = X[e];
      const bool fin = isfinite(x);
      out[e] = held[0] ? (T)NAN : x;
      hid += (held[0] && fin) ? 1.0 : 0.0;
      left += (!held[0] && fin) ? 1.0 : 0.0;
    }
  }
  const double h = block_sum(hid, red);
  __syncthreads();
  const double l = block_sum(left, red);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = h;
    part[2 * blockIdx.x + 1] = l;
  }
}

static int mask_blocks(int64_t nvec) {
  int64_t blocks = (nvec + 255) / 256;
  if (blocks < 1) blocks = 1;
  return (int)(blocks > kMaskMaxBlocks ? kMaskMaxBlocks : blocks);
}

template <typename T>
static int run_holdout_mask(const T* X, T* out, int64_t n, double fraction, uint64_t seed, uint32_t stream, uint64_t offset,
                            double* counts, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!X || !out || !counts || n <= 0 || !(fraction >= 0.0) || fraction > 1.0 || ranges_overlap(X, out, n)) {
    set_error("holdout_mask: bad argument (out must not overlap X)");
    return CMTFPLS_EINVAL;
  }
  const bool vec = ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int blocks = mask_blocks(vec ? n / VecOf<T>::N : n);
  if (!ws || ws_bytes < (size_t)blocks * 2 * sizeof(double)) { set_error("holdout_mask: workspace too small"); return CMTFPLS_EWORKSPACE; }
  double* part = static_cast<double*>(ws);
  if (vec) hipLaunchKernelGGL((holdout_mask_kernel<T, true>), dim3(blocks), dim3(256), 0, st, X, out, n, fraction, seed, stream, offset, part);
  else     hipLaunchKernelGGL((holdout_mask_kernel<T, false>), dim3(blocks), dim3(256), 0, st, X, out, n, fraction, seed, stream, offset, part);
  launch_reduce_rows(part, blocks, 2, counts, st);
  return check_launch("holdout_mask");
}

// (b), (c): the (column tile, row block) grid of model_cols.hpp -----------------------------------------------------------------
static size_t impute_most_blocks(int64_t I, int64_t P) {
  return most_over_vector_widths(I, P, [](const ColTilePlan& pl) { return (size_t)pl.col_tiles * pl.row_blocks; });
}

// part[blk][0 .. R-1] = sum (x - xhat_r)^2, [R] = sum (x - mean)^2, [R + 1] = count, over the held-out finite entries of the
// workgroup's tile; xhat_r = mean + the first r components, accumulated in component order
template <typename T, int RC, bool VEC>
__global__ __launch_bounds__(kSweepThreads) void heldout_resid_kernel(const T* __restrict__ X, const double* __restrict__ Tm, int ldt, int R,
                                                                     const double* __restrict__ WA, const double* __restrict__ WB, int B,
                                                                     const double* __restrict__ mean, int64_t I, int64_t P, int rows_per_block,
                                                                     double fraction, uint64_t seed, uint32_t stream, uint64_t offset,
                                                                     double* __restrict__ part) {
  __shared__ double red[16];
  constexpr int V = VEC ? VecOf<T>::N : 1;
  using VT = Pack<T, V>;
  const int64_t c = ((int64_t)blockIdx.x * kSweepThreads + threadIdx.x) * V;
  const bool live = c < P;
  const int64_t i0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t i1 = (i0 + rows_per_block < I) ? i0 + rows_per_block : I;
  double mu[V];
  const ModelCols<RC, V> m(live ? c : 0, B, R, WA, WB, mean, mu);
  double res[RC];
#pragma unroll
  for (int r = 0; r < RC; ++r) res[r] = 0.0;
  double base = 0.0, cnt = 0.0;
  if (live) {
    for (int64_t i = i0; i < i1; ++i) {
      const double* __restrict__ trow = Tm + i * ldt;
      const VT x = ld_stream(reinterpret_cast<const VT*>(X + i * P + c));
      bool held[V];
      holdout_draw<V>(offset + (uint64_t)(i * P + c), stream, seed, fraction, held);
      double acc[V], xv[V];
      bool use[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        xv[e] = (double)x.e[e];
        use[e] = held[e] && isfinite(xv[e]);
        acc[e] = mu[e];
        const double d = use[e] ? xv[e] - mu[e] : 0.0;
        base = fma(d, d, base);
        cnt += use[e] ? 1.0 : 0.0;
      }
#pragma unroll
      for (int r = 0; r < RC; ++r) {
        m.add(r, (r < R) ? trow[r] : 0.0, acc);             // one component, then the prefix model's residual
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const double d = use[e] ? xv[e] - acc[e] : 0.0;
          res[r] = fma(d, d, res[r]);
        }
      }
    }
  }
  const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  double* __restrict__ mine = part + blk * (R + 2);
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const double s = block_sum(res[r], red);
    __syncthreads();
    if (r < R && threadIdx.x == 0) mine[r] = s;
  }
  const double b = block_sum(base, red);
  __syncthreads();
  const double n = block_sum(cnt, red);
  if (threadIdx.x == 0) {
    mine[R] = b;
    mine[R + 1] = n;
  }
}

template <typename T>
static int run_heldout_resid(const T* X, int64_t I, int A, int B, const double* Tm, int ldt, int R, const double* WA, const double* WB,
                             const double* mean, double fraction, uint64_t seed, uint32_t stream, uint64_t offset, double* out,
                             void* ws, size_t ws_bytes, hipStream_t st) {
  if (!X || !Tm || !WA || !WB || !out || I <= 0 || R <= 0 || A <= 0 || B <= 0 || ldt < R || !(fraction >= 0.0) || fraction > 1.0) {
    set_error("heldout_resid: bad argument");
    return CMTFPLS_EINVAL;
  }
  if (R > kModelMaxR) { set_error("heldout_resid: more than 16 components"); return CMTFPLS_EUNSUPPORTED; }
  const bool vec = (B % VecOf<T>::N) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  const int V = vec ? VecOf<T>::N : 1;
  const int64_t P = (int64_t)A * B;
  const ColTilePlan pl = col_tile_plan(I, P, V);
  const size_t nblk = (size_t)pl.col_tiles * pl.row_blocks;
  if (!ws || ws_bytes < nblk * (R + 2) * sizeof(double)) { set_error("heldout_resid: workspace too small"); return CMTFPLS_EWORKSPACE; }
  double* part = static_cast<double*>(ws);
  const dim3 grid(pl.col_tiles, pl.row_blocks), block(kSweepThreads);
  dispatch_model(R, vec, [&](auto rcb, auto vb) {
    hipLaunchKernelGGL((heldout_resid_kernel<T, decltype(rcb)::value, decltype(vb)::value>), grid, block, 0, st, X, Tm, ldt, R, WA, WB, B,
                       mean, I, P, (int)pl.rpb, fraction, seed, stream, offset, part);
  });
  launch_reduce_rows(part, (int)nblk, R + 2, out, st);
  return check_launch("heldout_resid");
}

// X and out may be the same buffer (INPLACE): a thread reads its own vector before it writes it, and no other thread touches it
template <typename T, int RC, bool VEC, bool INPLACE>
__global__ __launch_bounds__(kSweepThreads) void impute_kernel(const T* X, T* out, const double* __restrict__ Tm, int ldt, int R,
                                                              const double* __restrict__ WA, const double* __restrict__ WB, int B,
                                                              const double* __restrict__ mean, int64_t I, int64_t P, int rows_per_block,
                                                              double* __restrict__ part) {
  __shared__ double red[16];
  constexpr int V = VEC ? VecOf<T>::N : 1;
  using VT = Pack<T, V>;
  const int64_t c = ((int64_t)blockIdx.x * kSweepThreads + threadIdx.x) * V;
  const bool live = c < P;
  const int64_t i0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t i1 = (i0 + rows_per_block < I) ? i0 + rows_per_block : I;
  double mu[V];
  const ModelCols<RC, V> m(live ? c : 0, B, R, WA, WB, mean, mu);
  double cnt = 0.0;
  if (live) {
    for (int64_t i = i0; i < i1; ++i) {
      VT x = ld_stream(reinterpret_cast<const VT*>(X + i * P + c));
      bool any = false;
#pragma unroll
      for (int e = 0; e < V; ++e) any = any || !isfinite(x.e[e]);
      if (any) {
        const double* __restrict__ trow = Tm + i * ldt;
        double acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = mu[e];
        m.add_all(trow, R, acc);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const bool fin = isfinite(x.e[e]);
          cnt += fin ? 0.0 : 1.0;
          x.e[e] = fin ? x.e[e] : (T)acc[e];
        }
      }
      if (!INPLACE || any) st_stream(reinterpret_cast<VT*>(out + i * P + c), x);
    }
  }
  const double n = block_sum(cnt, red);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = n;
}

template <typename T>
static int run_impute(const T* X, T* out, int64_t I, int A, int B, const double* Tm, int ldt, int R, const double* WA, const double* WB,
                      const double* mean, double* count, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!X || !out || !Tm || !WA || !WB || !count || I <= 0 || R <= 0 || A <= 0 || B <= 0 || ldt < R) { set_error("impute: bad argument"); return CMTFPLS_EINVAL; }
  if (R > kModelMaxR) { set_error("impute: more than 16 components"); return CMTFPLS_EUNSUPPORTED; }
  const bool inplace = static_cast<const void*>(X) == static_cast<const void*>(out);
  if (!inplace && ranges_overlap(X, out, I * (int64_t)A * B)) { set_error("impute: out overlaps X without being X"); return CMTFPLS_EINVAL; }
  const bool vec = (B % VecOf<T>::N) == 0 && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int V = vec ? VecOf<T>::N : 1;
  const int64_t P = (int64_t)A * B;
  const ColTilePlan pl = col_tile_plan(I, P, V);
  const size_t nblk = (size_t)pl.col_tiles * pl.row_blocks;
  if (!ws || ws_bytes < nblk * sizeof(double)) { set_error("impute: workspace too small"); return CMTFPLS_EWORKSPACE; }
  double* part = static_cast<double*>(ws);
  const dim3 grid(pl.col_tiles, pl.row_blocks), block(kSweepThreads);
  dispatch_model(R, vec, [&](auto rcb, auto vb) {
    constexpr int RC = decltype(rcb)::value;
    constexpr bool VEC = decltype(vb)::value;
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, st, X, out, Tm, ldt, R, WA, WB, B, mean, I, P, (int)pl.rpb, part); };
    if (inplace) launch(impute_kernel<T, RC, VEC, true>);
    else         launch(impute_kernel<T, RC, VEC, false>);
  });
  launch_reduce_rows(part, (int)nblk, 1, count, st);
  return check_launch("impute");
}

}  // namespace cmtfpls

using namespace cmtfpls;

extern "C" {
size_t cmtfpls_holdout_mask_workspace_bytes(int64_t n) {
  return n <= 0 ? 0 : (size_t)mask_blocks(n) * 2 * sizeof(double);
}
int cmtfpls_holdout_mask_f32(const float* X, float* out, int64_t n, double fraction, uint64_t seed, uint32_t stream, uint64_t offset,
                             double* counts, void* ws, size_t ws_bytes, void* hipstream) {
  return run_holdout_mask<float>(X, out, n, fraction, seed, stream, offset, counts, ws, ws_bytes, (hipStream_t)hipstream);
}
int cmtfpls_holdout_mask_f64(const double* X, double* out, int64_t n, double fraction, uint64_t seed, uint32_t stream, uint64_t offset,
                             double* counts, void* ws, size_t ws_bytes, void* hipstream) {
  return run_holdout_mask<double>(X, out, n, fraction, seed, stream, offset, counts, ws, ws_bytes, (hipStream_t)hipstream);
}
size_t cmtfpls_heldout_resid_workspace_bytes(int64_t I, int64_t P, int R) {
  if (I <= 0 || P <= 0 || R <= 0) return 0;
  return impute_most_blocks(I, P) * (size_t)(R + 2) * sizeof(double);
}
int cmtfpls_heldout_resid_f32(const float* X, int64_t I, int A, int B, const double* T, int ldt, int R, const double* WA, const double* WB,
                              const double* mean, double fraction, uint64_t seed, uint32_t stream, uint64_t offset, double* out,
                              void* ws, size_t ws_bytes, void* hipstream) {
  return run_heldout_resid<float>(X, I, A, B, T, ldt, R, WA, WB, mean, fraction, seed, stream, offset, out, ws, ws_bytes, (hipStream_t)hipstream);
}
int cmtfpls_heldout_resid_f64(const double* X, int64_t I, int A, int B, const double* T, int ldt, int R, const double* WA, const double* WB,
                              const double* mean, double fraction, uint64_t seed, uint32_t stream, uint64_t offset, double* out,
                              void* ws, size_t ws_bytes, void* hipstream) {
  return run_heldout_resid<double>(X, I, A, B, T, ldt, R, WA, WB, mean, fraction, seed, stream, offset, out, ws, ws_bytes, (hipStream_t)hipstream);
}
size_t cmtfpls_impute_workspace_bytes(int64_t I, int64_t P) {
  if (I <= 0 || P <= 0) return 0;
  return impute_most_blocks(I, P) * sizeof(double);
}
int cmtfpls_impute_f32(const float* X, float* out, int64_t I, int A, int B, const double* T, int ldt, int R, const double* WA,
                       const double* WB, const double* mean, double* count, void* ws, size_t ws_bytes, void* hipstream) {
  return run_impute<float>(X, out, I, A, B, T, ldt, R, WA, WB, mean, count, ws, ws_bytes, (hipStream_t)hipstream);
}
int cmtfpls_impute_f64(const double* X, double* out, int64_t I, int A, int B, const double* T, int ldt, int R, const double* WA,
                       const double* WB, const double* mean, double* count, void* ws, size_t ws_bytes, void* hipstream) {
  return run_impute<double>(X, out, I, A, B, T, ldt, R, WA, WB, mean, count, ws, ws_bytes, (hipStream_t)hipstream);
}
}
