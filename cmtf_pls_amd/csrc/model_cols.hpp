// The column-tile layout of the kernels that stream the fitted model  xhat[i, c] = mean[c] + sum_r T[i, r] WA[c / B, r] WB[c % B, r]
// past X without materialising it: recon / recon_r2 (recon.hip), resid_rows (resid.hip), heldout_resid / impute (impute.hip).
//   grid = (column tiles, row blocks), kSweepThreads threads; a thread owns V consecutive columns (one vector of X), keeps their
//   loading products w[r][e] = WA[j, r] WB[k + e, r] and mean in registers (ModelCols) and walks the rows of its row block; the
//   score row T[i, :] is workgroup-uniform (scalar loads); at most kModelMaxR components per launch, in brackets of 4.
// recon and resid_rows keep this layout written out in their kernels (why: recon.hip, resid.hip) and take the rest from here;
// contrib_rows (contrib.hip) keeps only the B side in registers: it takes the cap, the dispatch and dpp_mov.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace cmtfpls {

constexpr int kModelMaxR = 16;   // components held in registers per launch (recon accumulates more in passes)

struct ColTilePlan {
  int col_tiles, row_blocks;
  int64_t rpb;                   // rows per block
};

// ~2048 workgroups of at least 8 rows
static ColTilePlan col_tile_plan(int64_t I, int64_t P, int V) {
  ColTilePlan p;
  p.col_tiles = (int)(((P + V - 1) / V + kSweepThreads - 1) / kSweepThreads);       // (>= 1 for P >= 1: a block of fewer columns than a
  if (p.col_tiles < 1) p.col_tiles = 1;                                             //  vector made this 0 and the next line divide by it)
  const int64_t want = (2048 + p.col_tiles - 1) / p.col_tiles;
  p.rpb = (I + want - 1) / want;
  if (p.rpb < 8) p.rpb = 8;
  p.row_blocks = (int)((I + p.rpb - 1) / p.rpb);
  return p;
}

// the most bytes(plan) over the vector widths a call may take (1, 2, 4): what a *_workspace_bytes entry answers before the
// storage type and the alignment of X are known
template <typename F>
static size_t most_over_vector_widths(int64_t I, int64_t P, F&& bytes) {
  size_t most = 0;
  for (int V = 1; V <= 4; V *= 2) {
    const size_t nb = bytes(col_tile_plan(I, P, V));
    if (nb > most) most = nb;
  }
  return most;
}

// f(std::integral_constant<int, RC>, std::bool_constant<VEC>) with RC = the bracket (4, 8, 12, 16) that holds rc <= kModelMaxR
template <typename F>
static void dispatch_model(int rc, bool vec, F&& f) {
  auto form = [&](auto RC) {
    if (vec) f(RC, std::true_type{});
    else     f(RC, std::false_type{});
  };
  if (rc <= 4) form(std::integral_constant<int, 4>{});
  else if (rc <= 8) form(std::integral_constant<int, 8>{});
  else if (rc <= 12) form(std::integral_constant<int, 12>{});
  else form(std::integral_constant<int, 16>{});
}

// A thread's V columns c .. c + V - 1 of the model: components 0 .. RC - 1 (those >= R: 0); their mean (nullptr: 0) goes
// to the caller's mu.  mu is no member: w[16][4] alone is the largest private array next to which the compiler still keeps a
// kernel's small arrays in vector registers as before; with mu inside, heldout_resid<float, 16, vector> took 312 registers for
// 211 and lost a wave.
template <int RC, int V>
struct ModelCols {
  double w[RC][V];

  __device__ __forceinline__ ModelCols(int64_t c, int B, int R, const double* WA, const double* WB, const double* mean,
                                       double (&mu)[V]) {
    const int j = (int)(c / B), k = (int)(c % B);          // B % V == 0 in the vector form: one j for the whole vector
#pragma unroll
    for (int r = 0; r < RC; ++r)
#pragma unroll
      for (int e = 0; e < V; ++e) w[r][e] = (r < R) ? WA[(int64_t)j * R + r] * WB[(int64_t)(k + e) * R + r] : 0.0;
#pragma unroll
    for (int e = 0; e < V; ++e) mu[e] = mean ? mean[c + e] : 0.0;
  }

  // acc += tr * (component r of the columns)
  __device__ __forceinline__ void add(int r, double tr, double (&acc)[V]) const {
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = fma(tr, w[r][e], acc[e]);
  }

  // acc += the R <= RC components of the score row trow (uniform across the workgroup), in component order
  __device__ __forceinline__ void add_all(const double* trow, int R, double (&acc)[V]) const {
#pragma unroll
    for (int r = 0; r < RC; ++r) add(r, (r < R) ? trow[r] : 0.0, acc);
  }
};

// the value of another lane of the same 16-lane row, by a DPP control word; needs every lane of the row active
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

}  // namespace cmtfpls
