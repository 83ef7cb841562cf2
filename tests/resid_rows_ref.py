"""Restatement, bounds, plans and case tables for the residual pass cmtfpls_resid_rows_* (csrc/resid.hip) and the launch plan of
the contribution pass cmtfpls_contrib_rows_* (csrc/contrib.hip).  tests/test_resid_rows_ref_cpu.py checks this module on the
CPU; tests/test_gpu_resid_rows_forms.py and tests/test_gpu_contributions.py run the kernels against it.

The operation
-------------
x = X - mean over the STORED values of X (float32 widened), xhat = sum_r T[i, r] WA[c / B, r] WB[c % B, r], d = x - xhat where x
is finite, else the entry is skipped.  Per row i: (sum_c d^2, sum_c x^2, #finite x); per column c: (sum_i d^2, sum_i x^2).

Two references
--------------
`reference_ld` accumulates in np.longdouble (64-bit significand) with whole-array NumPy operations: the small shapes.
`reference_torch` is float64 torch on whatever device X lives on, by row chunks of 1/16 of X so that no temporary reaches the
size of X in float64: the tall shapes.  Its reconstruction is a matrix product T W^T and its sums are torch.sum -- neither
shares an operation order with the kernel (a thread's fma chain over r, DPP wavefront totals, an LDS combine, reduce_rows).

The bound (nothing in it is measured)
-------------------------------------
It is the recon_r2 bound of tests/small_algebra_ref.py's docstring, applied to every output on its own.  u = 2^-53.
* xhat has R terms of two products each: |xhathat - xhat| <= bh = gamma_(R+1) sum_r |T WA WB|.
* x = X - mean rounds once, ex = u |x| (0 without a mean: widening float32 is exact).
* d = x - xhat rounds once more: |dhat - d| <= ed = bh + ex + u (|d| + bh + ex).
* An output is a sum of n squares of values known to within ed (or ex for sum x^2):
  bound_two_level(|d|, ed, n) = sum (2 |d| ed + ed^2) + gamma_n sum (|d| + ed)^2, the sums over the finite entries of that row
  (n = P terms) or of that column (n = I terms).  gamma_n with n the number of TERMS holds in any order of addition, so the
  kernel's tree (shorter than n) and torch's are both covered.
* `reference_ld` is exact to 2^-64: REF_SLACK of small_algebra_ref covers it.  `reference_torch` is itself a float64
  evaluation that obeys the same bound, so against it the bound is DOUBLED (|got - want| <= |got - exact| + |want - exact|).
* The counts are integers below 2^53: exact.

Inputs and the discrimination condition
---------------------------------------
`small_algebra_ref.recon_r2_inputs("rounding", ...)`: |xhat| <= 0.85 and |x| in [1.5, 2.5], so |d| in [0.65, 3.35]: no square
of either sum is near zero.  A dropped, doubled or misplaced row then changes an output by at least one square, which is
`margin(n, R, doubled, lo, hi)` = min square / bound times the bound.  tests/test_resid_rows_ref_cpu.py asserts margin >= 1000 for every
case of the tables below (the tightest is a column of case c: 409603 squares against the doubled bound, 1009).
"""
import math

import numpy as np

import small_algebra_ref as SA

LD = np.longdouble
U = SA.U
THREADS, WAVE, UNROLL = 256, 64, 4          # kSweepThreads, kWave, kResidUnroll
D_LO, D_HI = math.sqrt(SA.RECON_R2_TERMS[0]), math.sqrt(SA.RECON_R2_TERMS[1])
X_LO, X_HI = 1.5, 2.5


def _cdiv(a, b):
    return -(-a // b)


# ---- plans -------------------------------------------------------------------------------------------------------------------------
def vec_width(st, B, misaligned=False):
    """Elements per thread: one 16-byte vector when B is a multiple of it and the base of X is 16-byte aligned, else one."""
    n = 4 if st == "f32" else 2
    return n if B % n == 0 and not misaligned else 1


def resid_plan(I, P, V):
    """(col_tiles, row_blocks, rows_per_block, rows in the last block) of resid_plan in csrc/resid.hip."""
    col_tiles = max(1, _cdiv(_cdiv(P, V), THREADS))
    want = _cdiv(2048, col_tiles)
    rpb = max(8, _cdiv(I, want))
    row_blocks = _cdiv(I, rpb)
    return col_tiles, row_blocks, rpb, I - (row_blocks - 1) * rpb


def resid_workspace_bytes(I, P, V):
    ct, rb, _, _ = resid_plan(I, P, V)
    return (ct * I * 3 + rb * P * 2) * 8


def chunks_per_block(rpb):
    """Trips of the kernel's loop over 64-row chunks in a full row block, and the rows of the last one."""
    return _cdiv(rpb, WAVE), rpb - (_cdiv(rpb, WAVE) - 1) * WAVE


CONTRIB_MAX_ROWS, CONTRIB_LDS_MAX = 8, 160 * 1024


def contrib_plan(n, R, A, B, V):
    """(G, lgLK, lds_bytes, fits) of contrib_plan in csrc/contrib.hip for the form with A sums (A > 1): G rows per workgroup,
    2^lgLK lanes along k.  `g_start` of `contrib_g_start` is G before the loop that halves it."""
    kv = B // V
    lg = 0
    while lg < 6 and (1 << lg) < kv:
        lg += 1
    slab = THREADS * V * 2
    th = A * R * 2
    G = contrib_g_start(n)
    while True:
        lds = (th + G * A * 2 + slab) * 8
        if lds <= CONTRIB_LDS_MAX or G == 1:
            break
        G //= 2
    return G, lg, lds, lds <= CONTRIB_LDS_MAX


def contrib_g_start(n):
    return max(1, min(CONTRIB_MAX_ROWS, _cdiv(n, 2048)))


# ---- the references: (rows (I, 3), cols (P, 2), bound_rows (I, 2), bound_cols (P, 2)) as NumPy arrays ------------------------------
def reference_ld(X, T, WA, WB, mu):
    """np.longdouble.  X: the stored values as float64 (I, P); T (I, R); mu (P,) or None."""
    I, P = X.shape
    R = T.shape[1]
    W = (WA.astype(LD)[:, None, :] * WB.astype(LD)[None, :, :]).reshape(P, R)
    xhat = T.astype(LD) @ W.T
    hmag = np.abs(T) @ np.abs(W.astype(np.float64)).T
    xc = X.astype(LD) - (np.zeros(P) if mu is None else mu).astype(LD)[None, :]
    fin = np.isfinite(xc)
    xc0 = np.where(fin, xc, 0)
    d = np.where(fin, xc0 - xhat, 0)
    xa, da = np.abs(xc0.astype(np.float64)), np.abs(d.astype(np.float64))
    bh = SA.bound_sum(R + 1, hmag)
    ex = np.where(fin, 0.0 if mu is None else U * xa, 0.0)
    ed = np.where(fin, bh + ex + U * (da + bh + ex), 0.0)
    rows = np.stack([np.sum(d * d, axis=1), np.sum(xc0 * xc0, axis=1), fin.sum(axis=1).astype(LD)], axis=1)
    cols = np.stack([np.sum(d * d, axis=0), np.sum(xc0 * xc0, axis=0)], axis=1)
    brows = np.array([[SA.bound_two_level(da[i], ed[i], P), SA.bound_two_level(xa[i], ex[i], P)] for i in range(I)])
    bcols = np.array([[SA.bound_two_level(da[:, c], ed[:, c], I), SA.bound_two_level(xa[:, c], ex[:, c], I)] for c in range(P)])
    return rows, cols, brows, bcols


def reference_torch(X2, T, WA, WB, mean, chunks=16):
    """float64 torch on the device of X2 (storage type, (I, P)), by row chunks; the bound is doubled (module docstring)."""
    import torch
    I, P = X2.shape
    R = T.shape[1]
    f64 = torch.float64
    W = (WA.to(f64)[:, None, :] * WB.to(f64)[None, :, :]).reshape(P, R)
    Wa = W.abs()
    gh, gP, gI = SA.gamma(R + 1) * SA.REF_SLACK, SA.gamma(P), SA.gamma(I)
    rows = torch.empty(I, 3, dtype=f64, device=X2.device)
    brows = torch.empty(I, 2, dtype=f64, device=X2.device)
    cols = torch.zeros(P, 2, dtype=f64, device=X2.device)
    bc1 = torch.zeros(P, 2, dtype=f64, device=X2.device)        # sum (2 |v| e + e^2)
    bc2 = torch.zeros(P, 2, dtype=f64, device=X2.device)        # sum (|v| + e)^2
    step = max(1, _cdiv(I, chunks))
    for a in range(0, I, step):
        b = min(I, a + step)
        x = X2[a:b].to(f64)
        if mean is not None:
            x = x - mean
        fin = torch.isfinite(x)
        x = torch.where(fin, x, 0.0)
        d = torch.where(fin, x - T[a:b] @ W.T, 0.0)
        bh = gh * (T[a:b].abs() @ Wa.T)
        xa, da = x.abs(), d.abs()
        ex = U * xa if mean is not None else torch.zeros_like(xa)
        ed = torch.where(fin, bh + ex + U * (da + bh + ex), 0.0)
        del bh
        rows[a:b, 0], rows[a:b, 1], rows[a:b, 2] = (d * d).sum(1), (x * x).sum(1), fin.sum(1).to(f64)
        cols[:, 0] += (d * d).sum(0)
        cols[:, 1] += (x * x).sum(0)
        for q, (v, e) in enumerate(((da, ed), (xa, ex))):
            first, second = 2.0 * v * e + e * e, (v + e) ** 2
            brows[a:b, q] = first.sum(1) + gP * second.sum(1)
            bc1[:, q] += first.sum(0)
            bc2[:, q] += second.sum(0)
    scale = 2.0 * SA.REF_SLACK
    return (rows.cpu().numpy(), cols.cpu().numpy(), (brows * scale).cpu().numpy(), ((bc1 + gI * bc2) * scale).cpu().numpy())


def margin(n, R, doubled, lo, hi, mean=True):
    """min square / bound of an output that sums n squares of values of magnitude in [lo, hi] (the d^2 sum: D_LO, D_HI; the x^2
    sum: X_LO, X_HI), every entry finite: the worst case, fewer finite entries only lower the bound."""
    if (lo, hi) == (X_LO, X_HI):
        e = U * hi if mean else 0.0
    else:
        bh = SA.gamma(R + 1) * 0.85 * SA.REF_SLACK
        ex = U * X_HI if mean else 0.0
        e = bh + ex + U * (hi + bh + ex)
    bound = (n * (2 * hi * e + e * e) + SA.gamma(n) * n * (hi + e) ** 2) * SA.REF_SLACK * (2.0 if doubled else 1.0)
    return lo * lo / bound


def inputs(rng, I, A, B, R, st, mean, nan_fraction=0.0, pad=3):
    """recon_r2_inputs' rounding form with `pad` columns of NaN behind T's R columns (ldt = R + pad): (X stored values as
    float64, T (I, R + pad), WA, WB, mean or None)."""
    X, T, WA, WB, mu = SA.recon_r2_inputs("rounding", rng, I, A, B, R, np.float32 if st == "f32" else np.float64, mean,
                                          ldt_extra=pad, nan_fraction=nan_fraction)
    T[:, R:] = np.nan
    return X, T, WA, WB, mu


# ---- case tables -------------------------------------------------------------------------------------------------------------------
STORAGE = ["f32", "f64"]


def _both(name, I, A, B, R, misaligned, mean, plan):
    return [(name, st, I, A, B, R, misaligned, mean, plan) for st in STORAGE]


# (name, storage, I, A, B, R, misaligned view, mean, plan = (col_tiles, row_blocks, rows_per_block, rows in the last block))
TALL_CASES = (
    # n = 21: lanes up to 20 hold rows, the unroll tail (21 % 4 = 1) inside every block
    _both("a", 43003, 2, 4, 3, False, True, (1, 2048, 21, 16)) +
    _both("a one element", 143357, 2, 3, 6, False, True, (1, 2048, 70, 67)) +
    _both("a view", 43003, 2, 4, 3, True, True, (1, 2048, 21, 16)) +
    # two chunks per block, the second of 6 rows (3 in the last block)
    _both("b", 143357, 2, 4, 5, False, True, (1, 2048, 70, 67)) +
    _both("b no mean", 143357, 2, 4, 5, False, False, (1, 2048, 70, 67)) +
    # four chunks per block, three of them full: all 64 lanes hold rows
    _both("c", 409603, 2, 4, 10, False, True, (1, 2038, 201, 166)) +
    # two column tiles, the second mostly dead lanes; all four wavefronts live in the first
    [("d", "f32", 66000, 4, 65, 16, False, True, (2, 1016, 65, 25)), ("d", "f64", 66000, 2, 260, 16, False, True, (2, 1016, 65, 25))] +
    # the first rows_per_block above the floor of 8
    _both("e", 18432, 2, 4, 2, False, True, (1, 2048, 9, 9)))

SPECIAL = (143357, 2, 4, 5)                         # I, A, B, R: the special rows and columns run on case b's shape
# NaN score rows of row block 5 (70 rows per block): local row 66 is lane 2 of the second chunk (which has 6 rows, so no lane
# of it is >= 8), local row 40 is lane 40 of the first chunk
SPECIAL_SCORE_ROWS = (5 * 70 + 66, 5 * 70 + 40)
CHUNK_R = [4, 5, 8, 9, 12, 13, 16]                  # both sides of every register-chunk boundary, and the last
CHUNK_SHAPES = [(300, 5, 7), (257, 6, 8)]           # one element per thread; vector loads

# contrib_rows: (n, A, B, R, storage) -> (G before the halving loop, G, lgLK)
CONTRIB_LDS_CASES = [((16385, 800, 4, 8, "f32"), (8, 2, 0)), ((16385, 520, 4, 16, "f32"), (8, 1, 0))]
# (n, A, B, R) -> (G, rows of the last group): 9000 = 1800 groups of 5 is not ragged, 9001 leaves a last group of one row
CONTRIB_ODD_G = [((9000, 16, 16, 10), (5, 5)), ((9001, 16, 16, 10), (5, 1))]
