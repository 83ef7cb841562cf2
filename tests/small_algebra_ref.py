"""NumPy restatements, input generators, bounds and case tables for the small f64 kernels of csrc/small.hip, csrc/solve.hip,
csrc/rank1_tensor.hip (kron) and the calcR2X pass of csrc/recon.hip.  No GPU and no torch here: tests/test_small_algebra_ref_cpu.py
checks this module on the CPU, tests/test_gpu_small_algebra_limits.py runs the kernels against it.  `fold_normal_solve` restates
the fold kernels' serial solve (csrc/fold_regress.hpp) operation by operation; tests/test_fold_regress_cpu.py compares the two.

Every restatement takes the arguments of the `HipBackend` method of the same name (as NumPy arrays, views included),
accumulates in `np.longdouble` (64-bit significand) and returns the value together with the magnitude sum of the same
expression, sum |terms|.

Two input forms
---------------
*Exact inputs*: integers uniform in -8 ... 8.  Every product and every partial sum of every operation below is then an integer
below 2^53 (`EXACT_LIMITS` lists the largest for the case tables), so any summation order, with or without fma contraction,
returns the same bits: the device result has to be EQUAL to the restatement.  This catches an element dropped, duplicated or
read from the wrong place without any tolerance.  normalize, colscale and scores_mean divide: there the comparison is with
NumPy doing the same correctly rounded operations in the same order on an exact sum.

*Rounding inputs*: magnitudes uniform in [0.5, 1.5] with random signs, so no term of a sum is negligible next to the others.

The bound
---------
u = 2^-53.  A sum of n products formed in float64 in ANY order, each product fused into its addition or not, satisfies
|computed - exact| <= gamma_n * sum|terms|, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, Lemma 3.1 / 8.4: every
term passes through at most n roundings).  n is the number of TERMS, not the depth of the kernel's tree -- the tree is shorter,
so the bound holds whatever the kernel's order is.  `REF_SLACK` = 1 + 2^-10 covers the restatement's own longdouble
error (n 2^-64 sum|terms| = 2^-11 of the bound).

Two-level results compose the same bound (all first-order terms and the squares are kept, nothing is fitted):

* `du2` of rowdot, du2 = sum_i d_i^2, d_i = u_old_i - u_i.  |uhat_i - u_i| <= bu_i = gamma_M sum_m |Y_im q_m|.  The subtraction
  rounds once: |dhat_i - d_i| <= ed_i = bu_i + u (|d_i| + bu_i).  Replacing d by dhat changes the sum by at most
  sum_i (2 |d_i| ed_i + ed_i^2); summing the I squares of dhat costs gamma_I sum_i (|d_i| + ed_i)^2.  The bound is their sum.
* `ssq` of y_deflate, ssq = sum_im v_im^2, v_im = Y_im - s_i q_m, s_i = T_i . b.  |shat_i - s_i| <= bs_i = gamma_R sum|T_ir b_r|;
  v is formed as fl(Y - fl(shat q)) or as one fma, either way
  |vhat - v| <= ev = bs |q| + u |Y| + (2u + u^2)(|s| + bs)|q|.   (ev is also the bound of Y in place.)
  Then as for du2 with n = I M squares: sum(2 |v| ev + ev^2) + gamma_IM sum(|v| + ev)^2.
* `G *= L^T L` of kr_gram: Ghat = fl(fl(G s) acchat), acc = sum_j L_jr L_js with |acchat - acc| <= ba = gamma_n sum|L_jr L_js|,
  and G itself known to within eg (0 when G is given, the first call's bound when two modes are chained):
  |Ghat - G s acc| <= (|G| + eg)|s| ba (1 + 2u) + (2u + u^2)(|G| + eg)|s||acc| + eg |s||acc|.
  `first` is the same with G = 1, eg = 0.
* recon_r2: xhat_ic = sum_r T_ir (WA_jr WB_kr) has R terms of two products each: |xhathat - xhat| <= gamma_(R+1) sum|T WA WB|;
  xc = x - mean rounds once (not at all without a mean); d = xhat - xc rounds once more.  res = sum d^2 and ssq = sum xc^2 over
  the finite entries are then composed as du2 is, with n = I P squares.

The discrimination condition
----------------------------
The rounding inputs can only expose a dropped term when one term is far above the bound.  With term magnitudes in [lo, hi] a
sum of n terms has min term / bound >= lo / (gamma_n n hi): `term_margin`.  The generators keep every SQUARE of a two-level
sum away from zero as well (u_old, Y and X are built around the exact first-level value plus a rounding input), so the same
closed form covers them.  tests/test_small_algebra_ref_cpu.py asserts a margin >= 1000 for every shape of the tables below;
where n terms do not give it the case carries `chain`, the longest chain of roundings a term really passes in the kernel
(rows per thread x width + the levels of its trees), stated next to the case, and the bound uses that length instead.
"""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
REF_SLACK = 1.0 + 2.0 ** -10
LO, HI = 0.5, 1.5


def gamma(n):
    return n * U / (1.0 - n * U)


def bound_sum(n, mag):
    """|error| of a float64 sum of n products in any order, fma or not, given sum|terms| (see the module docstring)."""
    return gamma(n) * np.asarray(mag, dtype=np.float64) * REF_SLACK


def bound_two_level(val, err, n):
    """sum of n squares of values known to within `err`: sum(2|v| e + e^2) + gamma_n sum(|v| + e)^2."""
    v, e = np.abs(np.asarray(val, dtype=np.float64)), np.asarray(err, dtype=np.float64)
    return (float(np.sum(2.0 * v * e + e * e)) + gamma(n) * float(np.sum((v + e) ** 2))) * REF_SLACK


def term_margin(chain, n_terms, lo, hi):
    """min |term| / bound for a sum of n_terms terms of magnitude in [lo, hi] bounded with chain length `chain`."""
    return lo / (gamma(chain) * n_terms * hi)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def exact_inputs(rng, *shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


def rounding_inputs(rng, *shape):
    return rng.uniform(LO, HI, size=shape) * rng.choice([-1.0, 1.0], size=shape)


def inputs(kind, rng, *shape):
    return exact_inputs(rng, *shape) if kind == "exact" else rounding_inputs(rng, *shape)


def away_from(kind, rng, centre):
    """`centre` plus an input of the same kind, rounded to float64: the difference from `centre` is then an integer (exact form)
    or of magnitude in [0.5, 1.5] up to one rounding (rounding form) -- the squares of a two-level sum stay away from zero."""
    c = np.asarray(centre, dtype=LD)
    step = inputs(kind, rng, *c.shape)
    if kind == "exact":
        step[step == 0] = 1.0
    return (c + step).astype(np.float64)


# ---- restatements: (value, sum |terms|) ----------------------------------------------------------------------------------
def _2d(A):
    A = np.asarray(A)
    return A.reshape(A.shape[0], 1) if A.ndim == 1 else A


def gram_tn(A, B):
    """C = A^T B; n = rows."""
    A, B = _2d(A), _2d(B)
    return A.astype(LD).T @ B.astype(LD), np.abs(A).T @ np.abs(B)


def rowdot(Y, q, u_old=None):
    """u = Y q (n = M) and, with u_old, du2 = sum (u_old - u)^2.  Returns (u, mag_u, du2 or None)."""
    u = Y.astype(LD) @ q.astype(LD)
    mag = np.abs(Y) @ np.abs(q)
    if u_old is None:
        return u, mag, None
    d = u_old.astype(LD) - u
    return u, mag, np.sum(d * d)


def bound_du2(Y, q, u_old):
    u, mag, _ = rowdot(Y, q, u_old)
    d = np.abs((u_old.astype(LD) - u).astype(np.float64))
    bu = bound_sum(Y.shape[1], mag)
    ed = bu + U * (d + bu)
    return bound_two_level(d, ed, Y.shape[0])


def y_deflate(Y, T, ncols, b, q):
    """Ynew = Y - (T[:, :ncols] b) q^T and ssq = |Ynew|_F^2.  Returns (Ynew, err_Y, ssq): err_Y is the elementwise bound `ev`."""
    s = T[:, :ncols].astype(LD) @ b[:ncols].astype(LD)
    smag = np.abs(T[:, :ncols]) @ np.abs(b[:ncols])
    V = Y.astype(LD) - np.outer(s, q.astype(LD))
    bs = bound_sum(ncols, smag)[:, None]
    aq = np.abs(q)[None, :]
    s_abs = np.abs(s.astype(np.float64))[:, None]
    ev = (bs * aq + U * np.abs(Y) + (2 * U + U * U) * (s_abs + bs) * aq) * REF_SLACK
    return V, ev, np.sum(V * V)


def bound_ssq(V, ev, chain=None):
    return bound_two_level(V.astype(np.float64), ev, chain or V.size)


def total(v):
    return math.fsum(v.tolist()), math.fsum(np.abs(v).tolist())


def normalize(v):
    """(v / |v|, |v|, relative bound of |v|, relative bound of an entry of v / |v|).  The float64 path is sum of squares ->
    correctly rounded sqrt -> correctly rounded division; sqrt(1 + t) <= 1 + |t|, so |v| carries gamma_n + u and an entry one
    more division: gamma_n + 2u, with second order 1.01."""
    nrm = np.sqrt(LD(np.sum(v.astype(LD) ** 2)))
    rel = (gamma(v.size) + U) * 1.01 * REF_SLACK
    return v.astype(LD) / nrm, nrm, rel, rel + 1.01 * U


def normalize_f64(v):
    """The exact form: the sum of squares is an exact integer, so float64 sqrt and division give the kernel's bits."""
    ssq = np.float64(math.fsum((v * v).tolist()))
    nrm = np.sqrt(ssq)
    return v / nrm, nrm


def scores_mean(Ts):
    """out = (sum_b Ts[b]) / nb; n = nb terms, then one division."""
    nb = Ts.shape[0]
    return np.sum(Ts.astype(LD), axis=0) / LD(nb), np.sum(np.abs(Ts), axis=0) / nb


def scores_mean_f64(Ts):
    """The kernel's operations in its order in float64: ((t0 + t1) + t2 ...) / nb."""
    s = Ts[0].copy()
    for b in range(1, Ts.shape[0]):
        s = s + Ts[b]
    return s / np.float64(Ts.shape[0])


def bound_scores_mean(Ts):
    val, mag = scores_mean(Ts)
    return bound_sum(Ts.shape[0], mag) * (1 + U) + U * np.abs(val.astype(np.float64)) * REF_SLACK


def axpy_scalar(y, a, x=None):
    """y - a[0] x (x = None: ones): two terms, fused or not."""
    ax = LD(a[0]) * (np.ones_like(y) if x is None else x).astype(LD)
    return y.astype(LD) - ax, np.abs(y) + np.abs(ax.astype(np.float64))


def colscale(Z, cnt, n_samples):
    """float64, the kernel's order: (z / cnt) * n where cnt > 0, else 0.  Correctly rounded operations: compared for equality."""
    out = np.zeros_like(Z)
    pos = cnt > 0
    out[pos] = Z[pos] / cnt[pos] * np.float64(n_samples)
    return out


def kr_gram(L, G, first, scale=1.0, G_err=0.0):
    """G_out = (first ? 1 : G) * scale * L^T L.  Returns (value, bound) with the composition of the module docstring."""
    acc = L.astype(LD).T @ L.astype(LD)
    amag = np.abs(L).T @ np.abs(L)
    R = L.shape[1]
    g = np.ones((R, R)) if first else np.asarray(G, dtype=np.float64).reshape(R, R)
    eg = 0.0 if first else G_err
    val = g.astype(LD) * LD(scale) * acc
    ba = bound_sum(L.shape[0], amag)
    ga, sa, aa = np.abs(g) + eg, abs(scale), np.abs(acc.astype(np.float64))
    bound = (ga * sa * ba * (1 + 2 * U) + (2 * U + U * U) * ga * sa * aa + eg * sa * aa) * REF_SLACK
    return val, bound


def kr_gram_row(L, a, g, first):
    """g[:a] (*)= L[:, :a]^T L[:, a]; entries at and past a untouched.  Returns (value of g[:a], bound)."""
    acc = L[:, :a].astype(LD).T @ L[:, a].astype(LD)
    amag = np.abs(L[:, :a]).T @ np.abs(L[:, a])
    g0 = np.ones(a) if first else np.asarray(g, dtype=np.float64)[:a]
    ba = bound_sum(L.shape[0], amag)
    bound = (np.abs(g0) * ba * (1 + U) + U * np.abs(g0) * np.abs(acc.astype(np.float64))) * REF_SLACK
    return g0.astype(LD) * acc, bound


def khatri_rao(Am, Bm):
    """out[(j nb + k), r] = Am[j, r] Bm[k, r]: one product per element, compared for equality."""
    return (Am[:, None, :] * Bm[None, :, :]).reshape(Am.shape[0] * Bm.shape[0], Am.shape[1])


def kron(a, b):
    return (a[:, None] * b[None, :]).reshape(-1)


def fold_normal_solve(G, g):
    """csrc/fold_regress.hpp's fold_normal_solve in plain Python floats, one correctly rounded operation per operator and in the
    header's order (no fused multiply-add): the header compiled for the host without contraction gives the same bits
    (tests/test_fold_regress_cpu.py).  Returns (b, dropped columns)."""
    k = len(g)
    A = [[float(G[i][j]) for j in range(k)] for i in range(k)]
    tiny = float(k) * 2.220446049250313e-16
    d = [1.0 / math.sqrt(A[i][i]) if A[i][i] > 0.0 and math.isfinite(A[i][i]) else 0.0 for i in range(k)]
    b = [0.0] * k
    for i in range(k):
        for j in range(k):
            A[i][j] = A[i][j] * (d[i] * d[j])
        b[i] = float(g[i]) * d[i]
    dropped = []
    for c in range(k):
        piv = A[c][c]
        if not piv > tiny:
            dropped.append(c)
            A[c][c] = 1.0
            for i in range(c + 1, k):
                A[i][c] = 0.0
            continue
        l = math.sqrt(piv)
        A[c][c] = l
        for i in range(c + 1, k):
            A[i][c] = A[i][c] / l
        for i in range(c + 1, k):
            for j in range(c + 1, i + 1):
                A[i][j] = A[i][j] - A[i][c] * A[j][c]
    for r in range(k):
        s = b[r]
        for j in range(r):
            s = s - A[r][j] * b[j]
        b[r] = 0.0 if r in dropped else s / A[r][r]
    for r in range(k - 1, -1, -1):
        s = b[r]
        for j in range(r + 1, k):
            s = s - A[j][r] * b[j]
        b[r] = 0.0 if r in dropped else s / A[r][r]
    return np.array([b[r] * d[r] for r in range(k)]), dropped


def recon(T, WA, WB, mean):
    """Xhat = T (WA (.) WB)^T + mean and its magnitude sum |T| |W|^T + |mean| (the bound is test_recon_matches_float64's)."""
    R = T.shape[1]
    W = (WA[:, None, :] * WB[None, :, :]).reshape(-1, R)
    mu = np.zeros(W.shape[0]) if mean is None else mean
    return T @ W.T + mu, np.abs(T) @ np.abs(W).T + np.abs(mu)


def recon_r2(X2, T, WA, WB, mean, chain=None):
    """[sum (xhat - xc)^2, sum xc^2] over the finite entries of xc = X2 - mean, X2 the STORED values (float32 widened).
    Returns (value (2,), bound (2,))."""
    I, P = X2.shape
    R = T.shape[1]
    W = (WA.astype(LD)[:, None, :] * WB.astype(LD)[None, :, :]).reshape(P, R)
    xhat = T.astype(LD) @ W.T
    hmag = np.abs(T) @ np.abs(W.astype(np.float64)).T
    mu = np.zeros(P) if mean is None else mean
    xc = X2.astype(LD) - mu.astype(LD)[None, :]
    fin = np.isfinite(xc)
    xc0 = np.where(fin, xc, 0)
    d = np.where(fin, xhat - xc0, 0)
    xa, da = np.abs(xc0.astype(np.float64)), np.abs(d.astype(np.float64))
    exc = np.where(fin, 0.0 if mean is None else U * xa, 0.0)
    ed = np.where(fin, bound_sum(R + 1, hmag) + exc + U * (da + bound_sum(R + 1, hmag) + exc), 0.0)
    n = chain or I * P
    val = np.array([np.sum(d * d), np.sum(xc0 * xc0)], dtype=LD)
    return val, np.array([bound_two_level(da, ed, n), bound_two_level(xa, exc, n)])


def recon_r2_plan(I, P, V):
    """(col_tiles, row_blocks, rows per block) of recon_r2_plan in csrc/recon.hip (256 lanes of V columns per tile)."""
    col_tiles = max(1, -(-(-(-P // V)) // 256))
    want = -(-2048 // col_tiles)
    rpb = max(8, -(-I // want))
    return col_tiles, -(-I // rpb), rpb


def recon_r2_inputs(kind, rng, I, A, B, R, np_dtype, mean, ldt_extra=0, nan_fraction=0.0):
    """(X stored values as float64, T (I, R + ldt_extra), WA, WB, mean).  Exact form: T = 0 and integer X, mean: both sums are the
    integer sum of squares.  Rounding form: scores scaled by 1 / (4R) so |xhat| <= 0.85, centred entries of magnitude in
    [1.5, 2.5]: |d| in [0.65, 3.35] and |xc| in [1.5, 2.5], no square near zero.  NaN entries include the last column of the last
    tile and the last row."""
    P = A * B
    WA, WB = inputs(kind, rng, A, R), inputs(kind, rng, B, R)
    mu = inputs(kind, rng, P) if mean else None
    if kind == "exact":
        T = np.zeros((I, R + ldt_extra))
        xc = exact_inputs(rng, I, P)
    else:
        T = rounding_inputs(rng, I, R + ldt_extra) / (4.0 * R)
        xc = rounding_inputs(rng, I, P)
        xc += np.sign(xc)
    X = (xc + (mu if mean else 0.0)).astype(np_dtype).astype(np.float64)
    if nan_fraction:
        X[rng.random(X.shape) < nan_fraction] = np.nan
        X[-1, -1] = np.nan
        X[-1, 0] = np.nan
        X[0, -1] = np.nan
    return X, T, WA, WB, mu


RECON_R2_TERMS = (0.65 ** 2, 3.35 ** 2)     # [lo, hi] of d^2; xc^2 lies in [2.25, 6.25], inside the same ratio


# ---- case tables (shared by the CPU check of the discrimination condition and the GPU tests) ---------------------------------
GEMV_I = [1, 255, 257, 32767, 32768, 32769, 70001]        # 128 workgroups x 256 rows = 32768 rows per grid round
GEMV_A = [1, 15, 16, 17, 33, 64, 200]                     # one pass of 16, a partial pass, several passes
# every width at the short lengths; the long ones (operands of tens of MB) take the widths around one pass, and 200 once
GEMV_CASES = [(I, a) for I in GEMV_I[:3] for a in GEMV_A] + [(I, a) for I in GEMV_I[3:] for a in (1, 16, 17, 64)] + \
             [(32769, 200), (70001, 15), (70001, 33)]

TILED_AB = [(2, 2), (16, 16), (17, 16), (32, 32), (33, 32), (64, 64), (65, 2), (2, 65), (65, 65), (130, 70), (129, 128)]
TILED_I = [1, 5, 127, 128, 129, 128 * 130 + 5]            # workgroups without rows; a last stage shorter than TR
TILED_WIDTH = 136                                         # every operand is a column range of one (I, 136) matrix


def tiled_columns(a, b):
    """Column offsets of A and B in the shared matrix: distinct offsets so that a wrong tile offset reads other values."""
    return min(3, TILED_WIDTH - a), min(5, TILED_WIDTH - b)


ROWDOT_CASES = [(I, M) for M in (1, 16, 64, 200) for I in (1, 257, 32769)] + [(I, 16) for I in (255, 32767, 32768, 70001)]

# (I, M, R, chain): ssq is a sum of I M squares in [0.25, 2.25]; chain = None means n = I M terms
Y_DEFLATE_CASES = [(I, M, R, None) for (M, R) in ((1, 1), (16, 7), (64, 16), (3, 70)) for I in (1, 257)] + \
                  [(I, 16, 7, None) for I in (32767, 32768, 32769)] + \
                  [(70001, 1, 1, None), (70001, 3, 70, None),
                   # 64 responses past one grid round: 2.1 M squares leave a margin of 470 with n = I M.  A square passes at most
                   # 2 rows x 64 fma in its thread, 6 + 4 levels of the workgroup sum, then 1 + 6 + 16 of the closing sum kernel
                   (32769, 64, 16, 2 * 64 + 6 + 4 + 1 + 6 + 16)]

SUM_N = [1, 63, 1024, 1025, 50001]
NORMALIZE_N = [1, 600, 1024, 1025, 9000]
SCORES_MEAN_CASES = [(nb, I) for nb in (1, 2, 3, 5) for I in (1, 255, 257, 100003)]
AXPY_N = [1, 256, 257, 262144, 262145, 600001]            # 1024 workgroups x 256 = 262144 elements per grid round
COLSCALE_P = [1, 256, 257, 5000]
KR_GRAM_CASES = [(1, 1), (9, 7), (128, 16), (130, 17), (40, 64), (5, 70)]
KR_GRAM_ROW_CASES = [(n, R, a) for n in (1, 15, 16, 17, 33, 128) for R in (2, 10, 64) for a in sorted({0, 1, R - 1})] + [(33, 301, 300)]
KR_SIZES = [(1, 1), (7, 9), (1, 300), (300, 1), (128, 128)]
KR_R = [1, 7, 64]

# (storage, A, B, I, chain): two and more column tiles (256 lanes of V columns) with a partly dead last tile
RECON_R2_SHAPES = [("f64", 5, 130, I, None) for I in (1, 7, 8, 9)] + [("f64", 1, 1030, 9, None), ("f32", 9, 132, 9, None),
                                                                     ("f32", 8, 520, 9, None), ("f32", 8, 520, 1, None)]
# f64 5 x 130, I = 8300: V = 2 -> 325 lanes = 2 column tiles, 1024 row blocks wanted -> 9 rows per block, 923 row blocks, the last
# with 2 rows.  5.4 M squares: n = I P leaves a margin below 1; a square passes 9 rows x 2 fma in its thread, 6 + 4 levels of the
# workgroup sum, then ceil(1846 / 8) + 8 additions in reduce_rows
RECON_R2_RAGGED = ("f64", 5, 130, 8300, 9 * 2 + 6 + 4 + 231 + 8)
RECON_R2_R = [1, 4, 5, 8, 9, 12, 13, 16]

# largest integer any exact-input case forms (all below 2^53 = 9.0e15)
EXACT_LIMITS = {
    "gram_tn": 70001 * 64,
    "rowdot": 200 * 64 + 8,                   # u, and u_old = u + a step: the differences are the steps, du2 <= 64 I
    "y_deflate": 70 * 64 * 8 + 8,             # (T b) q, and Y = (T b) q^T + a step: v is the step, ssq <= 64 I M
    "kr_gram two modes": 4 * (130 * 64) ** 2,
    "recon_r2": 8300 * 650 * 16 ** 2,
}
