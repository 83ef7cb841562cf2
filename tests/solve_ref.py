"""Long-double restatements, derived bounds, input builders and case tables for the two solves of csrc/solve.hip:
`normal_solve` (normal_solve_kernel for k <= 64, normal_solve_big_kernel for 64 < k <= 1024) and `unit_upper_solve_rows`.
No GPU and no torch here: tests/test_solve_ref_cpu.py checks this module on the CPU, tests/test_gpu_solve_limits.py runs the
kernels against it.  `U`, `gamma`, `LD` and `REF_SLACK` are those of tests/small_algebra_ref.py.

normal_solve: the algorithm
---------------------------
d_i = 1 / sqrt(G_ii), or 0 where G_ii is not positive and finite; A^ = D G D, y^ = D g; column Cholesky of A^ in which a column
whose pivot, as it is seen after the updates of the kept columns before it, is not above tiny = k 2^-52 (`!(piv > tiny)`: zero,
negative and NaN pivots included) is DROPPED: diagonal 1, zero sub-column, no update from it, coefficient 0; then L z = y^,
L^T x = z with x_c = 0 forced for a dropped c; b = D x.  The products with a dropped column's zeros are formed, not skipped
(0 * NaN = NaN reaches the same entries as in the kernels).  `normal_solve` below does this in np.longdouble, left-looking
(column c = A^[c:, c] - L[c:, :c] L[c, :c]: the same sums as the kernels' right-looking updates, vectorised).

normal_solve: the backward-error bound
--------------------------------------
u = 2^-53, K = the kept columns, n = |K|.  No term below depends on the conditioning of G: a forward error would, which is why
the tests assert the residual of the equilibrated system.  Quantities with a tilde are the device's.

* d~_i = fl(1 / fl(sqrt G_ii)) = d_i (1 + e2) / (1 + e1), |e1|, |e2| <= u (both operations are correctly rounded: the library
  is built without fast-math): two rounding factors per d~.
* A~_ij = fl(fl(G_ij d~_i) d~_j) (the two device kernels) or fl(G_ij fl(d~_i d~_j)) (the one-thread form): two products, so
  A~_ij = A^_ij (1 + alpha_ij) with 2 + 2 + 2 = 6 factors, |alpha_ij| <= gamma_6.  y~_i = fl(g_i d~_i) = y^_i (1 + beta_i),
  3 factors, |beta_i| <= gamma_3.
* A dropped column takes no part in any update (its sub-column is zero) and its row of L only ever multiplies its own zero
  coefficient, so the kept columns see exactly the Cholesky factorisation and the two triangular solves of A~_KK.  Higham,
  Accuracy and Stability of Numerical Algorithms, Thm 10.3: R^T R = A~_KK + dA1, |dA1| <= gamma_(n+1) |R^T||R|; Thm 10.4:
  the computed x~ solves (A~_KK + dA) x~ = y~_K, |dA| <= gamma_(3n+1) |R^T||R| (any order of the sums; a fused multiply-add
  removes a rounding and only tightens both).  By Cauchy-Schwarz (|R^T||R|)_ij <= |r_i||r_j|, and |r_i|^2 = (R^T R)_ii <=
  a~_ii + gamma_(n+1) |r_i|^2, so  |dA_ij| <= gamma_(3n+1) / (1 - gamma_(n+1)) sqrt(a~_ii a~_jj)
                                             <= gamma_(3n+1) / (1 - gamma_(n+1)) (1 + gamma_6) sqrt(A^_ii A^_jj).
* b~_i = fl(x~_i d~_i).  The test forms x^_i = b~_i / d_i in long double: x^_i = x~_i (1 + 3 factors), x~_i = x^_i (1 + eta_i),
  |eta_i| <= gamma_3.
* Substituting into sum_j (A~_ij + dA_ij) x~_j = y~_i, the residual r = A^_KK x^_K - y^_K of the restatement's system is
      r_i = - sum_j A^_ij x^_j ((1 + alpha_ij)(1 + eta_j) - 1) - sum_j dA_ij (1 + eta_j) x^_j + y^_i beta_i
  |r_i| <= gamma_9 sum_j |A^_ij||x^_j|
           + (1 + gamma_3)(1 + gamma_6) gamma_(3n+1) / (1 - gamma_(n+1)) sqrt(A^_ii) sum_j sqrt(A^_jj) |x^_j|  + gamma_3 |y^_i|.
  Times REF_SLACK for the long-double evaluation of A^, y^ and r (k 2^-64 of the same magnitude sums).  Underflow is excluded:
  the builders keep every entry of G above 1e-30 in magnitude or exactly zero.
`normal_solve_bound` returns (|r|, that bound) on K; a dropped column's coefficient is asserted to be exactly 0 separately.

Which inputs take part in drop-set assertions
---------------------------------------------
The three forms round the equilibration differently -- (G d_i) d_j against G (d_i d_j) -- and their update sums in different
orders, so a pivot within rounding of tiny may legitimately be kept by one and dropped by another.  The builders therefore
assert (`assert_pivot_margins`), in long double, that every pivot of the restatement is >= 1024 tiny, or else exactly 0, NaN or
<= tiny / 1024 (negative included); pivots are of order 1 after equilibration and the forms differ by a few n u, so 1024 tiny
= 2048 k u is far outside what rounding can move.  Three kinds of dropped column are built:
* a zero column: d = 0, its row and column of A^ are exactly 0 in every form;
* (exact inputs) a power-of-two multiple of an earlier column: A^_cs = 1 and the pivot 1 - 1 * 1 = 0 exactly in every form;
* (rounding inputs) a `shrunk` column: G_cc multiplied by 2^-6 after the Gram matrix is formed, so that A^_cj is 8 x the
  cosine between the columns and the pivot 1 - 64 x (the fraction of the column explained by the kept columns before it) is
  below -1 (asserted), negative in every form.  G is then indefinite, G_KK is still a Gram matrix, and -- unlike a zero or a
  dependent column, whose updated sub-column is 0 or of order sqrt(u) -- the sub-column that the drop rule has to zero holds
  entries of order 1.  A column dependent to rounding on earlier ones (a multiple that is no power of two, or of rounded
  data) has a pivot of a few u, next to tiny for small k: such columns stay with tests/test_gpu_round2.py and _round3.py.

Exact inputs (`exact_normal`)
-----------------------------
Score columns are columns of the Sylvester Hadamard matrix of order I (256 or 1024), column j scaled by 2^e_j: G = diag(I 4^e)
exactly, d_j = 2^-e_j / sqrt(I) is a power of two, A^ is the identity, y^ = g d and b = g d^2 are exact scalings of the
integers in g (u holds integers in -8 ... 8, so |T^T u| 2^-e <= 8 I).  With duplicated columns every entry of A^ and of L is 0
or 1 and every sum the solves form is an integer of that size times a power of two: any order of operations returns the same
bits, and the device result has to EQUAL the restatement.

unit_upper_solve_rows
---------------------
t_a = (m_a - shift_a) - sum_{j<a} t_j U[j, a], one row per thread, in this order (the kernel's loop is serial and the
compiler may not reassociate).  m_a passes the subtraction of the shift and a subtractions of products, a + 1 roundings;
product j rounds once (not at all when fused) and passes the a - j subtractions after it: at most a + 1 roundings as well.
With err_j = |t~_j - t_j| the products use t~_j, |t~_j| <= |t_j| + err_j:
      err_a <= gamma_(a+1) (|m_a| + |shift_a| + sum_j (|t_j| + err_j) |U[j, a]|) + sum_j err_j |U[j, a]|
a running componentwise bound, times REF_SLACK.  Exact inputs (`exact_upper`): integers with at most one non-zero per column
of triu(U, 1); the builder asserts that every product and every partial difference stays below 2^53, so the device result
equals the restatement.  Rounding inputs: magnitudes in [0.5, 1.5] with random signs, U scaled by 1 / sqrt(R) so that the
scores stay of order 1 at R = 64.
"""
import functools

import numpy as np

from small_algebra_ref import LD, REF_SLACK, U, gamma, rounding_inputs

EPS = 2.220446049250313e-16                  # the kernels' literal: tiny = k * EPS
MAX_K_LDS, MAX_K = 64, 1024                  # kSolveMax, kSolveBigMax
MAX_R = 64
SHRINK = 2.0 ** -6


# ---- normal_solve: restatement ----------------------------------------------------------------------------------------------------
class NormalRef:
    """b (long double), dropped (list), pivots (as seen, long double), Ahat, yhat, d (long double), kept (index array)."""

    def __init__(self, b, dropped, pivots, Ahat, yhat, d):
        self.b, self.dropped, self.pivots, self.Ahat, self.yhat, self.d = b, dropped, pivots, Ahat, yhat, d
        self.kept = np.array([c for c in range(len(b)) if c not in set(dropped)], dtype=np.int64)
        self.k = len(b)


def equilibrate(G, g):
    G = np.asarray(G, dtype=np.float64)
    k = G.shape[0]
    g = np.asarray(g, dtype=np.float64).reshape(k)
    diag = np.diagonal(G)
    ok = (diag > 0.0) & np.isfinite(diag)
    d = np.zeros(k, dtype=LD)
    d[ok] = LD(1) / np.sqrt(diag[ok].astype(LD))
    with np.errstate(invalid="ignore", over="ignore"):
        Ahat = G.astype(LD) * d[:, None] * d[None, :]
        yhat = g.astype(LD) * d
    return Ahat, yhat, d


def factor(Ahat, tiny, update_diagonal=True, leave_dropped=None):
    """Column Cholesky with the drop rule; returns (L, dropped, pivots).  The two options are the perturbations of
    tests/test_solve_ref_cpu.py, never used by a reference: `update_diagonal=False` is the update loop run to j < i;
    `leave_dropped=c` leaves the dropped column c as it stands below its diagonal of 1, so that it enters the later columns'
    updates as a kept column would."""
    k = Ahat.shape[0]
    L = np.zeros((k, k), dtype=LD)
    dropped, pivots = [], np.zeros(k, dtype=LD)
    finite = bool(np.isfinite(Ahat).all())
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(k):
            col = Ahat[c:, c].copy()
            if c and not (finite and not L[c, :c].any()):    # finite data, an all-zero row of L (exact inputs): exact zeros
                upd = L[c:, :c] @ L[c, :c]
                if not update_diagonal:
                    upd[0] = 0
                col -= upd
            piv = col[0]
            pivots[c] = piv
            if not piv > tiny:
                dropped.append(c)
                if leave_dropped != c:
                    col[:] = 0
                col[0] = 1
            else:
                l = np.sqrt(piv)
                col[1:] /= l
                col[0] = l
            L[c:, c] = col
    return L, dropped, pivots


def solve_factored(L, dropped, yhat, d):
    k = L.shape[0]
    dep = np.zeros(k, dtype=bool)
    dep[dropped] = True
    y = yhat.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(k):
            s = y[r] - (L[r, :r] @ y[:r] if r else 0)
            y[r] = 0 if dep[r] else s / L[r, r]
        for r in range(k - 1, -1, -1):
            s = y[r] - (L[r + 1:, r] @ y[r + 1:] if r + 1 < k else 0)
            y[r] = 0 if dep[r] else s / L[r, r]
        return y * d


def normal_solve(G, g, **perturb):
    Ahat, yhat, d = equilibrate(G, g)
    k = Ahat.shape[0]
    L, dropped, pivots = factor(Ahat, LD(k) * LD(EPS), **perturb)
    return NormalRef(solve_factored(L, dropped, yhat, d), dropped, pivots, Ahat, yhat, d)


def normal_solve_bound(ref, b_hat):
    """(|r|, bound) on the kept columns for a device result b_hat (float64, length k): r = Ahat_KK xhat_K - yhat_K, xhat = b_hat / d."""
    K = ref.kept
    n = len(K)
    if n == 0:
        return np.zeros(0), np.ones(0)
    xh = np.asarray(b_hat, dtype=np.float64)[K].astype(LD) / ref.d[K]
    A = ref.Ahat[np.ix_(K, K)]
    r = np.abs(A @ xh - ref.yhat[K]).astype(np.float64)
    ax = np.abs(xh).astype(np.float64)
    Aa = np.abs(A).astype(np.float64)
    sq = np.sqrt(np.diagonal(Aa))
    chol = (1 + gamma(3)) * (1 + gamma(6)) * gamma(3 * n + 1) / (1 - gamma(n + 1))
    bound = gamma(9) * (Aa @ ax) + chol * sq * float(sq @ ax) + gamma(3) * np.abs(ref.yhat[K]).astype(np.float64)
    return r, bound * REF_SLACK


def assert_pivot_margins(ref):
    tiny = LD(ref.k) * LD(EPS)
    p = ref.pivots
    with np.errstate(invalid="ignore"):
        ok = (p >= 1024 * tiny) | (p == 0) | np.isnan(p) | (p <= tiny / 1024)
    assert bool(ok.all()), ("pivot next to the threshold", np.flatnonzero(~ok)[:4], p[~ok][:4])


# ---- normal_solve: builders ---------------------------------------------------------------------------------------------------------
BOUNDARY_LOW = (0, 64, 255, 512, 767)        # one side of 64, 256, 512, 768 (and column 0) ...
BOUNDARY_HIGH = (63, 256, 511, 768)          # ... and the other side


def special_columns(k, variant):
    """(zero columns, {copy: source}) of the exact variants "plain", "zeros", "dups", "both".  "zeros" and "dups" put their kind
    at 0 (zeros only), k - 1 and on both sides of 64, 256, 512 and 768 as far as k allows; "both" puts a zero column on one side of
    each and a copy on the other.  A copy's source lies 261 columns before it -- in an earlier 256-row pass of the workspace
    form -- where that is an ordinary column, else it is the first ordinary column not yet used."""
    low = [p for p in BOUNDARY_LOW if p < k]
    high = sorted({p for p in BOUNDARY_HIGH + (k - 1,) if 0 < p < k} - set(low))
    if variant == "plain":
        return (), {}
    if variant == "zeros":
        return tuple(sorted(set(low) | set(high) | {k - 1})), {}
    zeros = tuple(low) if variant == "both" else ()
    copies = high if variant == "both" else sorted((set(low) | set(high)) - {0})
    taken, dups = set(zeros) | set(copies), {}
    for c in copies:
        s = c - 261
        if s < 1 or s in taken:
            s = next((j for j in list(range(1, c)) + [0] if j not in taken and j < c), None)
        if s is None:
            continue                                          # k = 2 with a zero column 0: nothing left to copy
        dups[c] = s
        taken.add(s)
    return zeros, dups


def hadamard_columns(I, k):
    """The first k columns of the Sylvester Hadamard matrix of order I: (-1)^popcount(i & j)."""
    i, j = np.arange(I, dtype=np.int64)[:, None], np.arange(k, dtype=np.int64)[None, :]
    v = i & j
    par = np.zeros_like(v)
    while v.any():
        par ^= v & 1
        v = v >> 1
    return 1.0 - 2.0 * par


def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def exact_normal(k, I, variant="plain"):
    """(G, g, ref): Hadamard scores scaled by powers of two (see the module docstring); zero and duplicated columns by `variant`."""
    assert I in (256, 1024) and k <= I
    rng = np.random.default_rng([11, k, I])
    zeros, dups = special_columns(k, variant)
    T = hadamard_columns(I, k) * 2.0 ** rng.integers(-6, 7, size=k)[None, :]
    for c, s in dups.items():
        T[:, c] = T[:, s] * 2.0 ** int(rng.integers(-3, 4))
    T[:, list(zeros)] = 0.0
    u = rng.integers(-8, 9, size=I).astype(np.float64)
    G, g = T.T @ T, T.T @ u
    ref = normal_solve(G, g)
    assert ref.dropped == sorted(set(zeros) | set(dups)), (ref.dropped, zeros, dups)
    return _readonly(G, g) + (ref,)


def rounding_zero_columns(k):
    return tuple(sorted({p for p in BOUNDARY_LOW if p < k} | ({k - 1} if k >= 4 else set())))


def rounding_shrunk_column(k):
    return (k // 2 + 1,) if k >= 8 else ()


@functools.lru_cache(maxsize=None)
def rounding_normal(k, seed=0, spread=None, zero=(), shrunk=()):
    """(G, g, ref): Gaussian scores with 3 k rows, column scales over `spread` decades (12 for k <= 64, 6 above) and a common
    component in every column, as in tests/test_gpu_round2.py and _round3.py; `zero` columns set to 0; the diagonal of the
    `shrunk` columns multiplied by 2^-6 (module docstring).  Asserts the pivot margins and that exactly zero + shrunk are dropped."""
    spread = (12 if k <= 64 else 6) if spread is None else spread
    rng = np.random.default_rng([13, k, seed])
    I = 3 * k
    scale = np.logspace(0, -spread, k)
    T = rng.normal(size=(I, k)) * scale[None, :]
    T[:, 1:] += 0.3 * T[:, :1] * scale[None, 1:]
    T[:, list(zero)] = 0.0
    u = rng.normal(size=I)
    G, g = T.T @ T, T.T @ u
    for c in shrunk:
        G[c, c] *= SHRINK
    assert float(np.abs(G[G != 0]).min(initial=1.0)) > 1e-30
    ref = normal_solve(G, g)
    assert_pivot_margins(ref)
    assert ref.dropped == sorted(set(zero) | set(shrunk)), (ref.dropped, zero, shrunk)
    assert all(ref.pivots[c] < -1 for c in shrunk)
    return _readonly(G, g) + (ref,)


def rounding_case(k, variant):
    """The rounding inputs of the GPU file: "plain", or "deficient" = zero columns at 0, k - 1 and one side of 64 ... 768, and one
    shrunk column past the middle (k >= 8)."""
    if variant == "plain":
        return rounding_normal(k)
    return rounding_normal(k, zero=rounding_zero_columns(k), shrunk=rounding_shrunk_column(k))


def embed(G, g, pos, k_big, diag=0.0):
    """The k_big system that holds (G, g) at the columns `pos`; the other columns are zero (or `diag` on the diagonal and in g)."""
    Gb, gb = np.zeros((k_big, k_big)), np.zeros(k_big)
    if diag:
        Gb[np.arange(k_big), np.arange(k_big)] = diag
        gb[:] = diag
    Gb[np.ix_(pos, pos)] = G
    gb[pos] = g
    return Gb, gb


NONFINITE_G = np.array([[1.0, np.nan], [np.nan, np.inf]])       # the case of tests/test_fold_regress_cpu.py
NONFINITE_g = np.array([1.0, 1.0])
NONFINITE_EMBED = (260, (70, 200), 4.0)                          # k, the two columns, the other columns' diagonal and g

BOTH_FORMS = (48, 300, tuple(5 + 6 * i for i in range(48)))      # a 48-column problem at columns 5, 11, ..., 287 of 300


# ---- unit_upper_solve_rows ------------------------------------------------------------------------------------------------------------
def unit_upper_solve_rows(M, Um, shift=None):
    """(T, err): rows of T solve T (I + triu(Um, 1)) = M - 1 shift^T in long double; err is the running componentwise bound of the
    module docstring for the float64 kernel.  The diagonal and the lower triangle of Um are never read."""
    M = np.asarray(M, dtype=np.float64)
    I, R = M.shape
    sh = np.zeros(R) if shift is None else np.asarray(shift, dtype=np.float64).reshape(R)
    Tt = np.zeros((R, I), dtype=LD)                            # transposed: the sums run over contiguous rows
    At, err = np.zeros((R, I)), np.zeros((R, I))               # |t| and its bound
    for a in range(R):
        ua = np.asarray(Um[:a, a], dtype=np.float64)
        au = np.abs(ua)
        acc, mag, prop = LD(0), 0.0, 0.0
        nz = np.flatnonzero(ua)
        if len(nz) > 4:
            acc, mag, prop = ua.astype(LD) @ Tt[:a], au @ (At[:a] + err[:a]), au @ err[:a]
        else:
            for j in nz:
                acc = acc + Tt[j] * LD(ua[j])
                mag = mag + (At[j] + err[j]) * au[j]
                prop = prop + err[j] * au[j]
        Tt[a] = (M[:, a].astype(LD) - LD(sh[a])) - acc
        At[a] = np.abs(Tt[a]).astype(np.float64)
        err[a] = (gamma(a + 1) * (np.abs(M[:, a]) + abs(sh[a]) + mag) + prop) * REF_SLACK
    T, err = np.ascontiguousarray(Tt.T), np.ascontiguousarray(err.T)
    return T, err


@functools.lru_cache(maxsize=None)
def exact_upper(I, R):
    """(M, Um, shift): integers, at most one non-zero (of magnitude 1 or 2) per column of triu(Um, 1), garbage below.  Asserts that
    every product and partial difference of the substitution stays below 2^53."""
    rng = np.random.default_rng([17, I, R])
    M = rng.integers(-8, 9, size=(I, R)).astype(np.float64)
    shift = rng.integers(-8, 9, size=R).astype(np.float64)
    Um = np.tril(rng.integers(-8, 9, size=(R, R))).astype(np.float64)
    for a in range(1, R):
        Um[rng.integers(0, a), a] = float(rng.choice([-2, -1, 1, 2]))
    assert int((np.triu(Um, 1) != 0).sum(axis=0).max(initial=0)) <= 1
    for sh in (shift, None):                                   # the tests run with and without the shift
        T, _ = unit_upper_solve_rows(M, Um, sh)
        col_max = np.abs(T).max(axis=0).astype(np.float64)
        largest = max(float(col_max.max()), float(np.abs(M).max() + np.abs(shift).max()), float((col_max[:, None] * np.abs(np.triu(Um, 1))).max()))
        assert largest < 2.0 ** 53, largest
    return _readonly(M, Um, shift)


@functools.lru_cache(maxsize=None)
def rounding_upper(I, R):
    rng = np.random.default_rng([19, I, R])
    M, shift = rounding_inputs(rng, I, R), rounding_inputs(rng, R)
    Um = rounding_inputs(rng, R, R) / np.sqrt(R)
    return _readonly(M, Um, shift)


def upper_inputs(kind, I, R):
    return exact_upper(I, R) if kind == "exact" else rounding_upper(I, R)


# ---- case tables (shared by the CPU check of the builder conditions and the GPU tests) ----------------------------------------------
NORMAL_K_LDS = [1, 2, 3, 63, 64]
NORMAL_K_WS = [65, 255, 256, 257, 511, 513, 768, 1024]     # 255 / 256 / 257, 511 / 513, 768, 1024: one to four passes of the row loop
NORMAL_K = NORMAL_K_LDS + NORMAL_K_WS
EXACT_VARIANTS = ["plain", "zeros", "dups", "both"]
ROUNDING_VARIANTS = ["plain", "deficient"]
ABI_COLUMN_CASES = [(8, 4), (72, 69)]                       # (R, a): k = a + 1 through the LDS form and through the workspace form


def exact_rows(k):
    return 256 if k <= 256 else 1024


UPPER_R = [1, 2, 7, 63, 64]
UPPER_I = [1, 255, 256, 257, 70001]
UPPER_CASES = [(257, R) for R in UPPER_R] + [(I, 64) for I in UPPER_I if I != 257]
UPPER_NAN_ROWS = {I: sorted({0, min(255, I - 1), I - 1}) for I in UPPER_I}   # row 0, the first block's last row, the last block's
