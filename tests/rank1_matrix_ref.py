"""Host side of the matrix rank-1 extraction tests (csrc/rank1.hip): NumPy float64 / longdouble only.

`model` restates the algorithm of the kernels -- Gram matrix of the smaller side, repeated squaring with a power-of-two scale
from the trace, the two thresholds on rho = |G|_F^2 / tr(G)^2, the seed row, one pass with Z, the sign rule -- WITHOUT claiming
bit parity with the device (the matrix cores add in another order).  It says which exit a case takes and how many squarings,
and `margin` says how far every step's 1 - rho stayed from either threshold, so that a case whose count could flip with
rounding is rejected on the CPU (tests/test_rank1_matrix_ref_cpu.py) before it reaches a GPU.  `exact_case` builds inputs whose
arithmetic is exact in every squaring (a permuted diagonal of powers of two): their outputs are known in advance.

The case lists of tests/test_gpu_rank1_matrix_limits.py live here, so that the CPU module screens exactly what the GPU runs.
"""
import numpy as np

TILE = 16
MAX_STEPS = 48            # kMaxSteps: the budget is clamped to it
CHAIN_MAX_STEPS = 31      # kChainMaxSteps: the largest budget the one-launch chain takes
T_IN = 1e-13              # rho >= 1 - T_IN: the step's input is the result ("rank_one_in")
T_OUT = 1e-7              # rho >= 1 - T_OUT: the step's output is the result ("rank_one_out")
MIN_MARGIN = 5.0          # a case asserts `info` only when margin(...) >= MIN_MARGIN
EPS = 2.0 ** -53


def clamp_budget(budget):
    return max(1, min(int(budget), MAX_STEPS))


def model(Z, budget):
    """(wA, wB, sigma, converged, steps, [1 - rho of every step's input]) of the extraction of Z (A x B) within `budget` squarings."""
    Z = np.asarray(Z, dtype=np.float64)
    A, B = Z.shape
    x_is_A = A <= B
    M = Z if x_is_A else Z.T                               # n x k, n the smaller side
    G0 = M @ M.T
    G, converged, steps, gaps = G0, False, 0, []
    with np.errstate(all="ignore"):
        for step in range(1, clamp_budget(budget) + 1):
            tr = float(np.trace(G))
            fro = float(np.sum(G * G))
            if not tr > 0.0:                               # (a zero Z: the input "is" the result, the loadings are 0 / 0)
                converged = True
                break
            rho = fro / (tr * tr)
            trl = np.longdouble(tr)
            gaps.append(float((trl * trl - np.sum(G.astype(np.longdouble) ** 2)) / (trl * trl)))
            if rho >= 1.0 - T_IN:
                converged = True
                break
            steps = step
            scale = np.ldexp(1.0, -int(np.frexp(tr)[1])) if np.isfinite(tr) else 1.0
            Gs = G * scale
            G = Gs @ Gs.T
            if rho >= 1.0 - T_OUT:
                converged = True
                break
        bi = int(np.argmax(np.diag(G)))                    # first index on ties
        seed = G[bi] / np.sqrt(np.sum(G[bi] * G[bi]))
        y = M.T @ seed
        x = G0 @ seed
        nx, ny = np.sqrt(np.sum(x * x)), np.sqrt(np.sum(y * y))
        x, y = x / nx, y / ny
        wA, wB = (x, y) if x_is_A else (y, x)
        if wB[int(np.argmax(np.abs(wB)))] < 0.0:           # the last mode's largest-|.| entry is positive
            wA, wB = -wA, -wB
        sigma = nx / ny
    return wA, wB, float(sigma), converged, steps, gaps


def margin(one_minus_rhos):
    """The smallest factor between any step's 1 - rho and either threshold (inf when no step came near: an exact 0 counts as far)."""
    best = np.inf
    for g in one_minus_rhos:
        g = abs(float(g))
        if g == 0.0:
            continue
        for t in (T_IN, T_OUT):
            best = min(best, max(g / t, t / g))
    return best


def residual(Z, wA, wB):
    """max(|Z wB - s wA|, |Z^T wA - s wB|) / s with s = wA^T Z wB, in np.longdouble."""
    Zl = np.asarray(Z, dtype=np.longdouble)
    a, b = np.asarray(wA, dtype=np.longdouble), np.asarray(wB, dtype=np.longdouble)
    s = a @ Zl @ b
    ra = Zl @ b - s * a
    rb = Zl.T @ a - s * b
    return float(max(np.sqrt(ra @ ra), np.sqrt(rb @ rb)) / s)


def residual_bound(Z, sigma1):
    """(n + k + 8) 2^-53 |Z|_F^2 / sigma1^2: the rounding of y = M^T seed (n terms) and of x = fl(M M^T) seed (k + n terms) relative
    to |x| ~ sigma1^2; plus 1e-13 sqrt(n): the off-direction share the 1 - 1e-13 threshold lets through (lambda2 / lambda1 <= 5e-14),
    taken twice for the rounding of rho itself, times sqrt(n) because the seed row has u1[i]^2 >= 1 / n."""
    A, B = Z.shape
    n, k = min(A, B), max(A, B)
    return (n + k + 8) * EPS * float(np.sum(np.asarray(Z, dtype=np.longdouble) ** 2)) / sigma1 ** 2 + 1e-13 * np.sqrt(n)


def sigma_bound(A, B, sigma1):
    return 8 * EPS * (A + B) * sigma1


def svd_pair(Z):
    """LAPACK's leading pair with the project's sign rule, and the singular values."""
    U, S, Vt = np.linalg.svd(Z, full_matrices=False)
    u, v = U[:, 0], Vt[0]
    if v[int(np.argmax(np.abs(v)))] < 0:
        u, v = -u, -v
    return u, v, S


def workspace_bytes(A, B):
    """cmtfpls_rank1_workspace_bytes restated: control block (64 bytes + (50 nt + 2 nt^2) doubles), three n x n buffers, Z^T, x,
    y, each rounded up to 256 bytes; then 32 x (n^2 + nt + nt^2) + 1 doubles of the one-launch chain where nt^2 <= 256."""
    up = lambda v: (v + 255) // 256 * 256
    n, k = min(A, B), max(A, B)
    nt = (n + TILE - 1) // TILE
    chain = up(((CHAIN_MAX_STEPS + 1) * (n * n + nt + nt * nt) + 1) * 8) if nt * nt <= 256 else 0
    return up(64 + ((MAX_STEPS + 2) * nt + 2 * nt * nt) * 8) + 3 * up(n * n * 8) + up(A * B * 8) + up(n * 8) + up(k * 8) + chain


# ---- family 1 / 2: a permuted diagonal of powers of two ----------------------------------------------------------------------------
def _spread(side, first, count):
    """`count` distinct indices below `side`: `first`, then the others spread over the whole side (so that tail chunks and the
    last tile hold entries too)."""
    rest = [v for v in range(side) if v not in first]
    m = count - len(first)
    return list(first) + [rest[(t * len(rest)) // m] for t in range(m)]


def exact_case(A, B, i, j, sign=1, tie=None):
    """Z[p(r), q(r)] = +-2^-r for r < min(A, B), zero elsewhere, p(0) = i, q(0) = j and the dominant entry `sign`; with tie =
    (i2, j2) the magnitudes are 1, 1, 1/2, 1/4, ... and the second 1 sits at (i2, j2).  Every product and sum of every squaring
    is exact (or underflows to the same zero everywhere), G stays a permuted diagonal, and the outputs are unit vectors:
    returns dict(Z, wA, wB, sigma).  With a tie the seed is the FIRST largest diagonal entry of the smaller side's Gram matrix."""
    n = min(A, B)
    lead = [(i, j)] if tie is None else [(i, j), tuple(tie)]
    assert len(lead) <= n and len({p for p, _ in lead}) == len(lead) and len({q for _, q in lead}) == len(lead)
    p = _spread(A, [a for a, _ in lead], n)
    q = _spread(B, [b for _, b in lead], n)
    Z = np.zeros((A, B))
    for r in range(n):
        e = r if tie is None else max(r - 1, 0)
        s = sign if r == 0 else (1 if (tie is not None and r == 1) else (-1) ** r)
        Z[p[r], q[r]] = s * 2.0 ** -e
    win = 0
    if tie is not None:
        assert sign == 1
        side = 0 if A <= B else 1
        win = 0 if lead[0][side] < lead[1][side] else 1
    wA, wB = np.zeros(A), np.zeros(B)
    wA[lead[win][0]] = float(sign)
    wB[lead[win][1]] = 1.0
    return dict(Z=Z, wA=wA, wB=wB, sigma=1.0)


F1_SHAPES = [(17, 129), (129, 17), (33, 257), (255, 256), (256, 256), (257, 257), (257, 40), (1, 9), (9, 1), (1, 1), (2, 2)]
F1_BUDGET = 30


def family1_positions(A, B):
    rows = sorted({v for v in (0, 15, 16, 17, A - 1) if 0 <= v < A})
    cols = sorted({v for v in (0, 7, 8, 31, 32, 127, 128, 129, B - 1) if 0 <= v < B})
    return [(i, j, s) for i in rows for j in cols for s in (1, -1)]


F2_SHAPES = [(20, 24), (256, 256), (257, 257)]
F2_BUDGETS = [30, 31, 32, 48, 60]


def family2_ties(A, B):
    """(dominant position, tied position): once with the first entry winning the first-index rule, once with the second."""
    return [((1, B - 1), (A - 1, 0)), ((A - 1, 0), (1, B - 1))]


def uses_chain(A, B, budget):
    n = min(A, B)
    nt = (n + TILE - 1) // TILE
    return nt * nt <= 256 and clamp_budget(budget) <= CHAIN_MAX_STEPS


# ---- family 3: dense Z with a known spectrum ---------------------------------------------------------------------------------------
F3_SHAPES = F1_SHAPES + [(16, 128), (31, 127), (15, 33), (272, 300), (48, 513), (3, 1025)]
F3_RATIOS = [0.5, 0.93]
F3_BUDGET = 30
CLOSE_GAP = ((33, 129), 0.99999)


def dense_case(A, B, ratio, zero_lines=True, second=None):
    """Z = (U * s) V^T with orthonormal random U, V and s = ratio^i (second: s[1] instead), then -- as the chain test of
    test_gpu_kernels.py -- row A // 2 and column B // 3 set to zero where that side has at least four entries."""
    rng = np.random.default_rng(1000 * A + B)
    n = min(A, B)
    U, _ = np.linalg.qr(rng.normal(size=(A, n)))
    V, _ = np.linalg.qr(rng.normal(size=(B, n)))
    s = float(ratio) ** np.arange(n)
    if second is not None and n > 1:
        s[1] = second
    Z = (U * s) @ V.T
    if zero_lines and A >= 4:
        Z[A // 2, :] = 0.0
    if zero_lines and B >= 4:
        Z[:, B // 3] = 0.0
    return np.ascontiguousarray(Z)


def close_gap_case():
    (A, B), r = CLOSE_GAP
    return dense_case(A, B, 0.5, zero_lines=False, second=r)


# family 3 cases whose step count sits within MIN_MARGIN of a threshold: `info` is not asserted there (the CPU module holds that
# these, and only these, are the cases below the margin)
F3_INFO_NOT_ASSERTED = {(17, 129, 0.93), (48, 513, 0.93)}      # margins 4.0 and 1.7


def family3_cases():
    return [(A, B, r) for (A, B) in F3_SHAPES for r in F3_RATIOS]


# ---- the exits, each on its own (family 2, second half) ----------------------------------------------------------------------------
EXIT_SHAPE = (40, 56)


def exit_cases():
    """(name, Z, budget, expected info).  rank_one_in: Z exactly rank one (small integers: G_0 is exact), taken at step 1 with no
    squaring counted, at an even and an odd budget; rank_one_out: the 0.5^i spectrum declares step 5 final, at budgets 5 and 6;
    budget out: the same Z at 3 and 4."""
    A, B = EXIT_SHAPE
    rng = np.random.default_rng(7)
    one = np.outer(rng.integers(1, 9, size=A), rng.integers(-8, 9, size=B)).astype(np.float64)
    Zd = dense_case(A, B, 0.5, zero_lines=False)
    return [("rank_one_in", one, 6, (1, 0)), ("rank_one_in", one, 7, (1, 0)),
            ("rank_one_out", Zd, 5, (1, 5)), ("rank_one_out", Zd, 6, (1, 5)),
            ("budget_out", Zd, 3, (0, 3)), ("budget_out", Zd, 4, (0, 4))]


# ---- family 4 ----------------------------------------------------------------------------------------------------------------------
SCALE_SHAPES = [(17, 129), (257, 40)]
SCALE_EXPONENTS = [-100, -20, 20, 100]
VIEW_SHAPES = [(33, 257), (257, 40)]
# (A, B, M, S offset in doubles): either side of M = 64, of P = 8192, odd A (padded LDS split), odd B, either side of the 60 KB
# LDS gate ((A + 1) & ~1) + B <= 7680, the larger side first, S 8 bytes off a 16-byte boundary
SCORE_CASES = [(64, 128, 64, 0), (64, 128, 65, 0), (64, 128, 3, 0), (63, 130, 3, 0), (65, 128, 4, 0), (128, 65, 4, 0),
               (2, 7678, 3, 0), (2, 7680, 3, 0), (256, 64, 5, 0), (64, 128, 3, 1)]


def score_is_fused(A, B, M, s_off):
    return M <= 64 and A * B >= 8192 and B % 2 == 0 and ((A + 1) & ~1) + B <= 7680 and s_off % 2 == 0


def tq_bound(S, wA, wB):
    """(P + 2) 2^-53 |S_row|^T |w| per row: P products and P - 1 additions of the row, and the rounding of w = wA (x) wB itself."""
    w = np.abs(np.kron(wA, wB))
    return (S.shape[1] + 2) * EPS * (np.abs(S) @ w)
