"""cmtfpls_loo_xcov_coupled_f64 (csrc/loo_xcov_coupled.hip: leave-one-out refits of a ctPLS, a 1024-thread workgroup per fold on the
cross-covariances of the fold's blocks) in plain NumPy float64 (TEST INFRASTRUCTURE): a mirror of the entry's shape rules, the
literal leave-one-out of validate.py:24-33 over the oracle's primitives, the same refits re-associated the way the kernel's header
describes (the yardstick of two correct float64 evaluations), and the case tables shared by tests/test_loo_coupled_ref_cpu.py (which
proves the input conditions without a GPU), tests/test_gpu_loo_coupled_kernel.py and tests/test_gpu_loo_coupled.py.  The
references of a case are computed once per process and are read-only.

The mirror is written from the kernel's header comment and the limits it lists, not by calling the library.  A block is given by its
trailing shape: (J,) a matrix block (A = 1, B = J), (J, K) an order-3 block (A = J, B = K); P_b = A_b B_b.
  limits     at most 8 blocks, order 2 or 3, min(A_b, B_b) <= 256, M <= 128, R <= 64, P_b <= 2^24, the workgroup's small vectors
             within 150 KB of dynamic LDS -- checked in this order, the first that fails is the reason;
  LDS        every block's wA_b (A_b) and wB_b (B_b), q, qn, tq, my (M each), G_y (M x M), xs (nmax), ys (kmax), coef (R x R),
             Qs (R x M), the normal equations Gn (R x R), gn, bb, dd (R each), nmax = max_b min(A_b, B_b), kmax = max_b max(A_b, B_b):
             sum A_b + sum B_b + 4 M + M^2 + nmax + kmax + 2 R^2 + R M + 3 R doubles;
  workspace  per resident fold (I + M) sumP + 3 Pmax + 2 nmax^2 + I (M + R + 2) + R (sum A_b + sum B_b) doubles.
With one block both formulas are loo_xcov_ref's."""
import functools

import numpy as np

import oracle as O
from loo_xcov_ref import CAP_ITER, CAP_TOL, EXCLUDED_CAP, MAX_ITER, TOL, normwise, on_threshold  # noqa: F401  (shared yardsticks)

MAX_BLOCKS, MAX_N, MAX_M, MAX_R = 8, 256, 128, 64
LDS_CAP = 150 * 1024
MAX_CELLS = 1 << 24


def split(trail):
    """(A, B) of a block's trailing shape."""
    return (1, trail[0]) if len(trail) == 1 else (trail[0], trail[1])


def lds_doubles(dims, M: int, R: int) -> int:
    ab = [split(d) for d in dims]
    return (sum(A + B for A, B in ab) + 4 * M + M * M + max(min(A, B) for A, B in ab) + max(max(A, B) for A, B in ab)
            + 2 * R * R + R * M + 3 * R)


def loo_coupled_form(I: int, dims, M: int, R: int):
    """(form, None), or (None, why) when the entry declines with status 4: why is "blocks", "order", "n", "M", "R", "cells" or "lds".
    dims: the trailing shape of every block.  form: the LDS and workspace bytes of one fold and what its launch looks like."""
    if len(dims) > MAX_BLOCKS:
        return None, "blocks"
    if any(len(d) > 2 for d in dims):
        return None, "order"
    ab = [split(d) for d in dims]
    if any(min(A, B) > MAX_N for A, B in ab):
        return None, "n"
    if M > MAX_M:
        return None, "M"
    if R > MAX_R:
        return None, "R"
    if any(A * B > MAX_CELLS for A, B in ab):
        return None, "cells"
    lds = 8 * lds_doubles(dims, M, R)
    if lds > LDS_CAP:
        return None, "lds"
    sumP, Pmax = sum(A * B for A, B in ab), max(A * B for A, B in ab)
    nmax, kmax = max(min(A, B) for A, B in ab), max(max(A, B) for A, B in ab)
    ws = 8 * ((I + M) * sumP + 3 * Pmax + 2 * nmax * nmax + I * (M + R + 2) + R * sum(A + B for A, B in ab))
    return {"lds_bytes": lds, "ws_bytes_per_fold": ws, "blocks": len(dims), "nmax": nmax, "kmax": kmax, "tiles": -(-nmax // 16),
            "transposed": [A > B for A, B in ab], "orders": [len(d) + 1 for d in dims], "over_48k": lds > 48 * 1024,
            "m_groups": -(-M // 16)}, None


def longest_row(others, M: int, R: int) -> int:
    """The largest J of a matrix block (J,) the LDS rule admits next to the blocks `others` with M responses and R components."""
    J = 1
    while 8 * lds_doubles(list(others) + [(J + 1,)], M, R) <= LDS_CAP:
        J += 1
    return J


# ---- the refits ------------------------------------------------------------------------------------------------------------------
def _outer(vecs):
    out = np.asarray(vecs[0]).ravel()
    for v in vecs[1:]:
        out = np.multiply.outer(out, np.asarray(v).ravel())
    return out


def _kron(vecs):
    return functools.reduce(np.kron, [np.asarray(v).ravel() for v in vecs])


def _refit(xts, yt, R, tol, max_iter, on_s):
    """oracle.fit_ctpls's loop on complete data (nipals_oracle._nipals with coupled=True, cmtf.py:85-139) operation for operation,
    keeping what it does not expose: the convergence norm |u_old - u| of every component's last pass and of the pass before it (inf on
    a first pass, cmtf.py:89).  on_s: the inner loop re-associated as loo_xcov_coupled.hip's header states it -- S_b = Y^T X_b of
    every block and G_y = Y^T Y once per component, Z_b = S_b^T q, Y^T t = (1 / nb) sum_b S_b (w_b1 (x) w_b2) in list order,
    |u_old - u|^2 = dq^T G_y dq, from q = e_0, no stop on the first pass."""
    Xs = [np.array(x, dtype=float) for x in xts]
    n = Xs[0].shape[0]
    Y2 = np.array(yt, dtype=float).reshape(n, -1)
    M = Y2.shape[1]
    nb = len(Xs)
    x_means, y_mean = [np.nanmean(X, axis=0) for X in Xs], np.nanmean(Y2, axis=0)
    work, Yc = [X - m for X, m in zip(Xs, x_means)], Y2 - y_mean
    fit = O.OracleFit(coupled=True, n_components=R, block_shapes=[X.shape for X in Xs], y_shape=Y2.shape, T=np.zeros((n, R)),
                      loadings=[[np.zeros((d, R)) for d in X.shape[1:]] for X in Xs], U=np.zeros((n, R)), Q=np.zeros((M, R)),
                      coef=np.zeros((R, R)), r2x=[np.zeros(R) for _ in Xs], r2y=np.zeros(R), x_means=x_means, y_mean=y_mean,
                      has_miss=[False] * nb)
    du_last, du_prev = np.full(R, np.inf), np.full(R, np.inf)
    for a in range(R):
        executed, du = 0, np.inf
        if on_s:
            S = [np.tensordot(Yc, X, axes=(0, 0)) for X in work]
            Gy = Yc.T @ Yc
            q = np.zeros(M)
            q[0] = 1.0
            for it in range(max_iter):
                executed += 1
                ws = [O.rank1_factors(np.tensordot(q, Sb, axes=(0, 0)), tol) for Sb in S]
                tq = np.zeros(M)
                for Sb, w in zip(S, ws):
                    tq = tq + Sb.reshape(M, -1) @ _kron(w)
                tq = tq / nb
                qn = tq / np.linalg.norm(tq)
                dq = qn - q
                du_prev[a], du = du, float(np.sqrt(max(dq @ Gy @ dq, 0.0))) if it > 0 else np.inf
                q = qn
                if it > 0 and du < tol:
                    break
            for b, w in enumerate(ws):
                for m, f in enumerate(w):
                    fit.loadings[b][m][:, a] = np.asarray(f).ravel()
            fit.T[:, a] = np.average([O.score_contract(X, w) for X, w in zip(work, ws)], axis=0)
            fit.Q[:, a] = q
            fit.U[:, a] = Yc @ q
        else:
            old_u = np.full(n, np.inf)
            fit.U[:, a] = Yc[:, 0]
            for _ in range(max_iter):
                executed += 1
                per_block = []
                for b, X in enumerate(work):
                    Z = O.mode0_contract(X, fit.U[:, a])
                    for m, f in enumerate(O.rank1_factors(Z, tol)):
                        fit.loadings[b][m][:, a] = np.asarray(f).ravel()
                    per_block.append(O.score_contract(X, [L[:, a] for L in fit.loadings[b]]))
                fit.T[:, a] = np.average(per_block, axis=0)
                q = Yc.T @ fit.T[:, a]
                q = q / np.linalg.norm(q)
                fit.Q[:, a] = q
                fit.U[:, a] = Yc @ q
                du_prev[a], du = du, float(np.linalg.norm(old_u - fit.U[:, a]))
                if du < tol:
                    break
                old_u = fit.U[:, a].copy()
        du_last[a] = du
        fit.n_iter.append(executed)
        for b in range(nb):
            work[b] = work[b] - _outer([fit.T[:, a]] + [L[:, a] for L in fit.loadings[b]])
        fit.coef[:, a] = np.linalg.lstsq(fit.T, fit.U[:, a], rcond=-1)[0]
        Yc = Yc - fit.T @ fit.coef[:, [a]] @ fit.Q[:, [a]].T
    return fit, du_last, du_prev


def _loo(xs, y, R, tol, max_iter, folds, on_s):
    xs, y = [np.asarray(x, dtype=float) for x in xs], np.asarray(y, dtype=float)
    I = xs[0].shape[0]
    folds = list(range(I)) if folds is None else [int(f) for f in folds]
    M = y.reshape(I, -1).shape[1]
    out = {"folds": np.array(folds), "pred": np.empty((len(folds), M)), "n_iter": np.empty((len(folds), R), dtype=np.int64),
           "du_last": np.empty((len(folds), R)), "du_prev": np.empty((len(folds), R))}
    for j, i in enumerate(folds):
        keep = np.arange(I) != i
        fit, out["du_last"][j], out["du_prev"][j] = _refit([x[keep] for x in xs], y[keep], R, tol, max_iter, on_s)
        out["pred"][j] = np.asarray(O.predict(fit, [x[i:i + 1] for x in xs])).reshape(M)
        out["n_iter"][j] = fit.n_iter
    return out


def loo_literal(xs, y, R, tol=TOL, max_iter=MAX_ITER, folds=None):
    """The literal leave-one-out of validate.py:24-33 of a coupled model for the requested folds (default: all): oracle.fit_ctpls's
    loop on the other I - 1 samples of every block, oracle.predict of the held-out one.  {"folds", "pred" (F, M), "n_iter" (F, R)
    inner-loop passes, "du_last" (F, R) the norm |u_old - u| of the last pass, "du_prev" (F, R) that of the pass before it}."""
    return _loo(xs, y, R, tol, max_iter, folds, on_s=False)


def loo_on_s(xs, y, R, tol=TOL, max_iter=MAX_ITER, folds=None):
    """The same refits iterated on the S_b (the kernel's association)."""
    return _loo(xs, y, R, tol, max_iter, folds, on_s=True)


def condition_probe(xs, y, R, tol=TOL, max_iter=MAX_ITER, folds=None) -> float:
    """How far two correct float64 evaluations of the same folds drift apart: `normwise` of the predictions of the refits iterated
    on the S_b against loo_literal's."""
    return normwise(loo_on_s(xs, y, R, tol, max_iter, folds)["pred"], loo_literal(xs, y, R, tol, max_iter, folds)["pred"])


def q2y(pred, y) -> float:
    """validate.py:35-37."""
    y = np.asarray(y, dtype=float).reshape(np.asarray(pred).shape)
    return float(1 - ((pred - y) ** 2).sum() / (y ** 2).sum())


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (I, trailing shapes of the blocks, M, R, latent rank, noise, seed, folds compared ("all" or "three"), branch values of the form)
_ROW_OTHERS = [(3, 4)]
_J_STAR = longest_row(_ROW_OTHERS, 3, 2)
_EIGHT = ((3, 4), (5,)) * 4
BASIC_CASES = [
    (12, ((5, 7), (9,)), 3, 3, 2, 1e-10, 1, "all", dict(blocks=2, orders=[3, 2], nmax=5)),                     # mixed orders
    (10, ((17, 33), (33, 17), (40,)), 2, 2, 3, 0.3, 0, "all",                                                  # a tile edge past 16, both transposes
     dict(blocks=3, nmax=17, tiles=2, transposed=[False, True, False])),
    (9, _EIGHT, 1, 2, 3, 0.3, 3, "all", dict(blocks=8, m_groups=1)),                                           # the block limit, the M = 1 loop
]
LIMIT_CASES = [
    (8, ((256, 256), (40,)), 2, 2, 3, 0.3, 11, "three", dict(nmax=256, kmax=256, tiles=16)),                   # min(A, B) at its maximum next to a matrix
    (12, ((5, 7), (9,)), 128, 3, 2, 1e-10, 0, "three", dict(m_groups=8, over_48k=True)),                       # M at its maximum
    (70, ((8, 9), (12,)), 2, 64, 4, 1e-10, 1, "three", dict(over_48k=True, nmax=8)),                           # R at its maximum: scv, dep full, Cholesky at kk = 64
    (10, ((3, 4), (_J_STAR,)), 3, 2, 3, 0.3, 37, "three", dict(kmax=_J_STAR, over_48k=True)),                  # the longest matrix row the LDS admits
]
MATCH_CASES = BASIC_CASES + LIMIT_CASES
RANGE_CASE, RANGE = BASIC_CASES[0], (3, 4)                     # fold0 = 3, nfolds = 4 into a sentinel-filled Ypred

# limit -> ((I, dims, M, R) one step inside, one step past)
_LDS_IN = (4, ((141, 256),), 128, 10)                          # exactly 150 KB (one block: loo_xcov_ref's)
DECLINES = {
    "blocks": ((4, ((3,),) * 8, 2, 2), (4, ((3,),) * 9, 2, 2)),
    "n": ((4, ((256, 257), (5,)), 2, 2), (4, ((257, 257), (5,)), 2, 2)),
    "M": ((4, ((8, 8), (5,)), 128, 2), (4, ((8, 8), (5,)), 129, 2)),
    "R": ((4, ((8, 8), (5,)), 2, 64), (4, ((8, 8), (5,)), 2, 65)),
    "lds": (_LDS_IN, (4, ((141, 256), (1,)), 128, 10)),        # a second block of one column: wA_1, wB_1, 16 bytes past
}


def case_id(case) -> str:
    dims = "+".join("x".join(str(d) for d in t) for t in case[1]) if len(case[1]) < 8 else f"{len(case[1])}blocks"
    return f"I{case[0]}-{dims}-M{case[2]}-R{case[3]}"


def three_folds(I: int):
    return (0, I // 2, I - 1)


def case_folds(case):
    return tuple(range(case[0])) if case[7] == "all" else three_folds(case[0])


@functools.lru_cache(maxsize=None)
def case_data(I, dims, M, latent, noise, seed):
    """Blocks that share their sample-mode factor: block 0 and Y are oracle.import_synthetic's (its sample factor, Y = T Yf^T + noise);
    block b > 0 is that sample factor times fresh N(0, 1) mode factors plus N(0, noise), from default_rng(seed + 1000 b)."""
    x0, y, cp = O.import_synthetic((I,) + tuple(dims[0]), M, latent, error=noise, seed=seed)
    xs = [x0]
    for b, trail in enumerate(dims[1:], start=1):
        rng = np.random.default_rng(seed + 1000 * b)
        factors = [cp.factors[0]] + [rng.normal(0, 1, size=(d, latent)) for d in trail]
        xs.append(O.cp_factors_to_tensor(factors) + rng.normal(0, noise, size=(I,) + tuple(trail)))
    y = np.asarray(y).reshape(I, M)
    for a in xs + [y]:
        a.setflags(write=False)
    return tuple(xs), y


def _data(case):
    return case_data(case[0], case[1], case[2], *case[4:7])


@functools.lru_cache(maxsize=None)
def case_reference(case_key, tol, max_iter):
    """loo_literal of the case's compared folds; read-only."""
    case = _CASES[case_key]
    xs, y = _data(case)
    ref = loo_literal(xs, y, case[3], tol, max_iter, case_folds(case))
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def case_probe(case_key, tol, max_iter) -> float:
    case = _CASES[case_key]
    xs, y = _data(case)
    on_s = loo_on_s(xs, y, case[3], tol, max_iter, case_folds(case))
    return normwise(on_s["pred"], case_reference(case_key, tol, max_iter)["pred"])


_CASES = {case_id(c): c for c in MATCH_CASES}
assert len(_CASES) == len(MATCH_CASES)


def case_bound(case, tol, max_iter) -> float:
    """The normwise bound of a case's predictions: max(1e-8, 10 x condition_probe) (test_gpu_loo_xcov_limits's rule; the ten: the
    kernel's third summation order)."""
    return max(1e-8, 10.0 * case_probe(case_id(case), tol, max_iter))


def reference(case, tol, max_iter):
    return case_reference(case_id(case), tol, max_iter)
