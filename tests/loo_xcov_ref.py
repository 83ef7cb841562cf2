"""cmtfpls_loo_xcov_f64 (csrc/loo_xcov.hip: leave-one-out refits, a 1024-thread workgroup per fold on the fold's cross-covariance)
in plain NumPy float64 (TEST INFRASTRUCTURE): a mirror of the entry's shape rules, the literal leave-one-out of validate.py:24-33
over the oracle's primitives, the same refits re-associated the way the kernel's header describes (the yardstick of two correct
float64 evaluations), and the case tables shared by tests/test_loo_xcov_ref_cpu.py (which proves the input conditions without a
GPU) and tests/test_gpu_loo_xcov_limits.py.  The references of a case are computed once per process and are read-only.

The mirror is written from the kernel's header comment and the limits it lists, not by calling the library:
  limits     min(A, B) <= 256, M <= 128, R <= 64, the workgroup's small vectors within 150 KB of dynamic LDS, A B <= 2^24;
  LDS        wA (A), wB (B), q, qn, tq, my (M each), G_y (M x M), xs (n), ys (k), coef (R x R), Qs (R x M), the normal equations
             Gn (R x R), gn, bb, dd (R each), n = min(A, B), k = max(A, B): A + B + 4 M + M^2 + n + k + 2 R^2 + R M + 3 R doubles;
  workspace  per resident fold I P + M P + 3 P + 2 n^2 + I (M + R + 2) + R (A + B) doubles, P = A B.
The A B > 2^24 decline cannot be reached: with min(A, B) <= 256 it needs max(A, B) > 2^16, and then wA, wB, xs and ys alone are more
than 2 * 65536 doubles = 1 MiB of LDS, far past 150 KB, so the "lds" reason always comes first.  No test tries to reach it."""
import functools

import numpy as np

import oracle as O

MAX_N, MAX_M, MAX_R = 256, 128, 64
LDS_CAP = 150 * 1024
MAX_CELLS = 1 << 24
TOL, MAX_ITER = 1e-8, 100                    # get_q2y's
CAP_TOL, CAP_ITER = 0.0, 3                   # the run whose every component stops at the cap: |du| < 0 is never true
EXCLUDED_CAP = 0.10                          # share of (fold, component) pairs whose pass count may sit on the threshold


def lds_doubles(A: int, B: int, M: int, R: int) -> int:
    n, k = min(A, B), max(A, B)
    return A + B + 4 * M + M * M + n + k + 2 * R * R + R * M + 3 * R


def loo_xcov_form(I: int, A: int, B: int, M: int, R: int):
    """(form, None), or (None, why) when the entry declines the shape with status 4: why is "n", "M", "R" or "lds" ("elements" is
    unreachable, see the head of the file).  form: what the launch of one fold looks like."""
    n, k, P = min(A, B), max(A, B), A * B
    lds = 8 * lds_doubles(A, B, M, R)
    if n > MAX_N:
        return None, "n"
    if M > MAX_M:
        return None, "M"
    if R > MAX_R:
        return None, "R"
    if lds > LDS_CAP:
        return None, "lds"
    assert P <= MAX_CELLS
    ws = 8 * (I * P + M * P + 3 * P + 2 * n * n + I * (M + R + 2) + R * (A + B))
    return {"lds_bytes": lds, "ws_bytes_per_fold": ws, "n": n, "k": k, "transposed": A > B, "tiles": -(-n // 16),
            "over_48k": lds > 48 * 1024, "m_groups": -(-M // 16)}, None


def longest_row(M: int, R: int) -> int:
    """The largest B of a matrix block (A = 1) the LDS rule admits with M responses and R components."""
    B = 1
    while 8 * lds_doubles(1, B + 1, M, R) <= LDS_CAP:
        B += 1
    return B


def normwise(got, want) -> float:
    """test_gpu_round4.test_q2y_beyond_the_lds_shapes_equals_literal_refits's measure: max|got - want| / max(1, max|want|)."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


# ---- the refits ------------------------------------------------------------------------------------------------------------------
def _outer(vecs):
    out = np.asarray(vecs[0]).ravel()
    for v in vecs[1:]:
        out = np.multiply.outer(out, np.asarray(v).ravel())
    return out


def _kron(vecs):
    return functools.reduce(np.kron, [np.asarray(v).ravel() for v in vecs])


def _refit(xt, yt, R, tol, max_iter, on_s):
    """oracle.fit_tpls's loop on complete data (nipals_oracle._nipals, tpls.py:73-113) operation for operation, keeping what it does
    not expose: the convergence norm |u_old - u| of every component's last pass and of the pass before it (inf on a first pass,
    tpls.py:77).  on_s: the inner loop re-associated as loo_xcov.hip's header states it -- S = Y^T X and G_y = Y^T Y once per
    component, Z = S^T q, Y^T t = S (w_1 (x) w_2), |u_old - u|^2 = dq^T G_y dq, from q = e_0, no stop on the first pass."""
    X = np.array(xt, dtype=float)
    Y2 = np.array(yt, dtype=float).reshape(X.shape[0], -1)
    n, M = Y2.shape
    x_mean, y_mean = np.nanmean(X, axis=0), np.nanmean(Y2, axis=0)
    work, Yc = X - x_mean, Y2 - y_mean
    fit = O.OracleFit(coupled=False, n_components=R, block_shapes=[X.shape], y_shape=Y2.shape, T=np.zeros((n, R)),
                      loadings=[[np.zeros((d, R)) for d in X.shape[1:]]], U=np.zeros((n, R)), Q=np.zeros((M, R)), coef=np.zeros((R, R)),
                      r2x=[np.zeros(R)], r2y=np.zeros(R), x_means=[x_mean], y_mean=y_mean, has_miss=[False])
    du_last, du_prev = np.full(R, np.inf), np.full(R, np.inf)
    for a in range(R):
        executed, du = 0, np.inf
        if on_s:
            S = np.tensordot(Yc, work, axes=(0, 0))
            Gy = Yc.T @ Yc
            q = np.zeros(M)
            q[0] = 1.0
            for it in range(max_iter):
                executed += 1
                w = O.rank1_factors(np.tensordot(q, S, axes=(0, 0)), tol)
                tq = S.reshape(M, -1) @ _kron(w)
                qn = tq / np.linalg.norm(tq)
                dq = qn - q
                du_prev[a], du = du, float(np.sqrt(max(dq @ Gy @ dq, 0.0))) if it > 0 else np.inf
                q = qn
                if it > 0 and du < tol:
                    break
            for m, f in enumerate(w):
                fit.loadings[0][m][:, a] = f
            fit.T[:, a] = O.score_contract(work, w)
            fit.Q[:, a] = q
            fit.U[:, a] = Yc @ q
        else:
            old_u = np.full(n, np.inf)
            fit.U[:, a] = Yc[:, 0]
            for _ in range(max_iter):
                executed += 1
                Z = O.mode0_contract(work, fit.U[:, a])
                for m, f in enumerate(O.rank1_factors(Z, tol)):
                    fit.loadings[0][m][:, a] = np.asarray(f).ravel()
                vecs = [L[:, a] for L in fit.loadings[0]]
                fit.T[:, a] = O.score_contract(work, vecs)
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
        work = work - _outer([fit.T[:, a]] + [L[:, a] for L in fit.loadings[0]])
        fit.coef[:, a] = np.linalg.lstsq(fit.T, fit.U[:, a], rcond=-1)[0]
        Yc = Yc - fit.T @ fit.coef[:, [a]] @ fit.Q[:, [a]].T
    return fit, du_last, du_prev


def _loo(x, y, R, tol, max_iter, folds, on_s):
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    I = x.shape[0]
    folds = list(range(I)) if folds is None else [int(f) for f in folds]
    M = y.reshape(I, -1).shape[1]
    out = {"folds": np.array(folds), "pred": np.empty((len(folds), M)), "n_iter": np.empty((len(folds), R), dtype=np.int64),
           "du_last": np.empty((len(folds), R)), "du_prev": np.empty((len(folds), R))}
    for j, i in enumerate(folds):
        keep = np.arange(I) != i
        fit, out["du_last"][j], out["du_prev"][j] = _refit(x[keep], y[keep], R, tol, max_iter, on_s)
        out["pred"][j] = np.asarray(O.predict(fit, x[i:i + 1])).reshape(M)
        out["n_iter"][j] = fit.n_iter
    return out


def loo_literal(x, y, R, tol=TOL, max_iter=MAX_ITER, folds=None):
    """The literal leave-one-out of validate.py:24-33 for the requested folds (default: all): fit on the other I - 1 samples,
    predict the held-out one.  {"folds", "pred" (F, M), "n_iter" (F, R) inner-loop passes, "du_last" (F, R) the norm |u_old - u| of
    the last pass, "du_prev" (F, R) that of the pass before it}."""
    return _loo(x, y, R, tol, max_iter, folds, on_s=False)


def condition_probe(x, y, R, tol=TOL, max_iter=MAX_ITER, folds=None) -> float:
    """How far two correct float64 evaluations of the same folds drift apart: `normwise` of the predictions of the refits iterated
    on S (the kernel's association, _refit(on_s=True)) against loo_literal's."""
    return normwise(_loo(x, y, R, tol, max_iter, folds, on_s=True)["pred"], loo_literal(x, y, R, tol, max_iter, folds)["pred"])


def on_threshold(ref, tol) -> np.ndarray:
    """(F, R) bool: the pairs whose pass count is a decision that sat on the threshold -- the reference's convergence norm within
    [tol / 2, 2 tol] on the passing step or on the step before it."""
    near = lambda d: (d >= tol / 2) & (d <= 2 * tol)
    return near(ref["du_last"]) | near(ref["du_prev"])


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (shape, M, R, latent rank, noise, seed, the branch values the case is there for).  Inputs: oracle.import_synthetic with noise.
_B_STAR = longest_row(3, 2)
MATCH_CASES = [
    # lx_syrk's tile edges: 16 x 16 tiles of the n x n Gram, columns in 32-wide chunks
    ((8, 255, 256), 2, 2, 3, 0.3, 13, dict(n=255, k=256, tiles=16, transposed=False)),      # top tile row ragged, k whole chunks
    ((8, 256, 255), 2, 2, 3, 0.3, 13, dict(n=255, k=256, tiles=16, transposed=True)),       # the same through Zt
    ((8, 241, 300), 3, 2, 3, 0.3, 6, dict(n=241, k=300, tiles=16, transposed=False)),      # 16 tile rows, the last of ONE row; k % 32 = 12
    ((8, 256, 256), 2, 2, 3, 0.3, 11, dict(n=256, k=256, tiles=16, transposed=False)),      # the declared maximum of n
    ((12, 15, 40), 3, 3, 4, 0.3, 14, dict(n=15, tiles=1, transposed=False)),                # below one tile
    ((12, 16, 33), 3, 3, 4, 0.3, 4, dict(n=16, k=33, tiles=1, transposed=False)),          # exactly one tile, k one past a chunk
    ((12, 17, 33), 3, 3, 4, 0.3, 7, dict(n=17, tiles=2, transposed=False)),                # one row into the second tile row
    ((12, 33, 17), 3, 3, 4, 0.3, 17, dict(n=17, tiles=2, transposed=True)),                 # transposed, small n
    # the LDS budget and the response groups of the S build (16 responses per group, guarded by mc + j < M)
    ((12, 141, 256), 128, 10, 10, 1e-10, 1, dict(lds_bytes=LDS_CAP, over_48k=True, m_groups=8, n=141)),   # LDS exactly 150 KB, M at its maximum
    ((40, 20, 70), 127, 3, 4, 0.3, 2, dict(m_groups=8, over_48k=True)),                    # ragged last group: 15 of 16
    ((40, 20, 70), 17, 3, 4, 0.3, 154, dict(m_groups=2, over_48k=False)),                    # ragged last group: 1 of 16
    ((70, 8, 72), 2, 64, 4, 1e-10, 2, dict(over_48k=True, n=8, tiles=1)),                    # R at its maximum: scv, dep full, Cholesky at kk = 64
    ((10, _B_STAR), 3, 2, 3, 0.3, 37, dict(n=1, k=_B_STAR, tiles=1, over_48k=True)),        # matrix block, the longest row the LDS admits
    ((6, 64, 65), 2, 4, 5, 0.3, 284, dict(n=64, k=65, tiles=4)),                             # the first shape the lds form declines by n
]
PROBED = [c for c in MATCH_CASES if c[2] == MAX_R or c[1] >= 127]     # tolerance from condition_probe, not fixed in advance

# chunking, bounds, reproducibility: more folds than a chunk, a ragged tile row
CHUNK_CASES = [((24, 33, 40), 5, 3, 4, 0.3, 49, dict(n=33, tiles=3, transposed=False)),
               ((9, 255, 256), 2, 2, 3, 0.3, 1, dict(n=255, tiles=16, transposed=False))]

# limit -> ((I, A, B, M, R) one step inside, one step past)
DECLINES = {
    "n": ((4, 256, 257, 2, 2), (4, 257, 257, 2, 2)),
    "M": ((4, 8, 8, 128, 2), (4, 8, 8, 129, 2)),
    "R": ((4, 8, 8, 2, 64), (4, 8, 8, 2, 65)),
    "lds": ((4, 141, 256, 128, 10), (4, 141, 257, 128, 10)),           # exactly 150 KB; B one longer: wB and ys, 16 bytes past
}


def case_id(case) -> str:
    return f"{case[0]}-M{case[1]}-R{case[2]}"


def split(shape):
    return (1, shape[1]) if len(shape) == 2 else (shape[1], shape[2])


def three_folds(I: int):
    return (0, I // 2, I - 1)


@functools.lru_cache(maxsize=None)
def case_data(shape, M, latent, noise, seed):
    x, y, _ = O.import_synthetic(shape, M, latent, error=noise, seed=seed)
    for a in (x, y):
        a.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def case_reference(shape, M, R, latent, noise, seed, tol, max_iter):
    """loo_literal of the case's first, middle and last fold; read-only."""
    x, y = case_data(shape, M, latent, noise, seed)
    ref = loo_literal(x, y, R, tol, max_iter, three_folds(shape[0]))
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def case_probe(shape, M, R, latent, noise, seed, tol, max_iter) -> float:
    x, y = case_data(shape, M, latent, noise, seed)
    on_s = _loo(x, y, R, tol, max_iter, three_folds(shape[0]), on_s=True)
    return normwise(on_s["pred"], case_reference(shape, M, R, latent, noise, seed, tol, max_iter)["pred"])


def case_bound(case, tol, max_iter) -> float:
    """The normwise bound of a case's predictions: 1e-8 (what test_q2y_beyond_the_lds_shapes_equals_literal_refits holds the kernel
    to); for the R = 64 and M >= 127 cases 10 x condition_probe, never less than 1e-8 (the ten: the kernel's third summation order)."""
    if case not in PROBED:
        return 1e-8
    return max(1e-8, 10.0 * case_probe(*case[:6], tol, max_iter))
