"""NumPy float64 restatement of the fold loop (csrc/fold_loop.hpp: lx_inner_loop) for X of order 4 (TEST INFRASTRUCTURE): the
inner loop of one component on a cross-covariance S (M x A B1 B2) with the rank-1 extraction of the A x B1 x B2 tensor S^T q by
oracle.nipals_oracle.rank1_factors.  Shared by tests/test_kfold_order4_cpu.py and tests/test_gpu_kfold_order4_kernel.py."""
import numpy as np

from oracle.nipals_oracle import rank1_factors


def inner_loop(S: np.ndarray, Gy: np.ndarray, dims, tol: float = 1e-8, max_iter: int = 100) -> dict:
    """tpls.py:77-107 on S = Y^T X (M x P) and G_y = Y^T Y: from q = e_0 (u = Y[:, 0]) until sqrt(dq^T G_y dq) < tol (never on
    the first pass) or max_iter passes.  Returns wA, wK, wL, wB = wK (x) wL, q and n_iter (the passes executed)."""
    M = S.shape[0]
    A, B1, B2 = dims
    q = np.zeros(M)
    q[0] = 1.0
    n_iter = 0
    for it in range(max_iter):
        n_iter = it + 1
        Z = (S.T @ q).reshape(A, B1, B2)                                         # X x_0 u = S^T q
        wA, wK, wL = rank1_factors(Z, tol)
        wB = np.kron(wK, wL)
        tq = S @ np.kron(wA, wB)                                                  # Y^T t = S (wA (x) wB)
        qn = tq / np.linalg.norm(tq)
        d = qn - q
        d2 = float(d @ Gy @ d)                                                    # |u_old - u|^2
        q = qn
        if it > 0 and np.sqrt(max(d2, 0.0)) < tol:
            break
    return {"wA": wA, "wK": wK, "wL": wL, "wB": wB, "q": q, "n_iter": n_iter}


def planted(dims, M: int, K: int, seed: int, noise: float = 0.05):
    """K models' S (K x M x P) whose Z = S^T q has a dominant rank-one term whatever q, plus `noise` (relative) of Gaussian noise,
    and an identity-like SPD G_y (M x M)."""
    rng = np.random.default_rng(seed)
    A, B1, B2 = dims
    P = A * B1 * B2
    S = np.empty((K, M, P))
    for k in range(K):
        w = np.kron(rng.standard_normal(A), np.kron(rng.standard_normal(B1), rng.standard_normal(B2)))
        c = 1.0 + rng.random(M)                                                   # every response loads on the planted term
        sig = np.outer(c, w)
        S[k] = sig + noise * np.linalg.norm(sig) / np.sqrt(M * P) * rng.standard_normal((M, P))
    E = rng.standard_normal((M, M))
    Gy = np.eye(M) + 0.1 * (E @ E.T) / M
    return S, Gy
