"""Leave-one-out of a tPLS whose X has order 4 (TEST INFRASTRUCTURE): planted low-rank inputs and float64 oracle refits (hold out row
i, oracle.fit_tpls on the rest -- its extraction is oracle.rank1_factors -- predict row i).  Shared by
tests/test_gpu_loo_order4_kernel.py and tests/test_loo_order4_cpu.py; the refits of a case are computed once."""
import functools

import numpy as np

import oracle as O


def planted_xy(shape, M: int, rank: int = 3, noise: float = 0.05, seed: int = 0):
    """X (I x A x B1 x B2, or any order) = sum_r s_r t_r o a_r o k_r o l_r with s_r = 1, 1/2, 1/3, .. and Y = T C, each plus `noise`
    (relative to the signal's rms) of Gaussian noise: the CP of every cross-covariance converges in a handful of sweeps."""
    rng = np.random.default_rng(seed)
    I = shape[0]
    T = rng.standard_normal((I, rank))
    X = np.zeros(shape)
    for r in range(rank):
        term = T[:, r]
        for d in shape[1:]:
            term = np.multiply.outer(term, rng.standard_normal(d))
        X += term / (r + 1.0)
    X += noise * np.sqrt(np.mean(X ** 2)) * rng.standard_normal(shape)
    Y = T @ rng.standard_normal((rank, M))
    Y += noise * np.sqrt(np.mean(Y ** 2)) * rng.standard_normal((I, M))
    return X + 0.3, Y - 0.2                                                         # (nonzero means: the fold's down-dated means matter)


@functools.lru_cache(maxsize=None)
def loo_case(shape, M: int, R: int, seed: int):
    """(X, Y, Ypred (I, M), n_iter (I, R)) of the oracle's leave-one-out refits; the arrays are read-only."""
    X, Y = planted_xy(shape, M, seed=seed)
    I = shape[0]
    pred = np.empty((I, M))
    n_iter = np.empty((I, R), dtype=np.int64)
    keep = np.ones(I, dtype=bool)
    for i in range(I):
        keep[i] = False
        fit = O.fit_tpls(X[keep], Y[keep], R)
        pred[i] = np.asarray(O.predict(fit, X[i:i + 1])).reshape(M)
        n_iter[i] = fit.n_iter
        keep[i] = True
    for a in (X, Y, pred, n_iter):
        a.setflags(write=False)
    return X, Y, pred, n_iter
