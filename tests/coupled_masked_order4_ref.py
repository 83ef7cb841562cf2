"""NumPy float64 restatement of ONE model of cmtfpls_cv_masked_coupled_tensor_f64 (csrc/cv_masked_coupled.hip) -- TEST
INFRASTRUCTURE ONLY.  It is coupled_masked_ref.coupled_masked_fit: the count-weighted coupled model with the missing-value
arithmetic switched on block by block, whose loading step hands a block's contraction Z, in the block's trailing shape, to
oracle.rank1_factors.  For a block of order 4 that Z is A x B1 x B2 (already / c_p * n when the block is masked) and rank1_factors is
the rank-1 CP (parafac(Z, 1, tol, init="svd", normalize_factors=True), the statement rank1_tensor_ref.als restates sweep by sweep);
the block's score and deflation then use wA (x) wK (x) wL on the I x A B1 B2 view, which is what the kernel's wA and wB = wK (x) wL
are.  Here the result is laid out as the kernel's outputs are: per block wA, wB, and for a block of order 4 wK and wL."""
import numpy as np

from coupled_masked_ref import coupled_masked_fit


def coupled_masked_order4_fit(Xs, Y, c, R, yrow=None, tol=1e-8, max_iter=100):
    """Returns (factors, Q (M, R), coef (R, R), pred (R, n_held, M), n_iter, info).  factors: per block a dict of (dim, R) arrays --
    "Wb" always (order 2: the loading; order 3: mode 2; order 4: wK (x) wL in C order), "Wa" for order 3 and 4, "Wk" and "Wl" for
    order 4.  At least one block must be of order 4 (the entry's own condition)."""
    assert any(np.ndim(X) == 4 for X in Xs) and all(np.ndim(X) in (2, 3, 4) for X in Xs)
    loadings, Q, coef, pred, n_iter, info = coupled_masked_fit(Xs, Y, c, R, yrow, tol, max_iter)
    factors = []
    for X, L in zip(Xs, loadings):
        if np.ndim(X) == 2:
            factors.append({"Wb": L[0]})
        elif np.ndim(X) == 3:
            factors.append({"Wa": L[0], "Wb": L[1]})
        else:
            wb = np.stack([np.kron(L[1][:, a], L[2][:, a]) for a in range(R)], axis=1)
            factors.append({"Wa": L[0], "Wk": L[1], "Wl": L[2], "Wb": wb})
    return factors, Q, coef, pred, n_iter, info
