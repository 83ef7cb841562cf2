"""Plain NumPy restatement of one inner iteration of the cross-covariance form and of the carry of S between
components -- TEST INFRASTRUCTURE ONLY (no backend, no torch).

Every function is written from the definition of its step, not from a kernel:

  S = Y^T X_(0)                       the cross-covariance the iteration runs on (M x P)
  Z = X_(0)^T (Y q) = S^T q           tpls.py:83 re-associated through S
  (wA, wB)                            leading singular pair of Z (order 3) / Z normalised (matrix block), tpls.py:84-90
  Y^T t = Y^T X_(0) w = S w           tpls.py:92-100 with w = kron(wA, wB)
  q' = Y^T t / |Y^T t|                tpls.py:101
  |Y q' - Y q|^2 = dq^T (Y^T Y) dq    tpls.py:103

The functions compute in the dtype of their inputs: float64 in, float64 out.  Given np.longdouble inputs they accumulate in
np.longdouble, which the device tests use so that the reference's own rounding does not eat into a kernel's error bound.
"""
import numpy as np


def z_of(S, q, colcnt=None, n_samples=None):
    """Z[c] = sum_m q[m] S[m, c]; with colcnt: Z[c] / colcnt[c] * n_samples, and 0 where colcnt[c] <= 0 (missingvals.py:17-19)."""
    S, q = np.asarray(S), np.asarray(q)
    Z = (q[:, None] * S).sum(axis=0)
    if colcnt is None:
        return Z
    colcnt = np.asarray(colcnt)
    seen = colcnt > 0
    out = np.zeros_like(Z)
    out[seen] = Z[seen] / colcnt[seen].astype(Z.dtype) * n_samples
    return out


def loadings_of(Z, A, B, order):
    """(wA, wB).  Order 3: the leading singular pair of Z (A x B), signed so that the entry of wB with the largest modulus is
    positive (the lowest index wins a tie).  Order 2: wB = Z / |Z| and wA = [1]."""
    Z = np.asarray(Z, dtype=np.float64)
    if order == 2:
        z = Z.reshape(-1)
        return np.ones(1), z / np.sqrt((z * z).sum())
    assert order == 3
    U, _, Vt = np.linalg.svd(Z.reshape(A, B), full_matrices=False)
    return sign_rule(U[:, 0].copy(), Vt[0].copy())


def sign_rule(u, v):
    """(u, v) or (-u, -v): whichever makes the entry of v with the largest modulus positive (argmax returns the first of equal maxima)."""
    if v[int(np.argmax(np.abs(v)))] < 0:
        return -u, -v
    return u, v


def tq_of(S, wA, wB):
    """Y^T t = S kron(wA, wB) for the M rows of S (or of S2, the cross-covariance with missing values zeroed)."""
    S = np.asarray(S)
    w = np.kron(np.asarray(wA), np.asarray(wB)).astype(S.dtype)
    return (S * w[None, :]).sum(axis=1)


def q_of(tqs):
    """The sum of the blocks' Y^T t, normalised -- the same vector as their normalised mean (the 1 / nb drops out)."""
    s = np.sum(np.stack([np.asarray(t) for t in tqs]), axis=0)
    return s / np.sqrt((s * s).sum())


def du2_of(G, q_new, q_cur):
    """(q_new - q_cur)^T G (q_new - q_cur) = |Y q_new - Y q_cur|^2 for G = Y^T Y."""
    d = np.asarray(q_new) - np.asarray(q_cur)
    return (d[:, None] * np.asarray(G) * d[None, :]).sum()


def du2_abs_terms(G, q_new, q_cur):
    """sum_ij |dq_i G_ij dq_j|: the scale of the rounding error of du2_of (not its value, which may cancel)."""
    d = np.abs(np.asarray(q_new) - np.asarray(q_cur))
    return (d[:, None] * np.abs(np.asarray(G)) * d[None, :]).sum()


def s_downdate_of(S, ya, wA, wB, q, v):
    """S+ = S - ya w^T - q v^T with w = kron(wA, wB): S carried across X+ = X - t w^T, Y+ = Y - yhat q^T when
    ya = Y^T t and v = X+^T yhat (tpls.py:109,113)."""
    w = np.kron(np.asarray(wA), np.asarray(wB))
    return np.asarray(S) - np.outer(np.asarray(ya).reshape(-1), w) - np.outer(np.asarray(q), np.asarray(v))


def kr_gram_row_of(L, a, g, first):
    """A copy of g with g[j] = (1 if first else g[j]) * sum_i L[i, j] L[i, a] for j < a: row a of L^T L, multiplied into g
    when not first (the Gram matrix of a Khatri-Rao product is the Hadamard product of its factors' Gram matrices)."""
    L = np.asarray(L)
    out = np.array(g, copy=True)
    row = (L[:, :a] * L[:, a:a + 1]).sum(axis=0)
    out[:a] = row if first else out[:a] * row
    return out
