"""The float64 restatement of the cross-covariance iteration (tests/xcov_iterate_ref.py) against the literal form of one inner
iteration on (X, Y), against the NumPy test backend, and the carry identity of S across a deflation -- no GPU.

The device tests (test_gpu_xcov_iterate.py) trust the restatement; this file is what entitles them to.
"""
import numpy as np
import pytest
import torch

import xcov_iterate_ref as R
from numpy_backend import NumpyBackend

# two float64 evaluations of one sum of n well-scaled terms in different orders: n * 2^-53 relative to the sum of moduli; the
# largest n here is I * P ~ 4e4 terms of O(1), so 1e-12 relative to the largest entry leaves a factor of ~100 (and it is the
# relative tolerance the project's xcov tests use)
RTOL = 1e-12


def _close(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max())
    assert err <= RTOL * scale, (what, err, RTOL * scale)


def _block(rng, I, A, B, M, latent=None):
    """X (I, A*B) with one clear component, so that Z has a clear leading pair."""
    latent = rng.normal(size=I) if latent is None else latent
    X = 3.0 * np.outer(latent, np.kron(rng.normal(size=A), rng.normal(size=B))) + rng.normal(size=(I, A * B))
    return X - X.mean(axis=0)


def _xy(rng, I, shapes, M):
    latent = rng.normal(size=I)
    Xs = [_block(rng, I, A, B, M, latent) for A, B in shapes]
    Y = np.outer(latent, rng.normal(size=M)) + 0.5 * rng.normal(size=(I, M))
    Y -= Y.mean(axis=0)
    q = rng.normal(size=M)
    return Xs, Y, q / np.linalg.norm(q)


def _literal_iteration(Xs, shapes, orders, Y, q):
    """One inner iteration written on (X, Y) (tpls.py:83-103, cmtf.py:91-125): returns per-block Z, loadings and Y^T t, then q', du2."""
    u = Y @ q
    out, ts = [], []
    for X, (A, B), order in zip(Xs, shapes, orders):
        Z = X.T @ u
        wA, wB = R.loadings_of(Z, A, B, order)
        t = X @ np.kron(wA, wB)
        ts.append(t)
        out.append((Z, wA, wB, Y.T @ t))
    t = np.mean(ts, axis=0)
    q_new = Y.T @ t / np.linalg.norm(Y.T @ t)
    du2 = float(np.sum((Y @ q_new - u) ** 2))
    return out, q_new, du2


@pytest.mark.parametrize("name,shapes,orders,M", [
    ("order3", [(9, 7)], [3], 5),
    ("matrix", [(1, 41)], [2], 4),
    ("coupled", [(6, 8), (1, 23)], [3, 2], 3),
    ("one_response", [(5, 7)], [3], 1),
])
def test_restatement_equals_the_literal_iteration(name, shapes, orders, M):
    rng = np.random.default_rng(len(name) * 101 + M)
    I = 60
    Xs, Y, q = _xy(rng, I, shapes, M)
    lit, q_lit, du2_lit = _literal_iteration(Xs, shapes, orders, Y, q)
    tqs = []
    for X, (A, B), order, (Z_lit, wA_lit, wB_lit, ytt_lit) in zip(Xs, shapes, orders, lit):
        S = Y.T @ X
        Z = R.z_of(S, q)
        _close(Z, Z_lit, "Z")
        wA, wB = R.loadings_of(Z, A, B, order)
        # (the SVD of two matrices 1e-12 apart: the pair moves by that over the relative gap, which is O(1) here)
        np.testing.assert_allclose(wA, wA_lit, rtol=0, atol=1e-10)
        np.testing.assert_allclose(wB, wB_lit, rtol=0, atol=1e-10)
        assert wB[np.argmax(np.abs(wB))] > 0
        if order == 2:
            assert wA.shape == (1,) and wA[0] == 1.0
        tq = R.tq_of(S, wA_lit, wB_lit)
        _close(tq, ytt_lit, "tq")
        tqs.append(ytt_lit)
    q_new = R.q_of(tqs)
    _close(q_new, q_lit, "q_new")
    np.testing.assert_allclose(np.linalg.norm(q_new), 1.0, rtol=1e-15)
    du2 = R.du2_of(Y.T @ Y, q_lit, q)
    assert abs(du2 - du2_lit) <= RTOL * R.du2_abs_terms(Y.T @ Y, q_lit, q), (du2, du2_lit)


def test_masked_contraction_is_the_observed_mean_times_n():
    """z_of with colcnt against missingvals.py:7-20 written column by column on an X with NaNs; a column never observed is 0."""
    rng = np.random.default_rng(5)
    I, P, M = 40, 19, 3
    X = rng.normal(size=(I, P))
    X[rng.random(X.shape) < 0.3] = np.nan
    X[:, 4] = np.nan
    Y = rng.normal(size=(I, M))
    q = rng.normal(size=M)
    u = Y @ q
    want = np.zeros(P)
    for c in range(P):
        m = np.where(~np.isnan(X[:, c]))[0]
        if len(m):
            want[c] = X[m, c] @ u[m] / len(m) * I
    S = Y.T @ np.nan_to_num(X)
    colcnt = (~np.isnan(X)).sum(axis=0).astype(np.float64)
    got = R.z_of(S, q, colcnt, I)
    _close(got, want, "masked Z")
    assert got[4] == 0.0
    assert R.z_of(S, q, -np.ones(P), I).tolist() == [0.0] * P


def test_sign_rule_lowest_index_wins_a_tie():
    u, v = R.sign_rule(np.array([1.0, 2.0]), np.array([-3.0, 1.0, 3.0]))   # two equal maxima: index 0 decides, and it is negative
    assert u.tolist() == [-1.0, -2.0] and v.tolist() == [3.0, -1.0, -3.0]
    u, v = R.sign_rule(np.array([1.0, 2.0]), np.array([3.0, 1.0, -3.0]))
    assert u.tolist() == [1.0, 2.0] and v.tolist() == [3.0, 1.0, -3.0]
    Z = np.outer([1.0, 2.0], [-3.0, 1.0, 2.0])
    wA, wB = R.loadings_of(Z.ravel(), 2, 3, 3)
    assert wB[0] > 0 and wA[0] < 0
    np.testing.assert_allclose(np.outer(wA, wB) * np.linalg.norm(Z), Z, atol=1e-14)


def test_q_of_is_the_normalised_mean():
    rng = np.random.default_rng(6)
    tqs = [rng.normal(size=7) for _ in range(3)]
    mean = np.mean(tqs, axis=0)
    _close(R.q_of(tqs), mean / np.linalg.norm(mean), "q_of")


def test_longdouble_inputs_are_accumulated_in_longdouble():
    LD = np.longdouble
    S = np.ones((2, 3), dtype=LD)
    assert R.z_of(S, np.ones(2, dtype=LD)).dtype == LD
    assert R.tq_of(S, np.ones(1, dtype=LD), np.ones(3, dtype=LD)).dtype == LD
    assert np.asarray(R.du2_of(np.eye(2, dtype=LD), np.ones(2, dtype=LD), np.zeros(2, dtype=LD))).dtype == LD


# ---- against the NumPy test backend ---------------------------------------------------------------------------------------

def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def test_numpy_backend_xcov_iterate_matches():
    rng = np.random.default_rng(7)
    A, B, M, I = 8, 6, 4, 50
    (X,), Y, q = _xy(rng, I, [(A, B)], M)
    S, G = Y.T @ X, Y.T @ Y
    be = NumpyBackend()
    Z, wA, wB, info, q_new, du2 = _t(np.zeros(A * B)), _t(np.zeros(A)), _t(np.zeros(B)), _t(np.zeros(2)), _t(np.zeros(M)), _t(np.zeros(1))
    be.xcov_iterate(_t(S), A, B, _t(q), Z, wA, wB, info, 30, q_new, _t(G), du2, True)
    _close(Z.numpy(), R.z_of(S, q), "Z")
    rA, rB = R.loadings_of(Z.numpy(), A, B, 3)
    np.testing.assert_allclose(wA.numpy(), rA, rtol=0, atol=1e-14)
    np.testing.assert_allclose(wB.numpy(), rB, rtol=0, atol=1e-14)
    _close(q_new.numpy(), R.q_of([R.tq_of(S, wA.numpy(), wB.numpy())]), "q_new")
    assert abs(float(du2[0]) - R.du2_of(G, q_new.numpy(), q)) <= RTOL * R.du2_abs_terms(G, q_new.numpy(), q)
    # first=False extracts from what is in Z
    Z2 = rng.normal(size=A * B) + 3.0 * np.kron(rng.normal(size=A), rng.normal(size=B))
    Z.copy_(_t(Z2))
    be.xcov_iterate(_t(S), A, B, _t(q), Z, wA, wB, info, 30, q_new, _t(G), du2, False)
    assert np.array_equal(Z.numpy(), Z2)
    rA, rB = R.loadings_of(Z2, A, B, 3)
    np.testing.assert_allclose(wB.numpy(), rB, rtol=0, atol=1e-14)
    np.testing.assert_allclose(wA.numpy(), rA, rtol=0, atol=1e-14)


def test_numpy_backend_xcov_blocks_plan_matches():
    """Order 3, order 3 with S2 / colcnt, and a matrix block: Z from S (scaled by n / colcnt), Y^T t from S2, q' from the sum."""
    rng = np.random.default_rng(8)
    M, I = 5, 30
    shapes, orders = [(4, 6), (3, 5), (1, 11)], [3, 3, 2]
    q = rng.normal(size=M)
    q /= np.linalg.norm(q)
    Y = rng.normal(size=(I, M))
    G = Y.T @ Y
    blocks, host = [], []
    for i, ((A, B), order) in enumerate(zip(shapes, orders)):
        P = A * B
        S = np.outer(q, 3.0 * np.kron(rng.normal(size=A), rng.normal(size=B))) + rng.normal(size=(M, P))
        S2 = rng.normal(size=(M, P)) if i == 1 else None
        colcnt = rng.integers(0, 4, size=P).astype(np.float64) if i == 1 else None
        host.append((S, S2, colcnt))
        blocks.append(dict(S=_t(S), S2=None if S2 is None else _t(S2), colcnt=None if colcnt is None else _t(colcnt), n_samples=float(I),
                           order=order, A=A, B=B, Z=_t(np.zeros(P)), wA=_t(np.ones(A)), wB=_t(np.zeros(B))))
    tq, q_new, status = _t(np.zeros(3 * M)), _t(np.zeros(M)), _t(np.full(7, -7.0))
    enqueue = NumpyBackend().xcov_blocks_plan(blocks, M, _t(q), tq, q_new, _t(G), status)
    enqueue([30, 30, 30], True)
    tqs = []
    for b, (S, S2, colcnt), (A, B), order in zip(blocks, host, shapes, orders):
        Z = R.z_of(S, q, colcnt, float(I))
        _close(b["Z"].numpy(), Z, "Z")
        if colcnt is not None:
            assert np.all(b["Z"].numpy()[colcnt == 0] == 0.0) and (colcnt == 0).any()
        rA, rB = R.loadings_of(b["Z"].numpy(), A, B, order)
        np.testing.assert_allclose(b["wB"].numpy(), rB, rtol=0, atol=1e-14)
        if order == 3:
            np.testing.assert_allclose(b["wA"].numpy(), rA, rtol=0, atol=1e-14)
        tqs.append(R.tq_of(S if S2 is None else S2, b["wA"].numpy()[:A], b["wB"].numpy()))
    _close(tq.numpy().reshape(3, M), np.stack(tqs), "tq")
    _close(q_new.numpy(), R.q_of(tqs), "q_new")
    assert abs(float(status[0]) - R.du2_of(G, q_new.numpy(), q)) <= RTOL * R.du2_abs_terms(G, q_new.numpy(), q)
    assert status.numpy()[5:7].tolist() == [-7.0, -7.0]      # the matrix block's status words are not written


def test_numpy_backend_s_downdate_matches():
    rng = np.random.default_rng(9)
    A, B, M = 3, 7, 4
    S = rng.normal(size=(M, A * B))
    ya, wA, wB, q, v = rng.normal(size=M), rng.normal(size=A), rng.normal(size=B), rng.normal(size=M), rng.normal(size=A * B)
    Sd = _t(S.copy())
    NumpyBackend().s_downdate(Sd, A, B, _t(ya), _t(wA), _t(wB), _t(q), _t(v))
    _close(Sd.numpy(), R.s_downdate_of(S, ya, wA, wB, q, v), "S+")


def test_numpy_backend_kr_gram_row_matches():
    rng = np.random.default_rng(10)
    n, Rk, a = 9, 6, 4
    L1, L2 = rng.normal(size=(n, Rk)), rng.normal(size=(n + 2, Rk))
    g = _t(np.full(Rk, -7.0))
    be = NumpyBackend()
    be.kr_gram_row(_t(L1), a, g, True)
    want = R.kr_gram_row_of(L1, a, np.full(Rk, -7.0), True)
    _close(g.numpy(), want, "first")
    be.kr_gram_row(_t(L2), a, g, False)
    want = R.kr_gram_row_of(L2, a, want, False)
    _close(g.numpy(), want, "second")
    _close(want[:a], ((L1.T @ L1) * (L2.T @ L2))[a, :a], "hadamard")
    assert want[a:].tolist() == [-7.0] * (Rk - a)
    assert R.kr_gram_row_of(L1, 0, np.full(Rk, -7.0), True).tolist() == [-7.0] * Rk


# ---- the carry of S across one deflation ---------------------------------------------------------------------------------

@pytest.mark.parametrize("A,B,M", [(7, 5, 3), (1, 30, 2), (4, 4, 1)])
def test_carry_identity(A, B, M):
    """S+ = s_downdate_of(S, Y^T t, wA, wB, q, X+^T yhat) is Y+^T X+ for X+ = X - t w^T, Y+ = Y - yhat q^T (any t, yhat, q):
    |S+ - S'|_inf <= 1e-12 |S'|_inf, the relative tolerance of the project's xcov tests."""
    rng = np.random.default_rng(A * 31 + B)
    I = 45
    (X,), Y, q = _xy(rng, I, [(A, B)], M)
    S = Y.T @ X
    wA, wB = R.loadings_of(R.z_of(S, q), A, B, 3 if A > 1 else 2)
    w = np.kron(wA, wB)
    t = X @ w
    yhat = t * (t @ (Y @ q) / (t @ t))                       # the inner relation's prediction of u = Y q from t
    Xp = X - np.outer(t, w)
    Yp = Y - np.outer(yhat, q)
    Sp = R.s_downdate_of(S, Y.T @ t, wA, wB, q, Xp.T @ yhat)
    want = Yp.T @ Xp
    assert np.abs(Sp - want).max() <= 1e-12 * np.abs(want).max()
