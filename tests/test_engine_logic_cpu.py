"""The engine's control flow against the oracle on CPU (NumPy test backend, tests/numpy_backend.py).

This checks everything in cmtf_pls_amd/engine.py that is NOT a kernel: the loop structure, the
R2X / R2Y identities that replace the reference's reconstruction passes, the normal-equation form
of the lstsq, masked scaling, coupled averaging, transform / predict.  Kernel parity is the job of
the -m gpu tests.
"""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.engine import default_options
from numpy_backend import NumpyBackend


def _canon(W_new, W_ref):
    """Per-component sign of W_new aligned with W_ref."""
    s = np.sign(np.sum(W_new * W_ref, axis=0))
    s[s == 0] = 1
    return W_new * s


def _check_fit(m, fit, block=0, rtol=1e-7):
    Xf = m.X_factors if hasattr(m, "X_factors") else m.Xs_factors[block]
    np.testing.assert_allclose(Xf[0], fit.T, rtol=rtol, atol=1e-8)
    loads = fit.loadings[block]
    # the product of the trailing loadings is sign-invariant; single loadings up to a paired sign
    for got, want in zip(Xf[1:], loads):
        np.testing.assert_allclose(np.abs(got), np.abs(want), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(m.Y_factors[0], fit.U, rtol=rtol, atol=1e-8)
    np.testing.assert_allclose(m.Y_factors[1], fit.Q, rtol=rtol, atol=1e-8)
    np.testing.assert_allclose(m.coef_, fit.coef, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(m.R2Y, fit.r2y, rtol=1e-7, atol=1e-9)
    assert list(m.n_iter_) == list(fit.n_iter)


def test_tpls_cfg1_matches_oracle():
    x, y, _ = O.import_synthetic((200, 10, 8), 4, 3, error=0.1)
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    fit = O.fit_tpls(x, y, 3)
    _check_fit(m, fit)
    np.testing.assert_allclose(m.R2X, fit.r2x[0], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(m.X_mean, fit.x_means[0])
    xt = np.random.default_rng(0).normal(size=(7, 10, 8))
    np.testing.assert_allclose(m.predict(xt), O.predict(fit, xt), rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(m.transform(x), fit.T, rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(m.X_reconstructed(), O.reconstruct(fit), rtol=1e-7, atol=1e-8)


def test_tpls_matrix_x_and_1d_y():
    x, y, _ = O.import_synthetic((60, 30), 1, 4, error=0.05, seed=2)
    assert y.ndim == 1
    m = tPLS(4, backend=NumpyBackend())
    m.fit(x, y)
    fit = O.fit_tpls(x, y, 4)
    np.testing.assert_allclose(m.X_factors[0], fit.T, rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(m.X_factors[1], fit.loadings[0][0], rtol=1e-7, atol=1e-8)   # vector case: no sign freedom
    np.testing.assert_allclose(m.R2X, fit.r2x[0], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(m.R2Y, fit.r2y, rtol=1e-7, atol=1e-9)
    xs, ys = m.transform(x, y)
    oxs, oys = O.transform(fit, x, y)
    np.testing.assert_allclose(xs, oxs, rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(ys, oys, rtol=1e-7, atol=1e-8)


def test_tpls_missing_values():
    rng = np.random.default_rng(5)
    x, y, _ = O.import_synthetic((50, 8, 6), 3, 3, error=0.1, seed=4)
    x[rng.random(x.shape) < 0.3] = np.nan
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    fit = O.fit_tpls(x, y, 3)
    assert m.X_hasMiss
    _check_fit(m, fit, rtol=1e-6)
    np.testing.assert_allclose(m.R2X, fit.r2x[0], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(m.transform(x), fit.T, rtol=1e-6, atol=1e-8)


def test_ctpls_tensor_plus_matrix():
    x3, y3, cp = O.import_synthetic((64, 8, 12), 3, 4, error=0.05, seed=5)
    xm = cp.factors[0] @ np.random.default_rng(216).normal(size=(20, 4)).T
    m = ctPLS(4, backend=NumpyBackend())
    m.fit([x3, xm], y3)
    fit = O.fit_ctpls([x3, xm], y3, 4)
    _check_fit(m, fit, block=0)
    for b in range(2):
        np.testing.assert_allclose(m.R2Xs[b], fit.r2x[b], rtol=1e-7, atol=1e-9)
    assert m.Xs_factors[0][0] is m.Xs_factors[1][0] is m.factor_T
    np.testing.assert_allclose(m.transform([x3, xm]), fit.T, rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(m.predict([x3, xm]), O.predict(fit, [x3, xm]), rtol=1e-7, atol=1e-8)


def test_api_surface_and_errors():
    x, y, _ = O.import_synthetic((30, 6, 5), 2, 2)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    assert len(m) == 3 and m[0] is m.X_factors and m[1] is m.Y_factors and m[2] is m.coef_
    assert [f is g for f, g in zip(list(m), [m.X_factors, m.Y_factors, m.coef_])] == [True] * 3
    with pytest.raises(IndexError):
        m[3]
    with pytest.raises(ValueError, match="Training X has shape"):
        m.predict(np.zeros((4, 6, 4)))
    with pytest.raises(ValueError, match="Training X has shape"):
        m.transform(np.zeros((4, 5, 5)))
    with pytest.raises(ValueError, match="Training Y has shape"):
        m.transform(x, np.zeros((30, 3)))
    with pytest.raises(ValueError, match="Only a matrix"):
        m.transform(x, np.zeros((30, 2, 1)))
    with pytest.raises(AssertionError):
        tPLS(2, backend=NumpyBackend()).fit(x, y[:-1])
    with pytest.raises(AssertionError):
        ctPLS(2, backend=NumpyBackend()).fit(x, y)            # not a list (cmtf.py:46)
    c = m.copy()
    assert c is not m and c.X_factors is m.X_factors           # shallow, like copy.copy (tpls.py:41-42)
    x0 = x.copy()
    m.predict(x)
    assert np.array_equal(x, x0)                               # inputs are never modified


def test_no_cpu_fallback_in_product_path():
    from cmtf_pls_amd import _lib
    x, y, _ = O.import_synthetic((10, 4, 3), 2, 2)
    with pytest.raises(_lib.CmtfplsError):
        tPLS(2).fit(x, y)                                      # no GPU here -> must fail loudly
    from cmtf_pls_amd.missingvals import miss_mmodedot, miss_tensordot
    with pytest.raises(_lib.CmtfplsError):
        miss_tensordot(x, y[:, 0])                             # the missing-value contractions too
    with pytest.raises(_lib.CmtfplsError):
        miss_mmodedot(x, [np.ones(4), np.ones(3)])
    with pytest.raises(AssertionError):
        miss_tensordot(x, y[:5, 0])                            # missingvals.py:10: sample counts must agree


@pytest.mark.parametrize("shape", [(20, 8, 6, 4), (12, 5, 4, 3, 2)])
def test_tpls_higher_order(shape):
    """X of order 4 / 5 (tests/test_tpls.py:132-155 use order 4): rank-1 CP of a tensor Z."""
    rng = np.random.default_rng(7)
    X, Y = rng.random(shape), rng.random((shape[0], 5))
    m = tPLS(4, backend=NumpyBackend())
    m.fit(X, Y)
    fit = O.fit_tpls(X, Y, 4)
    np.testing.assert_allclose(m.X_factors[0], fit.T, rtol=1e-7, atol=1e-8)
    for got, want in zip(m.X_factors[1:], fit.loadings[0]):
        np.testing.assert_allclose(got, want, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(m.R2X, fit.r2x[0], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(m.R2Y, fit.r2y, rtol=1e-7, atol=1e-9)
    order = rng.permutation(shape[0])
    xs, ys = m.transform(X[order], Y[order])
    assert np.allclose(xs, m.X_factors[0][order]) and np.allclose(ys, m.Y_factors[0][order])


def test_ctpls_mixed_orders():
    rng = np.random.default_rng(9)                              # tests/test_cmtf.py:18-29
    Xs = [rng.random(d) for d in [(10, 9, 8, 7), (10, 8, 7), (10, 8)]]
    Y = rng.random((10, 5))
    m = ctPLS(4, backend=NumpyBackend())
    m.fit(Xs, Y)
    fit = O.fit_ctpls(Xs, Y, 4)
    np.testing.assert_allclose(m.factor_T, fit.T, rtol=1e-6, atol=1e-8)
    assert np.allclose(m.factor_T, m.transform(Xs))
    np.testing.assert_allclose(m.R2Y, fit.r2y, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("case", ["plain", "nan", "matrix", "coupled"])
def test_xcov_algorithm_equals_direct(case):
    """algorithm="xcov" (inner loop on S = X^T Y) is the same iteration re-associated: identical
    iteration counts and factors to rounding, for plain / NaN / matrix-X / coupled fits."""
    rng = np.random.default_rng(31)
    x, y, cp = O.import_synthetic((80, 9, 8), 5, 3, error=0.2, seed=8)
    if case == "nan":
        x[rng.random(x.shape) < 0.25] = np.nan
    if case == "matrix":
        x = x.reshape(80, 72)
    if case == "coupled":
        xm = cp.factors[0] @ rng.normal(size=(11, 3)).T + 0.1 * rng.normal(size=(80, 11))
        a, b = ctPLS(3, backend=NumpyBackend()), ctPLS(3, backend=NumpyBackend(), algorithm="xcov")
        a.fit([x, xm], y)
        b.fit([x, xm], y)
        Ta, Tb = a.factor_T, b.factor_T
        r2a, r2b = a.R2Xs[0], b.R2Xs[0]
    else:
        a, b = tPLS(3, backend=NumpyBackend()), tPLS(3, backend=NumpyBackend(), algorithm="xcov")
        a.fit(x, y)
        b.fit(x, y)
        Ta, Tb = a.X_factors[0], b.X_factors[0]
        r2a, r2b = a.R2X, b.R2X
    assert a.n_iter_ == b.n_iter_
    np.testing.assert_allclose(Tb, Ta, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(b.Y_factors[0], a.Y_factors[0], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(b.Y_factors[1], a.Y_factors[1], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(b.coef_, a.coef_, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(r2b, r2a, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(b.R2Y, a.R2Y, rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("case", ["tpls3", "tpls4", "matrix", "coupled", "more_components_than_rank"])
def test_xcov_without_writing_x_equals_the_deflating_form(case, monkeypatch):
    """algorithm="xcov" on NaN-free blocks never deflates X (FitRun._finish_xcov_nowrite): X_a = X_0 - sum t_j w_j^T is
    carried implicitly.  Same scores, loadings, coefficients, R2X (from the norm recurrence) and iteration counts as the
    form that deflates in place (NipalsEngine.xcov_nowrite = False) and as the direct loop; the engine's copy of X ends
    the fit exactly as it was centred."""
    opt = {}                                              # EngineOptions fields this test overrides
    rng = np.random.default_rng(77)
    R = 4
    if case == "coupled":
        Xs = [rng.random((30, 6, 5, 4)), rng.random((30, 7, 3)), rng.random((30, 9))]
    elif case == "tpls4":
        Xs = [rng.random((30, 6, 5, 4))]
    elif case == "matrix":
        Xs = [rng.random((30, 24))]
    elif case == "more_components_than_rank":
        x, _, _ = O.import_synthetic((30, 7, 6), 3, 2, error=0.0, seed=3)       # X has CP rank 2, R = 4 asks for more
        Xs = [x]
    else:
        Xs = [rng.random((30, 7, 6))]
    Y = rng.random((30, 3))

    def fit(nowrite, algorithm="xcov"):
        opt["xcov_nowrite"] = nowrite
        if len(Xs) > 1:
            m = ctPLS(R, backend=NumpyBackend(), algorithm=algorithm, options=default_options().but(**opt))
            m.fit(Xs, Y)
            return m, m.factor_T, m.R2Xs, [f for fs in m.Xs_factors for f in fs[1:]]
        m = tPLS(R, backend=NumpyBackend(), algorithm=algorithm, options=default_options().but(**opt))
        m.fit(Xs[0], Y)
        return m, m.X_factors[0], [m.R2X], m.X_factors[1:]

    a, Ta, r2a, La = fit(False)
    b, Tb, r2b, Lb = fit(True)
    d, Td, r2d, Ld = fit(True, "direct")
    tight = case != "more_components_than_rank"        # beyond the rank of X the extra components are rounding noise
    ncmp = R if tight else 2
    assert a.n_iter_[:ncmp] == b.n_iter_[:ncmp] == d.n_iter_[:ncmp]
    for T_, r2_, L_, m_ in ((Ta, r2a, La, a), (Td, r2d, Ld, d)):
        np.testing.assert_allclose(Tb[:, :ncmp], T_[:, :ncmp], rtol=1e-9, atol=1e-9)
        for x1, x2 in zip(Lb, L_):
            np.testing.assert_allclose(x1[:, :ncmp], x2[:, :ncmp], rtol=1e-8, atol=1e-9)
        for x1, x2 in zip(r2b, r2_):                    # iterates agree to the convergence tolerance (1e-8), not to rounding
            np.testing.assert_allclose(x1[:ncmp], x2[:ncmp], rtol=0, atol=1e-8)
        np.testing.assert_allclose(b.R2Y[:ncmp], m_.R2Y[:ncmp], rtol=0, atol=1e-8)
        np.testing.assert_allclose(b.coef_[:ncmp, :ncmp], m_.coef_[:ncmp, :ncmp], rtol=1e-7, atol=1e-9)
    assert np.all(np.isfinite(b.coef_)) and np.all(np.isfinite(Tb))
    if len(Xs) == 1:                                   # (a coupled fit's R2Xs need not increase: tests/test_cmtf.py:27,39)
        assert np.all(np.diff(r2b[0]) >= -1e-9) and r2b[0][-1] <= 1 + 1e-9        # the norm recurrence stays monotone and <= 1
    # the never-write fit leaves its working copy as centred (with `xcov_raw` it would not even be centred: the next test)
    opt["xcov_nowrite"] = True
    opt["xcov_raw"] = False
    import torch
    Xd = torch.from_numpy(Xs[0].copy())
    m = (ctPLS if len(Xs) > 1 else tPLS)(R, backend=NumpyBackend(), algorithm="xcov", copy_X=False, options=default_options().but(**opt))
    if len(Xs) > 1:
        m.fit([Xd] + Xs[1:], Y)
    else:
        m.fit(Xd, Y)
    np.testing.assert_allclose(Xd.numpy(), Xs[0] - Xs[0].mean(axis=0), rtol=0, atol=1e-13)


@pytest.mark.parametrize("case", ["tpls3", "tpls4", "matrix", "declined", "more_components_than_rank", "coupled2", "coupled3"])
def test_xcov_one_read_per_component_equals_two_reads(case, monkeypatch):
    """The final score of the largest block and r_a = X_0^T t_a from ONE read of it (score_contract), its down-date vector
    X_0^T yhat = sum_j b_j r_j from the kept r_j instead of a second read (FitRun._finish_xcov_nowrite); with coupled blocks the
    kernel is handed the other blocks' scores and contracts with the block average.  Same fit as with the two reads
    (NipalsEngine.xcov_one_read = False); "declined": the backend refuses the shape and the engine makes the two passes."""
    opt = {}                                              # EngineOptions fields this test overrides
    rng = np.random.default_rng(78)
    R = 4
    shape = {"tpls3": (30, 7, 6), "tpls4": (30, 6, 5, 4), "matrix": (30, 24), "declined": (30, 7, 5),
             "more_components_than_rank": (30, 7, 6), "coupled2": (30, 7, 6), "coupled3": (30, 7, 6)}[case]
    if case == "more_components_than_rank":
        x, _, _ = O.import_synthetic(shape, 3, 2, error=0.0, seed=3)
    else:
        x = rng.random(shape) + 3.0
    blocks = [x]
    if case.startswith("coupled"):
        blocks = [rng.random((30, 9)) - 1.0, x] + ([rng.random((30, 3, 4))] if case == "coupled3" else [])   # the largest is not the first
    Y = rng.random((30, 3))
    calls = {"n": 0, "took": 0, "P": set()}
    orig = NumpyBackend.score_contract

    def counted(self, X2, *a, **kw):
        out = orig(self, X2, *a, **kw)
        calls["n"] += 1
        calls["took"] += out is not None
        calls["P"].add(X2.shape[1])
        return out
    monkeypatch.setattr(NumpyBackend, "score_contract", counted)

    def fit(one_read):
        opt["xcov_one_read"] = one_read
        m = (ctPLS if len(blocks) > 1 else tPLS)(R, backend=NumpyBackend(), algorithm="xcov", options=default_options().but(**opt))
        m.fit(blocks if len(blocks) > 1 else x, Y)
        return m

    two = fit(False)
    assert calls["n"] == 0
    one = fit(True)
    if case == "declined":
        assert (calls["n"], calls["took"]) == (1, 0)             # asked once, refused, not asked again
    else:
        assert (calls["n"], calls["took"]) == (R - 1, R - 1)     # the last component needs no down-date
        assert calls["P"] == {int(np.prod(shape[1:]))}           # ... and only the largest block is read this way
    ncmp = 2 if case == "more_components_than_rank" else R
    assert one.n_iter_[:ncmp] == two.n_iter_[:ncmp]
    if len(blocks) > 1:
        f1 = [one.factor_T] + [f for fs in one.Xs_factors for f in fs[1:]] + list(one.Y_factors)
        f2 = [two.factor_T] + [f for fs in two.Xs_factors for f in fs[1:]] + list(two.Y_factors)
        r1, r2 = np.concatenate(one.R2Xs), np.concatenate(two.R2Xs)
    else:
        f1, f2, r1, r2 = one.X_factors + one.Y_factors, two.X_factors + two.Y_factors, one.R2X, two.R2X
    for f, g in zip(f1, f2):
        np.testing.assert_allclose(f[:, :ncmp], g[:, :ncmp], rtol=1e-9, atol=1e-10)
    if len(blocks) == 1:
        np.testing.assert_allclose(r1[:ncmp], r2[:ncmp], rtol=0, atol=1e-10)
    else:
        np.testing.assert_allclose(r1, r2, rtol=0, atol=1e-10)
    np.testing.assert_allclose(one.R2Y[:ncmp], two.R2Y[:ncmp], rtol=0, atol=1e-10)
    np.testing.assert_allclose(one.coef_[:ncmp, :ncmp], two.coef_[:ncmp, :ncmp], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("stats_with_s", [True, False])
@pytest.mark.parametrize("case", ["tpls3", "coupled", "matrix"])
def test_xcov_on_the_uncentred_tensor_equals_the_centred_form_cpu(case, stats_with_s, monkeypatch):
    """NipalsEngine.xcov_raw through the NumPy backend: the fit reads the caller's uncentred blocks (never written, never centred)
    and applies the centring algebraically; |X - X_mean|^2 comes out of the S-build read (xcov_ssq) -- and since round 4 the
    column statistics too (xcov_stats: ONE read of a block before its first component; stats_with_s = False keeps the
    statistics pass and xcov_ssq).  Same fit as on centred copies."""
    opt = {"xcov_stats_with_s": stats_with_s}             # EngineOptions fields this test overrides
    import torch
    rng = np.random.default_rng(5)
    x, y, cp = O.import_synthetic((40, 6, 5), 3, 3, error=0.2, seed=8)
    x = x + 5.0
    xm = cp.factors[0] @ rng.normal(size=(7, 3)).T - 2.0
    blocks = {"tpls3": [x], "coupled": [x, xm], "matrix": [xm]}[case]
    coupled = len(blocks) > 1
    calls = {"xcov_ssq": 0, "xcov_stats": 0, "center": 0, "colstats": 0}
    for name in calls:
        orig = getattr(NumpyBackend, name)

        def counted(self, *a, __orig=orig, __name=name, **k):
            calls[__name] += 1
            return __orig(self, *a, **k)
        monkeypatch.setattr(NumpyBackend, name, counted)

    def fit(raw):
        opt["xcov_raw"] = raw
        held = [torch.from_numpy(b.copy()) for b in blocks]
        m = (ctPLS if coupled else tPLS)(3, backend=NumpyBackend(), algorithm="xcov", copy_X=False, options=default_options().but(**opt))
        m.fit(held if coupled else held[0], y)
        return m, held

    raw, held = fit(True)
    assert calls["center"] == 1                                                # (the one centring call is Y's)
    if stats_with_s:
        assert calls["xcov_stats"] == len(blocks) and calls["xcov_ssq"] == 0 and raw.fit_report_["stats_with_s"] is True
    else:
        assert calls["xcov_ssq"] == len(blocks) and calls["xcov_stats"] == 0 and raw.fit_report_["stats_with_s"] is False
    for h, b in zip(held, blocks):
        assert np.array_equal(h.numpy(), b)                                    # the caller's blocks: same bits afterwards
    cen, _ = fit(False)
    assert raw.n_iter_ == cen.n_iter_
    f1 = ([raw.factor_T] + [f for fs in raw.Xs_factors for f in fs[1:]]) if coupled else raw.X_factors
    f2 = ([cen.factor_T] + [f for fs in cen.Xs_factors for f in fs[1:]]) if coupled else cen.X_factors
    for f, g in zip(f1 + list(raw.Y_factors), f2 + list(cen.Y_factors)):
        np.testing.assert_allclose(f, g, rtol=1e-9, atol=1e-10)
    for a, b in zip(raw.R2Xs if coupled else [raw.R2X], cen.R2Xs if coupled else [cen.R2X]):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-10)
    np.testing.assert_allclose(raw.R2Y, cen.R2Y, rtol=0, atol=1e-10)


class _StingyBackend(NumpyBackend):
    """A rank-1 extraction that fails (garbage loadings, convergence flag 0) whenever it is given fewer squarings than the maximum:
    every iteration after the first has to redo its tail -- the retry path of both inner loops."""
    retries = 0

    def rank1(self, Z, A, B, wA, wB, info=None, n_squarings=None):
        if n_squarings is not None and n_squarings < self.rank1_squarings:
            type(self).retries += 1
            wA.fill_(float("nan"))
            wB.fill_(float("nan"))
            info[0], info[1] = 0.0, float(n_squarings)
            return
        super().rank1(Z, A, B, wA, wB, info=info, n_squarings=n_squarings)
        info[1] = 3.0                                             # "3 squarings were enough": the next budget is 4 < max


@pytest.mark.parametrize("backend", [NumpyBackend, _StingyBackend])
@pytest.mark.parametrize("max_iter", [100, 1, 2, 5])
def test_xcov_pipelined_inner_loop_is_bit_identical_to_the_waiting_loop(backend, max_iter, monkeypatch):
    """FitRun._inner_loop_xcov_pipelined enqueues iteration it + 1 before the host has seen iteration it's norm (second buffer
    set, three q buffers): same kernels on the same data in the same order as the loop that waits after every iteration --
    identical bits, identical iteration counts, also when max_iter cuts the loop and when tails have to be redone."""
    opt = {}                                              # EngineOptions fields this test overrides
    x, y, _ = O.import_synthetic((60, 9, 7), 4, 3, error=0.3, seed=11)

    def fit(pipeline):
        opt["xcov_pipeline"] = pipeline
        backend.retries = 0
        m = tPLS(4, backend=backend(), algorithm="xcov", options=default_options().but(**opt))
        m.fit(x, y, max_iter=max_iter)
        return m, backend.retries

    wait, r_wait = fit(False)
    pipe, r_pipe = fit(True)
    assert pipe.n_iter_ == wait.n_iter_ and max(wait.n_iter_) <= max_iter
    if backend is _StingyBackend and max_iter > 1:
        assert r_wait > 0 and r_pipe > 0                          # (how many differs: the pipelined budget is one iteration older)
    for f, g in zip(pipe.X_factors + pipe.Y_factors, wait.X_factors + wait.Y_factors):
        assert np.array_equal(f, g)
    assert np.array_equal(pipe.coef_, wait.coef_) and np.array_equal(pipe.R2X, wait.R2X) and np.array_equal(pipe.R2Y, wait.R2Y)
    if max_iter == 100:
        ref = O.fit_tpls(x, y, 4)
        assert pipe.n_iter_ == ref.n_iter
        np.testing.assert_allclose(pipe.X_factors[0], ref.T, rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("case", ["coupled", "coupled_nan", "nan", "matrix", "coupled3"])
def test_xcov_pipelined_inner_loop_for_coupled_and_masked_blocks(case, monkeypatch):
    """The pipelined inner loop through the several-blocks entry (backend.xcov_blocks_plan: coupled blocks, blocks with missing
    values, matrix blocks): same iteration counts and factors as the loop that waits after every iteration, and as the oracle."""
    opt = {}                                              # EngineOptions fields this test overrides
    rng = np.random.default_rng(21)
    x, y, cp = O.import_synthetic((50, 8, 6), 3, 3, error=0.2, seed=5)
    xm = cp.factors[0] @ rng.normal(size=(11, 3)).T + 0.2 * rng.normal(size=(50, 11))
    if case in ("coupled_nan", "nan"):
        x = x.copy()
        x[rng.random(x.shape) < 0.15] = np.nan
    blocks = {"coupled": [x, xm], "coupled_nan": [x, xm], "nan": [x], "matrix": [xm],
              "coupled3": [xm, x, rng.normal(size=(50, 4, 5))]}[case]
    coupled = len(blocks) > 1
    used = {"plans": 0}
    orig = NumpyBackend.xcov_blocks_plan

    def counted(self, *a, **k):
        used["plans"] += 1
        return orig(self, *a, **k)
    monkeypatch.setattr(NumpyBackend, "xcov_blocks_plan", counted)

    def fit(pipeline):
        opt["xcov_pipeline"] = pipeline
        m = (ctPLS if coupled else tPLS)(3, backend=NumpyBackend(), algorithm="xcov", options=default_options().but(**opt))
        m.fit(blocks if coupled else blocks[0], y)
        return m

    wait = fit(False)
    assert used["plans"] == 0
    pipe = fit(True)
    assert used["plans"] > 0
    assert pipe.n_iter_ == wait.n_iter_
    f1 = ([pipe.factor_T] + [f for fs in pipe.Xs_factors for f in fs[1:]]) if coupled else pipe.X_factors
    f2 = ([wait.factor_T] + [f for fs in wait.Xs_factors for f in fs[1:]]) if coupled else wait.X_factors
    for f, g in zip(f1 + list(pipe.Y_factors), f2 + list(wait.Y_factors)):
        np.testing.assert_allclose(f, g, rtol=1e-12, atol=1e-13)
    ref = O.fit_ctpls(blocks, y, 3) if coupled else O.fit_tpls(blocks[0], y, 3)
    assert pipe.n_iter_ == ref.n_iter
    np.testing.assert_allclose(f1[0], ref.T, rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("coupled", [False, True])
def test_xcov_masked_blocks_build_both_cross_covariances_in_one_pass(coupled, monkeypatch):
    """A block with missing values needs S = X0^T Y (contraction) and S2 = X0^T (Y * rowscale) (the masked score's P / n_obs(i)
    folded into Y): with 2 M <= 64 both are the halves of ONE xcov pass over X with [Y, Y * rowscale]; same fit as two passes."""
    opt = {}                                              # EngineOptions fields this test overrides
    rng = np.random.default_rng(9)
    x = rng.random((40, 6, 5))
    x[rng.random(x.shape) < 0.2] = np.nan
    blocks = [x, rng.random((40, 8))] if coupled else [x]         # (the NaN-free block keeps its single S)
    Y = rng.random((40, 3))
    passes = {"n": 0, "widths": []}
    orig = NumpyBackend.xcov

    def counted(self, X2, Yd, *a, **k):
        passes["n"] += 1
        passes["widths"].append(Yd.shape[1])
        return orig(self, X2, Yd, *a, **k)
    monkeypatch.setattr(NumpyBackend, "xcov", counted)

    def fit(pair):
        opt["xcov_pair_build"] = pair
        passes["n"], passes["widths"] = 0, []
        m = (ctPLS if coupled else tPLS)(3, backend=NumpyBackend(), algorithm="xcov", options=default_options().but(**opt))
        m.fit(blocks if coupled else x, Y)
        return m, passes["n"], set(passes["widths"])

    two, n2, w2 = fit(False)
    one, n1, w1 = fit(True)
    assert w2 == {3} and w1 == ({6, 3} if coupled else {6})
    assert n2 - n1 == 3                                           # one pass less per component for the masked block
    assert one.n_iter_ == two.n_iter_
    f1 = ([one.factor_T] + [f for fs in one.Xs_factors for f in fs[1:]]) if coupled else one.X_factors
    f2 = ([two.factor_T] + [f for fs in two.Xs_factors for f in fs[1:]]) if coupled else two.X_factors
    for f, g in zip(f1 + list(one.Y_factors), f2 + list(two.Y_factors)):
        np.testing.assert_allclose(f, g, rtol=1e-12, atol=1e-13)
    fit_o = O.fit_ctpls(blocks, Y, 3) if coupled else O.fit_tpls(x, Y, 3)
    assert one.n_iter_ == fit_o.n_iter
    np.testing.assert_allclose(f1[0], fit_o.T, rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("case", ["tpls3", "tpls4", "matrix", "coupled"])
def test_one_pass_projection_equals_sequential(case):
    """transform/predict through one MTTKRP + R x R triangular solve == R project-and-deflate passes."""
    from cmtf_pls_amd.tpls import to_device_copy
    rng = np.random.default_rng(41)
    if case == "coupled":
        Xs = [rng.random((15, 6, 5, 4)), rng.random((15, 7, 3)), rng.random((15, 9))]
        Y = rng.random((15, 4))
        m = ctPLS(5, backend=NumpyBackend())
        m.fit(Xs, Y)
        new = [rng.random((8,) + x.shape[1:]) for x in Xs]
        want = O.transform(O.fit_ctpls(Xs, Y, 5), new)
    else:
        shape = {"tpls3": (20, 8, 6), "tpls4": (20, 6, 5, 4), "matrix": (20, 30)}[case]
        X, Y = rng.random(shape), rng.random((20, 4))
        m = tPLS(5, backend=NumpyBackend())
        m.fit(X, Y)
        new = [rng.random((8,) + shape[1:])]
        want = O.transform(O.fit_tpls(X, Y, 5), new[0])
    eng = m._get_engine()
    dev = lambda xs: [to_device_copy(x, torch.float64, "cpu") for x in xs]
    one = eng.project(m._state, dev(new), one_pass=True).numpy()
    seq = eng.project(m._state, dev(new), one_pass=False).numpy()
    np.testing.assert_allclose(one, seq, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(one, want, rtol=1e-7, atol=1e-9)


def test_get_q2y_leave_one_out():
    """validate.get_q2y (validate.py:7-37) against a literal LOO loop over the oracle."""
    from cmtf_pls_amd.validate import get_q2y
    x, y, _ = O.import_synthetic((14, 5, 4), 2, 2, error=0.3, seed=6)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    got = get_q2y(m)
    pred = np.zeros_like(y)
    for i in range(14):
        keep = np.arange(14) != i
        pred[i] = O.predict(O.fit_tpls(x[keep], y[keep], 2), x[i:i + 1])[0]
    want = 1 - ((pred - y) ** 2).sum() / (y ** 2).sum()
    np.testing.assert_allclose(got, want, rtol=1e-8)


def test_miss_attributes_lazy():
    rng = np.random.default_rng(3)
    x, y = rng.random((12, 4, 3)), rng.random((12, 2))
    x[2, 1, 1] = np.nan
    m = tPLS(1, backend=NumpyBackend())
    m.fit(x, y)
    assert m.X_hasMiss and m.X_miss.shape == x.shape and m.X_miss[2, 1, 1] and m.X_miss.sum() == 1
    c = ctPLS(1, backend=NumpyBackend())
    c.fit([x], y)
    assert c.Xs_hasMiss == [True] and c.Xs_miss[0][2, 1, 1]


def _random_case(seed):
    rng = np.random.default_rng(seed)
    order = int(rng.integers(2, 6))
    I = int(rng.integers(8, 25))
    dims = tuple(int(rng.integers(2, 6)) for _ in range(order - 1))
    M = int(rng.integers(1, 5))
    X = rng.normal(size=(I,) + dims)
    Y = rng.normal(size=(I, M)) if M > 1 or rng.random() < 0.5 else rng.normal(size=I)
    if rng.random() < 0.4:
        X[rng.random(X.shape) < 0.15] = np.nan
    R = int(rng.integers(1, 4))
    algorithm = "xcov" if rng.random() < 0.5 else "direct"
    coupled = rng.random() < 0.35
    return X, Y, R, algorithm, coupled, rng


@pytest.mark.parametrize("seed", range(16))
def test_random_problems_match_oracle(seed):
    """Random orders (2-5), NaNs, 1-D or 2-D Y, tPLS or ctPLS (with an extra matrix block), both
    algorithms: engine + NumPy backend == oracle (factors up to the paired sign, R2, iteration counts)."""
    X, Y, R, algorithm, coupled, rng = _random_case(seed)
    if coupled:
        Xm = rng.normal(size=(X.shape[0], int(rng.integers(2, 7))))
        m = ctPLS(R, backend=NumpyBackend(), algorithm=algorithm)
        m.fit([X, Xm], Y)
        fit = O.fit_ctpls([X, Xm], Y, R)
        T, r2x = m.factor_T, m.R2Xs[0]
        new = [X[::2].copy(), Xm[::2].copy()]
        tr, want_tr = m.transform(new), O.transform(fit, new)
    else:
        m = tPLS(R, backend=NumpyBackend(), algorithm=algorithm)
        m.fit(X, Y)
        fit = O.fit_tpls(X, Y, R)
        T, r2x = m.X_factors[0], m.R2X
        tr, want_tr = m.transform(X[::2]), O.transform(fit, X[::2])
    ok = ~np.isnan(fit.T).any()
    if not ok:                       # an all-NaN row makes the reference itself produce NaN scores
        assert np.isnan(T).any()
        return
    assert list(m.n_iter_) == list(fit.n_iter)
    np.testing.assert_allclose(T, fit.T, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(m.Y_factors[1], fit.Q, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(m.coef_, fit.coef, rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(r2x, fit.r2x[0], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(m.R2Y, fit.r2y, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(tr, want_tr, rtol=1e-6, atol=1e-8)


def test_stdout_side_effects_follow_the_reference_order(capsys):
    """tpls.py:62-63 prints the missing-value notice during preprocess, tpls.py:104-105 the 0-based break index per
    component under verbose; cmtf.py:78-79, 125-126 likewise."""
    x, y, _ = O.import_synthetic((40, 6, 5), 2, 2, error=0.1, seed=8)
    x[3, 2, 1] = np.nan
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y, verbose=1)
    out = capsys.readouterr().out.strip().splitlines()
    assert out[0] == "X has missing values"
    assert [ln.split(":")[0] for ln in out[1:]] == ["Comp 0", "Comp 1"]
    assert out[1] == "Comp 0: converged after {} iterations".format(m.n_iter_[0] - 1)
    c = ctPLS(2, backend=NumpyBackend())
    c.fit([x, x[:, :, 0]], y)
    assert capsys.readouterr().out.strip().splitlines()[0] == "At least one X has missing values"
    q = tPLS(2, backend=NumpyBackend())
    q.fit(np.nan_to_num(x), y)
    assert capsys.readouterr().out == ""


def test_limits_are_validated_before_the_backend_is_touched():
    """VERDICT r2 #4 / ADVICE r2: a fit the kernels cannot finish is refused BEFORE the first sweep (round 2 found out after
    the centring pass, or after 64 components of work)."""
    from cmtf_pls_amd import engine

    class Untouchable:
        name = "none"

        device = None                     # (read by device_ctx: not a kernel)

        def __getattr__(self, item):
            raise AssertionError(f"backend.{item} was reached before the limits were checked")

    eng = engine.NipalsEngine(Untouchable())
    Y = torch.zeros(6, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="n_components"):
        eng.begin([torch.zeros(6, 3, 3)], Y, engine.MAX_COMPONENTS + 1, coupled=False)
    with pytest.raises(ValueError, match="n_components"):
        eng.begin([torch.zeros(6, 3, 3)], Y, 0, coupled=False)
    with pytest.raises(NotImplementedError, match="order > 8"):
        eng.begin([torch.zeros(6, 2, 2, 2, 2, 2, 2, 2, 2)], Y, 1, coupled=False)
    with pytest.raises(ValueError, match="rank-1 kernel"):
        engine.validate_limits([(6, engine.MAX_RANK1_SIDE + 1, engine.MAX_RANK1_SIDE + 5)], 2)
    with pytest.raises(ValueError, match="trailing mode"):
        engine.validate_limits([(6, 4, engine.MAX_TENSOR_MODE + 1, 3)], 2)
    engine.validate_limits([(6, engine.MAX_RANK1_SIDE, 10 ** 6), (6, 10 ** 7)], engine.MAX_COMPONENTS)   # a long side / a wide matrix are fine


def test_fit_with_more_than_64_components_numpy_backend():
    """The engine's control flow for n_components > 64 (inner regression beyond the one-workgroup LDS solve, one-pass
    projection declined, xcov keeping the deflating form) against the oracle, through the NumPy backend."""
    rng = np.random.default_rng(3)
    x, y = rng.normal(size=(90, 9, 9)), rng.normal(size=(90, 2))
    R = 66
    fit = O.fit_tpls(x, y, R)
    for algorithm in ("direct", "xcov"):
        m = tPLS(R, backend=NumpyBackend(), algorithm=algorithm)
        m.fit(x, y)
        np.testing.assert_allclose(m.R2X, fit.r2x[0], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(m.R2Y, fit.r2y, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(m.transform(x), m.X_factors[0], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("order", [2, 3])
def test_small_fit_of_a_singleton_first_trailing_mode_takes_parafacs_sign(order):
    """cmtfpls_fit_small_f64 treats A == 1 as a vector (wA = 1, wB = Z / |Z|, unsigned: tpls.py:84).  For an order-3 block
    (I, 1, B) the engine turns that into parafac's sign, as the regular engine and the oracle give it: wB's largest-|.| entry
    positive, wA = -1 where that flips wB.  An order-2 block keeps the unsigned vector."""
    from cmtf_pls_amd import engine

    I, B, R = 5, 4, 3
    WB = torch.tensor([[0.5, -0.1, 0.6], [-0.7, 0.2, -0.6], [0.1, -0.9, 0.0], [0.3, 0.1, 0.4]], dtype=torch.float64)

    class KernelOutput:                   # what the kernel's A == 1 branch hands back
        name = "stub"
        device = None

        def fit_small(self, X2, Y, A, B_, R_, tol, max_iter):
            assert A == 1 and B_ == B and R_ == R
            z = lambda *s: torch.zeros(*s, dtype=torch.float64)
            return {"T": z(I, R), "U": z(I, R), "WA": torch.ones(1, R, dtype=torch.float64), "WB": WB.clone(), "Q": z(2, R),
                    "x_mean": z(B), "y_mean": z(2), "coef": np.eye(R), "ssq": np.ones((R + 1, 2)), "n_iter": [2] * R}

    eng = engine.NipalsEngine(KernelOutput(), options=engine.EngineOptions(small_fit=True))
    X = torch.zeros((I, 1, B) if order == 3 else (I, B), dtype=torch.float64)
    st = eng._fit_small([X], torch.zeros(I, 2, dtype=torch.float64), R, 1e-8, 100, False, 0, None)
    loads = [L.numpy() for L in st.blocks[0].loadings]
    if order == 2:
        assert len(loads) == 1 and np.array_equal(loads[0], WB.numpy())
        return
    # largest |.| per column: -0.7 (row 1, flipped), -0.9 (row 2, flipped), 0.6 / -0.6 tie (row 0 first, kept)
    sgn = np.array([-1.0, -1.0, 1.0])
    assert np.array_equal(loads[0], sgn[None, :]) and np.array_equal(loads[1], WB.numpy() * sgn)
    assert np.array_equal(loads[0] * loads[1], WB.numpy())          # wA (x) wB, hence every score, is unchanged


def _oracle_of(m):
    """OracleFit carrying the model's OWN factors and means: O.transform then centres first and runs the reference's
    sequence in float64 NumPy (tpls.py:151-165)."""
    R = m.n_components
    return O.OracleFit(coupled=False, n_components=R, block_shapes=[m.X_shape], y_shape=m.Y_shape, T=m.X_factors[0],
                       loadings=[list(m.X_factors[1:])], U=m.Y_factors[0], Q=m.Y_factors[1], coef=m.coef_,
                       r2x=[np.zeros(R)], r2y=m.R2Y, x_means=[m.X_mean], y_mean=m.Y_mean, has_miss=[False])


@pytest.mark.parametrize("offset,centred", [(20.0, False), (1e6, True), (1e10, True)])
def test_transform_of_badly_offset_rows_centres_them_first(offset, centred):
    """The one-pass transform computes X W - 1 (mean^T W)^T on the caller's uncentred rows: error ~ 1e-16 * max|mean| / spread.
    Beyond `project_raw_max_offset` (1e4, estimated from <= 256 rows, NaN-aware) the rows are centred first, and transform
    matches the reference's centre-then-project to 1e-9 -- on new rows and on the training rows (the fitted scores)."""
    rng = np.random.default_rng(17)
    x = rng.normal(size=(80, 6, 5)) + offset
    y = rng.normal(size=(80, 3))
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    new = rng.normal(size=(9, 6, 5)) + offset
    new[2, 1, 3] = np.nan                                          # NaN-aware probe; the row takes the masked sequence
    fit = _oracle_of(m)
    got = m.transform(new)
    rep = m.projection_report_
    assert (rep["offset_ratio"] > 1e4) == centred, rep
    assert rep["form"].startswith("one-pass MTTKRP") != centred, rep
    if centred:
        assert rep["why"].startswith("max|column mean| / spread"), rep
    tol = 1e-9 * np.abs(fit.T).max()
    np.testing.assert_allclose(got, O.transform(fit, new), rtol=0, atol=tol)
    np.testing.assert_allclose(m.transform(x), m.X_factors[0], rtol=0, atol=tol)
    np.testing.assert_allclose(m.predict(x[:5]), O.predict(fit, x[:5]), rtol=0, atol=1e-9 * np.abs(y).max())
    if centred:                                                    # the guard is what kept the digits
        forced = tPLS(3, backend=NumpyBackend(), options=default_options().but(project_raw_max_offset=float("inf")))
        forced.fit(x, y)
        raw = forced.transform(x[:40])
        assert forced.projection_report_["form"].startswith("one-pass MTTKRP (one read"), forced.projection_report_
        err = np.abs(raw - forced.X_factors[0][:40]).max() / np.abs(forced.X_factors[0]).max()
        print(f"offset {offset:g}: uncentred one-pass transform {err:.2e} normwise off the fitted scores")
        if offset >= 1e10:
            assert err > 1e-9


def test_projection_report_names_the_mttkrp_decline_without_missing_values():
    """A complete batch the MTTKRP declines (R > 32) must not be reported as having missing values."""
    from cmtf_pls_amd.tpls import to_device_copy
    rng = np.random.default_rng(3)
    m = tPLS(4, backend=NumpyBackend())
    m.fit(rng.normal(size=(30, 5, 4)), rng.normal(size=(30, 2)))
    eng = m._get_engine()
    eng.be.project_rows = lambda X2, A, B, WA, WB, mean, out, rows=None: None if rows is not None else out.zero_()
    try:
        eng.be.mttkrp = lambda *a, **k: None                      # the MTTKRP declines the shape
        got = eng.project_readonly(m._state, [to_device_copy(rng.normal(size=(6, 5, 4)), torch.float64, "cpu")])
    finally:
        del eng.be.project_rows, eng.be.mttkrp
    rep = eng.last_projection
    assert got is not None and rep["form"] == "masked sequence, every row in registers (one read)", rep
    assert rep["why"] == "one-pass MTTKRP declined: loadings beyond its LDS", rep
