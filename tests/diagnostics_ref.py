"""Float64 NumPy restatement of validate.sample_diagnostics for the tests, built from a fitted model's own loadings and means:
the sequential masked project-and-deflate of new samples (tpls.py:128-142, missingvals.py:23-38, cmtf.py:143-177), then the
explicit residual e = (X - mean) - T W^T over the finite entries of X - mean, and the limits written out with scipy.stats."""
import numpy as np
from scipy import stats


def _model(m):
    if hasattr(m, "Xs_factors"):
        return True, [f[1:] for f in m.Xs_factors], list(m.Xs_mean)
    return False, [m.X_factors[1:]], [m.X_mean]


def _kr(loads):
    """(P, R) Khatri-Rao product of the trailing-mode loadings, the first mode varying slowest (C order of X.shape[1:])."""
    W = loads[0]
    for L in loads[1:]:
        W = (W[:, None, :] * L[None, :, :]).reshape(-1, W.shape[1])
    return W


def project(m, blocks):
    coupled, loads, means = _model(m)
    I = blocks[0].shape[0]
    work = [np.asarray(X, dtype=np.float64).reshape(I, -1) - mu.ravel() for X, mu in zip(blocks, means)]
    miss = [np.isnan(x) for x in work]
    R = m.n_components
    T = np.zeros((I, R))
    for a in range(R):
        per = []
        for x, ms, L in zip(work, miss, loads):
            w = _kr([l[:, a:a + 1] for l in L])[:, 0]
            if ms.any():
                obs = ~ms
                with np.errstate(divide="ignore", invalid="ignore"):
                    per.append(np.where(obs, x, 0.0) @ w / obs.sum(axis=1) * w.size)
            else:
                per.append(x @ w)
        T[:, a] = np.mean(per, axis=0) if coupled else per[0]
        for b, L in enumerate(loads):
            w = _kr([l[:, a:a + 1] for l in L])[:, 0]
            work[b] = work[b] - np.outer(T[:, a], w)
    return T


def residuals(m, blocks, T):
    """Per block: (spe, ssq, n_observed, r2x_per_variable) with scores T."""
    _, loads, means = _model(m)
    out = []
    for X, L, mu in zip(blocks, loads, means):
        I = X.shape[0]
        x = np.asarray(X, dtype=np.float64).reshape(I, -1) - mu.ravel()
        fin = np.isfinite(x)
        e = np.where(fin, x - T @ _kr(L).T, 0.0)
        x0 = np.where(fin, x, 0.0)
        ce, cx = (e * e).sum(axis=0), (x0 * x0).sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            r2v = np.where(cx > 0, 1 - ce / cx, np.nan)
        out.append(((e * e).sum(axis=1), (x0 * x0).sum(axis=1), fin.sum(axis=1).astype(float), r2v.reshape(X.shape[1:])))
    return out


def limits(T_train, spe_train, R, level, new):
    I = T_train.shape[0]
    t2 = (I - 1) ** 2 / I * stats.beta.ppf(level, R / 2, (I - R - 1) / 2) if not new else \
        R * (I - 1) * (I + 1) / (I * (I - R)) * stats.f.ppf(level, R, I - R)
    m, v = spe_train.mean(), spe_train.var(ddof=1)
    return t2, v / (2 * m) * stats.chi2.ppf(level, 2 * m * m / v)


def check_against_restatement(m, X, y, d, rtol, new, Xn=None, yn=None, level=0.95):
    coupled, _, _ = _model(m)
    blocks = list(X) if coupled else [X]
    T_fit = m.factor_T if coupled else m.X_factors[0]
    if new:
        nblocks = list(Xn) if coupled else [Xn]
        T = project(m, nblocks)
        np.testing.assert_allclose(d["scores"], T, rtol=rtol, atol=rtol * np.abs(T).max())
        want = residuals(m, nblocks, T)
        Y = yn
    else:
        T = T_fit
        np.testing.assert_array_equal(d["scores"], T)
        want = residuals(m, blocks, T)
        Y = y
    train = residuals(m, blocks, T_fit)
    got = [d[k] if coupled else [d[k]] for k in ("spe", "ssq", "n_observed", "r2x_per_variable", "spe_limit")]
    for b, (spe, ssq, nobs, r2v) in enumerate(want):
        np.testing.assert_allclose(got[0][b], spe, rtol=rtol, atol=rtol * spe.max())
        np.testing.assert_allclose(got[1][b], ssq, rtol=rtol)
        np.testing.assert_array_equal(got[2][b], nobs)
        np.testing.assert_allclose(got[3][b], r2v, rtol=rtol, atol=rtol)
        t2_lim, spe_lim = limits(T_fit, train[b][0], m.n_components, level, new)
        np.testing.assert_allclose(got[4][b], spe_lim, rtol=max(rtol, 1e-9) * 100)
        np.testing.assert_allclose(d["t2_limit"], t2_lim, rtol=1e-12)
    Tc = T_fit - T_fit.mean(axis=0)
    S = Tc.T @ Tc / (T_fit.shape[0] - 1)
    Z = T - T_fit.mean(axis=0)
    np.testing.assert_allclose(d["t2"], np.einsum("ir,rs,is->i", Z, np.linalg.pinv(S), Z), rtol=rtol * 100, atol=rtol * 100)
    if Y is not None:
        yh = T @ m.coef_ @ m.Y_factors[1].T + m.Y_mean
        np.testing.assert_allclose(d["y_residual"], ((np.asarray(Y, float).reshape(len(yh), -1) - yh) ** 2).sum(axis=1), rtol=rtol * 100)
