"""Float64 NumPy restatement of validate.sample_contributions for the tests, from a fitted model's public attributes only
(X_factors / Xs_factors, X_mean / Xs_mean, transform, the training scores): W materialised, dense e and d, mode sums by reshape
and sum.  Shares no code with the product."""
import numpy as np


def _model(m):
    if hasattr(m, "Xs_factors"):
        return True, [f[1:] for f in m.Xs_factors], list(m.Xs_mean), m.factor_T
    return False, [m.X_factors[1:]], [m.X_mean], m.X_factors[0]


def _kr(loads):
    W = loads[0]
    for L in loads[1:]:
        W = (W[:, None, :] * L[None, :, :]).reshape(-1, W.shape[1])
    return W


def contributions(m, X=None, rows=None, train=None):
    """The dict of sample_contributions (always with the cells).  X=None: the training blocks `train` with the fitted scores."""
    coupled, loads, means, T_fit = _model(m)
    if X is None:
        blocks = list(train) if coupled else [train]
        T = T_fit
    else:
        blocks = list(X) if coupled else [X]
        T = m.transform(X)
    n_all = T.shape[0]
    rows = np.arange(n_all) if rows is None else np.asarray(rows)
    T = T[rows]
    R = T.shape[1]
    tbar = T_fit.mean(axis=0)
    Zc = T_fit - tbar
    S_pinv = np.linalg.pinv(Zc.T @ Zc / (T_fit.shape[0] - 1))
    Z = T - tbar
    g = Z @ S_pinv
    Ws = [_kr(L) for L in loads]
    U = np.eye(R) + np.triu(np.mean([W.T @ W for W in Ws], axis=0), 1)
    h = np.linalg.solve(U, g.T).T
    out = {"rows": rows, "scores": T, "t2": np.einsum("ir,ir->i", g, Z), "t2_closure": np.einsum("ir,ir->i", g, T),
           "spe": [], "spe_mode": [], "t2_mode": [], "spe_cells": [], "t2_cells": [], "abs_d": []}
    for Xb, W, mu in zip(blocks, Ws, means):
        xb = np.asarray(Xb, dtype=np.float64)[rows]
        x = xb.reshape(len(rows), -1) - np.asarray(mu, dtype=np.float64).ravel()
        fin = np.isfinite(x)
        e = np.where(fin, x - T @ W.T, 0.0).reshape(xb.shape)
        d = np.where(fin, x * (h @ W.T) / len(blocks), 0.0).reshape(xb.shape)
        axes = range(1, xb.ndim)
        out["spe"].append((e * e).reshape(len(rows), -1).sum(axis=1))
        out["spe_mode"].append([(e * e).sum(axis=tuple(a for a in axes if a != k)) for k in axes])
        out["t2_mode"].append([d.sum(axis=tuple(a for a in axes if a != k)) for k in axes])
        out["spe_cells"].append(e)
        out["t2_cells"].append(d)
        out["abs_d"].append(np.abs(d).reshape(len(rows), -1).sum(axis=1))
    if not coupled:
        for k in ("spe", "spe_mode", "t2_mode", "spe_cells", "t2_cells", "abs_d"):
            out[k] = out[k][0]
    return out


def check(got, want, coupled, rtol, score_rtol=None):
    """got (the product) against want (this restatement).  Squared sums relatively; the signed T^2 sums cancel, so they are held to
    rtol of the row's sum of |d| instead of their own size."""
    np.testing.assert_array_equal(got["rows"], want["rows"])
    sr = score_rtol or rtol
    np.testing.assert_allclose(got["scores"], want["scores"], rtol=sr, atol=sr * np.abs(want["scores"]).max())
    np.testing.assert_allclose(got["t2"], want["t2"], rtol=rtol * 100, atol=rtol * 100)
    np.testing.assert_allclose(got["t2_closure"], want["t2_closure"], rtol=rtol * 100, atol=rtol * 100)
    lst = (lambda v: v) if coupled else (lambda v: [v])
    for b, (spe, sm, tm, absd) in enumerate(zip(lst(want["spe"]), lst(want["spe_mode"]), lst(want["t2_mode"]), lst(want["abs_d"]))):
        np.testing.assert_allclose(lst(got["spe"])[b], spe, rtol=rtol, atol=rtol * spe.max())
        assert len(lst(got["spe_mode"])[b]) == len(sm) and len(lst(got["t2_mode"])[b]) == len(tm)
        for k in range(len(sm)):
            assert lst(got["spe_mode"])[b][k].shape == sm[k].shape and lst(got["spe_mode"])[b][k].dtype == np.float64
            np.testing.assert_allclose(lst(got["spe_mode"])[b][k], sm[k], rtol=rtol, atol=rtol * spe.max())
            err = np.abs(lst(got["t2_mode"])[b][k] - tm[k])
            assert (err <= rtol * 100 * (absd[:, None] + 1e-300)).all(), (b, k, float((err / (absd[:, None] + 1e-300)).max()))
