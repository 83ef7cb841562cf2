"""Float64 NumPy restatement of validate.selectivity_ratio and validate.vip_scores for the tests, from a fitted model's public
attributes only: centre first, loop over the responses, dense masks.  No torch, nothing of the package."""
import numpy as np


def _blocks(m):
    if hasattr(m, "Xs_factors"):
        return True, [f[1:] for f in m.Xs_factors], list(m.Xs_mean), m.factor_T
    return False, [m.X_factors[1:]], [m.X_mean], m.X_factors[0]


def f_limit(I, level=0.95):
    from scipy import stats

    return float(stats.f.ppf(level, I - 2, I - 3)) if I > 3 else float("nan")


def sums(X, mean, tau):
    """(a, d, s, n, absxt): the four sums of one block over the finite entries of x = X - mean, and sum_i |x tau| per (m, cell)."""
    X = np.asarray(X, dtype=np.float64)
    x = X.reshape(X.shape[0], -1) - np.asarray(mean, dtype=np.float64).ravel()
    o = np.isfinite(x)
    x0 = np.where(o, x, 0.0)
    M, P = tau.shape[1], x.shape[1]
    a, d, absxt = np.zeros((M, P)), np.zeros((M, P)), np.zeros((M, P))
    for m in range(M):
        t = tau[:, m]
        a[m] = (x0 * t[:, None]).sum(axis=0)
        d[m] = (o * (t * t)[:, None]).sum(axis=0)
        absxt[m] = np.abs(x0 * t[:, None]).sum(axis=0)
    return a, d, (x0 * x0).sum(axis=0), o.sum(axis=0).astype(np.float64), absxt


def ratios(a, d, s, n, shape):
    """The per-cell arrays (M, *shape) and the per-mode ratios of one block, by explicit loops over the slices."""
    M = a.shape[0]
    tp, ex, rs, sr = (np.full(a.shape, np.nan) for _ in range(4))
    for m in range(M):
        for c in range(a.shape[1]):
            if d[m, c] > 0 and n[c] > 0:
                tp[m, c] = a[m, c] / d[m, c]
                ex[m, c] = a[m, c] ** 2 / d[m, c]
                rs[m, c] = max(s[c] - ex[m, c], 0.0)
                if rs[m, c] > 0:
                    sr[m, c] = ex[m, c] / rs[m, c]
                elif ex[m, c] > 0:
                    sr[m, c] = np.inf
    full = (M,) + tuple(shape)
    exf, rsf = ex.reshape(full), rs.reshape(full)
    modes = []
    for k in range(1, len(full)):
        out = np.full((M, full[k]), np.nan)
        for m in range(M):
            for j in range(full[k]):
                e, r = np.take(exf[m], j, axis=k - 1).ravel(), np.take(rsf[m], j, axis=k - 1).ravel()
                ok = np.isfinite(e)
                if ok.any():
                    es, rsum = e[ok].sum(), r[ok].sum()
                    out[m, j] = es / rsum if rsum > 0 else (np.inf if es > 0 else np.nan)
        modes.append(out)
    return tp.reshape(full), ex.reshape(full), rs.reshape(full), sr.reshape(full), modes


def selectivity(m, X=None, train=None, level=0.95):
    """The dict of selectivity_ratio (always with the cells) plus "s" (the column sums of squares) per block.  X=None: the
    training blocks `train` with the fitted scores."""
    coupled, _, means, T_fit = _blocks(m)
    if X is None:
        blocks, T = (list(train) if coupled else [train]), T_fit
    else:
        blocks, T = (list(X) if coupled else [X]), m.transform(X)
    tau = T @ m.coef_ @ m.Y_factors[1].T
    out = {k: [] for k in ("sr", "explained", "residual", "tp_loading", "n_observed", "sr_mode", "s")}
    for Xb, mu in zip(blocks, means):
        shape = np.asarray(Xb).shape[1:]
        a, d, s, n, _ = sums(Xb, mu, tau)
        tp, ex, rs, sr, modes = ratios(a, d, s, n, shape)
        for k, v in zip(("sr", "explained", "residual", "tp_loading", "n_observed", "sr_mode", "s"),
                        (sr, ex, rs, tp, n.reshape(shape), modes, s.reshape(shape))):
            out[k].append(v)
    if not coupled:
        out = {k: v[0] for k, v in out.items()}
    out["f_limit"], out["level"] = f_limit(T_fit.shape[0], level), level
    return out


def vip(m, per_component=False):
    coupled, loads, _, _ = _blocks(m)
    r2y = np.asarray(m.R2Y, dtype=np.float64)
    R = r2y.shape[0]
    w = np.array([max(r2y[r] - (r2y[r - 1] if r else 0.0), 0.0) for r in range(R)])
    out = []
    for L in loads:
        modes = []
        for W in L:
            W = np.asarray(W, dtype=np.float64)
            W = W / np.linalg.norm(W, axis=0)
            J = W.shape[0]
            rows = [np.sqrt(J * (W[:, :p] ** 2 * w[:p]).sum(axis=1) / w[:p].sum()) if w[:p].sum() > 0 else np.full(J, np.nan)
                    for p in range(1, R + 1)]
            modes.append(np.array(rows) if per_component else rows[-1])
        out.append(modes)
    return (out if coupled else out[0]), w


def check(got, want, coupled, rtol):
    """got (the product) against want (this restatement): explained and residual to rtol of the column's s (sr amplifies error
    where the residual is small), sr_mode relatively to rtol, the patterns of NaN / inf equal."""
    lst = (lambda v: v) if coupled else (lambda v: [v])
    assert got["f_limit"] == want["f_limit"] or (np.isnan(got["f_limit"]) and np.isnan(want["f_limit"]))
    for b in range(len(lst(want["s"]))):
        s = lst(want["s"])[b]
        np.testing.assert_array_equal(lst(got["n_observed"])[b], lst(want["n_observed"])[b])
        for key in ("explained", "residual"):
            g, w = lst(got[key])[b], lst(want[key])[b]
            assert g.shape == w.shape and g.dtype == np.float64, key
            assert np.array_equal(np.isnan(g), np.isnan(w)), key
            ok = ~np.isnan(w)
            err = np.abs(np.where(ok, g - w, 0.0))
            assert (err <= rtol * np.broadcast_to(s, w.shape) + 1e-300).all(), (key, b, float((err / (s + 1e-300)).max()))
        g, w = lst(got["tp_loading"])[b], lst(want["tp_loading"])[b]
        assert np.array_equal(np.isnan(g), np.isnan(w))
        if np.isfinite(w).any():
            np.testing.assert_allclose(g, w, rtol=rtol * 100, atol=rtol * 100 * np.nanmax(np.abs(w)))
        g, w = lst(got["sr"])[b], lst(want["sr"])[b]
        assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w))
        gm, wm = lst(got["sr_mode"])[b], lst(want["sr_mode"])[b]
        assert len(gm) == len(wm)
        for g, w in zip(gm, wm):
            assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w))
            fin = np.isfinite(w)
            assert np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)])
            np.testing.assert_allclose(g[fin], w[fin], rtol=rtol, atol=0)
