"""NumPy float64 restatement of ONE model of cmtfpls_cv_masked_models_f64 (csrc/cv_masked.hip, its count-weighted form) -- TEST
INFRASTRUCTURE ONLY.  Row r of X appears c_r times in the model's training data, paired with Y row yrow[r]; every sum over rows is
weighted by c_r, with the reference's missing-value arithmetic (missingvals.py:7-38) when some column has fewer weighted
observations than n = sum c_r.  The rows with c_r = 0 are predicted as one batch, centred and then masked (tpls.py:122-143).
The rank-1 step is the oracle's, so the result can be compared with oracle.fit_tpls on the literally duplicated rows."""
import numpy as np

import oracle as O


def weighted_masked_fit(X, Y, c, R, yrow=None, tol=1e-8, max_iter=100):
    """Returns (loadings [(dim, R) per trailing mode], Q (M, R), coef (R, R), pred (R, n_held, M) of the rows with c = 0 with the
    first r = 1..R components, n_iter)."""
    I = X.shape[0]
    X2 = np.asarray(X, np.float64).reshape(I, -1)
    P = X2.shape[1]
    Yp = np.asarray(Y, np.float64).reshape(I, -1)[np.arange(I) if yrow is None else np.asarray(yrow)]
    M = Yp.shape[1]
    c = np.asarray(c, np.float64)
    n = c.sum()
    tr = c > 0
    obs = ~np.isnan(X2)
    cp = (c[:, None] * obs).sum(axis=0)                                       # c_p
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = (c @ np.where(obs, X2, 0.0)) / cp                                # np.nanmean over the duplicated rows (NaN at c_p = 0)
    nu = (c @ Yp) / n
    miss = bool((cp < n).any())                                               # X_hasMiss of the duplicated rows
    Xf = np.where(obs & tr[:, None], X2 - mu, 0.0)
    Yf = np.where(tr[:, None], Yp - nu, 0.0)
    o = obs.sum(axis=1)
    shape = X.shape[1:]
    loadings = [np.zeros((d, R)) for d in shape]
    T, Q, coef, n_iter = np.zeros((I, R)), np.zeros((M, R)), np.zeros((R, R)), []
    for a in range(R):
        u = Yf[:, 0].copy()
        old = np.full(I, np.inf)
        for it in range(max_iter):
            s = Xf.T @ (c * u)
            if miss:
                s = np.where(cp > 0, s / np.where(cp > 0, cp, 1.0) * n, 0.0)   # miss_tensordot
            fac = O.rank1_factors(s.reshape(shape), tol)
            w = O.nipals_oracle._kron_all(fac)
            t = Xf @ w
            if miss:
                t = t / np.where(tr, o, 1) * P                                 # miss_mmodedot
            t[~tr] = 0.0
            q = Yf.T @ (c * t)
            q = q / np.linalg.norm(q)
            u = Yf @ q
            if np.sqrt(np.sum(c[tr] * (old[tr] - u[tr]) ** 2)) < tol:      # held-out rows: c = 0, u = 0
                break
            old = u
        n_iter.append(it + 1)
        for m, f in enumerate(fac):
            loadings[m][:, a] = np.asarray(f).ravel()
        T[:, a], Q[:, a] = t, q
        Xf = Xf - np.where(obs & tr[:, None], np.outer(t, w), 0.0)
        sc = np.sqrt(c)
        coef[:, a] = np.linalg.lstsq(sc[:, None] * T, sc * u, rcond=-1)[0]
        Yf = Yf - T @ coef[:, [a]] @ q[None, :]
    # the held-out batch
    Xh = X2[~tr] - mu
    mh = np.isnan(Xh)
    hm = bool(mh.any())
    Xh = np.where(mh, 0.0, Xh)
    oh = (~mh).sum(axis=1)
    S = np.zeros((Xh.shape[0], R))
    for a in range(R):
        w = O.nipals_oracle._kron_all([L[:, a] for L in loadings])
        s = Xh @ w
        with np.errstate(divide="ignore", invalid="ignore"):
            S[:, a] = s / oh * P if hm else s
        Xh = Xh - np.where(mh, 0.0, np.outer(S[:, a], w)) if hm else Xh - np.outer(S[:, a], w)
    pred = np.stack([(S[:, :r] @ coef[:r, :r]) @ Q[:, :r].T + nu for r in range(1, R + 1)])
    return loadings, Q, coef, pred, n_iter
