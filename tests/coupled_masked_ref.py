"""NumPy float64 restatement of ONE model of cmtfpls_cv_masked_coupled_f64 (csrc/cv_masked_coupled.hip) -- TEST
INFRASTRUCTURE ONLY.  Row r of EVERY block appears c_r times in the model's training data, paired with Y row yrow[r]; every sum
over rows is weighted by c_r; a block takes the reference's missing-value arithmetic (missingvals.py:7-38) when one of its columns
has fewer weighted observations than n = sum c_r (Xs_hasMiss per block, cmtf.py:77), a complete block the plain sums; the blocks'
scores are averaged (cmtf.py:119).  The rows with c_r = 0 are predicted as one batch, each block centred and then masked
(cmtf.py:141-175).  The rank-1 step is the oracle's, so the result can be compared with oracle.fit_ctpls on the literally
duplicated rows."""
import numpy as np

import oracle as O


def coupled_masked_fit(Xs, Y, c, R, yrow=None, tol=1e-8, max_iter=100):
    """Returns (loadings per block [(dim, R) per trailing mode], Q (M, R), coef (R, R), pred (R, n_held, M) of the rows with c = 0
    with the first r = 1..R components, n_iter, info = (bit b: block b's training rows masked, bit b: its held-out batch masked))."""
    I = Xs[0].shape[0]
    nb = len(Xs)
    X2 = [np.asarray(X, np.float64).reshape(I, -1) for X in Xs]
    Ps = [x.shape[1] for x in X2]
    shapes = [X.shape[1:] for X in Xs]
    Yp = np.asarray(Y, np.float64).reshape(I, -1)[np.arange(I) if yrow is None else np.asarray(yrow)]
    M = Yp.shape[1]
    c = np.asarray(c, np.float64)
    n = c.sum()
    tr = c > 0
    obs = [~np.isnan(x) for x in X2]
    cp = [(c[:, None] * o).sum(axis=0) for o in obs]                          # c_p per block
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = [(c @ np.where(o, x, 0.0)) / k for x, o, k in zip(X2, obs, cp)]  # np.nanmean over the duplicated rows (NaN at c_p = 0)
    nu = (c @ Yp) / n
    miss = [bool((k < n).any()) for k in cp]                                  # Xs_hasMiss of the duplicated rows, per block
    Xf = [np.where(o & tr[:, None], x - m, 0.0) for x, o, m in zip(X2, obs, mu)]
    Yf = np.where(tr[:, None], Yp - nu, 0.0)
    ro = [o.sum(axis=1) for o in obs]
    loadings = [[np.zeros((d, R)) for d in shape] for shape in shapes]
    T, Q, coef, n_iter = np.zeros((I, R)), np.zeros((M, R)), np.zeros((R, R)), []
    for a in range(R):
        u = Yf[:, 0].copy()
        old = np.full(I, np.inf)
        for it in range(max_iter):
            facs, ws, ts = [], [], []
            for b in range(nb):
                s = Xf[b].T @ (c * u)
                if miss[b]:
                    s = np.where(cp[b] > 0, s / np.where(cp[b] > 0, cp[b], 1.0) * n, 0.0)   # miss_tensordot
                fac = O.rank1_factors(s.reshape(shapes[b]), tol)
                w = O.nipals_oracle._kron_all(fac)
                tb = Xf[b] @ w
                if miss[b]:
                    tb = tb / np.where(tr, ro[b], 1) * Ps[b]                                # miss_mmodedot
                facs.append(fac)
                ws.append(w)
                ts.append(tb)
            t = np.average(ts, axis=0)                                                      # cmtf.py:119
            t[~tr] = 0.0
            q = Yf.T @ (c * t)
            q = q / np.linalg.norm(q)
            u = Yf @ q
            if np.sqrt(np.sum(c[tr] * (old[tr] - u[tr]) ** 2)) < tol:                      # held-out rows: c = 0, u = 0
                break
            old = u
        n_iter.append(it + 1)
        for b in range(nb):
            for m, f in enumerate(facs[b]):
                loadings[b][m][:, a] = np.asarray(f).ravel()
            Xf[b] = Xf[b] - np.where(obs[b] & tr[:, None], np.outer(t, ws[b]), 0.0)
        T[:, a], Q[:, a] = t, q
        sc = np.sqrt(c)
        coef[:, a] = np.linalg.lstsq(sc[:, None] * T, sc * u, rcond=-1)[0]
        Yf = Yf - T @ coef[:, [a]] @ q[None, :]
    # the held-out batch: per block centred, then masked
    Xh = [x[~tr] - m for x, m in zip(X2, mu)]
    mh = [np.isnan(x) for x in Xh]
    hm = [bool(m.any()) for m in mh]
    Xh = [np.where(m, 0.0, x) for x, m in zip(Xh, mh)]
    oh = [(~m).sum(axis=1) for m in mh]
    S = np.zeros((Xh[0].shape[0], R))
    for a in range(R):
        ts, ws = [], []
        for b in range(nb):
            w = O.nipals_oracle._kron_all([L[:, a] for L in loadings[b]])
            s = Xh[b] @ w
            with np.errstate(divide="ignore", invalid="ignore"):
                ts.append(s / oh[b] * Ps[b] if hm[b] else s)
            ws.append(w)
        S[:, a] = np.average(ts, axis=0) if ts[0].size else 0.0
        for b in range(nb):
            with np.errstate(invalid="ignore"):
                step = np.outer(S[:, a], ws[b])
            Xh[b] = Xh[b] - (np.where(mh[b], 0.0, step) if hm[b] else step)
    with np.errstate(invalid="ignore"):
        pred = np.stack([(S[:, :r] @ coef[:r, :r]) @ Q[:, :r].T + nu for r in range(1, R + 1)])
    info = (sum(1 << b for b in range(nb) if miss[b]), sum(1 << b for b in range(nb) if hm[b]))
    return loadings, Q, coef, pred, n_iter, info
