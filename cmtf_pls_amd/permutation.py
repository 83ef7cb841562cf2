"""Response-permutation test of K-fold cross-validated Q2Y (validate.permutation_test_q2y).

Permutation p replaces Y by Y[pi_p] (X is never permuted, the folds stay tied to the rows of X) and computes get_q2y_kfold's Q2Y
with Y[pi_p] as the actual values; the p-value is (1 + #{null >= observed}) / (P + 1).

Device form (tPLS): a permuted response differs from the observed one only in Y, so G = floor(32 / K) permutations x
K folds = n models share each read of X, model m = k G + p holding out fold k with Y[pi_p].  Per pass:
  kfold_wide_xcov           every model's training cross-covariance from ONE pass over X (the fold-grouped X[rows_f]^T Y' with
                            Y' = [Y[pi_1] - ybar .. Y[pi_G] - ybar] on the f64 matrix cores, then the all-minus-own identity)
  per component             kfold_inner_grouped, the MTTKRP with n columns, kfold_epilogue_grouped stage 1, the contraction with n
                            columns and stage 2 (the K-fold form of kfold.py with model_fold[m] = m // G)
The pass's Y side (each model's centred, held-out-zeroed Y) is built on the device from one upload of the permutation index, and
so are the held-out predictions and the Q2Y numerators: per pass only status, n_iter and G x R numerators come back.  2R reads of
X per pass, ceil(P / G) passes.  A pass whose status is set refits its permutations; anything outside the device form (a ctPLS
among it) refits every permutation with kfold.refit_predictions.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from .kfold import MAX_FOLDS, _decline_blocks, _dims, _host, _stats_why, fold_ids, refit_predictions

_ENTRIES = ("kfold_wide_xcov", "kfold_inner_grouped", "kfold_epilogue_grouped", "mttkrp", "xcov")
_LDS_BYTES = 152 * 1024            # the score pass's bound on the models' loadings (kfold._decline_blocks)


def permutations_for(I: int, n_permutations: int, permutations, random_state) -> np.ndarray:
    """The (P, I) permutation index: `permutations` checked, or P draws of default_rng(random_state).permutation(I) in order."""
    if int(n_permutations) < 1:
        raise ValueError(f"n_permutations must be at least 1, got {n_permutations}")
    if permutations is None:
        rng = np.random.default_rng(random_state)
        return np.stack([rng.permutation(I) for _ in range(int(n_permutations))]).astype(np.int64)
    pm = np.asarray(permutations)
    if pm.ndim != 2 or pm.shape[1] != I or pm.shape[0] < 1:
        raise ValueError(f"permutations must be a (P, {I}) integer array with P >= 1, got shape {pm.shape}")
    if pm.dtype.kind not in "iu":
        raise ValueError("permutations must hold integer row indices")
    pm = pm.astype(np.int64)
    ok = np.sort(pm, axis=1) == np.arange(I)
    bad = np.flatnonzero(~ok.all(axis=1))
    if bad.size:
        raise ValueError(f"row {int(bad[0])} of permutations is not a permutation of 0..{I - 1}")
    return pm


def _groups(pls, X, K: int, P: int) -> int:
    """Permutations per pass: floor(32 / K), fewer when the n models' loadings would exceed the LDS of the score pass."""
    A, B = _dims(X)
    G = min(MAX_FOLDS // K, P)
    while G > 1 and (A + B) * 16 * ((K * G + 15) // 16) * 8 > _LDS_BYTES:
        G -= 1
    return G


def _perm_y(Y, pi: np.ndarray):
    return Y[torch.from_numpy(pi).to(Y.device)] if isinstance(Y, torch.Tensor) else Y[pi]


def _refit_numerators(pls, X, Y, ids, K, pi, tol, max_iter):
    """(numerators (R,), n_iter K x R) of one permutation from literal refits."""
    Yp = _perm_y(Y, pi)
    pred, n_iter = refit_predictions(pls, X, Yp, ids, K, tol, max_iter)
    y = _host(Yp).reshape(pred.shape[1], -1).astype(np.float64)
    return ((pred - y) ** 2).reshape(pred.shape[0], -1).sum(axis=1), n_iter


def _device_numerators(Tout, coef, Q, nu, Yp, rows, K: int, g: int, R: int, M: int) -> torch.Tensor:
    """The Q2Y numerators (g x R) of a pass on the device: sum over rows of |pred_r - y_p|^2 for every component count r, pred_r
    = nu + sum_{c < r} h_c q_c with h = scores @ coef_ (coef_ upper triangular: the r-component model's prediction)."""
    num = torch.zeros(g, R, dtype=torch.float64, device=Tout.device)
    coef = coef.view(K, g, R, R)
    Q = Q.view(K, g, R, M)
    step = max(1, (1 << 24) // (g * R * M))
    for k in range(K):
        for lo in range(0, rows[k].numel(), step):
            idx = rows[k][lo:lo + step]
            H = torch.bmm(Tout[:, idx], coef[k])                                     # g x n x R
            C = torch.cumsum(H.unsqueeze(-1) * Q[k].unsqueeze(1), dim=2)            # g x n x R x M
            res = C + (nu[:, k].unsqueeze(1) - Yp[:, idx]).unsqueeze(2)
            num += (res * res).sum(dim=(1, 3))
    return num


def _device_null(pls, X, Y, ids: np.ndarray, K: int, perms: np.ndarray, G: int, tol: float, max_iter: int):
    """The device form: (numerators P x R with NaN rows for failed passes, n_iter per permutation (None: failed), passes, failed
    pass messages) or (None, why) when it does not run at all."""
    from .tpls import _as_torch_dtype, to_device_copy

    eng = pls._get_engine()
    be = eng.be
    R = pls.n_components
    I = X.shape[0]
    A, B = _dims(X)
    P = A * B
    NP = perms.shape[0]
    Yh = _host(Y).reshape(I, -1).astype(np.float64)
    M = Yh.shape[1]
    dev = be.device
    nums = np.full((NP, R), np.nan)
    n_iters = [None] * NP
    notes = []
    passes = 0
    with eng.device_ctx():
        Xd = to_device_copy(X, _as_torch_dtype(pls._dtype, X), dev, copy=False)     # a device tensor of the storage type: as it is
        X2 = Xd.view(I, P)
        counts = np.bincount(ids, minlength=K)
        order = np.argsort(ids, kind="stable").astype(np.int32)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
        Yd, order_d, off_d, fold_of = t(Yh), t(order, torch.int32), t(off, torch.int32), t(ids, torch.int32)
        ybar = Yd.mean(dim=0)
        colsum = Yd.sum(dim=0)
        onehot = (fold_of.long().unsqueeze(0) == torch.arange(K, device=dev).unsqueeze(1)).to(torch.float64)   # K x I
        train = (onehot == 0).view(K, 1, I, 1)
        ntr = t(I - counts).view(1, K, 1)
        rows = [torch.from_numpy(np.flatnonzero(ids == k)).to(dev) for k in range(K)]
        perms_d = torch.from_numpy(perms).to(dev)                                         # one upload of the index
        mean = be.empty(K, P)
        NT, stride = be.kfold_row_tiles(I)
        for p0 in range(0, NP, G):
            g = min(G, NP - p0)
            n = K * g
            Yp = Yd[perms_d[p0:p0 + g]]                                                    # g x I x M
            nu = (colsum - torch.matmul(onehot, Yp)) / ntr                                # g x K x M: training means
            Yw = (Yp - ybar).permute(1, 0, 2).reshape(I, g * M).contiguous()            # Y': column p M + j
            ydev = (nu - ybar).permute(1, 0, 2).reshape(K, g * M).contiguous()
            S = be.empty(n, M, P)                                                          # = K x (g M) x P: model k g + p
            stats = be.kfold_wide_xcov(X2, A, B, Yw, order_d, off_d, K, ydev, S, mean)
            if stats is None:
                return None, "shape outside cmtfpls_kfold_wide_xcov"
            if passes == 0:
                why = _stats_why(stats, P, I, eng.opt.xcov_raw_max_offset, "X")
                if why is not None:
                    return None, why
            Yk = torch.where(train, Yp.unsqueeze(0) - nu.permute(1, 0, 2).unsqueeze(2), 0.0).reshape(n, I, M)
            mf = torch.arange(n, dtype=torch.int32, device=dev) // g
            buf = {
                "fold_of": fold_of, "S": S, "mean": mean, "Yk": Yk, "Gy": be.empty(n, NT, M, M), "WA": be.empty(A, n),
                "WB": be.empty(B, n), "Q": be.zeros(n, R, M), "Wa": be.zeros(n, R, A), "Wb": be.zeros(n, R, B), "T": be.zeros(n, I, R),
                "Gt": be.zeros(n, R, R), "coef": be.zeros(n, R, R), "Rm": be.zeros(n, R, P), "tm": be.empty(I, n),
                "Tout": be.zeros(g, I, R), "vec": be.zeros(n, 3 * R + M + 2), "n_iter": torch.zeros(n, R, dtype=torch.int32, device=dev),
                "status": torch.zeros(n, dtype=torch.int32, device=dev), "part": be.empty(n, NT, stride),
            }
            st = _lib.KfoldState(I, A, B, M, n, R, *[buf[f].data_ptr() for f, _ in _lib.KfoldState._fields_[6:]])
            ws = torch.empty(max(be.kfold_inner_workspace_bytes(A, B, n), 256), dtype=torch.uint8, device=dev)
            sc = be.empty(I, n)
            rs = be.empty(n, P)
            if be.kfold_epilogue_grouped(st, mf, g, 0, 0, None) is None:
                return None, "shape outside cmtfpls_kfold_epilogue_grouped_f64"
            for a in range(R):
                if be.kfold_inner_grouped(st, mf, g, a, tol, max_iter, ws) is None:
                    return None, "shape outside cmtfpls_kfold_inner_grouped_f64"
                if be.mttkrp(X2, A, B, buf["WA"], buf["WB"], sc) is None:               # X_0 [w_1 .. w_n]: one read
                    return None, "the models' loadings outside cmtfpls_mttkrp_*"
                be.kfold_epilogue_grouped(st, mf, g, 1, a, sc)
                if a + 1 < R:
                    be.xcov(X2, buf["tm"], False, out=rs)                               # X_0^T [t_m * train_m]: one read
                    be.kfold_epilogue_grouped(st, mf, g, 2, a, rs)
            num = _device_numerators(buf["Tout"], buf["coef"], buf["Q"], nu, Yp, rows, K, g, R, M)
            status = buf["status"].cpu().numpy()
            n_iter = buf["n_iter"].cpu().numpy().reshape(K, g, R)
            num = num.cpu().numpy()
            passes += 1
            if status.any():
                bad = np.flatnonzero(status)
                notes.append(f"pass {passes - 1} (permutations {p0}..{p0 + g - 1}): non-finite loadings or coefficients in models "
                             f"{bad.tolist()}, refitted")
                continue
            nums[p0:p0 + g] = num
            for p in range(g):
                n_iters[p0 + p] = n_iter[:, p].tolist()
    return nums, n_iters, passes, notes


def permutation_test(pls, n_permutations: int = 99, n_splits: int = 5, folds=None, permutations=None, random_state=0,
                     per_component: bool = False, device_folds: bool = True, tol: float = 1e-8, max_iter: int = 100) -> dict:
    from .cmtf import ctPLS
    from .validate import get_q2y_kfold

    coupled = isinstance(pls, ctPLS)
    if coupled:
        assert getattr(pls, "original_Xs", None) is not None, "PLS Tensor must be fit prior to calculating Q2Y"
        X, Y = list(pls.original_Xs), pls.original_Y
    else:
        assert getattr(pls, "original_X", None) is not None, "PLS Tensor must be fit prior to calculating Q2Y"
        X, Y = pls.original_X, pls.original_Y
    I = Y.shape[0]
    ids, K = fold_ids(I, n_splits, folds)
    perms = permutations_for(I, n_permutations, permutations, random_state)
    NP = perms.shape[0]
    R = pls.n_components
    q2y = get_q2y_kfold(pls, n_splits, folds, per_component, device_folds)           # the observed value, exactly
    observed = pls.q2y_report_
    den = float((_host(Y).astype(np.float64) ** 2).sum())

    why: Optional[str] = None
    G = 0
    if not device_folds:
        why = "device folds switched off"
    elif coupled:
        why = "coupled model: permutation device form not built"
    else:
        G = _groups(pls, X, K, NP) if K <= MAX_FOLDS else 0
        why = _decline_blocks(pls, [X], ["X"], Y, K * G if G else K, _ENTRIES)     # the checks with K made with the n models
    nums = np.full((NP, R), np.nan)
    n_iters = [None] * NP
    passes, notes = 0, []
    if why is None:
        out = _device_null(pls, X, Y, ids, K, perms, G, tol, max_iter)
        if out[0] is None:
            why = out[1]
        else:
            nums, n_iters, passes, notes = out
            if notes:
                why = "; ".join(notes)
    for p in range(NP):                                                              # the refit path: whatever the device left
        if n_iters[p] is None:
            nums[p], n_iters[p] = _refit_numerators(pls, X, Y, ids, K, perms[p], tol, max_iter)
    null_all = 1.0 - nums / den                                                       # P x R: every component count
    null = null_all if per_component else null_all[:, -1]
    p_value = (1.0 + (null >= q2y).sum(axis=0)) / (NP + 1.0)
    if passes:
        form = (f"{K * G} models per pass ({G} permutations x {K} folds) from shared reads of X (cmtfpls_kfold_wide_xcov_*, "
                "cmtfpls_kfold_inner_grouped_f64, cmtfpls_mttkrp_*, cmtfpls_kfold_epilogue_grouped_f64, cmtfpls_xcov_*)")
        if notes:
            form += "; failed passes refitted per fold on the regular engine"
    else:
        form = "one refit per fold and permutation on the regular engine"
    rep = {"form": form, "permutations": int(NP), "passes": int(passes), "models_per_pass": int(K * G) if passes else None,
           "x_reads": 2 * R * passes if passes else None, "n_iter": n_iters, "observed": observed}
    if why is not None:
        rep["why"] = why
    pls.q2y_report_ = rep
    return {"q2y": q2y, "null": null, "p_value": p_value if per_component else float(p_value), "permutations": perms}
