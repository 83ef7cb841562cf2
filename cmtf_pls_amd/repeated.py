"""Repeated K-fold cross-validated Q2Y (validate.get_q2y_repeated_kfold): S shuffled K-fold splits, Q2Y of each, their mean and spread.

Split g's value is get_q2y_kfold(pls, folds=ids_g)'s: 1 - sum (pred - y)^2 / sum y^2 over the split's held-out predictions.  The
splits are sklearn's RepeatedKFold(n_splits, n_repeats, random_state) test folds (kfold.repeated_fold_ids), or an (S, I) array.

Device form (tPLS and ctPLS): G = min(floor(32 / K), floor(I / K), S) splits x K folds = n models per pass share every
MTTKRP and contraction of X, split-major: model m = g K + k holds out fold k of split g, so each split's models are a contiguous
K-model slice of every per-model buffer.  Per pass and block:
  kfold_xcov            once per split with that split's fold-sorted order, straight into S / mean[g K:(g + 1) K]     G reads
  per component         kfold_inner (a ctPLS: kfold_inner_coupled on n-model block views), the MTTKRP with n columns
                        (a ctPLS: then kfold_combine_scores), kfold_epilogue_splits stage 1 (fold_of is G x I, held-out
                        scores to Tout slot g), and but for the last component the contraction and stage 2          2R - 1 reads
The Y side, the held-out predictions and the R Q2Y numerators of every split are built on the device: per pass only status,
n_iter and G x R numerators come back.  The passes run through kfold._device_passes: a pass whose status is set refits its own
splits; anything outside the device form refits every fold of every split with kfold.refit_predictions.

With EngineOptions.masked_folds, a tPLS whose X has missing values runs every split x fold as a workgroup of
cmtfpls_cv_masked_models_f64 instead (kfold.masked_fold_numerators; X of order 4 with EngineOptions.masked_tensor_folds:
cmtfpls_cv_masked_tensor_models_f64); with EngineOptions.masked_folds_coupled, a ctPLS
with a missing value in some block runs them as workgroups of cmtfpls_cv_masked_coupled_f64, and with a block of
order 4 and EngineOptions.masked_tensor_folds_coupled of cmtfpls_cv_masked_coupled_tensor_f64.

The route (kfold._route), the body of a pass (kfold._device_pass: one kfold_xcov read per split, each into its split's slice of S and
mean, the statistics checked after the first) and the report (kfold._passes_report) are the shared ones of kfold.py.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from .kfold import (MASKED, MASKED_COUPLED, MAX_FOLDS, OFF, PASSES, REFIT, _decline_blocks, _device_blocks, _device_numerators, _device_pass,
                    _device_passes, _fold_means, _groups, _host, _masked_declined, _masked_run_report, _names, _passes_report,
                    _refit_numerators, _route, _tensor_dims, _to_dev, _training_data, masked_fold_numerators, repeated_fold_ids)
from .storage import FOLDS_WHY, reports_storage

_ENTRIES = ("kfold_xcov", "kfold_inner", "kfold_epilogue_splits", "mttkrp", "xcov")
_ENTRIES_COUPLED = ("kfold_xcov", "kfold_inner_coupled", "kfold_combine_scores", "kfold_epilogue_splits", "mttkrp", "xcov")


def _device_splits(pls, Xs, Y, ids: np.ndarray, K: int, tol: float, max_iter: int, coupled: bool):
    """The device form's run(pass, g0, g) of kfold._device_passes (a ctPLS: the coupled kernels, one block included): splits
    g0 .. g0 + g - 1 as g K split-major models, each split's S and mean built into its K-model slice of every block's."""
    be = pls._get_engine().be
    R = pls.n_components
    I = ids.shape[1]
    dev = be.device
    Yh = _host(Y).reshape(I, -1).astype(np.float64)
    M = Yh.shape[1]
    blocks = _device_blocks(pls, Xs, dev)
    Yd = _to_dev(Yh, dev)
    ydev = _to_dev(Yh - Yh.mean(axis=0), dev)                                         # shared by every split
    kk = torch.arange(K, device=dev)

    def run(passes, g0, g):
        n = K * g
        fold_of = _to_dev(ids[g0:g0 + g], dev, torch.int32)
        Yk = be.empty(n, I, M)
        Ss, means = zip(*[(be.empty(n, M, A * B), be.empty(n, A * B)) for _, A, B in blocks])   # every split builds into its slice
        nu, rows = [], []

        def builds():                                                                 # split g0 + j: models j K .. j K + K - 1
            for j in range(g):
                order, off, _, nu_j = _fold_means(Yh, ids[g0 + j], K)                 # kfold._fold_y's bits
                order_d, off_d, nu_d = _to_dev(order, dev, torch.int32), _to_dev(off, dev, torch.int32), _to_dev(nu_j, dev)
                nudev = _to_dev(nu_j - Yh.mean(axis=0), dev)
                sl = slice(j * K, (j + 1) * K)
                train = (fold_of[j].long().unsqueeze(0) != kk.unsqueeze(1)).unsqueeze(2)                   # K x I x 1
                Yk[sl] = torch.where(train, Yd.unsqueeze(0) - nu_d.unsqueeze(1), 0.0)
                nu.append(nu_d)
                order_l = order_d.long()
                rows.append([order_l[int(off[k]):int(off[k + 1])] for k in range(K)])
                # one read of each block per split, into the split's K-model slice of S and mean
                yield lambda X2, A, B, S, mean: be.kfold_xcov(X2, A, B, ydev, order_d, off_d, K, nudev, S[sl], mean[sl])

        got = _device_pass(pls, Xs, blocks, coupled, "kfold_xcov", builds(), fold_of, Yk, g, passes == 0, tol, max_iter,
                           _tensor_dims(Xs, coupled), Ss=Ss, means=means, splits=g)
        if isinstance(got, str):
            return got
        shared, _ = got
        num = torch.cat([_device_numerators(shared["Tout"][j:j + 1], shared["coef"][j * K:(j + 1) * K], shared["Q"][j * K:(j + 1) * K],
                                            nu[j].unsqueeze(0), Yd.unsqueeze(0), rows[j], K, 1, R, M) for j in range(g)])
        n_iter = shared["n_iter"].cpu().numpy().reshape(g, K, R)
        return num.cpu().numpy(), [n_iter[j].tolist() for j in range(g)], shared["status"].cpu().numpy()
    return run


@reports_storage("q2y_report_", FOLDS_WHY)
def repeated_kfold(pls, n_splits: int = 5, n_repeats: int = 10, folds=None, random_state=0, per_component: bool = False,
                   device_folds: bool = True, tol: float = 1e-8, max_iter: int = 100) -> dict:
    X, Y = _training_data(pls)
    coupled = isinstance(X, list)
    Xs = X if coupled else [X]
    I = Y.shape[0]
    ids, K = repeated_fold_ids(I, n_splits, n_repeats, random_state, folds)
    NS = ids.shape[0]
    R = pls.n_components
    den = float((_host(Y).astype(np.float64) ** 2).sum())

    G = 0
    masked = None
    route, detail = _route(pls, X, device_folds)
    why: Optional[str] = detail if route in (OFF, REFIT) else None
    if route in (MASKED, MASKED_COUPLED):       # EngineOptions.masked_folds, masked_tensor_folds (8s), masked_folds_coupled (8j)
        got = masked_fold_numerators(pls, X, Y, ids, K, None, tol, max_iter, coupled=route == MASKED_COUPLED)
        if got[0] is None:
            why = _masked_declined(detail, got[1])
        else:
            nums, n_iters, masked = got
    elif route == PASSES:
        G = min(_groups(X, K, min(NS, I // K)) for X in Xs) if K <= MAX_FOLDS else 0   # n <= I models, the LDS of every block
        why = _decline_blocks(pls, Xs, _names(Xs, coupled), Y, K * G if G else K, _ENTRIES_COUPLED if coupled else _ENTRIES,
                              tensor_ok=True)
    identity = np.arange(I)
    if masked is None:
        nums, n_iters, passes, why = _device_passes(pls, NS, G, "splits", why,
                                                    lambda: _device_splits(pls, Xs, Y, ids, K, tol, max_iter, coupled),
                                                    lambda g: _refit_numerators(pls, X, Y, ids[g], K, identity, tol, max_iter))
    q_all = 1.0 - nums / den                                                          # S x R: every component count
    q2y = q_all if per_component else q_all[:, -1]
    if masked is not None:
        pls.q2y_report_ = _masked_run_report(masked, "splits", NS, "splits_per_pass", n_iters)
    else:
        pls.q2y_report_ = _passes_report(f"{K * G} models per pass ({G} splits x {K} folds)", "cmtfpls_kfold_xcov_* per split",
                                         "cmtfpls_kfold_epilogue_splits_f64", Xs, coupled, passes, NS + passes * (2 * R - 1), why, "fold",
                                         "one refit per fold and split on the regular engine", {"splits": int(NS)},
                                         ("splits_per_pass", G), n_iters, _tensor_dims(Xs, coupled))   # reads: G + 2R - 1 per pass
    return dict(summary(q2y), folds=ids)


def summary(q2y: np.ndarray) -> dict:
    """q2y (S,) or (S, R) over S splits: its mean and std (ddof=0) over the splits; for (S, R) also one_se, the smallest r (from
    1) whose mean is at least max(mean) - std[argmax] / sqrt(S) (the one-standard-error rule)."""
    q2y = np.asarray(q2y, dtype=np.float64)
    mean, std = q2y.mean(axis=0), q2y.std(axis=0)
    if q2y.ndim == 1:
        return {"q2y": q2y, "mean": float(mean), "std": float(std)}
    best = int(np.argmax(mean))
    one_se = int(np.flatnonzero(mean >= mean[best] - std[best] / math.sqrt(q2y.shape[0]))[0]) + 1
    return {"q2y": q2y, "mean": mean, "std": std, "one_se": one_se}
