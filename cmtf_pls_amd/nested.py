"""Nested ("double") K-fold Q2Y (validate.get_q2y_nested_kfold): the Q2Y of a model whose component count was chosen by
cross-validation, scored on rows that had no part in the choice.

An outer K_o-fold split; the training rows of outer fold o are split again into K_i inner folds.  n = K_o (K_i + 1) models, each a
0/1 weighting of the fitted rows, outer-major (model o (K_i + 1) is outer model o, the K_i after it are its inner models):
  inner model (o, i)  trains on the rows with outer != o and inner[o] != i, scored on the rows with inner[o] == i
  outer model o       trains on the rows with outer != o, scored on (and predicting) the rows with outer == o
inner_q2y[o] is the Q2Y (validate.py:35-37, uncentred y) of the inner predictions over o's training rows with r = 1..R components,
selected[o] its argmax (the smallest r on a tie), and row i is predicted by outer model outer[i] with selected[outer[i]]
components: q2y is the Q2Y of those predictions.  outer_q2y is the Q2Y of the outer predictions with a fixed r (what
get_q2y_kfold(folds=outer, per_component=True) gives): max(outer_q2y) - q2y is the optimism of choosing R on the scored rows.

Device form (tPLS and ctPLS): the bootstrap's pass (bootstrap._device_resamples) with 0/1 counts.  G <= 32
models per pass share every read of X: kfold_weighted_xcov builds every model's S and mean from ONE read (the count columns
scaled by I / N_b, N_b the model's training rows, so that the mean is over those rows), then per component kfold_inner (a ctPLS:
kfold_inner_coupled), one MTTKRP, kfold_epilogue_weighted and, but for the last, one contraction: 2R reads of each block per pass,
X never written or copied.  The pass leaves T, coef and Q on the device; cmtfpls_press_rows_f64 scores them there: the (g, R)
squared-error sums of the models' scored rows, and the outer models' r-component predictions into one (R, I, M) buffer that stays
on the device until the last pass.  Per pass only status, n_iter and those sums come back.  The passes run through
kfold._device_passes: a pass whose status is set refits its own models; anything outside the device form (the NumPy backend,
device_folds=False, what kfold._decline_blocks declines, missing values in X) refits every model on the regular engine.

The route (kfold._route, without a masked form), the body of a pass (kfold._device_pass over kfold._weighted_models with
kfold_weighted_xcov as the read) and the report (kfold._passes_report) are the shared ones of kfold.py.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from .bootstrap import _ENTRIES, _ENTRIES_COUPLED, MAX_COLUMNS
from .kfold import (MAX_FOLDS, PASSES, _decline_blocks, _device_blocks, _device_pass, _device_passes, _groups, _host, _names, _passes_report,
                    _route, _rows, _tensor_dims, _to_dev, _training_data, _weighted_models, fold_ids, refit_fold, repeated_fold_ids)
from .storage import FOLDS_WHY, reports_storage

PRESS_FORM = "cmtfpls_press_rows_f64"


def nested_fold_ids(n_samples: int, n_outer: int = 5, n_inner: int = 5, outer_folds=None, inner_folds=None,
                    random_state=0) -> Tuple[np.ndarray, int, np.ndarray, int]:
    """(outer (I,), K_o, inner (K_o, I), K_i).  outer_folds=None: one shuffled K-fold split, repeated_fold_ids(I, n_outer, 1,
    random_state)[0][0] (sklearn's KFold(n_outer, shuffle=True, random_state) test folds); otherwise an (I,) id array checked by
    fold_ids.  inner_folds=None: the training rows of outer fold o, in ascending row order, split by repeated_fold_ids(I_o,
    n_inner, 1, random_state + 1 + o)[0][0]; otherwise a (K_o, I) integer array whose row o holds -1 exactly on the rows of outer
    fold o and ids 0..K_i-1 elsewhere, no fold empty, the same K_i in every row."""
    I = int(n_samples)
    if outer_folds is None or inner_folds is None:
        if isinstance(random_state, bool) or not isinstance(random_state, (int, np.integer)):
            raise ValueError(f"random_state must be an int (reproducible splits), got {random_state!r}")
    if outer_folds is None:
        ids, Ko = repeated_fold_ids(I, n_outer, 1, random_state)
        outer = ids[0]
    else:
        outer, Ko = fold_ids(I, folds=outer_folds)
    if inner_folds is None:
        inner = np.full((Ko, I), -1, dtype=np.int64)
        Ki = int(n_inner)
        for o in range(Ko):
            train = np.flatnonzero(outer != o)
            inner[o, train] = repeated_fold_ids(train.size, n_inner, 1, int(random_state) + 1 + o)[0][0]
        return outer, Ko, inner, Ki
    f = np.asarray(inner_folds)
    if f.ndim != 2 or f.shape != (Ko, I):
        raise ValueError(f"inner_folds must be a ({Ko}, {I}) array of fold ids (one row per outer fold), got shape {f.shape}")
    if f.dtype.kind not in "iu":
        if f.dtype.kind != "f" or not np.all(np.isfinite(f)) or not np.all(f == np.round(f)):
            raise ValueError("inner_folds must hold integer fold ids")
    f = f.astype(np.int64)
    Ks = []
    for o in range(Ko):
        held = outer == o
        if not np.array_equal(f[o] == -1, held):
            raise ValueError(f"inner_folds[{o}] must hold -1 exactly on the rows of outer fold {o}")
        try:
            _, K = fold_ids(int((~held).sum()), folds=f[o][~held])
        except ValueError as e:
            raise ValueError(f"inner_folds[{o}]: {e}") from None
        Ks.append(K)
    if len(set(Ks)) != 1:
        raise ValueError(f"every outer fold must have the same number of inner folds, got {sorted(set(Ks))}")
    return outer, Ko, f, Ks[0]


def model_rows(outer: np.ndarray, Ko: int, inner: np.ndarray, Ki: int):
    """(counts (n, I) int32: 1 on a model's training rows; ev (n, I) int32: 1 on an inner model's scored rows, 2 on an outer
    model's) of the n = K_o (K_i + 1) models, outer-major."""
    n, I = Ko * (Ki + 1), outer.shape[0]
    counts = np.zeros((n, I), dtype=np.int32)
    ev = np.zeros((n, I), dtype=np.int32)
    for o in range(Ko):
        e = o * (Ki + 1)
        counts[e] = outer != o
        ev[e] = 2 * (outer == o)
        for i in range(Ki):
            counts[e + 1 + i] = (outer != o) & (inner[o] != i)
            ev[e + 1 + i] = inner[o] == i
    return counts, ev


def torch_press(T, coef, Q, nu, Y, ev, pred=None) -> torch.Tensor:
    """What cmtfpls_press_rows_f64 computes, with torch ops in kfold._device_numerators' formulation (the r-component predictions
    of a model's scored rows as a cumsum over a rows x R x M tensor): the scoring when a shape is outside the kernel."""
    n, I, R = T.shape
    M = Y.shape[1]
    press = torch.zeros(n, R, dtype=torch.float64, device=T.device)
    step = max(1, (1 << 24) // (R * M))
    for j in range(n):
        rows = torch.nonzero(ev[j] > 0).squeeze(1)
        for lo in range(0, rows.numel(), step):
            idx = rows[lo:lo + step]
            H = T[j, idx] @ coef[j]                                                   # rows x R
            C = torch.cumsum(H.unsqueeze(2) * Q[j].unsqueeze(0), dim=1) + nu[j]       # rows x R x M
            res = C - Y[idx].unsqueeze(1)
            press[j] += (res * res).sum(dim=(0, 2))
            if pred is not None:
                w = ev[j, idx] == 2
                pred[:, idx[w]] = C[w].permute(1, 0, 2)
    return press


def _device_nested(pls, Xs, Y, counts: np.ndarray, ev: np.ndarray, tol: float, max_iter: int, coupled: bool, pred_d: torch.Tensor,
                   scored: list):
    """The device form's run(pass, e0, g) of kfold._device_passes: models e0 .. e0 + g - 1 as the models of one weighted state (a
    one-model pass as two copies of its model).  A pass without a status adds its outer models' predictions to pred_d (R, I, M)
    and returns its models' squared-error sums (g, R); scored collects what scored each pass."""
    be = pls._get_engine().be
    R = pls.n_components
    dev = be.device
    I = counts.shape[1]
    Yd = _to_dev(_host(Y).reshape(I, -1).astype(np.float64), dev)
    M = Yd.shape[1]
    blocks = _device_blocks(pls, Xs, dev)
    counts_d = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(dev)  # one upload of the weights and the rows to score
    ev_d = torch.from_numpy(np.ascontiguousarray(ev, dtype=np.int32)).to(dev)

    def run(passes, e0, g):
        n, C, Cf = _weighted_models(counts_d, e0, g)
        N = Cf.sum(dim=1, keepdim=True)                                               # n x 1: the models' training rows
        nu = (Cf @ Yd) / N                                                            # n x M: their means of Y
        Yk = (Cf.unsqueeze(2) * (Yd.unsqueeze(0) - nu.unsqueeze(1))).contiguous()     # n x I x M: rows with weight 0 are 0
        Yw = torch.cat([Yk.permute(1, 0, 2).reshape(I, n * M), (Cf * (I / N)).t()], dim=1).contiguous()   # the mean: X^T c / N
        got = _device_pass(pls, Xs, blocks, coupled, "kfold_weighted_xcov",           # one read of each block
                           [lambda X2, A, B, S, mean: be.kfold_weighted_xcov(X2, A, B, Yw, n, M, S, mean)],
                           C, Yk, 1, passes == 0, tol, max_iter, _tensor_dims(Xs, coupled), weighted=True)
        if isinstance(got, str):
            return got
        shared, _ = got
        status = shared["status"][:g].cpu().numpy()
        n_iter = shared["n_iter"][:g].cpu().numpy()
        press = np.zeros((g, R))
        if not status.any():
            args = (shared["T"][:g], shared["coef"][:g], shared["Q"][:g], nu[:g].contiguous(), Yd, ev_d[e0:e0 + g], pred_d)
            out = be.press_rows(*args)
            scored.append(PRESS_FORM if out is not None else "torch ops")
            if out is None:                                                           # a shape outside the kernel
                out = torch_press(*args)
            press = out.cpu().numpy()
        return press, [n_iter[j].tolist() for j in range(g)], status
    return run


def _take_y(Y, sel: np.ndarray):
    return Y[torch.from_numpy(sel).to(Y.device)] if isinstance(Y, torch.Tensor) else Y[sel]


@reports_storage("q2y_report_", FOLDS_WHY)
def nested_kfold(pls, n_outer: int = 5, n_inner: int = 5, outer_folds=None, inner_folds=None, random_state=0,
                 device_folds: bool = True, tol: float = 1e-8, max_iter: int = 100) -> dict:
    X, Y = _training_data(pls)
    coupled = isinstance(X, list)
    Xs = X if coupled else [X]
    I = Y.shape[0]
    outer, Ko, inner, Ki = nested_fold_ids(I, n_outer, n_inner, outer_folds, inner_folds, random_state)
    n = Ko * (Ki + 1)
    R = pls.n_components
    counts, ev = model_rows(outer, Ko, inner, Ki)
    Yh = _host(Y).reshape(I, -1).astype(np.float64)
    M = Yh.shape[1]

    G = 0
    route, why = _route(pls, X, device_folds, masked=False)                           # (missing values in X: _decline_blocks says so)
    if route == PASSES:
        G = min(_groups(Xb, 1, min(n, I, MAX_FOLDS, MAX_COLUMNS // (M + 1))) for Xb in Xs)   # the LDS of every block's score pass
        tidy = G - G % (Ki + 1)                                                       # an outer model and its inner models in one pass,
        if tidy and -(-n // tidy) == -(-n // G):                                      # where that costs no pass
            G = tidy
        why = _decline_blocks(pls, Xs, _names(Xs, coupled), Y, max(G, 2), _ENTRIES_COUPLED if coupled else _ENTRIES, tensor_ok=True)
    dev = pls._get_engine().be.device if why is None else torch.device("cpu")
    pred_d = torch.zeros(R, I, M, dtype=torch.float64, device=dev)
    refit_pred, scored = {}, []
    sub = [None, None, None]                                                          # (o, X[train_o], Y[train_o]) of the last o

    def refit_one(e):
        o, i = divmod(e, Ki + 1)
        held = outer == o
        if i == 0:                                                                    # outer model o
            pred, n_iter = refit_fold(pls, X, Y, held, tol, max_iter)
            refit_pred[o] = pred
            y = Yh[held]
        else:                                                                         # inner model (o, i - 1): a fold of X[train_o]
            if sub[0] != o:
                sub[:] = [o, [_rows(b, ~held) for b in X] if coupled else _rows(X, ~held), _take_y(Y, ~held)]
            test = inner[o][~held] == i - 1
            pred, n_iter = refit_fold(pls, sub[1], sub[2], test, tol, max_iter)
            y = Yh[~held][test]
        return ((pred - y) ** 2).reshape(R, -1).sum(axis=1), n_iter

    press, n_iters, passes, why = _device_passes(pls, n, G, "models", why,
                                                 lambda: _device_nested(pls, Xs, Y, counts, ev, tol, max_iter, coupled, pred_d, scored),
                                                 refit_one)
    pred = pred_d.cpu().numpy()                                                       # (R, I, M): row i by outer model outer[i]
    for o, p in refit_pred.items():
        pred[:, outer == o] = p

    press = press.reshape(Ko, Ki + 1, R)
    den_inner = np.array([(Yh[outer != o] ** 2).sum() for o in range(Ko)])
    inner_q2y = 1.0 - press[:, 1:].sum(axis=1) / den_inner[:, None]                   # validate.py:35-37 over o's training rows
    selected = np.argmax(inner_q2y, axis=1) + 1                                       # the smallest r on an exact tie
    den = (Yh ** 2).sum()
    outer_q2y = 1.0 - ((pred - Yh) ** 2).reshape(R, -1).sum(axis=1) / den
    chosen = pred[selected[outer] - 1, np.arange(I)]                                  # (I, M)
    q2y = float(1.0 - ((chosen - Yh) ** 2).sum() / den)

    by = " and ".join(sorted(set(scored))) if scored else PRESS_FORM
    pls.q2y_report_ = _passes_report(f"{G} 0/1-weighted models per pass", "cmtfpls_kfold_weighted_xcov_*", "cmtfpls_kfold_epilogue_weighted_f64",
                                     Xs, coupled, passes, 2 * R * passes, why, "model", "one refit per model on the regular engine",
                                     {"models": int(n), "outer_folds": int(Ko), "inner_folds": int(Ki)}, ("models_per_pass", G), n_iters,
                                     _tensor_dims(Xs, coupled), scored=f", scored by {by}")
    return {"q2y": q2y, "selected": selected.astype(np.int64), "inner_q2y": inner_q2y, "outer_q2y": outer_q2y,
            "predictions": chosen.reshape(tuple(Y.shape)), "outer_folds": outer, "inner_folds": inner}
