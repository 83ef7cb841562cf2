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
X per pass, ceil(P / G) passes, run by kfold._device_passes.  A pass whose status is set refits its permutations; anything
outside the device form (a ctPLS without EngineOptions.coupled_permutations among it) refits every permutation with
kfold.refit_predictions.

A ctPLS on complete data with EngineOptions.coupled_permutations ("coupled") runs the same pass on a state view per
block: the Y side of the pass is built once, kfold_wide_xcov once per block into that block's S (n x M x P_b) and per-fold mean
(K x P_b), then per component kfold_inner_coupled_grouped (model m reads row model_fold[m] of every block's mean), one MTTKRP per
block, kfold_combine_scores, kfold_epilogue_grouped stage 1 on the shared score, one contraction and stage 2 per block: 2R reads of
each block per pass, G the smallest of the blocks' G.  With EngineOptions.tensor_folds_coupled as well, blocks of order 4 are
taken: the inner entry is then kfold_inner_coupled_tensor in the grouped layout.

With EngineOptions.masked_folds, a tPLS whose X has missing values runs every permutation x fold as a workgroup of
cmtfpls_cv_masked_models_f64 instead (kfold.masked_fold_numerators; X of order 4 with EngineOptions.masked_tensor_folds:
cmtfpls_cv_masked_tensor_models_f64); with EngineOptions.masked_folds_coupled, a ctPLS
with a missing value in some block runs them as workgroups of cmtfpls_cv_masked_coupled_f64, and with a block of
order 4 and EngineOptions.masked_tensor_folds_coupled of cmtfpls_cv_masked_coupled_tensor_f64.

The route (kfold._route: the coupled masked form is asked first, a ctPLS without coupled_permutations refits), the body of a pass
(kfold._device_pass with kfold_wide_xcov as the read) and the report (kfold._passes_report) are the shared ones of kfold.py.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .kfold import (MASKED, MASKED_COUPLED, MAX_FOLDS, OFF, PASSES, REFIT, _decline_blocks, _device_blocks, _device_numerators, _device_pass,
                    _device_passes, _groups, _host, _masked_declined, _masked_run_report, _names, _passes_report, _refit_numerators,
                    _route, _tensor_dims, _to_dev, _training_data, fold_ids, masked_fold_numerators)
from .storage import FOLDS_WHY, reports_storage

_ENTRIES = ("kfold_wide_xcov", "kfold_inner_grouped", "kfold_epilogue_grouped", "mttkrp", "xcov")
_ENTRIES_COUPLED = ("kfold_wide_xcov", "kfold_inner_coupled_grouped", "kfold_combine_scores", "kfold_epilogue_grouped", "mttkrp", "xcov")


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


def _device_null(pls, Xs, Y, ids: np.ndarray, K: int, perms: np.ndarray, tol: float, max_iter: int, coupled: bool = False):
    """The device form's run(pass, p0, g) of kfold._device_passes: permutations p0 .. p0 + g - 1 as K g models, model k g + p
    holding out fold k with Y[pi_p0+p].  Xs: [X] of a tPLS, or the blocks of a ctPLS (coupled: a state view per block, the Y side
    shared)."""
    be = pls._get_engine().be
    R = pls.n_components
    blocks = _device_blocks(pls, Xs, be.device)
    I = blocks[0][0].shape[0]
    dev = be.device
    Yh = _host(Y).reshape(I, -1).astype(np.float64)
    M = Yh.shape[1]
    counts = np.bincount(ids, minlength=K)
    order = np.argsort(ids, kind="stable").astype(np.int32)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    Yd, order_d, off_d, fold_of = _to_dev(Yh, dev), _to_dev(order, dev, torch.int32), _to_dev(off, dev, torch.int32), \
        _to_dev(ids, dev, torch.int32)
    ybar = Yd.mean(dim=0)
    colsum = Yd.sum(dim=0)
    onehot = (fold_of.long().unsqueeze(0) == torch.arange(K, device=dev).unsqueeze(1)).to(torch.float64)   # K x I
    train = (onehot == 0).view(K, 1, I, 1)
    ntr = _to_dev(I - counts, dev).view(1, K, 1)
    rows = [torch.from_numpy(np.flatnonzero(ids == k)).to(dev) for k in range(K)]
    perms_d = torch.from_numpy(perms).to(dev)                                         # one upload of the index
    means = [be.empty(K, A * B) for _, A, B in blocks]                                # per fold: shared by the G models of a fold

    def run(passes, p0, g):
        n = K * g
        Yp = Yd[perms_d[p0:p0 + g]]                                                    # g x I x M
        nu = (colsum - torch.matmul(onehot, Yp)) / ntr                                # g x K x M: training means
        Yw = (Yp - ybar).permute(1, 0, 2).reshape(I, g * M).contiguous()            # Y': column p M + j
        ydev = (nu - ybar).permute(1, 0, 2).reshape(K, g * M).contiguous()
        Yk = torch.where(train, Yp.unsqueeze(0) - nu.permute(1, 0, 2).unsqueeze(2), 0.0).reshape(n, I, M)
        mf = torch.arange(n, dtype=torch.int32, device=dev) // g
        got = _device_pass(pls, Xs, blocks, coupled, "kfold_wide_xcov",                # one read of each block: S = K x (g M) x P, model k g + p
                           [lambda X2, A, B, S, mean: be.kfold_wide_xcov(X2, A, B, Yw, order_d, off_d, K, ydev, S, mean)],
                           fold_of, Yk, g, passes == 0, tol, max_iter, _tensor_dims(Xs, coupled), means=means, grouped=(mf, g))
        if isinstance(got, str):
            return got
        shared, _ = got
        num = _device_numerators(shared["Tout"], shared["coef"], shared["Q"], nu, Yp, rows, K, g, R, M)
        n_iter = shared["n_iter"].cpu().numpy().reshape(K, g, R)
        return num.cpu().numpy(), [n_iter[:, p].tolist() for p in range(g)], shared["status"].cpu().numpy()
    return run


@reports_storage("q2y_report_", FOLDS_WHY)
def permutation_test(pls, n_permutations: int = 99, n_splits: int = 5, folds=None, permutations=None, random_state=0,
                     per_component: bool = False, device_folds: bool = True, tol: float = 1e-8, max_iter: int = 100) -> dict:
    from .validate import get_q2y_kfold

    X, Y = _training_data(pls)
    I = Y.shape[0]
    ids, K = fold_ids(I, n_splits, folds)
    perms = permutations_for(I, n_permutations, permutations, random_state)
    NP = perms.shape[0]
    q2y = get_q2y_kfold(pls, n_splits, folds, per_component, device_folds)           # the observed value, exactly
    observed = pls.q2y_report_
    den = float((_host(Y).astype(np.float64) ** 2).sum())

    coupled = isinstance(X, list)
    Xs = X if coupled else [X]
    G = 0
    masked = None
    # EngineOptions.coupled_permutations: without it a ctPLS refits
    gate = (coupled and pls._get_engine().opt.coupled_permutations, "coupled model: permutation device form not built")
    route, detail = _route(pls, X, device_folds, coupled_first=True, coupled_gate=gate)
    why: Optional[str] = detail if route in (OFF, REFIT) else None
    if route in (MASKED, MASKED_COUPLED):       # EngineOptions.masked_folds, masked_tensor_folds (8s), masked_folds_coupled (8j)
        got = masked_fold_numerators(pls, X, Y, np.broadcast_to(ids, (NP, I)), K, perms, tol, max_iter, coupled=route == MASKED_COUPLED)
        if got[0] is None:
            why = _masked_declined(detail, got[1])
        else:
            nums, n_iters, masked = got
    elif route == PASSES:
        G = min(_groups(b, K, NP) for b in Xs) if K <= MAX_FOLDS else 0               # the LDS of every block's score pass
        why = _decline_blocks(pls, Xs, _names(Xs, coupled), Y, K * G if G else K, _ENTRIES_COUPLED if coupled else _ENTRIES,
                              tensor_ok=True)                                         # the checks with K made with the n models
    if masked is None:
        nums, n_iters, passes, why = _device_passes(pls, NP, G, "permutations", why,
                                                    lambda: _device_null(pls, Xs, Y, ids, K, perms, tol, max_iter, coupled),
                                                    lambda p: _refit_numerators(pls, X, Y, ids, K, perms[p], tol, max_iter))
    null_all = 1.0 - nums / den                                                       # P x R: every component count
    null = null_all if per_component else null_all[:, -1]
    p_value = (1.0 + (null >= q2y).sum(axis=0)) / (NP + 1.0)
    if masked is not None:
        pls.q2y_report_ = _masked_run_report(masked, "permutations", NP, "models_per_pass", n_iters, observed=observed)
    else:
        R = pls.n_components
        # behaviour: the form of a ctPLS does not say that failed passes refitted
        pls.q2y_report_ = _passes_report(f"{K * G} models per pass ({G} permutations x {K} folds)", "cmtfpls_kfold_wide_xcov_*",
                                         "cmtfpls_kfold_epilogue_grouped_f64", Xs, coupled, passes, 2 * R * passes, why,
                                         None if coupled else "fold", "one refit per fold and permutation on the regular engine",
                                         {"permutations": int(NP)}, ("models_per_pass", K * G), n_iters, _tensor_dims(Xs, coupled),
                                         grouped=True, more={"observed": observed})
    return {"q2y": q2y, "null": null, "p_value": p_value if per_component else float(p_value), "permutations": perms}
