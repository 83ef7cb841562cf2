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
n_iter and G x R numerators come back.  A pass whose status is set refits its own splits; anything outside the device form
refits every fold of every split with kfold.refit_predictions.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from .kfold import MAX_FOLDS, _decline_blocks, _dims, _fold_means, _host, _stats_why, repeated_fold_ids
from .permutation import _device_numerators, _groups, _refit_numerators

_ENTRIES = ("kfold_xcov", "kfold_inner", "kfold_epilogue_splits", "mttkrp", "xcov")
_ENTRIES_COUPLED = ("kfold_xcov", "kfold_inner_coupled", "kfold_combine_scores", "kfold_epilogue_splits", "mttkrp", "xcov")


def _splits_per_pass(Xs, K: int, S: int, I: int) -> int:
    """floor(32 / K) splits, at most floor(I / K) (n <= I models) and S, fewer while the n models' loadings exceed the LDS of the
    score pass of any block (permutation._groups per block)."""
    return min(_groups(None, X, K, min(S, I // K)) for X in Xs)


def _device_splits(pls, Xs, Y, ids: np.ndarray, K: int, G: int, tol: float, max_iter: int, coupled: bool):
    """The device form (a ctPLS: the coupled kernels, one block included): (numerators S x R with NaN rows for failed passes,
    n_iter per split (None: failed), passes, failed pass messages, reads of each block) or (None, why) when it does not run at all.
    A block view's own fields are S, mean, WA, WB, Wa, Wb and Rm; every other field is one buffer shared by the views."""
    from .tpls import _as_torch_dtype, to_device_copy

    eng = pls._get_engine()
    be = eng.be
    R = pls.n_components
    nb = len(Xs)
    NS, I = ids.shape
    Yh = _host(Y).reshape(I, -1).astype(np.float64)
    M = Yh.shape[1]
    dev = be.device
    nums = np.full((NS, R), np.nan)
    n_iters = [None] * NS
    notes = []
    passes, reads = 0, 0
    with eng.device_ctx():
        X2s, dims = [], []
        for X in Xs:
            Xd = to_device_copy(X, _as_torch_dtype(pls._dtype, X), dev, copy=False)  # a device tensor of the storage type: as it is
            X2s.append(Xd.view(I, -1))
            dims.append(_dims(X))
        t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
        Yd = t(Yh)
        ydev = t(Yh - Yh.mean(axis=0))                                                # shared by every split
        NT, stride = be.kfold_row_tiles(I)
        kk = torch.arange(K, device=dev)
        for g0 in range(0, NS, G):
            g = min(G, NS - g0)
            n = K * g
            shared = {
                "fold_of": t(ids[g0:g0 + g], torch.int32), "Yk": be.empty(n, I, M), "Gy": be.empty(n, NT, M, M), "Q": be.zeros(n, R, M),
                "T": be.zeros(n, I, R), "Gt": be.zeros(n, R, R), "coef": be.zeros(n, R, R), "tm": be.empty(I, n),
                "Tout": be.zeros(g, I, R), "vec": be.zeros(n, 3 * R + M + 2), "n_iter": torch.zeros(n, R, dtype=torch.int32, device=dev),
                "status": torch.zeros(n, dtype=torch.int32, device=dev), "part": be.empty(n, NT, stride),
            }
            own = [{"S": be.empty(n, M, A * B), "mean": be.empty(n, A * B), "WA": be.empty(A, n), "WB": be.empty(B, n),
                    "Wa": be.zeros(n, R, A), "Wb": be.zeros(n, R, B), "Rm": be.zeros(n, R, A * B)} for A, B in dims]
            nu, rows = [], []
            for j in range(g):                                                        # split g0 + j: models j K .. j K + K - 1
                order, off, _, nu_j = _fold_means(Yh, ids[g0 + j], K)                 # kfold._fold_y's bits
                order_d, off_d, nu_d = t(order, torch.int32), t(off, torch.int32), t(nu_j)
                nudev = t(nu_j - Yh.mean(axis=0))
                sl = slice(j * K, (j + 1) * K)
                train = (shared["fold_of"][j].long().unsqueeze(0) != kk.unsqueeze(1)).unsqueeze(2)          # K x I x 1
                shared["Yk"][sl] = torch.where(train, Yd.unsqueeze(0) - nu_d.unsqueeze(1), 0.0)
                for b in range(nb):                                                   # one read of each block per split
                    A, B = dims[b]
                    stats = be.kfold_xcov(X2s[b], A, B, ydev, order_d, off_d, K, nudev, own[b]["S"][sl], own[b]["mean"][sl])
                    pre = f"block {b}: " if coupled else ""
                    if stats is None:
                        return None, f"{pre}shape outside cmtfpls_kfold_xcov"
                    if passes == 0 and j == 0:
                        why = _stats_why(stats, A * B, I, eng.opt.xcov_raw_max_offset, f"block {b}" if coupled else "X")
                        if why is not None:
                            return None, why
                nu.append(nu_d)
                order_l = order_d.long()
                rows.append([order_l[int(off[k]):int(off[k + 1])] for k in range(K)])
            views = [_lib.KfoldState(I, A, B, M, n, R, *[(o[f] if f in o else shared[f]).data_ptr() for f, _ in _lib.KfoldState._fields_[6:]])
                     for (A, B), o in zip(dims, own)]
            st = (_lib.KfoldState * nb)(*views)
            if coupled:
                ws = torch.empty(max(be.kfold_inner_coupled_workspace_bytes(st), 256), dtype=torch.uint8, device=dev)
                inner = lambda a: be.kfold_inner_coupled(st, a, tol, max_iter, ws)
            else:
                ws = torch.empty(max(be.kfold_inner_workspace_bytes(*dims[0], n), 256), dtype=torch.uint8, device=dev)
                inner = lambda a: be.kfold_inner(st[0], a, tol, max_iter, ws)
            scs = be.empty(nb, I, n)
            sc = scs[0] if not coupled else be.empty(I, n)
            rs = be.empty(n * max(A * B for A, B in dims))
            if be.kfold_epilogue_splits(st[0], g, 0, 0, None) is None:
                return None, "shape outside cmtfpls_kfold_epilogue_splits_f64"
            for a in range(R):
                if inner(a) is None:
                    return None, "shape outside cmtfpls_kfold_inner_coupled_f64" if coupled else "shape outside cmtfpls_kfold_inner_f64"
                for b in range(nb):                                                   # X_b,0 [w_1 .. w_n]: one read each
                    if be.mttkrp(X2s[b], *dims[b], own[b]["WA"], own[b]["WB"], scs[b]) is None:
                        return None, "the models' loadings outside cmtfpls_mttkrp_*"
                if coupled:
                    be.kfold_combine_scores(scs, sc)                                  # t: the average of the blocks' scores
                be.kfold_epilogue_splits(st[0], g, 1, a, sc)
                if a + 1 < R:
                    for b in range(nb):                                               # X_b,0^T [t_m * train_m]: one read each
                        r = rs[: n * X2s[b].shape[1]].view(n, X2s[b].shape[1])
                        be.xcov(X2s[b], shared["tm"], False, out=r)
                        be.kfold_epilogue_splits(st[b], g, 2, a, r)
            num = torch.cat([_device_numerators(shared["Tout"][j:j + 1], shared["coef"][j * K:(j + 1) * K], shared["Q"][j * K:(j + 1) * K],
                                                nu[j].unsqueeze(0), Yd.unsqueeze(0), rows[j], K, 1, R, M) for j in range(g)])
            status = shared["status"].cpu().numpy()
            n_iter = shared["n_iter"].cpu().numpy().reshape(g, K, R)
            num = num.cpu().numpy()
            passes += 1
            reads += g + 2 * R - 1
            if status.any():
                bad = np.flatnonzero(status)
                notes.append(f"pass {passes - 1} (splits {g0}..{g0 + g - 1}): non-finite loadings or coefficients in models "
                             f"{bad.tolist()}, refitted")
                continue
            nums[g0:g0 + g] = num
            for j in range(g):
                n_iters[g0 + j] = n_iter[j].tolist()
    return nums, n_iters, passes, notes, reads


def repeated_kfold(pls, n_splits: int = 5, n_repeats: int = 10, folds=None, random_state=0, per_component: bool = False,
                   device_folds: bool = True, tol: float = 1e-8, max_iter: int = 100) -> dict:
    from .cmtf import ctPLS

    coupled = isinstance(pls, ctPLS)
    if coupled:
        assert getattr(pls, "original_Xs", None) is not None, "PLS Tensor must be fit prior to calculating Q2Y"
        X, Y = list(pls.original_Xs), pls.original_Y
    else:
        assert getattr(pls, "original_X", None) is not None, "PLS Tensor must be fit prior to calculating Q2Y"
        X, Y = pls.original_X, pls.original_Y
    Xs = X if coupled else [X]
    I = Y.shape[0]
    ids, K = repeated_fold_ids(I, n_splits, n_repeats, random_state, folds)
    NS = ids.shape[0]
    R = pls.n_components
    den = float((_host(Y).astype(np.float64) ** 2).sum())

    why: Optional[str] = None
    G = 0
    if not device_folds:
        why = "device folds switched off"
    else:
        G = _splits_per_pass(Xs, K, NS, I) if K <= MAX_FOLDS else 0
        names = [f"block {b}" for b in range(len(Xs))] if coupled else ["X"]
        why = _decline_blocks(pls, Xs, names, Y, K * G if G else K, _ENTRIES_COUPLED if coupled else _ENTRIES)   # K: the n models
    nums = np.full((NS, R), np.nan)
    n_iters = [None] * NS
    passes, notes, reads = 0, [], 0
    if why is None:
        out = _device_splits(pls, Xs, Y, ids, K, G, tol, max_iter, coupled)
        if out[0] is None:
            why = out[1]
        else:
            nums, n_iters, passes, notes, reads = out
            if notes:
                why = "; ".join(notes)
    identity = np.arange(I)
    for g in range(NS):                                                              # the refit path: whatever the device left
        if n_iters[g] is None:
            nums[g], n_iters[g] = _refit_numerators(pls, X, Y, ids[g], K, identity, tol, max_iter)
    q_all = 1.0 - nums / den                                                          # S x R: every component count
    q2y = q_all if per_component else q_all[:, -1]
    if passes:
        entries = ("cmtfpls_kfold_xcov_* per split, cmtfpls_kfold_inner_f64, cmtfpls_mttkrp_*, cmtfpls_kfold_epilogue_splits_f64, "
                   "cmtfpls_xcov_*") if not coupled else \
                  ("cmtfpls_kfold_xcov_* per split, cmtfpls_kfold_inner_coupled_f64, cmtfpls_mttkrp_*, cmtfpls_kfold_combine_scores_f64, "
                   "cmtfpls_kfold_epilogue_splits_f64, cmtfpls_xcov_*")
        form = f"{K * G} models per pass ({G} splits x {K} folds) from shared reads of {'every block' if coupled else 'X'} ({entries})"
        if notes:
            form += "; failed passes refitted per fold on the regular engine"
    else:
        form = "one refit per fold and split on the regular engine"
    x_reads = None
    if passes:
        x_reads = [reads] * len(Xs) if coupled else reads
    rep = {"form": form, "splits": int(NS), "passes": int(passes), "splits_per_pass": int(G) if passes else None,
           "x_reads": x_reads, "n_iter": n_iters}
    if why is not None:
        rep["why"] = why
    pls.q2y_report_ = rep
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
