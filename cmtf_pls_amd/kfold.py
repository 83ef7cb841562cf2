"""K-fold cross-validated predictions of a tPLS or ctPLS model (validate.kfold_predictions / get_q2y_kfold).

Device form: the folds share every read of the caller's uncentred X.  Per component a, all K folds at once:
  kfold_inner      the inner loop of every fold on its training cross-covariance S_k       (a workgroup per fold, no X)
  mttkrp           X_0 [w_1,a .. w_K,a]: every row's score under every fold's loadings        one read of X
  kfold_epilogue 1 t_k = X_0 w_k - (mu_k^T w_k) 1 - T_k g_k; the held-out rows' t_k is the projection predict makes;
                   inner regression on the training rows, Y side, Gy
  xcov             X_0^T [t_1 * train_1 .. t_K * train_K]                                      one read of X (not after the last)
  kfold_epilogue 2 the down-date of S_k (fitrun_xcov._finish_xcov_nowrite's algebra)
Before the first component kfold_xcov builds every S_k from one read (the all-minus-own identity).  2R reads of X in all,
nothing written to X, no copy of it.  NIPALS components are sequential and coef_ is upper triangular, so the predictions
with the first r components are those of an r-component model: every component count comes out of one run.

A ctPLS runs the same steps per block with the score shared (device_predictions_coupled): kfold_inner_coupled goes
through the blocks inside each fold's workgroup, one MTTKRP per block, the blocks' scores averaged (kfold_combine_scores), stage 1
once on the shared t, one contraction and stage 2 per block: 2R reads of each block.

Anything outside the device form refits once per fold on the regular engine (X[train] -> fit -> transform of X[test]).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

MAX_FOLDS, MAX_RESPONSES, MAX_COMPONENTS, MAX_SIDE = 32, 64, 64, 256
MAX_BLOCKS = 8                    # blocks of a coupled model (cmtfpls_kfold_inner_coupled_f64)


def fold_ids(n_samples: int, n_splits: int = 5, folds=None) -> Tuple[np.ndarray, int]:
    """Fold id of every sample and the number of folds.  folds=None: contiguous folds with the sizes of sklearn's
    KFold(n_splits, shuffle=False) (the first n_samples % n_splits folds one sample larger); otherwise `folds` itself, an
    integer array of length n_samples with ids 0..K-1 (shuffled, stratified or grouped splits)."""
    if folds is None:
        K = int(n_splits)
        if K < 2:
            raise ValueError(f"n_splits must be at least 2, got {n_splits}")
        if K > n_samples:
            raise ValueError(f"n_splits = {K} is larger than the number of samples ({n_samples}): a fold would be empty")
        sizes = np.full(K, n_samples // K, dtype=np.int64)
        sizes[: n_samples % K] += 1
        return np.repeat(np.arange(K, dtype=np.int64), sizes), K
    f = np.asarray(folds)
    if f.ndim != 1 or f.shape[0] != n_samples:
        raise ValueError(f"folds must be a 1-d array of length {n_samples}, got shape {f.shape}")
    if f.dtype.kind not in "iu":
        if f.dtype.kind != "f" or not np.all(np.isfinite(f)) or not np.all(f == np.round(f)):
            raise ValueError("folds must hold integer fold ids")
    f = f.astype(np.int64)
    if f.min() < 0:
        raise ValueError(f"fold id out of range: {int(f.min())} (ids are 0..K-1)")
    K = int(f.max()) + 1
    if K < 2:
        raise ValueError("folds must hold at least two folds")
    empty = np.flatnonzero(np.bincount(f, minlength=K) == 0)
    if empty.size:
        raise ValueError(f"fold {int(empty[0])} is empty (ids must cover 0..{K - 1})")
    return f, K


def repeated_fold_ids(n_samples: int, n_splits: int = 5, n_repeats: int = 10, random_state=0, folds=None) -> Tuple[np.ndarray, int]:
    """The (S, n_samples) fold ids of S shuffled K-fold splits and K.  folds=None: the test folds of sklearn's
    RepeatedKFold(n_splits, n_repeats, random_state=int) in its order (one RandomState(random_state) shuffles arange(n_samples)
    once per repeat; contiguous blocks of the shuffled index are folds 0..K-1 with KFold's sizes); otherwise `folds` itself, an
    (S, n_samples) integer array, each row checked as fold_ids checks a split, with the same K in every row."""
    if folds is None:
        if isinstance(random_state, bool) or not isinstance(random_state, (int, np.integer)):
            raise ValueError(f"random_state must be an int (reproducible splits), got {random_state!r}")
        if int(n_repeats) < 1:
            raise ValueError(f"n_repeats must be at least 1, got {n_repeats}")
        base, K = fold_ids(n_samples, n_splits)                   # KFold's contiguous fold of every position
        rs = np.random.RandomState(int(random_state))
        ids = np.empty((int(n_repeats), n_samples), dtype=np.int64)
        for g in range(int(n_repeats)):
            idx = np.arange(n_samples)
            rs.shuffle(idx)
            ids[g, idx] = base                                    # sample idx[j] is in the fold of position j
        return ids, K
    f = np.asarray(folds)
    if f.ndim != 2 or f.shape[1] != n_samples or f.shape[0] < 1:
        raise ValueError(f"folds must be an (S, {n_samples}) array of fold ids with S >= 1, got shape {f.shape}")
    rows = [fold_ids(n_samples, folds=row) for row in f]
    Ks = sorted({K for _, K in rows})
    if len(Ks) != 1:
        raise ValueError(f"every split must have the same number of folds, got {Ks}")
    return np.stack([r for r, _ in rows]), Ks[0]


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _from_scores(scores: np.ndarray, coef: np.ndarray, Qrows: np.ndarray, y_mean: np.ndarray, r: int) -> np.ndarray:
    """What an r-component model predicts from the first r scores: scores @ coef_ @ Q^T + Y_mean (tpls.py:143)."""
    return (scores[:, :r] @ coef[:r, :r]) @ Qrows[:r] + y_mean


def _rows(X, sel: np.ndarray):
    """X[sel] for a boolean row mask; a device tensor by index_select on its device."""
    if isinstance(X, torch.Tensor):
        return X.index_select(0, torch.from_numpy(np.flatnonzero(sel)).to(X.device))
    return X[sel]


def refit_predictions(pls, X, Y, ids: np.ndarray, K: int, tol: float, max_iter: int):
    """One literal refit per fold on the regular engine with the model's storage type, algorithm, backend and options:
    returns (pred (R, I, M), n_iter K x R).  X a list of blocks: ctPLS refits (each block's rows taken alike)."""
    from .cmtf import ctPLS
    from .tpls import tPLS

    coupled = isinstance(X, list)
    R = pls.n_components
    I = ids.shape[0]
    Y2 = Y.reshape(I, -1)
    pred = np.zeros((R, I, Y2.shape[1]))
    n_iter = []
    for k in range(K):
        test = ids == k
        if coupled:
            Xtr, Xte = [_rows(b, ~test) for b in X], [_rows(b, test) for b in X]
        else:
            Xtr, Xte = _rows(X, ~test), _rows(X, test)
        Ytr = Y[torch.from_numpy(~test).to(Y.device)] if isinstance(Y, torch.Tensor) else Y[~test]
        m = (ctPLS if coupled else tPLS)(R, dtype=pls._dtype, device=pls._device, backend=pls._backend, algorithm=pls._algorithm,
                                         graphs=pls._graphs, matrix_precision="f32" if pls._mixed else "f64", options=pls._options)
        m.fit(Xtr, Ytr, tol=tol, max_iter=max_iter)
        scores = m.transform(Xte)
        for r in range(1, R + 1):
            pred[r - 1, test] = _from_scores(scores, m.coef_, m.Y_factors[1].T, m.Y_mean, r)
        n_iter.append([int(v) for v in m.n_iter_])
    return pred, n_iter


def _dims(X) -> Tuple[int, int]:
    return (1, X.shape[1]) if X.ndim == 2 else (X.shape[1], X.shape[2])


def _decline_blocks(pls, Xs, names, Y, K: int, entries) -> Optional[str]:
    """Why the device form does not take these blocks / this Y (None: it does, as far as can be told before reading them)."""
    eng = pls._get_engine()
    be = eng.be
    if not all(hasattr(be, f) for f in entries):
        kind = "coupled " if "kfold_inner_coupled" in entries else ""
        return f"the {getattr(be, 'name', type(be).__name__)} backend has no {kind}K-fold kernels"
    if pls._comm is not None:
        return "sharded model (comm)"
    if len(Xs) > MAX_BLOCKS:
        return f"{len(Xs)} blocks > {MAX_BLOCKS}"
    for X, name in zip(Xs, names):
        if X.ndim not in (2, 3):
            return f"{name} of order {X.ndim} (the device form takes order 2 and 3)"
    M = int(np.prod(Y.shape[1:])) if Y.ndim > 1 else 1
    R = pls.n_components
    if K > MAX_FOLDS:
        return f"K = {K} folds > {MAX_FOLDS}"
    if M > MAX_RESPONSES:
        return f"M = {M} responses > {MAX_RESPONSES}"
    if R > MAX_COMPONENTS:
        return f"R = {R} components > {MAX_COMPONENTS}"
    for X, name in zip(Xs, names):
        A, B = _dims(X)
        pre = "" if name == "X" else f"{name}: "
        if min(A, B) > MAX_SIDE:
            return f"{pre}min(J, K) = {min(A, B)} > {MAX_SIDE}"
        if (A + B) * 16 * ((K + 15) // 16) * 8 > 152 * 1024:
            return f"{pre}the folds' loadings exceed the LDS of the score pass (cmtfpls_mttkrp_*)"
    if np.isnan(_host(Y)).any():
        return "missing values in Y"
    for X, name in zip(Xs, names):
        if not isinstance(X, torch.Tensor) and np.isnan(np.asarray(X)).any():
            return f"missing values in {name}"
    return None


def _decline(pls, X, Y, ids, K) -> Optional[str]:
    """Why the device form does not take this model / data (None: it does, as far as can be told before reading X)."""
    return _decline_blocks(pls, [X], ["X"], Y, K, ("kfold_xcov", "kfold_inner", "kfold_epilogue", "mttkrp", "xcov"))


def _fold_means(Yh: np.ndarray, ids: np.ndarray, K: int):
    """The fold-sorted row order and offsets, the mean of all rows and each fold's training means nu of Y."""
    I = Yh.shape[0]
    counts = np.bincount(ids, minlength=K)
    order = np.argsort(ids, kind="stable").astype(np.int32)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ybar = Yh.mean(axis=0)
    colsum = Yh.sum(axis=0)
    nu = np.stack([(colsum - Yh[ids == k].sum(axis=0)) / (I - counts[k]) for k in range(K)])   # training means of Y
    return order, off, ybar, nu


def _fold_y(Yh: np.ndarray, ids: np.ndarray, K: int):
    """What the folds need of Y: _fold_means and each fold's centred training Y (held-out rows 0)."""
    I, M = Yh.shape
    order, off, ybar, nu = _fold_means(Yh, ids, K)
    Yk = np.empty((K, I, M))
    for k in range(K):
        Yk[k] = Yh - nu[k]                                                          # tpls.py:70 on the training rows
        Yk[k][ids == k] = 0.0
    return order, off, ybar, nu, Yk


def _stats_why(stats: torch.Tensor, P: int, I: int, max_offset: float, name: str) -> Optional[str]:
    """From the column sums / sums of squares of kfold_xcov: non-finite values, or an offset the uncentred form cannot take."""
    sh = stats.cpu().numpy()
    if not np.all(np.isfinite(sh)):
        return f"missing (or non-finite) values in {name}"
    cm = sh[:P] / I
    spread = math.sqrt(max(float(np.mean(sh[P:] / I - cm * cm)), 0.0))
    top = float(np.abs(cm).max())
    ratio = 0.0 if top == 0.0 else (top / spread if spread > 0.0 else float("inf"))
    if not ratio <= max_offset:
        pre = "" if name == "X" else f"{name}: "
        return f"{pre}max|column mean| / spread = {ratio:.3g} > {max_offset:g} (the uncentred form would lose digits)"
    return None


def _held_out_predictions(Tout, coef, Qh, nu, ids, K, R, M) -> np.ndarray:
    pred = np.empty((R, ids.shape[0], M))
    for k in range(K):
        rows = ids == k
        for r in range(1, R + 1):
            pred[r - 1, rows] = _from_scores(Tout[rows], coef[k], Qh[k], nu[k], r)
    return pred


def device_predictions(pls, X, Y, ids: np.ndarray, K: int, tol: float, max_iter: int, grouped: bool = False):
    """The device form: (pred (R, I, M), report) or (None, why).  grouped=True runs the inner loop and the epilogue through the
    permutation test's grouped entries with model k = fold k in one group (the same bits: tests/test_gpu_permutation.py)."""
    from .tpls import _as_torch_dtype, to_device_copy

    eng = pls._get_engine()
    be = eng.be
    R = pls.n_components
    I = X.shape[0]
    A, B = _dims(X)
    P = A * B
    Yh = _host(Y).reshape(I, -1).astype(np.float64)
    M = Yh.shape[1]
    dev = be.device
    with eng.device_ctx():
        Xd = to_device_copy(X, _as_torch_dtype(pls._dtype, X), dev, copy=False)     # a device tensor of the storage type: as it is
        X2 = Xd.view(I, P)
        order, off, ybar, nu, Yk = _fold_y(Yh, ids, K)
        t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
        S = be.empty(K, M, P)
        mean = be.empty(K, P)
        stats = be.kfold_xcov(X2, A, B, t(Yh - ybar), t(order, torch.int32), t(off, torch.int32), K, t(nu - ybar), S, mean)
        if stats is None:
            return None, "shape outside cmtfpls_kfold_xcov"
        why = _stats_why(stats, P, I, eng.opt.xcov_raw_max_offset, "X")
        if why is not None:
            return None, why
        NT, stride = be.kfold_row_tiles(I)
        buf = {
            "fold_of": t(ids, torch.int32), "S": S, "mean": mean, "Yk": t(Yk), "Gy": be.empty(K, NT, M, M), "WA": be.empty(A, K),
            "WB": be.empty(B, K), "Q": be.zeros(K, R, M), "Wa": be.zeros(K, R, A), "Wb": be.zeros(K, R, B), "T": be.zeros(K, I, R),
            "Gt": be.zeros(K, R, R), "coef": be.zeros(K, R, R), "Rm": be.zeros(K, R, P), "tm": be.empty(I, K), "Tout": be.zeros(I, R),
            "vec": be.zeros(K, 3 * R + M + 2), "n_iter": torch.zeros(K, R, dtype=torch.int32, device=dev),
            "status": torch.zeros(K, dtype=torch.int32, device=dev), "part": be.empty(K, NT, stride),
        }
        st = _lib.KfoldState(I, A, B, M, K, R, *[b.data_ptr() for b in (buf[f] for f, _ in _lib.KfoldState._fields_[6:])])
        ws = torch.empty(max(be.kfold_inner_workspace_bytes(A, B, K), 256), dtype=torch.uint8, device=dev)
        sc = be.empty(I, K)
        rs = be.empty(K, P)
        if grouped:
            mf = torch.arange(K, dtype=torch.int32, device=dev)
            inner = lambda a: be.kfold_inner_grouped(st, mf, 1, a, tol, max_iter, ws)
            epilogue = lambda stage, a, src: be.kfold_epilogue_grouped(st, mf, 1, stage, a, src)
        else:
            inner = lambda a: be.kfold_inner(st, a, tol, max_iter, ws)
            epilogue = lambda stage, a, src: be.kfold_epilogue(st, stage, a, src)
        if epilogue(0, 0, None) is None:
            return None, "shape outside cmtfpls_kfold_epilogue_f64"
        for a in range(R):
            if inner(a) is None:
                return None, "shape outside cmtfpls_kfold_inner_f64"
            if be.mttkrp(X2, A, B, buf["WA"], buf["WB"], sc) is None:                   # X_0 [w_1 .. w_K]: one read
                return None, "the folds' loadings outside cmtfpls_mttkrp_*"
            epilogue(1, a, sc)
            if a + 1 < R:
                be.xcov(X2, buf["tm"], False, out=rs)                                   # X_0^T [t_k * train_k]: one read
                epilogue(2, a, rs)
        status = buf["status"].cpu().numpy()
        if status.any():
            return None, f"non-finite loadings or coefficients in folds {np.flatnonzero(status).tolist()} of the device form"
        n_iter = buf["n_iter"].cpu().numpy()
        Tout = buf["Tout"].cpu().numpy()
        coef = buf["coef"].cpu().numpy()
        Qh = buf["Q"].cpu().numpy()
    pred = _held_out_predictions(Tout, coef, Qh, nu, ids, K, R, M)
    report = {"form": "K folds from shared reads of X (cmtfpls_kfold_xcov_*, cmtfpls_kfold_inner_f64, cmtfpls_mttkrp_*, "
                      "cmtfpls_kfold_epilogue_f64, cmtfpls_xcov_*)",
              "folds": int(K), "x_reads": 2 * R, "n_iter": n_iter.tolist()}
    return pred, report


_SHARED = ("fold_of", "Yk", "Gy", "Q", "T", "Gt", "coef", "tm", "Tout", "vec", "n_iter", "status", "part")


def device_predictions_coupled(pls, Xs, Y, ids: np.ndarray, K: int, tol: float, max_iter: int):
    """The device form of a ctPLS: (pred (R, I, M), report) or (None, why).  Each block has a state view of its own (S, mean,
    loadings, X_c^T t); the Y side, the scores and the solve are one set of buffers shared by every view.  Per component: the
    coupled inner loop, one MTTKRP per block, the blocks' scores averaged, stage 1 once, and per block one contraction and its
    down-date: 2R reads of each block for all folds."""
    from .tpls import _as_torch_dtype, to_device_copy

    eng = pls._get_engine()
    be = eng.be
    R = pls.n_components
    nb = len(Xs)
    I = Xs[0].shape[0]
    Yh = _host(Y).reshape(I, -1).astype(np.float64)
    M = Yh.shape[1]
    dev = be.device
    with eng.device_ctx():
        order, off, ybar, nu, Yk = _fold_y(Yh, ids, K)
        t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
        NT, stride = be.kfold_row_tiles(I)
        shared = {
            "fold_of": t(ids, torch.int32), "Yk": t(Yk), "Gy": be.empty(K, NT, M, M), "Q": be.zeros(K, R, M), "T": be.zeros(K, I, R),
            "Gt": be.zeros(K, R, R), "coef": be.zeros(K, R, R), "tm": be.empty(I, K), "Tout": be.zeros(I, R),
            "vec": be.zeros(K, 3 * R + M + 2), "n_iter": torch.zeros(K, R, dtype=torch.int32, device=dev),
            "status": torch.zeros(K, dtype=torch.int32, device=dev), "part": be.empty(K, NT, stride),
        }
        ydev, order_d, off_d, nudev = t(Yh - ybar), t(order, torch.int32), t(off, torch.int32), t(nu - ybar)
        X2s, dims, own, views = [], [], [], []
        for b, X in enumerate(Xs):
            Xd = to_device_copy(X, _as_torch_dtype(pls._dtype, X), dev, copy=False)  # a device tensor of the storage type: as it is
            A, B = _dims(X)
            P = A * B
            X2 = Xd.view(I, P)
            S = be.empty(K, M, P)
            mean = be.empty(K, P)
            stats = be.kfold_xcov(X2, A, B, ydev, order_d, off_d, K, nudev, S, mean)
            if stats is None:
                return None, f"block {b}: shape outside cmtfpls_kfold_xcov"
            why = _stats_why(stats, P, I, eng.opt.xcov_raw_max_offset, f"block {b}")
            if why is not None:
                return None, why
            o = {"S": S, "mean": mean, "WA": be.empty(A, K), "WB": be.empty(B, K), "Wa": be.zeros(K, R, A), "Wb": be.zeros(K, R, B),
                 "Rm": be.zeros(K, R, P)}
            views.append(_lib.KfoldState(I, A, B, M, K, R, *[(o[f] if f in o else shared[f]).data_ptr()
                                                             for f, _ in _lib.KfoldState._fields_[6:]]))
            X2s.append(X2)
            dims.append((A, B))
            own.append(o)
        st = (_lib.KfoldState * nb)(*views)
        ws = torch.empty(max(be.kfold_inner_coupled_workspace_bytes(st), 256), dtype=torch.uint8, device=dev)
        scs = be.empty(nb, I, K)
        sc = be.empty(I, K)
        rs = be.empty(K * max(A * B for A, B in dims))
        if be.kfold_epilogue(st[0], 0, 0, None) is None:
            return None, "shape outside cmtfpls_kfold_epilogue_f64"
        for a in range(R):
            if be.kfold_inner_coupled(st, a, tol, max_iter, ws) is None:
                return None, "shape outside cmtfpls_kfold_inner_coupled_f64"
            for b in range(nb):                                                         # X_b,0 [w_b,1 .. w_b,K]: one read each
                if be.mttkrp(X2s[b], *dims[b], own[b]["WA"], own[b]["WB"], scs[b]) is None:
                    return None, f"block {b}: the folds' loadings outside cmtfpls_mttkrp_*"
            be.kfold_combine_scores(scs, sc)                                            # t: the average of the blocks' scores
            be.kfold_epilogue(st[0], 1, a, sc)
            if a + 1 < R:
                for b in range(nb):                                                     # X_b,0^T [t_k * train_k]: one read each
                    r = rs[: K * X2s[b].shape[1]].view(K, X2s[b].shape[1])
                    be.xcov(X2s[b], shared["tm"], False, out=r)
                    be.kfold_epilogue(st[b], 2, a, r)
        status = shared["status"].cpu().numpy()
        if status.any():
            return None, f"non-finite loadings or coefficients in folds {np.flatnonzero(status).tolist()} of the device form"
        n_iter = shared["n_iter"].cpu().numpy()
        Tout = shared["Tout"].cpu().numpy()
        coef = shared["coef"].cpu().numpy()
        Qh = shared["Q"].cpu().numpy()
    pred = _held_out_predictions(Tout, coef, Qh, nu, ids, K, R, M)
    report = {"form": "K folds from shared reads of every block (cmtfpls_kfold_xcov_*, cmtfpls_kfold_inner_coupled_f64, "
                      "cmtfpls_mttkrp_*, cmtfpls_kfold_combine_scores_f64, cmtfpls_kfold_epilogue_f64, cmtfpls_xcov_*)",
              "folds": int(K), "x_reads": [2 * R] * nb, "n_iter": n_iter.tolist()}
    return pred, report


def kfold_run(pls, n_splits: int = 5, folds=None, tol: float = 1e-8, max_iter: int = 100, device_folds: bool = True) -> np.ndarray:
    """pred (R, *Y.shape): pred[r - 1, i] = prediction for sample i by the model fitted without sample i's fold, with its first
    r components.  `pls` a fitted tPLS or ctPLS.  Sets pls.q2y_report_."""
    from .cmtf import ctPLS

    coupled = isinstance(pls, ctPLS)
    if coupled:
        assert getattr(pls, "original_Xs", None) is not None, "PLS Tensor must be fit prior to calculating Q2Y"
        X, Y = list(pls.original_Xs), pls.original_Y
    else:
        assert getattr(pls, "original_X", None) is not None, "PLS Tensor must be fit prior to calculating Q2Y"
        X, Y = pls.original_X, pls.original_Y
    I = Y.shape[0]
    ids, K = fold_ids(I, n_splits, folds)
    R = pls.n_components
    if not device_folds:
        why = "device folds switched off"
    elif coupled:
        why = _decline_blocks(pls, X, [f"block {b}" for b in range(len(X))], Y, K,
                              ("kfold_xcov", "kfold_inner_coupled", "kfold_combine_scores", "kfold_epilogue", "mttkrp", "xcov"))
    else:
        why = _decline(pls, X, Y, ids, K)
    pred = None
    if why is None:
        pred, rep = (device_predictions_coupled if coupled else device_predictions)(pls, X, Y, ids, K, tol, max_iter)
        if pred is None:
            why = rep
    if pred is None:
        pred, n_iter = refit_predictions(pls, X, Y, ids, K, tol, max_iter)
        rep = {"form": "one refit per fold on the regular engine", "folds": int(K), "x_reads": None, "n_iter": n_iter, "why": why}
    pls.q2y_report_ = rep
    return pred.reshape((R,) + tuple(Y.shape))
