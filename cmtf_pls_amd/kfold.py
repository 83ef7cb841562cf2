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

A ctPLS runs the same steps per block with the score shared (device_predictions): kfold_inner_coupled goes through
the blocks inside each fold's workgroup, one MTTKRP per block, the blocks' scores averaged (kfold_combine_scores), stage 1 once on
the shared t, one contraction and stage 2 per block: 2R reads of each block.

A tPLS whose X has order 4 (I x A x B1 x B2), with EngineOptions.tensor_folds: every step above on the I x A x B1 B2
view with the Kronecker loading wB = wK (x) wL; only the inner loop differs (kfold_inner_tensor: the rank-1 CP of each fold's
A x B1 x B2 cross-covariance inside its workgroup).  The bootstrap's weighted models take the same entry and carry wK / wL out of it
(bootstrap.py).  A ctPLS with blocks of order 4, with EngineOptions.tensor_folds_coupled (DESIGN
8n): the coupled steps with every order-4 block seen that way; only the inner loop differs (kfold_inner_coupled_tensor).

Anything outside the device form refits once per fold on the regular engine (X[train] -> fit -> transform of X[test]).

The permutation test (permutation.py), repeated K-fold (repeated.py), nested K-fold (nested.py) and the bootstrap (bootstrap.py)
run the same state with more models per pass, and share every step of a driver with kfold_run, each defined here once:
  _route            which way the fitted data goes: device folds off, the masked tPLS or coupled form, the device passes, refits only
                    (a driver's own precedence and option gate are its arguments); _masked_declined words a masked decline
  _device_pass      one pass: every block's S and mean built by the driver's read (allocation, the "shape outside" wording, the
                    statistics check of the first pass), then _state (a view per block) and _components, which makes every launch
                    with the inner and epilogue entries of the form, chosen from _INNER_ENTRIES and _EPILOGUE_ENTRIES; a driver's
                    run() keeps the Y side of its models and what it reads from the state; _weighted_models is the count side
                    of the two weighted drivers
  _device_passes    runs the passes and refits whatever they leave
  _passes_report    the report of a driver of passes (form from _form_entries, x_reads, passes, its own keys, why, rank1), and
                    _masked_run_report a masked run's report as such a driver's; _models_report is the skeleton and status table of
                    masked_models_report and masked_coupled_report
  _masked_setup     what the three masked routines check and upload before they look at X

Missing values in X (opt-in): a tPLS with EngineOptions.masked_folds refits every fold in a workgroup of cmtfpls_cv_masked_f64
(masked_predictions) or, count-weighted, of cmtfpls_cv_masked_models_f64 (masked_models); a ctPLS with
EngineOptions.masked_folds_coupled and a NaN in at least one block refits every model in a workgroup of
cmtfpls_cv_masked_coupled_f64 (masked_models_coupled, masked_predictions_coupled).  A tPLS whose X has order 4 and a NaN,
with EngineOptions.masked_tensor_folds: the same two routines through cmtfpls_cv_masked_tensor_f64 and
cmtfpls_cv_masked_tensor_models_f64, the rank-1 CP of the fold's contraction inside its workgroup.  A ctPLS with a
block of order 4 and a NaN in some block, with EngineOptions.masked_tensor_folds_coupled: masked_models_coupled through
cmtfpls_cv_masked_coupled_tensor_f64, the CP of every order-4 block's contraction inside the model's workgroup.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .backend import _int_pairs, _scratch
from .cmtf import ctPLS
from .storage import FOLDS_WHY, HALF_ENTRIES, _as_torch_dtype, half_route, notes_of, reports_storage, to_device_copy, to_device_read
from .tpls import tPLS

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
    R = pls.n_components
    I = ids.shape[0]
    Y2 = Y.reshape(I, -1)
    pred = np.zeros((R, I, Y2.shape[1]))
    n_iter = []
    for k in range(K):
        test = ids == k
        pred[:, test], it = refit_fold(pls, X, Y, test, tol, max_iter)
        n_iter.append(it)
    return pred, n_iter


def refit_fold(pls, X, Y, test: np.ndarray, tol: float, max_iter: int):
    """One literal refit on the rows outside the boolean mask `test` (refit_predictions' per-fold step): (the predictions
    (R, n_test, M) of the rows in `test` with the first r = 1..R components, n_iter)."""
    coupled = isinstance(X, list)
    R = pls.n_components
    if coupled:
        Xtr, Xte = [_rows(b, ~test) for b in X], [_rows(b, test) for b in X]
    else:
        Xtr, Xte = _rows(X, ~test), _rows(X, test)
    Ytr = Y[torch.from_numpy(~test).to(Y.device)] if isinstance(Y, torch.Tensor) else Y[~test]
    m = (ctPLS if coupled else tPLS)(R, dtype=pls._dtype, device=pls._device, backend=pls._backend, algorithm=pls._algorithm,
                                     graphs=pls._graphs, matrix_precision="f32" if pls._mixed else "f64", options=pls._options, sparsity=getattr(pls, "sparsity", None))
    m.fit(Xtr, Ytr, tol=tol, max_iter=max_iter)
    scores = m.transform(Xte)
    pred = np.stack([_from_scores(scores, m.coef_, m.Y_factors[1].T, m.Y_mean, r) for r in range(1, R + 1)])
    return pred, [int(v) for v in m.n_iter_]


def _dims(X) -> Tuple[int, int]:
    """(A, B) of the I x A x B view the passes take: order 2 is 1 x J, order 4 (I x A x B1 x B2) is A x B1 B2."""
    if X.ndim == 4:
        return X.shape[1], X.shape[2] * X.shape[3]
    return (1, X.shape[1]) if X.ndim == 2 else (X.shape[1], X.shape[2])


TENSOR_RANK1 = "cp3 in the fold loop"         # q2y_report_["rank1"] of an order-4 run
TENSOR_LDS_CAP = 150 * 1024


def _tensor_dims(Xs, coupled: bool = False):
    """(B1, B2) of a tPLS's order-4 X (the inner loop is then cmtfpls_kfold_inner_tensor_f64), else None.  coupled (a ctPLS with a
    block of order 4): a list with (B1, B2) per block, (0, 0) for a block of another order (the inner loop is then
    cmtfpls_kfold_inner_coupled_tensor_f64), else None."""
    if coupled:
        if not any(X.ndim == 4 for X in Xs):
            return None
        return [(int(X.shape[2]), int(X.shape[3])) if X.ndim == 4 else (0, 0) for X in Xs]
    return (int(Xs[0].shape[2]), int(Xs[0].shape[3])) if len(Xs) == 1 and Xs[0].ndim == 4 else None


# ---- LDS and workspace sizes are the library's alone (include/cmtfpls.h): host arithmetic on a description of the blocks, asked
# before an upload with block pointers of NULL.  dims = [(A, B), ..]; tensor = [(B1, B2), ..], (0, 0) for a block of order 2 or 3.
def _size_blocks(block, dims, tensor=None):
    """The blocks as an array of `block` (_lib.LooCoupledBlock or _lib.CvCoupledBlock) for a size function of the library: order 4
    where tensor has (B1, B2), else 2 (A = 1) or 3."""
    orders = [4 if B2 > 0 else 2 if A == 1 else 3 for (A, _), (_, B2) in zip(dims, tensor or [(0, 0)] * len(dims))]
    return (block * len(dims))(*[block(order=o, A=int(A), B=int(B)) for o, (A, B) in zip(orders, dims)])


def _size_states(dims, M: int):
    """The blocks as an array of _lib.KfoldState for cmtfpls_kfold_inner_coupled_tensor_lds_bytes, which reads A, B and M alone."""
    return (_lib.KfoldState * len(dims))(*[_lib.KfoldState(A=int(A), B=int(B), M=int(M)) for A, B in dims])


def coupled_tensor_lds_bytes(dims, tensor, M: int) -> int:
    """The LDS of a workgroup of cmtfpls_kfold_inner_coupled_tensor_f64, from the library."""
    return _lib.load().cmtfpls_kfold_inner_coupled_tensor_lds_bytes(_size_states(dims, M), len(dims), _int_pairs(tensor))


def masked_tensor_lds_bytes(I: int, A: int, B1: int, B2: int, M: int, R: int) -> int:
    """The LDS of a workgroup of the masked order-4 entries, from the library."""
    return _lib.load().cmtfpls_cv_masked_tensor_lds_bytes(I, A, B1, B2, M, R)


def coupled_lds_bytes(dims, I: int, M: int, R: int) -> int:
    """The LDS of a workgroup of cmtfpls_cv_masked_coupled_f64, from the library."""
    return _lib.load().cmtfpls_cv_masked_coupled_lds_bytes(_size_blocks(_lib.CvCoupledBlock, dims), len(dims), I, M, R)


def _coupled_tensor_masked(what: str, dims, tensor, I: int, M: int, R: int) -> int:
    fn = getattr(_lib.load(), f"cmtfpls_cv_masked_coupled_tensor_{what}_bytes")
    return fn(_size_blocks(_lib.CvCoupledBlock, dims, tensor), len(dims), _int_pairs(tensor), I, M, R)


def coupled_tensor_masked_lds_bytes(dims, tensor, I: int, M: int, R: int) -> int:
    """The LDS of a workgroup of cmtfpls_cv_masked_coupled_tensor_f64, from the library."""
    return _coupled_tensor_masked("lds", dims, tensor, I, M, R)


def coupled_tensor_masked_workspace_bytes(dims, tensor, I: int, M: int, R: int) -> int:
    """The workspace of one resident model of cmtfpls_cv_masked_coupled_tensor_f64, from the library (what a caller sizes
    `max_ws_bytes` by)."""
    return _coupled_tensor_masked("workspace", dims, tensor, I, M, R)


def masked_tensor_side(A: int, B1: int, B2: int) -> int:
    """The largest short side of the three unfoldings of an A x B1 x B2 tensor: the number the masked entries hold against their
    side limit, which the decline texts print next to it (the limits stay on this side)."""
    P = A * B1 * B2
    return max(min(d, P // d) for d in (A, B1, B2))


def _decline_tensor(be, A: int, B1: int, B2: int, M: int) -> Optional[str]:
    """Why cmtfpls_kfold_inner_tensor_f64 does not take an A x B1 x B2 cross-covariance (its limits, checked here before a read)."""
    if not hasattr(be, "kfold_inner_tensor"):
        return f"the {getattr(be, 'name', type(be).__name__)} backend has no order-4 K-fold kernel"
    P = A * B1 * B2
    for mode, d in enumerate((A, B1, B2)):
        if min(d, P // d) > MAX_SIDE:
            return f"mode-{mode} unfolding: min({d}, {P // d}) = {min(d, P // d)} > {MAX_SIDE}"
    lds = _lib.load().cmtfpls_kfold_inner_tensor_lds_bytes(A, B1, B2, M)
    if lds > TENSOR_LDS_CAP:
        return f"the fold's vectors need {lds} bytes of LDS > {TENSOR_LDS_CAP} (cmtfpls_kfold_inner_tensor_f64)"
    return None


def _decline_coupled_tensor(be, dims, tensor, M: int) -> Optional[str]:
    """Why cmtfpls_kfold_inner_coupled_tensor_f64 does not take these blocks (its limits, checked here before a read): per tensor
    block _decline_tensor's unfoldings, then the LDS of all blocks together."""
    if not hasattr(be, "kfold_inner_coupled_tensor"):
        return f"the {getattr(be, 'name', type(be).__name__)} backend has no order-4 coupled K-fold kernel"
    for b, ((A, _), (B1, B2)) in enumerate(zip(dims, tensor)):
        P = A * B1 * B2
        for mode, d in enumerate((A, B1, B2) if B2 > 0 else ()):
            if min(d, P // d) > MAX_SIDE:
                return f"block {b}: mode-{mode} unfolding: min({d}, {P // d}) = {min(d, P // d)} > {MAX_SIDE}"
    lds = coupled_tensor_lds_bytes(dims, tensor, M)
    if lds > TENSOR_LDS_CAP:
        return f"the blocks' vectors need {lds} bytes of LDS > {TENSOR_LDS_CAP} (cmtfpls_kfold_inner_coupled_tensor_f64)"
    return None


def _with_rank1(rep: dict, tensor, passes=True) -> dict:
    """The report of a run whose device passes took an order-4 X: the form names the tensor entry, and `rank1` says where the
    rank-1 CP ran."""
    if tensor is None or not passes:
        return rep
    if isinstance(tensor, list):                                                 # a ctPLS: the coupled tensor entry
        form = rep["form"].replace("cmtfpls_kfold_inner_coupled_grouped_f64", "cmtfpls_kfold_inner_coupled_tensor_f64") \
                          .replace("cmtfpls_kfold_inner_coupled_f64", "cmtfpls_kfold_inner_coupled_tensor_f64")
        return dict(rep, form=form, rank1=TENSOR_RANK1)
    form = rep["form"].replace("cmtfpls_kfold_inner_grouped_f64", "cmtfpls_kfold_inner_tensor_f64") \
                      .replace("cmtfpls_kfold_inner_f64", "cmtfpls_kfold_inner_tensor_f64")
    return dict(rep, form=form, rank1=TENSOR_RANK1)


def _training_data(pls):
    """(X, Y) the model was fitted on; a ctPLS's blocks as a list."""
    from .cmtf import ctPLS

    if isinstance(pls, ctPLS):
        assert getattr(pls, "original_Xs", None) is not None, "PLS Tensor must be fit prior to calculating Q2Y"
        return list(pls.original_Xs), pls.original_Y
    assert getattr(pls, "original_X", None) is not None, "PLS Tensor must be fit prior to calculating Q2Y"
    return pls.original_X, pls.original_Y


def _names(Xs, coupled: bool):
    return [f"block {b}" for b in range(len(Xs))] if coupled else ["X"]


def _loadings_fit(A: int, B: int, n: int) -> bool:
    """Whether n models' loadings of an A x B block fit the LDS of the score pass (cmtfpls_mttkrp_*)."""
    return (A + B) * 16 * ((n + 15) // 16) * 8 <= 152 * 1024


def _groups(X, K: int, P: int) -> int:
    """Entries (permutations, splits) per pass: floor(32 / K), at most P, fewer while the n models' loadings exceed the LDS of the
    score pass."""
    A, B = _dims(X)
    G = min(MAX_FOLDS // K, P)
    while G > 1 and not _loadings_fit(A, B, K * G):
        G -= 1
    return G


def _decline_blocks(pls, Xs, names, Y, K: int, entries, tensor_ok: bool = False) -> Optional[str]:
    """Why the device form does not take these blocks / this Y (None: it does, as far as can be told before reading them).
    tensor_ok: the caller's passes take a tPLS's order-4 X under EngineOptions.tensor_folds (_tensor_dims) and a
    ctPLS's blocks of order 4 under EngineOptions.tensor_folds_coupled."""
    eng = pls._get_engine()
    be = eng.be
    if not all(hasattr(be, f) for f in entries):
        kind = "coupled " if any(e.startswith("kfold_inner_coupled") for e in entries) else ""
        return f"the {getattr(be, 'name', type(be).__name__)} backend has no {kind}K-fold kernels"
    if pls._comm is not None:
        return "sharded model (comm)"
    if len(Xs) > MAX_BLOCKS:
        return f"{len(Xs)} blocks > {MAX_BLOCKS}"
    coupled = any(e.startswith("kfold_inner_coupled") for e in entries)
    tensor = _tensor_dims(Xs, coupled) if tensor_ok and (eng.opt.tensor_folds_coupled if coupled else eng.opt.tensor_folds) else None
    for X, name in zip(Xs, names):
        if X.ndim not in (2, 3) and not (tensor is not None and X.ndim == 4):
            return f"{name} of order {X.ndim} (the device form takes order 2 and 3)"
    M = int(np.prod(Y.shape[1:])) if Y.ndim > 1 else 1
    R = pls.n_components
    if K > MAX_FOLDS:
        return f"K = {K} folds > {MAX_FOLDS}"
    if M > MAX_RESPONSES:
        return f"M = {M} responses > {MAX_RESPONSES}"
    if R > MAX_COMPONENTS:
        return f"R = {R} components > {MAX_COMPONENTS}"
    if coupled and tensor is not None:
        why = _decline_coupled_tensor(be, [_dims(X) for X in Xs], tensor, M)
        if why is not None:
            return why
    for X, name in zip(Xs, names):
        A, B = _dims(X)
        pre = "" if name == "X" else f"{name}: "
        if tensor is not None and not coupled:
            why = _decline_tensor(be, A, *tensor, M)
            if why is not None:
                return why
        if min(A, B) > MAX_SIDE:
            return f"{pre}min(J, K) = {min(A, B)} > {MAX_SIDE}"
        if not _loadings_fit(A, B, K):
            return f"{pre}the folds' loadings exceed the LDS of the score pass (cmtfpls_mttkrp_*)"
    if np.isnan(_host(Y)).any():
        return "missing values in Y"
    for X, name in zip(Xs, names):
        if not isinstance(X, torch.Tensor) and np.isnan(np.asarray(X)).any():
            return f"missing values in {name}"
    return None


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


def _to_dev(a, dev, dt=torch.float64) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)


# the five entries through which the device passes read X: the three builders of S and the mean, the score pass, the contraction
HALF_READS = HALF_ENTRIES["folds"]
# why the routes without 16-bit kernels copy 16-bit storage (the report's storage_fallback under EngineOptions.half_folds)
HALF_MASKED_WHY = "the masked routes (cmtfpls_cv_masked_*) have no 16-bit form and read a float64 upload of the data"
HALF_LOO_WHY = "leave-one-out (cmtfpls_loo_*) takes float64 X and reads a float64 upload of the data"


def _device_blocks(pls, Xs, dev):
    """Each block as (X2, A, B): the device tensor of the storage type (the caller's own when it is one: never copied), I x P.
    16-bit storage: an exact float32 upcast of the rounded data, noted for the report -- or, under EngineOptions.half_folds on a
    backend with the 16-bit form of every entry of HALF_READS, the 16-bit tensor itself: the caller's own, or the once-rounded upload."""
    in_place, why = half_route(pls, "half_folds", HALF_READS)
    blocks = []
    for X in Xs:
        dtype = _as_torch_dtype(pls._dtype, X)                                       # in place: _device_pass notes the entries that read it
        X2 = to_device_copy(X, dtype, dev, copy=False) if in_place else to_device_read(X, dtype, dev, pls=pls, why=why)
        blocks.append((X2.view(X.shape[0], -1), *_dims(X)))
    return blocks


def _state(be, fold_of: torch.Tensor, Yk: torch.Tensor, blocks, R: int, slots: int):
    """The cmtfpls_kfold_state of n = Yk.shape[0] models: (views, shared, own).  blocks: (A, B, S, mean) each; views: a ctypes array
    of _lib.KfoldState, one per block; own: each block's S, mean, WA, WB, Wa, Wb and Rm; every other field is in shared, one buffer
    for every view.  Tout has `slots` slots of held-out scores (slots x I x R)."""
    n, I, M = Yk.shape
    dev = be.device
    NT, stride = be.kfold_row_tiles(I)
    shared = {
        "fold_of": fold_of, "Yk": Yk, "Gy": be.empty(n, NT, M, M), "Q": be.zeros(n, R, M), "T": be.zeros(n, I, R), "Gt": be.zeros(n, R, R),
        "coef": be.zeros(n, R, R), "tm": be.empty(I, n), "Tout": be.zeros(slots, I, R), "vec": be.zeros(n, 3 * R + M + 2),
        "n_iter": torch.zeros(n, R, dtype=torch.int32, device=dev), "status": torch.zeros(n, dtype=torch.int32, device=dev),
        "part": be.empty(n, NT, stride),
    }
    own = [{"S": S, "mean": mean, "WA": be.empty(A, n), "WB": be.empty(B, n), "Wa": be.zeros(n, R, A), "Wb": be.zeros(n, R, B),
            "Rm": be.zeros(n, R, A * B)} for A, B, S, mean in blocks]
    views = [_lib.KfoldState(I, A, B, M, n, R, *[{**shared, **o}[f].data_ptr() for f, _ in _lib.KfoldState._fields_[6:]])
             for (A, B, _, _), o in zip(blocks, own)]
    return (_lib.KfoldState * len(views))(*views), shared, own


# The entries of _components, one row each: the HipBackend method (cmtfpls_<method>_f64 is the entry it binds and the name a decline
# gives), and how its arguments are laid out.  Inner entries, by (coupled, form): the method that sizes the workspace and its
# arguments (st, n, tensor), the arguments before (a, tol, max_iter) from (st, grouped, tensor), and whether (model_fold, groups,
# Wk, Wl) follow the workspace (the tensor entries serve the plain and the grouped layout: model_fold None, groups 1 is plain).
_INNER_ENTRIES = {
    (False, "plain"): ("kfold_inner", "kfold_inner_workspace_bytes", lambda st, n, t: (st[0].A, st[0].B, n), lambda st, g, t: (st[0],), False),
    (False, "grouped"): ("kfold_inner_grouped", "kfold_inner_workspace_bytes", lambda st, n, t: (st[0].A, st[0].B, n),
                         lambda st, g, t: (st[0], *g), False),
    (False, "tensor"): ("kfold_inner_tensor", "kfold_inner_tensor_workspace_bytes", lambda st, n, t: (st[0].A, *t, n),
                        lambda st, g, t: (st[0], *t), True),
    (True, "plain"): ("kfold_inner_coupled", "kfold_inner_coupled_workspace_bytes", lambda st, n, t: (st,), lambda st, g, t: (st,), False),
    (True, "grouped"): ("kfold_inner_coupled_grouped", "kfold_inner_coupled_workspace_bytes", lambda st, n, t: (st,),
                        lambda st, g, t: (st, *g), False),
    (True, "tensor"): ("kfold_inner_coupled_tensor", "kfold_inner_coupled_tensor_workspace_bytes", lambda st, n, t: (st, t),
                       lambda st, g, t: (st, t), True),
}
# Epilogue entries, by layout (the first of grouped, splits, weighted that is asked for, else plain): the arguments between the
# state view and (stage, a, src) from (grouped, splits).
_EPILOGUE_ENTRIES = {
    "grouped": ("kfold_epilogue_grouped", lambda g, s: tuple(g)),
    "splits": ("kfold_epilogue_splits", lambda g, s: (s,)),
    "weighted": ("kfold_epilogue_weighted", lambda g, s: ()),
    "plain": ("kfold_epilogue", lambda g, s: ()),
}


def _components(be, X2s, st, shared, own, R: int, tol: float, max_iter: int, coupled: bool, grouped=None, splits: int = 0,
                weighted: bool = False, tensor=None, tensor_out=None):
    """Every component of the n = st[0].K models of a state: stage 0, then per component the inner loop, one MTTKRP per block (a
    ctPLS, one block included: then the blocks' scores averaged), stage 1 and, but for the last, one contraction and stage 2 per
    block.  The inner entry: kfold_inner, kfold_inner_coupled (coupled), kfold_inner_grouped or kfold_inner_coupled_grouped (coupled
    and grouped: every view's mean is per fold); the epilogue: kfold_epilogue,
    kfold_epilogue_grouped (grouped = (model_fold, groups)), kfold_epilogue_splits (splits > 0) or kfold_epilogue_weighted
    (weighted: fold_of holds the models' row counts).  tensor = (B1, B2): a tPLS's order-4 X, st[0].B = B1 B2; the inner entry is
    kfold_inner_tensor in the plain or the grouped layout and everything else is unchanged.  coupled with tensor = [(B1, B2), ..]
    (_tensor_dims: a ctPLS with a block of order 4): likewise kfold_inner_coupled_tensor.  tensor_out = (Wk (n x R x B1), Wl
    (n x R x B2)): where kfold_inner_tensor leaves the models' mode loadings (the bootstrap's per-mode stacks); coupled: where
    kfold_inner_coupled_tensor leaves them, the tensor blocks' n x R x B1_b (B2_b) slices one after another in block order.  None, or
    why a kernel declined."""
    nb, n, I = len(st), st[0].K, st[0].I
    inner_method, ws_bytes, ws_args, head, layout = _INNER_ENTRIES[(bool(coupled), "tensor" if tensor is not None else
                                                                    "grouped" if grouped else "plain")]
    ws = _scratch(getattr(be, ws_bytes)(*ws_args(st, n, tensor)), be.device)
    head = head(st, grouped, tensor)
    tail = (ws, *(grouped if grouped else (None, 1)), *(tensor_out if tensor_out else (None, None))) if layout else (ws,)
    epilogue_method, extra = _EPILOGUE_ENTRIES["grouped" if grouped else "splits" if splits else "weighted" if weighted else "plain"]
    extra = extra(grouped, splits)

    def inner(a):
        return getattr(be, inner_method)(*head, a, tol, max_iter, *tail)

    def epilogue(b, *args):
        return getattr(be, epilogue_method)(st[b], *extra, *args)

    scs = be.empty(nb, I, n)
    sc = be.empty(I, n) if coupled else scs[0]
    rs = be.empty(n * max(v.A * v.B for v in st))
    if epilogue(0, 0, 0, None) is None:
        return f"shape outside cmtfpls_{epilogue_method}_f64"
    for a in range(R):
        if inner(a) is None:
            return f"shape outside cmtfpls_{inner_method}_f64"
        for b in range(nb):                                                         # X_b,0 [w_1 .. w_n]: one read each
            if be.mttkrp(X2s[b], st[b].A, st[b].B, own[b]["WA"], own[b]["WB"], scs[b]) is None:
                return f"{f'block {b}: ' if coupled else ''}the models' loadings outside cmtfpls_mttkrp_*"
        if coupled:
            be.kfold_combine_scores(scs, sc)                                        # t: the average of the blocks' scores
        epilogue(0, 1, a, sc)
        if a + 1 < R:
            for b in range(nb):                                                     # X_b,0^T [t_m * train_m]: one read each
                P = X2s[b].shape[1]
                r = rs[: n * P].view(n, P)
                be.xcov(X2s[b], shared["tm"], False, out=r)
                epilogue(b, 2, a, r)
    return None


def _held_out_predictions(Tout, coef, Qh, nu, ids, K, R, M) -> np.ndarray:
    pred = np.empty((R, ids.shape[0], M))
    for k in range(K):
        rows = ids == k
        for r in range(1, R + 1):
            pred[r - 1, rows] = _from_scores(Tout[rows], coef[k], Qh[k], nu[k], r)
    return pred


def _form_entries(build: str, coupled: bool, epilogue: str, grouped: bool = False) -> str:
    """The entries of a device pass as a report's form lists them (grouped: the inner entries of the permutation test's layout)."""
    g = "_grouped" if grouped else ""
    inner = f"cmtfpls_kfold_inner_coupled{g}_f64, cmtfpls_mttkrp_*, cmtfpls_kfold_combine_scores_f64" if coupled else \
        f"cmtfpls_kfold_inner{g}_f64, cmtfpls_mttkrp_*"
    return f"({build}, {inner}, {epilogue}, cmtfpls_xcov_*)"


def _x_reads(reads: int, Xs, coupled: bool):
    """`x_reads` of a report: the reads of X, a ctPLS one entry per block."""
    return [reads] * len(Xs) if coupled else reads


def _weighted_models(counts_d: torch.Tensor, e0: int, g: int):
    """(n, C, Cf) of a pass of the weighted drivers (bootstrap.py, nested.py) over models e0 .. e0 + g - 1 of the uploaded counts:
    their n x I counts as int32 and float64.  n = max(g, 2): a one-model pass runs two copies of its model (the K-fold kernels take
    at least two models); the caller reads the first g."""
    C = counts_d[e0:e0 + g] if g > 1 else counts_d[e0:e0 + 1].expand(2, counts_d.shape[1]).contiguous()
    return max(g, 2), C, C.to(torch.float64)


def _device_pass(pls, Xs, blocks, coupled: bool, builder: str, builds, fold_of: torch.Tensor, Yk: torch.Tensor, slots: int, first: bool,
                 tol: float, max_iter: int, tensor, Ss=None, means=None, mode_loadings: bool = False, **layout):
    """One device pass of the n = Yk.shape[0] models of a driver: every block's S and mean built, the state (_state, Tout with
    `slots` slots) and every component (_components with the layout arguments grouped / splits / weighted): (shared, own), or why
    the device form declined.  blocks: _device_blocks(pls, Xs); tensor: _tensor_dims of the blocks the inner entry is to take.
    builds: the reads that build S and mean, each a callable (X2, A, B, S, mean) -> the column statistics or None, made on every
    block in turn; one read builds all models (cmtfpls_<builder>), repeated.py passes one per split, each into its split's slice
    (`builds` may be a generator: what it does before a yield happens before that read).  S (n x M x P) and mean (n x P) of block b
    are Ss[b] / means[b] where the driver passes them in (the permutation test's per-fold means), else allocated before the
    block's first read.  fold_of and Yk as host arrays are uploaded once the builds have passed.  The statistics are checked
    (_stats_why) after the first read of the first pass (`first`) only.
    mode_loadings: the tensor inner entry leaves the models' wK and wL in shared["Wk"], shared["Wl"] (the bootstrap's per-mode
    stacks): n x R x B1 and n x R x B2 of a tPLS, of a ctPLS the tensor blocks' slices one after another."""
    eng = pls._get_engine()
    be = eng.be
    n, I, M = Yk.shape
    R = pls.n_components
    built = []
    for step, build in enumerate(builds):
        for b, ((X2, A, B), name) in enumerate(zip(blocks, _names(Xs, coupled))):
            if step == 0:
                S = Ss[b] if Ss is not None else be.empty(n, M, A * B)
                built.append((A, B, S, means[b] if means is not None else be.empty(n, A * B)))
            stats = build(X2, A, B, *built[b][2:])
            if stats is None:
                return f"{'' if name == 'X' else name + ': '}shape outside cmtfpls_{builder}"
            if first and step == 0:
                why = _stats_why(stats, A * B, I, eng.opt.xcov_raw_max_offset, name)
                if why is not None:
                    return why
    if isinstance(Yk, np.ndarray):                                               # kfold_run's: uploaded once the builds have passed
        fold_of, Yk = _to_dev(fold_of, be.device, torch.int32), _to_dev(Yk, be.device)
    st, shared, own = _state(be, fold_of, Yk, built, R, slots)
    tensor_out = None
    if mode_loadings and isinstance(tensor, list):
        tensor_out = (be.zeros(n * R * sum(B1 for B1, B2 in tensor if B2 > 0)), be.zeros(n * R * sum(B2 for _, B2 in tensor if B2 > 0)))
    elif mode_loadings and tensor is not None:
        tensor_out = (be.zeros(n, R, tensor[0]), be.zeros(n, R, tensor[1]))
    if tensor_out is not None:
        shared["Wk"], shared["Wl"] = tensor_out
    why = _components(be, [X2 for X2, _, _ in blocks], st, shared, own, R, tol, max_iter, coupled, tensor=tensor, tensor_out=tensor_out,
                      **layout)
    if why is not None:
        return why
    for X2, _, _ in blocks:                                                      # EngineOptions.half_folds: 16-bit blocks read in place
        notes_of(pls).in_place(X2.dtype, (builder, "mttkrp", *(("xcov",) if R > 1 else ())))
    return shared, own


def device_predictions(pls, Xs, Y, ids: np.ndarray, K: int, tol: float, max_iter: int, coupled: bool):
    """The device form of a tPLS (Xs = [X]) or a ctPLS (coupled, DESIGN 8c: a state view per block): (pred (R, I, M), report) or
    (None, why)."""
    eng = pls._get_engine()
    be = eng.be
    R = pls.n_components
    I = Xs[0].shape[0]
    Yh = _host(Y).reshape(I, -1).astype(np.float64)
    M = Yh.shape[1]
    dev = be.device
    with eng.device_ctx():
        order, off, ybar, nu, Yk = _fold_y(Yh, ids, K)
        ydev, order_d, off_d, nudev = _to_dev(Yh - ybar, dev), _to_dev(order, dev, torch.int32), _to_dev(off, dev, torch.int32), \
            _to_dev(nu - ybar, dev)
        tensor = _tensor_dims(Xs, coupled)
        got = _device_pass(pls, Xs, _device_blocks(pls, Xs, dev), coupled, "kfold_xcov",
                           [lambda X2, A, B, S, mean: be.kfold_xcov(X2, A, B, ydev, order_d, off_d, K, nudev, S, mean)],
                           ids, Yk, 1, True, tol, max_iter, tensor)
        if isinstance(got, str):
            return None, got
        shared, _ = got
        status = shared["status"].cpu().numpy()
        if status.any():
            return None, f"non-finite loadings or coefficients in folds {np.flatnonzero(status).tolist()} of the device form"
        n_iter = shared["n_iter"].cpu().numpy()
        Tout = shared["Tout"][0].cpu().numpy()
        coef = shared["coef"].cpu().numpy()
        Qh = shared["Q"].cpu().numpy()
    pred = _held_out_predictions(Tout, coef, Qh, nu, ids, K, R, M)
    source = "every block" if coupled else "X"
    report = {"form": f"K folds from shared reads of {source} "
                      + _form_entries("cmtfpls_kfold_xcov_*", coupled, "cmtfpls_kfold_epilogue_f64"),
              "folds": int(K), "x_reads": _x_reads(2 * R, Xs, coupled), "n_iter": n_iter.tolist()}
    return pred, _with_rank1(report, tensor)


MASKED_FORM = "cmtfpls_cv_masked_f64"
MASKED_TENSOR_FORM = "cmtfpls_cv_masked_tensor_f64"           # order-4 X under EngineOptions.masked_tensor_folds
MODELS_TENSOR_FORM = "cmtfpls_cv_masked_tensor_models_f64"
MASKED_LDS_CAP = 150 * 1024


def wants_masked_tensor(pls, X) -> bool:
    """Whether the masked order-4 form is asked for: a tPLS whose X has order 4 and holds a NaN, with
    EngineOptions.masked_tensor_folds."""
    return not isinstance(X, list) and X.ndim == 4 and pls._get_engine().opt.masked_tensor_folds and has_missing(X)


def wants_masked(pls, X) -> bool:
    """Whether a tPLS's X takes masked_predictions / masked_models: a NaN under EngineOptions.masked_folds, or wants_masked_tensor."""
    return not isinstance(X, list) and ((pls._get_engine().opt.masked_folds and has_missing(X)) or wants_masked_tensor(pls, X))


def masked_forms(pls, X):
    """(the fold entry, the models entry) that masked_predictions / masked_models take for X."""
    return (MASKED_TENSOR_FORM, MODELS_TENSOR_FORM) if wants_masked_tensor(pls, X) else (MASKED_FORM, MODELS_FORM)


def _masked_tensor_outside(form: str, I: int, A: int, B1: int, B2: int, M: int, R: int) -> str:
    return (f"shape outside {form} (it takes the short side of every unfolding <= 64, M <= 64, R <= 16 and its vectors within "
            f"{MASKED_LDS_CAP} bytes of LDS): largest short side = {masked_tensor_side(A, B1, B2)}, M = {M}, R = {R}, LDS = "
            f"{masked_tensor_lds_bytes(I, A, B1, B2, M, R)} bytes")


def _f64(a, dev):
    """The original data in float64, on the device."""
    return a.detach().to(device=dev, dtype=torch.float64) if isinstance(a, torch.Tensor) else _to_dev(np.asarray(a, np.float64), dev)


def _upload(pls, a, I: int, dev, why: Optional[str] = None) -> torch.Tensor:
    """The original data in float64 on the device, as I x -1 (the same bits as a copy through the host).  `why`: `a` is a block of X,
    read by a route without 16-bit kernels: under EngineOptions.half_folds the copy of 16-bit storage is noted with that reason."""
    if why is not None and half_route(pls, "half_folds", ())[0]:
        notes_of(pls).upcast(_as_torch_dtype(pls._dtype, a), why)
    return _f64(a, dev).contiguous().view(I, -1)


def has_missing(X) -> bool:
    """Whether X (a host array or a device tensor) holds a NaN."""
    if isinstance(X, torch.Tensor):
        return bool(torch.isnan(X).any().item())
    return bool(np.isnan(np.asarray(X)).any())


def _masked_setup(pls, Xs, names, Y, kernel: str, what: str, tensor=None):
    """What masked_predictions, masked_models and masked_models_coupled check before they look at X, in this order: the backend's
    kernel (`what` names it in the decline), a sharded model, the order of every block (tensor: _tensor_dims of a tPLS's order-4 X
    under EngineOptions.masked_tensor_folds, which the order-4 entries take), NaN in Y.  (why, None), or (None, (eng, be, M,
    upload)): upload(a, I) is _upload on the backend's device; upload(X, I, True) for a block of X (HALF_MASKED_WHY)."""
    eng = pls._get_engine()
    be = eng.be
    if not hasattr(be, kernel):
        return f"the {getattr(be, 'name', type(be).__name__)} backend has no {what} kernel", None
    if pls._comm is not None:
        return "sharded model (comm)", None
    for X, name in zip(Xs, names):
        if X.ndim not in (2, 3) and tensor is None:
            return f"{name} of order {X.ndim} (the masked form takes order 2 and 3)", None
    if has_missing(Y):
        return "missing values in Y", None
    M = int(np.prod(Y.shape[1:])) if Y.ndim > 1 else 1

    def upload(a, I, block=False):
        return _upload(pls, a, I, be.device, HALF_MASKED_WHY if block else None)

    return None, (eng, be, M, upload)


def _masked_outside(form: str, A: int, B: int, M: int, R: int) -> str:
    return (f"shape outside {form} (it takes min(J, K) <= 64, M <= 64, R <= 16 and its vectors within {MASKED_LDS_CAP // 1024} KB of "
            f"LDS): min(J, K) = {min(A, B)}, M = {M}, R = {R}")


def masked_predictions(pls, X, Y, ids: np.ndarray, K: int, tol: float, max_iter: int):
    """Refits of a tPLS on X with missing values, a workgroup per fold in one launch (cmtfpls_cv_masked_f64), in float64
    on the original data whatever the model's storage type: (pred (R, I, M), report) or (None, why).  Leave-one-out: ids =
    arange(I), K = I.  X of order 4 under EngineOptions.masked_tensor_folds: cmtfpls_cv_masked_tensor_f64, the report
    with `rank1` and `launches`."""
    R = pls.n_components
    I = ids.shape[0]
    tensor = _tensor_dims([X]) if pls._get_engine().opt.masked_tensor_folds else None
    why, ctx = _masked_setup(pls, [X], ["X"], Y, "cv_masked_tensor" if tensor else "cv_masked",
                             f"masked {'order-4 ' if tensor else ''}fold", tensor)
    if why is not None:
        return None, why
    eng, be, M, upload = ctx
    train = I - np.bincount(ids, minlength=K)
    if train.min() < 2:
        return None, f"fold {int(np.argmin(train))} leaves {int(train.min())} training rows (the masked form needs 2)"
    A, B = _dims(X)
    dev = be.device

    with eng.device_ctx():
        data = (upload(X, I, True), upload(Y, I), _to_dev(ids, dev, torch.int32), K)
        if tensor:
            out = be.cv_masked_tensor(*data, A, *tensor, R, tol, max_iter)
            if out is None:
                return None, _masked_tensor_outside(MASKED_TENSOR_FORM, I, A, *tensor, M, R)
            launches = out[4]
        else:
            out = be.cv_masked(*data, A, B, R, tol, max_iter)
            if out is None:
                return None, _masked_outside(MASKED_FORM, A, B, M, R)
        pred, n_iter, status, info = (t.cpu().numpy() for t in out[:4])
    if status.any():
        empty, small = np.flatnonzero(status == 1).tolist(), np.flatnonzero(status == 2).tolist()
        return None, "; ".join(w for w in (f"training rows without an observed entry of X in folds {empty}" if empty else "",
                                            f"fewer than 2 training rows in folds {small}" if small else "") if w)
    report = {"form": f"a workgroup per fold on X with missing values, all folds in one launch ({MASKED_FORM})", "folds": int(K),
              "x_reads": None, "n_iter": n_iter.tolist(), "masked_folds": int(info[:, 0].sum()),
              "masked_batches": int(info[:, 1].sum())}
    if tensor:
        report.update(form=f"a workgroup per fold on order-4 X with missing values, all folds in {launches} launch(es) "
                           f"({MASKED_TENSOR_FORM})", rank1=TENSOR_RANK1, launches=int(launches))
    return pred, report


MODELS_FORM = "cmtfpls_cv_masked_models_f64"


def masked_models(pls, X, Y, counts: np.ndarray, yrow: Optional[np.ndarray], tol: float, max_iter: int, factors: bool = False,
                  max_ws_bytes: Optional[int] = None):
    """Refits of a tPLS on X with missing values on count-weighted rows, a workgroup per model in one launch per chunk
    (cmtfpls_cv_masked_models_f64), in float64 on the original data whatever the model's storage type.  Model m trains on
    counts[m, r] copies of X row r paired with Y row yrow[m, r] (yrow None: identity) and predicts its rows with count 0.  Returns
    (out, None) -- out the backend's dict on the host (Ypred (n, R, I, M), n_iter, status, info, launches, with `factors` Wa, Wb,
    coef, Q) -- or (None, why) with masked_predictions' declines.  Models with a status are the caller's to refit.  X of order 4
    under EngineOptions.masked_tensor_folds: cmtfpls_cv_masked_tensor_models_f64, `factors` then Wa, Wk, Wl in place
    of Wa, Wb, and out["tensor"] = (B1, B2)."""
    R = pls.n_components
    I = counts.shape[1]
    tensor = _tensor_dims([X]) if pls._get_engine().opt.masked_tensor_folds else None
    why, ctx = _masked_setup(pls, [X], ["X"], Y, "cv_masked_tensor_models" if tensor else "cv_masked_models",
                             f"masked {'order-4 ' if tensor else ''}model", tensor)
    if why is not None:
        return None, why
    eng, be, M, upload = ctx
    A, B = _dims(X)
    dev = be.device

    with eng.device_ctx():
        data = (upload(X, I, True), upload(Y, I), _to_dev(counts, dev, torch.int32),
                None if yrow is None else _to_dev(yrow, dev, torch.int32))
        if tensor:
            out = be.cv_masked_tensor_models(*data, A, *tensor, R, tol, max_iter, factors, max_ws_bytes)
            if out is None:
                return None, _masked_tensor_outside(MODELS_TENSOR_FORM, I, A, *tensor, M, R)
            out["tensor"] = tensor
        else:
            out = be.cv_masked_models(*data, A, B, R, tol, max_iter, factors, max_ws_bytes)
            if out is None:
                return None, _masked_outside(MODELS_FORM, A, B, M, R)
        return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}, None


_STATUS_NAMES = {2: "fewer than 2 training rows", 3: "bad counts or Y rows"}        # status 1: named by the form (no observed entry)


def _models_report(out: dict, refitted, what: str, form: str, masked: dict, no_entry: str, rank1: bool = False) -> dict:
    """The report entries that masked_models_report and masked_coupled_report share: form (with the refit note), models, launches,
    the form's own counts `masked`, x_reads, and for the models in `refitted` the reason by status in `why` (`no_entry` names
    status 1)."""
    status = out["status"]
    rep = {"form": form + ("; models with a status refitted alone on the regular engine" if len(refitted) else ""),
           "models": int(len(status)), "launches": int(out["launches"]), **masked, "x_reads": None}
    if rank1:
        rep["rank1"] = TENSOR_RANK1
    if len(refitted):
        names = {1: no_entry, **_STATUS_NAMES}
        rep["refitted"] = [int(m) for m in refitted]
        rep["why"] = "; ".join(f"{names[s]} in {what} {np.flatnonzero(status == s).tolist()}" for s in (1, 2, 3) if (status == s).any())
    return rep


def masked_models_report(out: dict, refitted, what: str) -> dict:
    """The report entries of a masked-models run (form, models, launches, masked_models, masked_batches, x_reads); `refitted`
    the models whose status made them refit alone on the regular engine."""
    ok = out["status"] == 0
    form = f"a workgroup per model on X with missing values, {len(ok)} models in {out['launches']} launch(es) ({MODELS_FORM})"
    if "tensor" in out:                                                          # order-4 X (masked_tensor_folds)
        form = form.replace("on X", "on order-4 X").replace(MODELS_FORM, MODELS_TENSOR_FORM)
    return _models_report(out, refitted, what, form, {"masked_models": int(out["info"][ok, 0].sum()),
                                                      "masked_batches": int(out["info"][ok, 1].sum())},
                          "a training row without an observed entry of X", rank1="tensor" in out)


def masked_fold_numerators(pls, X, Y, ids: np.ndarray, K: int, yrows: Optional[np.ndarray], tol: float, max_iter: int,
                           coupled: bool = False):
    """The Q2Y numerators of N K-fold entries (permutations, splits) from masked_models (coupled: X a list of blocks, from
    masked_models_coupled): entry e has the fold ids ids[e] (N x I) and pairs X row r with Y row yrows[e, r] (None: identity);
    model e K + k holds out its fold k.  Returns (numerators N x R, n_iter per entry (K x R lists), report) or (None, why, None).
    A model with a status refits alone (refit_fold)."""
    N, I = ids.shape
    R = pls.n_components
    counts = (ids[:, None, :] != np.arange(K)[None, :, None]).reshape(N * K, I).astype(np.int32)
    models, report = (masked_models_coupled, masked_coupled_report) if coupled else (masked_models, masked_models_report)
    out, why = models(pls, X, Y, counts, None if yrows is None else np.repeat(yrows, K, axis=0), tol, max_iter)
    if out is None:
        return None, why, None
    Yh = _host(Y).reshape(I, -1).astype(np.float64)
    pred = out["Ypred"].reshape(N, K, R, I, Yh.shape[1])
    status = out["status"].reshape(N, K)
    n_iter = out["n_iter"].reshape(N, K, R).tolist()
    nums = np.zeros((N, R))
    refitted = []
    for e in range(N):
        y = Yh if yrows is None else Yh[yrows[e]]
        pe = np.zeros((R,) + Yh.shape)
        for k in range(K):
            test = ids[e] == k
            if status[e, k]:
                pe[:, test], n_iter[e][k] = refit_fold(pls, X, Y if yrows is None else _perm_y(Y, yrows[e]), test, tol, max_iter)
                refitted.append(e * K + k)
            else:
                pe[:, test] = pred[e, k][:, test]
        nums[e] = ((pe - y) ** 2).reshape(R, -1).sum(axis=1)                   # _refit_numerators' sum
    return nums, n_iter, report(out, refitted, "models")


# ---- a ctPLS with missing values in its blocks (EngineOptions.masked_folds_coupled) ---------------------------------
COUPLED_FORM = "cmtfpls_cv_masked_coupled_f64"
COUPLED_LDS_CAP = 150 * 1024

# a ctPLS with a block of order 4 among them (EngineOptions.masked_tensor_folds_coupled)
COUPLED_TENSOR_FORM = "cmtfpls_cv_masked_coupled_tensor_f64"


def wants_masked_coupled_tensor(pls, X) -> bool:
    """Whether the coupled masked order-4 form is asked for: a ctPLS (X a list of blocks) with at least one block of order 4,
    EngineOptions.masked_tensor_folds_coupled and a missing value in at least one block (of any order)."""
    return (isinstance(X, list) and pls._get_engine().opt.masked_tensor_folds_coupled and any(b.ndim == 4 for b in X)
            and any(has_missing(b) for b in X))


def wants_masked_coupled(pls, X) -> bool:
    """Whether a coupled masked form is asked for: a ctPLS (X a list of blocks) with EngineOptions.masked_folds_coupled and a
    missing value in at least one block, or wants_masked_coupled_tensor."""
    return isinstance(X, list) and ((pls._get_engine().opt.masked_folds_coupled and any(has_missing(b) for b in X))
                                    or wants_masked_coupled_tensor(pls, X))


def coupled_form(pls, X) -> str:
    """The entry that masked_models_coupled takes for the blocks X."""
    return COUPLED_TENSOR_FORM if wants_masked_coupled_tensor(pls, X) else COUPLED_FORM


def masked_models_coupled(pls, Xs, Y, counts: np.ndarray, yrow: Optional[np.ndarray], tol: float, max_iter: int,
                          factors: bool = False, max_ws_bytes: Optional[int] = None):
    """Refits of a ctPLS whose blocks Xs have missing values on count-weighted rows, a workgroup per model in one launch per chunk
    (cmtfpls_cv_masked_coupled_f64), in float64 on the original data whatever the model's storage type.  Model m trains
    on counts[m, r] copies of row r of every block paired with Y row yrow[m, r] (yrow None: identity) and predicts its rows with
    count 0.  Returns (out, None) -- out the backend's dict on the host (Ypred (n, R, I, M), n_iter, status, info, launches, with
    `factors` Wa, Wb (per block), coef, Q) -- or (None, why) with masked_models' declines.  Models with a status are the caller's to
    refit.  With a block of order 4 under EngineOptions.masked_tensor_folds_coupled: cmtfpls_cv_masked_coupled_tensor_f64,
    `factors` then also Wk, Wl (per block, None for a block of order 2 or 3), and out["tensor"] = [(B1, B2), ..]."""
    R = pls.n_components
    I = counts.shape[1]
    tensor = _tensor_dims(Xs, coupled=True) if wants_masked_coupled_tensor(pls, Xs) else None
    why, ctx = _masked_setup(pls, Xs, _names(Xs, True), Y, "cv_masked_coupled_tensor" if tensor else "cv_masked_coupled",
                             f"coupled masked {'order-4 ' if tensor else ''}model", tensor)
    if why is None and tensor:
        why = next((f"block {b} of order {X.ndim} (the masked form takes order 2, 3 and 4)" for b, X in enumerate(Xs)
                    if X.ndim not in (2, 3, 4)), None)
    if why is not None:
        return None, why
    eng, be, M, upload = ctx
    dims = [_dims(X) for X in Xs]
    dev = be.device

    def to_host(v):
        return v.cpu().numpy() if isinstance(v, torch.Tensor) else v

    with eng.device_ctx():
        out = None
        if len(Xs) <= MAX_BLOCKS:                                                # (the entry declines more blocks itself)
            data = ([upload(X, I, True) for X in Xs], [(X.ndim, A, B) for X, (A, B) in zip(Xs, dims)])
            rest = (upload(Y, I), _to_dev(counts, dev, torch.int32), None if yrow is None else _to_dev(yrow, dev, torch.int32), R, tol,
                    max_iter, factors, max_ws_bytes)
            out = be.cv_masked_coupled_tensor(*data, tensor, *rest) if tensor else be.cv_masked_coupled(*data, *rest)
        if out is None and tensor:
            sides = [masked_tensor_side(A, *t) if t[1] > 0 else min(A, B) for (A, B), t in zip(dims, tensor)]
            lds = coupled_tensor_masked_lds_bytes(dims, tensor, I, M, R)
            return None, (f"shape outside {COUPLED_TENSOR_FORM} (it takes at most {MAX_BLOCKS} blocks, min(J, K) <= 64 in every block "
                          f"of order 2 or 3 and the short side of every unfolding of a block of order 4 <= 64, M <= 64, R <= 16 and its "
                          f"vectors within {COUPLED_LDS_CAP} bytes of LDS): {len(Xs)} blocks, largest short side = {sides}, M = {M}, "
                          f"R = {R}, LDS = {lds} bytes")
        if out is None:
            return None, (f"shape outside {COUPLED_FORM} (it takes at most {MAX_BLOCKS} blocks, min(J, K) <= 64 in every block, "
                          f"M <= 64, R <= 16 and its vectors within {COUPLED_LDS_CAP} bytes of LDS): {len(Xs)} blocks, min(J, K) = "
                          f"{[min(A, B) for A, B in dims]}, M = {M}, R = {R}, LDS = {coupled_lds_bytes(dims, I, M, R)} bytes")
        host = {k: ([to_host(t) for t in v] if isinstance(v, list) else to_host(v)) for k, v in out.items()}
        return dict(host, blocks=len(Xs), **({"tensor": tensor} if tensor else {})), None


def _block_bits(mask: np.ndarray, nb: int):
    """Per block, how many entries of the bit masks `mask` have the block's bit set."""
    return [int(((mask >> b) & 1).sum()) for b in range(nb)]


def masked_coupled_report(out: dict, refitted, what: str) -> dict:
    """The report entries of a coupled masked-models run: form, models, launches, masked_blocks / masked_batches (per block: the
    models whose training rows / held-out batch took the masked arithmetic in that block), x_reads; `refitted` (always present)
    the models whose status made them refit alone on the regular engine, with the reason in `why`."""
    ok = out["status"] == 0
    nb = int(out["blocks"])
    form = (f"a workgroup per model on {nb} coupled blocks with missing values, {len(ok)} models in {out['launches']} "
            f"launch(es) ({COUPLED_FORM})")
    if "tensor" in out:                                                          # order-4 blocks (masked_tensor_folds_coupled)
        form = form.replace("coupled blocks", "coupled blocks, order-4 blocks among them,").replace(COUPLED_FORM, COUPLED_TENSOR_FORM)
    rep = _models_report(out, refitted, what, form, {"masked_blocks": _block_bits(out["info"][ok, 0], nb),
                                                     "masked_batches": _block_bits(out["info"][ok, 1], nb)},
                         "a training row without an observed entry in some block", rank1="tensor" in out)
    return dict(rep, refitted=[int(m) for m in refitted])                        # behaviour: this form lists `refitted` even when empty


def masked_predictions_coupled(pls, Xs, Y, ids: np.ndarray, K: int, tol: float, max_iter: int):
    """K-fold (leave-one-out: ids = arange(I), K = I) predictions of a ctPLS whose blocks have missing values from
    masked_models_coupled, fold k as the model with count 0 on its rows: (pred (R, I, M), report) or (None, why).  A fold with a
    status refits alone (refit_fold) and is listed in the report's `refitted`."""
    I = ids.shape[0]
    R = pls.n_components
    counts = (ids[None, :] != np.arange(K)[:, None]).astype(np.int32)
    out, why = masked_models_coupled(pls, Xs, Y, counts, None, tol, max_iter)
    if out is None:
        return None, why
    n_iter = out["n_iter"].tolist()
    pred = np.zeros((R, I, out["Ypred"].shape[3]))
    refitted = []
    for k in range(K):
        test = ids == k
        if out["status"][k]:
            pred[:, test], n_iter[k] = refit_fold(pls, Xs, Y, test, tol, max_iter)
            refitted.append(k)
        else:
            pred[:, test] = out["Ypred"][k][:, test]
    return pred, dict(masked_coupled_report(out, refitted, "folds"), folds=int(K), n_iter=n_iter)


# ---- the route of a resampling driver (kfold_run, permutation.py, repeated.py, nested.py, bootstrap.py) -------------------------------
OFF, MASKED, MASKED_COUPLED, PASSES, REFIT = "off", "masked", "masked coupled", "passes", "refit"


def _masked_declined(entry: str, why: str) -> str:
    """The `why` of a run whose masked form (`entry`, the cmtfpls_cv_masked_* it would have taken) declined."""
    return f"the masked form ({entry}) declined: {why}"


SPARSE_WHY = ("sparse loadings (sparsity set): the fold kernels extract dense loadings inside their workgroups, "
              "so every model refits on the regular engine")


def is_sparse(pls) -> bool:
    """A model constructed with `sparsity`: none of the resampling device forms applies to it."""
    return getattr(pls, "sparsity", None) is not None


def _route(pls, X, device_folds: bool, models: bool = True, masked: bool = True, coupled_first: bool = False, coupled_gate=None):
    """Which way a driver takes the fitted data X: (route, detail).  OFF (device_folds is False) and REFIT (no device form for this
    model): every model refits, detail is the report's `why`.  MASKED (kfold.wants_masked) and MASKED_COUPLED
    (wants_masked_coupled): the workgroup-per-model refits, detail names their entry for _masked_declined (`models`: the
    count-weighted entry, else the fold entry).  PASSES: the driver's device passes, which it still checks with _decline_blocks;
    detail is None.  masked=False: a driver without a masked form (nested.py).  coupled_gate = (on, why): the driver's passes take
    a ctPLS only when `on` (an EngineOptions switch), else it is REFIT with `why`."""
    if not device_folds:
        return OFF, "device folds switched off"
    if is_sparse(pls):
        return REFIT, SPARSE_WHY
    asks = ((MASKED, wants_masked, lambda: masked_forms(pls, X)[int(models)]), (MASKED_COUPLED, wants_masked_coupled, lambda: coupled_form(pls, X)))
    # behaviour: permutation_test asks the coupled masked form first, kfold_run, repeated_kfold and bootstrap the tPLS one (at most one holds)
    for route, wants, entry in (asks[::-1] if coupled_first else asks) if masked else ():
        if wants(pls, X):
            return route, entry()
    # (permutation_test had this gate between its two masked tests: the same, a ctPLS is a list, which wants_masked turns away unread)
    if coupled_gate is not None and isinstance(X, list) and not coupled_gate[0]:
        return REFIT, coupled_gate[1]
    return PASSES, None


def _passes_report(lead: str, build: str, epilogue: str, Xs, coupled: bool, passes: int, reads: int, why: Optional[str], failed,
                   refit_form: str, counts: dict, per_pass, n_iter, tensor, grouped: bool = False, scored: str = "", more=None) -> dict:
    """The report of a driver of _device_passes.  With passes the form is "<lead> from shared reads of X | every block (<the
    entries: _form_entries(build, coupled, epilogue, grouped)>)<scored>", and with a why and `failed` (what a failed pass refits:
    "fold", "model", ..) it says that failed passes refitted; without, refit_form.  Then the driver's own `counts`, passes,
    per_pass = (key, value: None without passes), x_reads (`reads` per block, None without passes), n_iter, `more`, why, and
    _with_rank1 for the blocks `tensor` the inner entry took."""
    if passes:
        form = f"{lead} from shared reads of {'every block' if coupled else 'X'} {_form_entries(build, coupled, epilogue, grouped)}{scored}"
        if why is not None and failed:
            form += f"; failed passes refitted per {failed} on the regular engine"
    else:
        form = refit_form
    rep = {"form": form, **counts, "passes": int(passes), per_pass[0]: int(per_pass[1]) if passes else None,
           "x_reads": _x_reads(reads, Xs, coupled) if passes else None, "n_iter": n_iter, **(more or {})}
    if why is not None:
        rep["why"] = why
    return _with_rank1(rep, tensor, passes)


def _masked_run_report(masked: dict, count: str, N: int, per_pass: str, n_iter, **more) -> dict:
    """A masked run's report (masked_models_report / masked_coupled_report) as the report of a driver of N entries: its launches
    are the passes, `per_pass` the entries (for "models_per_pass": the models) of one."""
    per = masked["models"] if per_pass == "models_per_pass" else N
    return dict(masked, **{count: int(N)}, passes=masked["launches"], **{per_pass: -(-per // masked["launches"])}, n_iter=n_iter, **more)


@reports_storage("q2y_report_", FOLDS_WHY)
def kfold_run(pls, n_splits: int = 5, folds=None, tol: float = 1e-8, max_iter: int = 100, device_folds: bool = True) -> np.ndarray:
    """pred (R, *Y.shape): pred[r - 1, i] = prediction for sample i by the model fitted without sample i's fold, with its first
    r components.  `pls` a fitted tPLS or ctPLS.  Sets pls.q2y_report_."""
    X, Y = _training_data(pls)
    coupled = isinstance(X, list)
    Xs = X if coupled else [X]
    I = Y.shape[0]
    ids, K = fold_ids(I, n_splits, folds)
    R = pls.n_components
    pred = None
    route, detail = _route(pls, X, device_folds, models=False)
    why = detail if route in (OFF, REFIT) else None
    if route in (MASKED, MASKED_COUPLED):
        pred, rep = (masked_predictions if route == MASKED else masked_predictions_coupled)(pls, X, Y, ids, K, tol, max_iter)
        why = None if pred is not None else _masked_declined(detail, rep)
    elif route == PASSES:
        inner = ("kfold_inner_coupled", "kfold_combine_scores") if coupled else ("kfold_inner",)
        why = _decline_blocks(pls, Xs, _names(Xs, coupled), Y, K, ("kfold_xcov", *inner, "kfold_epilogue", "mttkrp", "xcov"),
                              tensor_ok=True)
    if why is None and pred is None:
        pred, rep = device_predictions(pls, Xs, Y, ids, K, tol, max_iter, coupled)
        if pred is None:
            why = rep
    if pred is None:
        pred, n_iter = refit_predictions(pls, X, Y, ids, K, tol, max_iter)
        rep = {"form": "one refit per fold on the regular engine", "folds": int(K), "x_reads": None, "n_iter": n_iter, "why": why}
    pls.q2y_report_ = rep
    return pred.reshape((R,) + tuple(Y.shape))


# ---- passes of many models (permutation.py, repeated.py) --------------------------------------------------------------------
def _perm_y(Y, pi: np.ndarray):
    return Y[torch.from_numpy(pi).to(Y.device)] if isinstance(Y, torch.Tensor) else Y[pi]


def _refit_numerators(pls, X, Y, ids, K, pi, tol, max_iter):
    """(numerators (R,), n_iter K x R) of Y[pi] with the folds `ids` from literal refits."""
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


def _device_passes(pls, N: int, G: int, what: str, why: Optional[str], prepare, refit):
    """N entries (permutations, splits), G per device pass, then a literal refit of every entry the device left: (numerators N x R,
    n_iter per entry, passes, why; with passes > 0 a why is the notes of the failed passes).  Nothing runs on the device when `why`
    is set.  prepare() (under the device context) returns
    run(pass, e0, g): entries e0 .. e0 + g - 1 as (numerators g x R, their n_iter, status per model), or why the device form
    declined (then every entry refits); refit(e): (numerators (R,), n_iter)."""
    R = pls.n_components
    nums = np.full((N, R), np.nan)
    n_iters = [None] * N
    passes, notes = 0, []
    if why is None:
        with pls._get_engine().device_ctx():
            run = prepare()
            for e0 in range(0, N, G):
                g = min(G, N - e0)
                out = run(passes, e0, g)
                if isinstance(out, str):
                    why, passes, notes = out, 0, []
                    nums[:] = np.nan
                    n_iters = [None] * N
                    break
                num, n_iter, status = out
                passes += 1
                if status.any():
                    notes.append(f"pass {passes - 1} ({what} {e0}..{e0 + g - 1}): non-finite loadings or coefficients in models "
                                 f"{np.flatnonzero(status).tolist()}, refitted")
                    continue
                nums[e0:e0 + g] = num
                n_iters[e0:e0 + g] = n_iter
        if notes:
            why = "; ".join(notes)
    for e in range(N):                                                               # the refit path: whatever the device left
        if n_iters[e] is None:
            nums[e], n_iters[e] = refit(e)
    return nums, n_iters, passes, why
