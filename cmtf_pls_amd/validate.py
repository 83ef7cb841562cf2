"""Leave-one-out Q2Y with the reference's definition (cmtf_pls/validate.py:7-37).

The reference reads ``pls_tensor.original_X / original_Y``, which its own ``tPLS.fit`` never stores
(they are locals at tpls.py:74), so ``get_q2y`` fails there on any fitted model; the estimator here
keeps them.  One refit per held-out sample (validate.py:27-33).  On the GPU the folds run side by side, a workgroup per
fold doing the whole fit for it with the fold's means down-dated from shared column sums: ``cmtfpls_loo_tpls_f64`` when the
fold's vectors fit the LDS (min(J, K) <= 64), ``cmtfpls_loo_xcov_f64`` beyond (min(J, K) <= 256: the fold's NIPALS loop on its
cross-covariance, Gram squarings on the matrix cores) -- X of order 2 or 3 without missing values, M <= 64 / R <= 16 (LDS form), M <= 128 / R <= 64 (xcov form).  Anything else
refits once per fold on the regular engine with the fitted model's storage type, algorithm and backend.  X of order 4 without
missing values takes ``cmtfpls_loo_xcov_tensor_f64`` when ``EngineOptions.tensor_folds`` is on (the xcov form with the rank-1 CP of
each fold's cross-covariance inside its workgroup).  A fitted ``ctPLS`` on complete data (at most 8 blocks of order 2 or
3, min(J, K) <= 256 in every block, M <= 128, R <= 64) takes ``cmtfpls_loo_xcov_coupled_f64``: a workgroup per fold on the
cross-covariances of all blocks, which share the fold's score; with a NaN in a block and
``EngineOptions.masked_folds_coupled`` it takes ``cmtfpls_cv_masked_coupled_f64``, and with a block of order 4 among them and
``EngineOptions.masked_tensor_folds_coupled`` ``cmtfpls_cv_masked_coupled_tensor_f64`` (the rank-1 CP of every order-4 block's
contraction inside the model's workgroup); anything else refits ``ctPLS`` once per fold and says why.  With ``EngineOptions.tensor_resamples_coupled`` a ``ctPLS`` on complete data with a block of order 4 among blocks of
order 2, 3 and 4 takes ``cmtfpls_loo_xcov_coupled_tensor_f64``: the same workgroup per fold with the rank-1 CP of every order-4 block's
cross-covariance inside it.  X with missing values
(order 2 or 3, Y complete) takes ``cmtfpls_cv_masked_f64`` when ``EngineOptions.masked_folds`` is on (a workgroup per fold with
the reference's masked arithmetic, kfold.masked_predictions; K-fold too).  X of order 4 with missing values takes
``cmtfpls_cv_masked_tensor_f64`` when ``EngineOptions.masked_tensor_folds`` is on: the same workgroup per fold on the I x A x B1 B2
view, the rank-1 CP of the fold's contraction inside it; ``tensor_folds`` and ``masked_folds`` alone leave such an X to
the refits.  Which form ran is recorded on the model (``q2y_report_``).
"""
import numpy as np

from . import _lib
from .backend import _int_pairs
from .kfold import (HALF_LOO_WHY, MASKED_FORM, MASKED_TENSOR_FORM, MAX_BLOCKS, MAX_SIDE, SPARSE_WHY, TENSOR_LDS_CAP, TENSOR_RANK1, _dims, _host,
                    _masked_declined, _size_blocks, _tensor_dims, _training_data, _upload, coupled_form, has_missing, is_sparse, masked_predictions,
                    masked_predictions_coupled, refit_predictions, wants_masked_coupled, wants_masked_tensor)
from .storage import FOLDS_WHY, reports_storage
from .tpls import tPLS

LOO_TENSOR_FORM = "a workgroup per fold on the fold's cross-covariance, order-4 X (cmtfpls_loo_xcov_tensor_f64)"
LOO_COUPLED_FORM = "a workgroup per fold on the cross-covariances of the coupled blocks (cmtfpls_loo_xcov_coupled_f64)"
LOO_COUPLED_TENSOR_FORM = ("a workgroup per fold on the cross-covariances of the coupled blocks, order-4 blocks among them "
                           "(cmtfpls_loo_xcov_coupled_tensor_f64)")
LOO_REFIT_FORM = "one refit per fold on the regular engine"
LOO_MAX_RESPONSES, LOO_MAX_COMPONENTS, LOO_MAX_CELLS = 128, 64, 1 << 24
LOO_COUPLED_LDS_CAP = 150 * 1024


def _decline_loo_tensor(be, A: int, B1: int, B2: int, M: int, R: int):
    """Why cmtfpls_loo_xcov_tensor_f64 does not take an I x A x B1 x B2 X (its limits, checked here before X is uploaded)."""
    if not hasattr(be, "loo_tpls_tensor"):
        return f"the {getattr(be, 'name', type(be).__name__)} backend has no order-4 leave-one-out kernel"
    P = A * B1 * B2
    for mode, d in enumerate((A, B1, B2)):
        if min(d, P // d) > MAX_SIDE:
            return f"mode-{mode} unfolding: min({d}, {P // d}) = {min(d, P // d)} > {MAX_SIDE}"
    if M > LOO_MAX_RESPONSES:
        return f"M = {M} > {LOO_MAX_RESPONSES} responses (cmtfpls_loo_xcov_tensor_f64)"
    if R > LOO_MAX_COMPONENTS:
        return f"R = {R} > {LOO_MAX_COMPONENTS} components (cmtfpls_loo_xcov_tensor_f64)"
    if P > LOO_MAX_CELLS:
        return f"A B1 B2 = {P} > {LOO_MAX_CELLS} (cmtfpls_loo_xcov_tensor_f64)"
    lds = _lib.load().cmtfpls_loo_xcov_tensor_lds_bytes(A, B1, B2, M, R)
    if lds > TENSOR_LDS_CAP:
        return f"the fold's vectors need {lds} bytes of LDS > {TENSOR_LDS_CAP} (cmtfpls_loo_xcov_tensor_f64)"
    return None


@reports_storage("q2y_report_", FOLDS_WHY)
def loo_predictions(pls_tensor, tol: float = 1e-8, max_iter: int = 100):
    """Y_pred[i] = prediction for sample i by the model refitted without it (validate.py:24-33), all folds in one
    launch; None when the device form does not apply (see get_q2y).  `pls_tensor` is a fitted tPLS or ctPLS."""
    if _is_coupled(pls_tensor):
        return _loo_device_coupled(pls_tensor, tol, max_iter)[0]
    return _loo_device(pls_tensor, tol, max_iter)[0]


def _is_coupled(pls) -> bool:
    from .cmtf import ctPLS

    return isinstance(pls, ctPLS)


def _loo_coupled_why(pls, Xs, Y, tensor: bool):
    """The one list of checks behind _decline_loo_coupled (cmtfpls_loo_xcov_coupled_f64) and, tensor, _decline_loo_coupled_tensor
    (cmtfpls_loo_xcov_coupled_tensor_f64): the entry's limits in its order, checked before a block is uploaded."""
    be = pls._get_engine().be
    name = "cmtfpls_loo_xcov_coupled_tensor_f64" if tensor else "cmtfpls_loo_xcov_coupled_f64"
    if not hasattr(be, "loo_ctpls_tensor" if tensor else "loo_ctpls"):
        return f"the {getattr(be, 'name', type(be).__name__)} backend has no {'order-4 ' if tensor else ''}coupled leave-one-out kernel"
    if pls._comm is not None:
        return "sharded model (comm)"
    top = 4 if tensor else 3
    count = f"{len(Xs)} blocks > {MAX_BLOCKS} ({name})" if len(Xs) > MAX_BLOCKS else None
    order = next((f"block {b} of order {X.ndim} > {top} ({name})" for b, X in enumerate(Xs) if X.ndim > top), None)
    if count or order:                               # behaviour: the tensor entry names a block's order before the block count
        return (order or count) if tensor else (count or order)
    note = f"{name} is the complete-data form" if tensor else f"EngineOptions.masked_folds_coupled is off; {name} is the complete-data form"
    for b, X in enumerate(Xs):
        if has_missing(X):
            return f"missing values in block {b} ({note})"
    if has_missing(Y):
        return "missing values in Y"
    dims = [_dims(X) for X in Xs]
    tensors = _tensor_dims(Xs, coupled=True) if tensor else [(0, 0)] * len(Xs)
    M = int(np.prod(Y.shape[1:])) if Y.ndim > 1 else 1
    R = pls.n_components
    for b, ((A, B), (_, B2)) in enumerate(zip(dims, tensors)):
        if B2 == 0 and min(A, B) > MAX_SIDE:
            return f"block {b}: min(J, K) = {min(A, B)} > {MAX_SIDE} ({name})"
    for b, ((A, _), (B1, B2)) in enumerate(zip(dims, tensors)):
        P = A * B1 * B2
        for mode, d in enumerate((A, B1, B2) if B2 > 0 else ()):
            if min(d, P // d) > MAX_SIDE:
                return f"block {b}: mode-{mode} unfolding: min({d}, {P // d}) = {min(d, P // d)} > {MAX_SIDE} ({name})"
    if M > LOO_MAX_RESPONSES:
        return f"M = {M} > {LOO_MAX_RESPONSES} responses ({name})"
    if R > LOO_MAX_COMPONENTS:
        return f"R = {R} > {LOO_MAX_COMPONENTS} components ({name})"
    for b, (A, B) in enumerate(dims):
        if A * B > LOO_MAX_CELLS:
            return f"block {b}: J K = {A * B} > {LOO_MAX_CELLS} ({name})"
    blocks, lib = _size_blocks(_lib.LooCoupledBlock, dims, tensors), _lib.load()
    lds = (lib.cmtfpls_loo_xcov_coupled_tensor_lds_bytes(blocks, len(dims), _int_pairs(tensors), Y.shape[0], M, R) if tensor
           else lib.cmtfpls_loo_xcov_coupled_lds_bytes(blocks, len(dims), Y.shape[0], M, R))
    if lds > LOO_COUPLED_LDS_CAP:
        return f"the fold's vectors need {lds} bytes of LDS > {LOO_COUPLED_LDS_CAP} ({name})"
    return None


def _decline_loo_coupled(pls, Xs, Y):
    """Why cmtfpls_loo_xcov_coupled_f64 does not take these blocks (_loo_coupled_why); None: it does."""
    return _loo_coupled_why(pls, Xs, Y, False)


def _decline_loo_coupled_tensor(pls, Xs, Y):
    """Why cmtfpls_loo_xcov_coupled_tensor_f64 does not take these blocks, at least one of them of order 4 (_loo_coupled_why);
    None: it does."""
    return _loo_coupled_why(pls, Xs, Y, True)


def _wants_loo_coupled_tensor(pls, Xs) -> bool:
    """EngineOptions.tensor_resamples_coupled with a block of order 4 (or above: that one declines with its reason)."""
    return bool(pls._get_engine().opt.tensor_resamples_coupled) and any(X.ndim >= 4 for X in Xs)


def _loo_report(form: str, folds: int, n_iter_total, blocks=None, rank1: bool = False, why=None) -> dict:
    """q2y_report_ of a leave-one-out form (blocks: a ctPLS's; rank1: an order-4 form; why: of the refits)."""
    rep = {"form": form, **({"rank1": TENSOR_RANK1} if rank1 else {}), "folds": int(folds), **({} if blocks is None else {"blocks": blocks}),
           "n_iter_total": int(n_iter_total)}
    return rep if why is None else dict(rep, why=why)


def _loo_result(pls, out, entry: str, form: str, Y, blocks=None, rank1: bool = False):
    """(Y_pred, None) and q2y_report_ from what a workgroup-per-fold entry returned, or (None, why) when it declined the shape."""
    if out is None:
        return None, f"{entry} declined the shape"
    pls.q2y_report_ = _loo_report(form, Y.shape[0], out[1].sum().item(), blocks, rank1)
    return out[0].cpu().numpy().reshape(tuple(Y.shape)), None


def _loo_device_coupled(pls, tol: float, max_iter: int):
    """_loo_device for a fitted ctPLS: (Y_pred, None) from a device form (q2y_report_ set), or (None, why)."""
    if is_sparse(pls):
        return None, SPARSE_WHY
    Xs, Y = _training_data(pls)
    I = Y.shape[0]
    # EngineOptions.masked_folds_coupled: cmtfpls_cv_masked_coupled_f64; masked_tensor_folds_coupled with a block of order 4:
    # cmtfpls_cv_masked_coupled_tensor_f64
    if wants_masked_coupled(pls, Xs):
        pred, rep = masked_predictions_coupled(pls, Xs, Y, np.arange(I), I, tol, max_iter)
        if pred is None:
            return None, _masked_declined(coupled_form(pls, Xs), rep)
        pls.q2y_report_ = dict(rep, blocks=len(Xs), n_iter_total=int(np.sum(rep["n_iter"])))
        return pred[-1].reshape(Y.shape), None
    tensor = _wants_loo_coupled_tensor(pls, Xs)                           # EngineOptions.tensor_resamples_coupled
    why = _decline_loo_coupled_tensor(pls, Xs, Y) if tensor else _decline_loo_coupled(pls, Xs, Y)
    if why is not None:
        return None, why
    eng = pls._get_engine()
    be = eng.be
    with eng.device_ctx():
        data = ([_upload(pls, X, I, be.device, HALF_LOO_WHY) for X in Xs], _upload(pls, Y, I, be.device), [(X.ndim, *_dims(X)) for X in Xs])
        if tensor:
            out = be.loo_ctpls_tensor(*data, _tensor_dims(Xs, coupled=True), pls.n_components, tol, max_iter)
            return _loo_result(pls, out, "cmtfpls_loo_xcov_coupled_tensor_f64", LOO_COUPLED_TENSOR_FORM, Y, len(Xs), rank1=True)
        out = be.loo_ctpls(*data, pls.n_components, tol, max_iter)
        return _loo_result(pls, out, "cmtfpls_loo_xcov_coupled_f64", LOO_COUPLED_FORM, Y, len(Xs))


def _get_q2y_coupled(pls, device_folds: bool):
    """get_q2y of a fitted ctPLS: the device forms of _loo_device_coupled, else one ctPLS refit per fold with the model's storage
    type, algorithm, backend and options (kfold.refit_predictions), the reason in q2y_report_["why"]."""
    Xs, Y = _training_data(pls)
    I = Y.shape[0]
    Y_pred, why = _loo_device_coupled(pls, 1e-8, 100) if device_folds else (None, "device folds switched off")
    Y_actual = _host(Y).astype(float)
    if Y_pred is None:
        pred, n_iter = refit_predictions(pls, Xs, Y, np.arange(I), I, 1e-8, 100)
        pls.q2y_report_ = _loo_report(LOO_REFIT_FORM, I, np.sum(n_iter), len(Xs), why=why)
        Y_pred = pred[-1].reshape(Y_actual.shape)
    numerator = (Y_pred - Y_actual) ** 2                     # validate.py:35-37
    denominator = Y_actual ** 2
    return 1 - numerator.sum() / denominator.sum()


LOO_FORMS = {"lds": "all folds in one launch, a workgroup per fold, vectors in LDS (cmtfpls_loo_tpls_f64)",
             "xcov": "a workgroup per fold on the fold's cross-covariance (cmtfpls_loo_xcov_f64)"}


def _loo_device(pls_tensor, tol: float, max_iter: int):
    """(Y_pred, None) from a device form, or (None, why): why is None when no form was tried (get_q2y then names the limits)."""
    import torch

    if is_sparse(pls_tensor):
        return None, SPARSE_WHY
    X = pls_tensor.original_X
    Y = pls_tensor.original_Y
    eng = pls_tensor._get_engine()
    I = X.shape[0]
    tensor = wants_masked_tensor(pls_tensor, X)                            # EngineOptions.masked_tensor_folds: cmtfpls_cv_masked_tensor_f64
    if tensor or (eng.opt.masked_folds and X.ndim in (2, 3) and has_missing(X)):   # EngineOptions.masked_folds: cmtfpls_cv_masked_f64
        pred, rep = masked_predictions(pls_tensor, X, Y, np.arange(I), I, tol, max_iter)
        if pred is None:
            return None, _masked_declined(MASKED_TENSOR_FORM if tensor else MASKED_FORM, rep)
        rep["n_iter_total"] = int(np.sum(rep["n_iter"]))
        pls_tensor.q2y_report_ = rep
        return pred[-1].reshape(Y.shape), None
    be = eng.be
    order4 = X.ndim == 4 and bool(eng.opt.tensor_folds)                    # EngineOptions.tensor_folds: cmtfpls_loo_xcov_tensor_f64
    if not order4 and (not hasattr(be, "loo_tpls") or X.ndim not in (2, 3)):
        return None, None
    if has_missing(X) or has_missing(Y):             # behaviour: the tPLS forms name no reason for NaN; get_q2y names the limits itself
        return None, None
    R = pls_tensor.n_components
    if order4:                                       # (its limits are checked here, before X is uploaded)
        A, B1, B2 = (int(d) for d in X.shape[1:])
        why = _decline_loo_tensor(be, A, B1, B2, int(np.prod(Y.shape[1:])) if Y.ndim > 1 else 1, R)
        if why is not None:
            return None, why
    with torch.cuda.device(be.device):
        Xd, Yd = _upload(pls_tensor, X, I, be.device, HALF_LOO_WHY), _upload(pls_tensor, Y, I, be.device)
        if order4:
            return _loo_result(pls_tensor, be.loo_tpls_tensor(Xd, Yd, A, B1, B2, R, tol, max_iter), "cmtfpls_loo_xcov_tensor_f64",
                               LOO_TENSOR_FORM, Y, rank1=True)
        out = be.loo_tpls(Xd, Yd, *_dims(X), R, tol, max_iter)
        if out is None:                              # behaviour: neither form took the shape; get_q2y names the limits itself
            return None, None
        return _loo_result(pls_tensor, out, "", LOO_FORMS[out[2]], Y)


@reports_storage("q2y_report_", FOLDS_WHY)
def get_q2y(pls_tensor, device_folds: bool = True):
    if _is_coupled(pls_tensor):
        return _get_q2y_coupled(pls_tensor, device_folds)
    assert getattr(pls_tensor, "original_X", None) is not None, "PLS Tensor must be fit prior to calculating Q2Y"
    X = np.asarray(pls_tensor.original_X) if not hasattr(pls_tensor.original_X, "cpu") else pls_tensor.original_X.cpu().numpy()
    Y = np.asarray(pls_tensor.original_Y) if not hasattr(pls_tensor.original_Y, "cpu") else pls_tensor.original_Y.cpu().numpy()
    n = X.shape[0]
    Y_pred, why = _loo_device(pls_tensor, 1e-8, 100) if device_folds else (None, None)
    Y_actual = Y.astype(float)
    if Y_pred is None:
        why = ("device folds switched off" if not device_folds else why or
               "order > 3, missing values, min(J, K) > 256, M > 128 (or an M x M Gram beyond the LDS) or R > 64: outside both workgroup-per-fold kernels")
        pls_tensor.q2y_report_ = {"form": LOO_REFIT_FORM, "folds": int(n), "why": why}
        # behaviour: this loop is the reference's, and its tPLS is built without the fitted model's graphs, matrix_precision and
        # options, unlike kfold.refit_fold
        refit = tPLS(pls_tensor.n_components, dtype=pls_tensor._dtype, device=pls_tensor._device,
                     backend=pls_tensor._backend, algorithm=pls_tensor._algorithm, sparsity=getattr(pls_tensor, "sparsity", None))
        Y_pred = np.zeros(Y.shape)
        keep = np.ones(n, dtype=bool)
        for i in range(n):                                   # LeaveOneOut().split(X, Y)     validate.py:24,27
            keep[i] = False
            refit.fit(X[keep], Y[keep])                      # validate.py:30
            Y_pred[i] = refit.predict(X[i:i + 1]).reshape(Y_pred[i].shape)   # validate.py:32
            keep[i] = True
    numerator = (Y_pred - Y_actual) ** 2                     # validate.py:35-37
    denominator = Y_actual ** 2
    return 1 - numerator.sum() / denominator.sum()


def kfold_predictions(pls_tensor, n_splits: int = 5, folds=None, tol: float = 1e-8, max_iter: int = 100,
                      device_folds: bool = True) -> np.ndarray:
    """K-fold cross-validated predictions, (R, *Y.shape): entry [r - 1, i] is the prediction for sample i by the model
    fitted without sample i's fold, using its first r components.  folds=None: contiguous folds with the sizes of sklearn's
    KFold(n_splits, shuffle=False); otherwise an int array of fold ids 0..K-1, one per sample.  On the GPU every fold is served
    by the same reads of X (2R in all, X never copied or written: kfold.py); anything outside that form refits once per fold.
    `pls_tensor` is a fitted tPLS or ctPLS (a coupled model: 2R reads of each block, ``x_reads`` one entry per block).
    With missing values in X a tPLS takes cmtfpls_cv_masked_f64 under EngineOptions.masked_folds, and a ctPLS with a NaN in some
    block takes cmtfpls_cv_masked_coupled_f64 under EngineOptions.masked_folds_coupled (every fold a workgroup, leave-one-out is
    n_splits = I), and a tPLS whose X has order 4 takes cmtfpls_cv_masked_tensor_f64 under
    EngineOptions.masked_tensor_folds, and a ctPLS with a block of order 4 and a NaN in some block takes
    cmtfpls_cv_masked_coupled_tensor_f64 under EngineOptions.masked_tensor_folds_coupled; the permutation test, repeated
    K-fold and the bootstrap below route the same way.  What still refits by class is nested K-fold of data with missing values.
    Which form ran is recorded on the model (``q2y_report_``)."""
    from .kfold import kfold_run

    return kfold_run(pls_tensor, n_splits, folds, tol, max_iter, device_folds)


def get_q2y_kfold(pls_tensor, n_splits: int = 5, folds=None, per_component: bool = False, device_folds: bool = True):
    """Q2Y (validate.py:35-37: 1 - sum (pred - y)^2 / sum y^2) of K-fold cross-validated predictions; per_component=True:
    the (R,) array of Q2Y with the first r = 1..R components, all from the same run."""
    pred = kfold_predictions(pls_tensor, n_splits, folds, device_folds=device_folds)
    Y = np.asarray(pls_tensor.original_Y) if not hasattr(pls_tensor.original_Y, "cpu") else pls_tensor.original_Y.cpu().numpy()
    Y_actual = Y.astype(float)
    numerator = ((pred - Y_actual) ** 2).reshape(pred.shape[0], -1).sum(axis=1)
    q = 1 - numerator / (Y_actual ** 2).sum()
    return q if per_component else float(q[-1])


def permutation_test_q2y(pls_tensor, n_permutations: int = 99, n_splits: int = 5, folds=None, permutations=None, random_state=0,
                         per_component: bool = False, device_folds: bool = True) -> dict:
    """Response-permutation test of K-fold Q2Y: permutation p refits the K folds on Y[pi_p] (X and the folds stay as they are) and
    scores them with get_q2y_kfold's formula against Y[pi_p].  Permutations: P = n_permutations draws of
    np.random.default_rng(random_state).permutation(I), in order, or `permutations`, a (P, I) array whose rows are permutations of
    0..I-1 (ValueError otherwise, or when n_permutations < 1).  Returns {"q2y": get_q2y_kfold(pls_tensor, n_splits, folds,
    per_component), "null": (P,) or (P, R), "p_value": (1 + #{null >= q2y}) / (P + 1) (per component with per_component),
    "permutations": (P, I)}.  On the GPU a tPLS runs floor(32 / K) permutations x K folds per pass from shared reads of X (2R reads
    per pass, permutation.py).  A tPLS whose X has missing values (order 2 or 3, Y complete) takes cmtfpls_cv_masked_models_f64 when
    EngineOptions.masked_folds is on: every permutation x fold is a workgroup with the reference's masked arithmetic;
    X of order 4 with missing values takes cmtfpls_cv_masked_tensor_models_f64 when EngineOptions.masked_tensor_folds is on.
    A ctPLS with a NaN in some block takes cmtfpls_cv_masked_coupled_f64 under EngineOptions.masked_folds_coupled, with a
    block of order 4 cmtfpls_cv_masked_coupled_tensor_f64 under EngineOptions.masked_tensor_folds_coupled.
    Anything else refits every fold of every permutation.  Which form ran is recorded on the model (``q2y_report_``)."""
    from .permutation import permutation_test

    return permutation_test(pls_tensor, n_permutations, n_splits, folds, permutations, random_state, per_component, device_folds)


def get_q2y_repeated_kfold(pls_tensor, n_splits: int = 5, n_repeats: int = 10, folds=None, random_state=0, per_component: bool = False,
                           device_folds: bool = True) -> dict:
    """Repeated K-fold Q2Y: S shuffled K-fold splits, split g scored exactly as get_q2y_kfold(pls_tensor, folds=ids_g,
    per_component) scores it.  Splits: the test folds of sklearn's RepeatedKFold(n_splits, n_repeats, random_state) in its order
    (S = n_repeats; random_state must be an int), or `folds`, an (S, I) integer array with one split per row, each row holding
    ids 0..K-1 with no empty fold and the same K in every row (ValueError otherwise; n_splits, n_repeats and random_state are
    then ignored).  Returns {"q2y": (S,) or (S, R), "mean" and "std" (ddof=0) over the splits, "folds": (S, I)}, and with
    per_component "one_se": the smallest component count r (from 1) whose mean is at least max(mean) - std[argmax] / sqrt(S).
    On the GPU floor(32 / K) splits x K folds of a tPLS or ctPLS share every MTTKRP and contraction of X (G + 2R - 1 reads
    per pass and block, repeated.py).  A tPLS whose X has missing values (order 2 or 3, Y complete) takes
    cmtfpls_cv_masked_models_f64 when EngineOptions.masked_folds is on: every split x fold is a workgroup with the reference's
    masked arithmetic; X of order 4 with missing values takes cmtfpls_cv_masked_tensor_models_f64 when
    EngineOptions.masked_tensor_folds is on.  A ctPLS with a NaN in some block takes cmtfpls_cv_masked_coupled_f64 under
    EngineOptions.masked_folds_coupled, with a block of order 4 cmtfpls_cv_masked_coupled_tensor_f64 under
    EngineOptions.masked_tensor_folds_coupled.  Anything else refits every fold of every split.  Which form ran is recorded on the model
    (``q2y_report_``)."""
    from .repeated import repeated_kfold

    return repeated_kfold(pls_tensor, n_splits, n_repeats, folds, random_state, per_component, device_folds)


def get_q2y_nested_kfold(pls_tensor, n_outer: int = 5, n_inner: int = 5, outer_folds=None, inner_folds=None, random_state=0,
                         device_folds: bool = True) -> dict:
    """Nested ("double") K-fold Q2Y of a fitted tPLS or ctPLS: the Q2Y of a model whose component count is chosen by
    cross-validation, on rows that had no part in the choice.  Every outer fold o chooses its own r by an inner K-fold over its
    training rows, and its held-out rows are predicted by the model fitted on those training rows with that r.
    Splits: outer_folds=None draws one shuffled split, the test folds of sklearn's KFold(n_outer, shuffle=True, random_state);
    otherwise an (I,) integer array of ids 0..K_o-1 with no empty fold.  inner_folds=None splits the training rows of outer fold o
    (ascending row order) the same way with random_state + 1 + o; otherwise a (K_o, I) integer array whose row o holds -1 exactly
    on the rows of outer fold o and ids 0..K_i-1 elsewhere, no fold empty, the same K_i in every row.  random_state must be an int
    when a split is drawn; ValueError for anything malformed.
    Returns {"q2y": the nested estimate, the Q2Y (validate.py:35-37: 1 - sum (pred - y)^2 / sum y^2) of "predictions";
    "predictions": Y's shape, row i by outer model outer[i] with selected[outer[i]] components; "selected": (K_o,) ints in 1..R,
    the argmax of inner_q2y[o] (the smallest r on an exact tie); "inner_q2y": (K_o, R), for outer fold o the Q2Y of the inner
    folds' predictions over o's training rows with r = 1..R components (get_q2y_kfold of a model fitted on X[train_o] with
    folds=inner[o][train_o], per_component=True); "outer_q2y": (R,) the Q2Y of the outer models' predictions with a fixed r
    (get_q2y_kfold(pls_tensor, folds=outer, per_component=True)): max(outer_q2y) - q2y is the optimism of choosing R on the
    scored rows; "outer_folds": (I,), "inner_folds": (K_o, I)}.
    On the GPU the K_o (K_i + 1) models are 0/1-weighted models of the bootstrap's pass, up to 32 per pass from shared reads of X
    (2R reads per pass and block), scored where their state lies by cmtfpls_press_rows_f64 (nested.py).  Anything
    else -- missing values in X included -- refits every model.  Which form ran is recorded on the model (``q2y_report_``)."""
    from .nested import nested_kfold

    return nested_kfold(pls_tensor, n_outer, n_inner, outer_folds, inner_folds, random_state, device_folds)


def bootstrap_factors(pls_tensor, n_resamples: int = 100, resamples=None, random_state=0, level: float = 0.95,
                      device_folds: bool = True) -> dict:
    """Bootstrap of a fitted tPLS or ctPLS: resample b refits the model, with its dtype, device, backend, algorithm and options,
    on X[idx_b], Y[idx_b] (a ctPLS: every block with the same rows), and is aligned to the fitted model (bootstrap.align_factors:
    every X-mode loading column flipped to a nonnegative inner product with the fitted one, a zero counting as +1; d_a the product
    of the first block's flips of component a; q_a -> d_a q_a and coef_ -> D coef_ D, D = diag(d)).  Resamples: B = n_resamples
    rows of np.random.default_rng(random_state).integers(0, I, size=(B, I)), or `resamples`, a (B, I) integer array of row indices
    in [0, I) (ValueError otherwise, when B < 2 or when level is not in (0, 1)).
    Returns {"resamples": (B, I), "X_factors": per mode 1.. a (B, dim, R) stack laid out like X_factors[1:] (a ctPLS: one such
    list per block), "Y_loadings": (B, M, R), "coef": (B, R, R), "se": those three with the std over the resamples (ddof 1),
    "ci": with np.percentile at 100 (1 -/+ level) / 2 on a leading axis of 2, "oob_q2y": (R,) the Q2Y (validate.py:35-37) of the
    out-of-bag predictions with r = 1..R components (row i's: the mean over the resamples that left it out of their models'
    predictions) over "oob_rows" rows, those left out at least once}.  On the GPU up to 32 resamples per pass share every read of X
    (2R reads per pass and block, bootstrap.py).  A tPLS whose X has missing values (order 2 or 3, Y complete) takes
    cmtfpls_cv_masked_models_f64 when EngineOptions.masked_folds is on: every resample is a count-weighted workgroup with the
    reference's masked arithmetic; X of order 4 with missing values takes cmtfpls_cv_masked_tensor_models_f64 when
    EngineOptions.masked_tensor_folds is on, its per-mode stacks [wA, wK, wL].  A tPLS whose X has order 4 takes the same passes with cmtfpls_kfold_inner_tensor_f64
    when EngineOptions.tensor_folds is on.  A ctPLS with a NaN in some block takes cmtfpls_cv_masked_coupled_f64 under
    EngineOptions.masked_folds_coupled, with a block of order 4 cmtfpls_cv_masked_coupled_tensor_f64 under
    EngineOptions.masked_tensor_folds_coupled, such a block's per-mode stacks [wA, wK, wL].  Anything else refits every
    resample.  Which form ran is recorded on the model
    (``bootstrap_report_``)."""
    from .bootstrap import bootstrap

    return bootstrap(pls_tensor, n_resamples, resamples, random_state, level, device_folds)


def sample_diagnostics(pls_tensor, X=None, Y=None, level: float = 0.95, device: bool = True) -> dict:
    """Which samples and variables a fitted tPLS or ctPLS fails to describe.  X=None: the training rows (their fitted scores and
    ``original_X``; ValueError after a copy_X=False fit); otherwise new rows (a ctPLS: a list of blocks, as for transform), scored
    as transform scores them.  Y (training rows: ``original_Y`` by default) adds the prediction residual.
    Returns {"scores": (I', R), "t2": (I',) Hotelling's T^2 against the training scores' mean and covariance (ddof 1, pseudo-
    inverse), "t2_limit", "spe" (I',) the Q residual sum_c e^2 of x = X - X_mean over its finite entries, "ssq" (I',) sum_c x^2,
    "n_observed" (I',), "spe_limit" (Box's chi^2 approximation from the training SPE), "r2x_per_variable" (X.shape[1:]: 1 -
    sum_i e^2 / sum_i x^2 over the diagnosed rows, NaN without an observed entry or variance), "y_residual" (I',) sum_m (y -
    y_hat)^2 or None, "level"}; a ctPLS gives spe, ssq, n_observed, spe_limit and r2x_per_variable as lists over its blocks.
    Limits at `level` (in (0, 1), ValueError otherwise), NaN with a why in the report when I <= R + 1 or the SPE has no spread.
    On the GPU every block is read once per residual pass (cmtfpls_resid_rows_*); device=False, or R > 16, takes torch ops
    instead.  The training statistics are cached on the model.  Which form ran: ``diagnostics_report_`` (diagnostics.py)."""
    from .diagnostics import sample_diagnostics as _run

    return _run(pls_tensor, X, Y, level, device)


def sample_contributions(pls_tensor, X=None, rows=None, cells: bool = False, device: bool = True) -> dict:
    """Contribution plot data: for each diagnosed sample, which slice of which mode carries its Q residual (SPE) and its Hotelling
    T^2.  X=None: the training rows (fitted scores and ``original_X``; ValueError after a copy_X=False fit); otherwise new rows (a
    ctPLS: a list of blocks), scored as transform scores them.  rows: a 1-D integer array of distinct row indices (ValueError
    otherwise), None for every row; only those rows are read by the contribution pass.
    Returns {"rows": (n,), "scores": (n, R), "t2": (n,) as sample_diagnostics, "t2_closure": (n,) t_i^T S^+ (t_i - tbar), "spe",
    "spe_mode", "t2_mode"}.  For a tPLS spe is (n,) and spe_mode / t2_mode are lists with one (n, D_m) float64 array per trailing
    mode of X: spe_mode[m][i, j] is the sum of e^2, and t2_mode[m][i, j] the sum of d = x * (W U^-1 S^+ (t - tbar)) / n_blocks, over
    the observed cells of sample i whose index along mode m is j.  For a ctPLS each of the three is a list over blocks.  Every
    spe_mode[m] sums over j to spe.  Over a sample without missing values t2_mode[m] sums (over j and blocks) to t2_closure, which
    equals t2 when the training scores have zero mean (a fit on complete data) and differs from it by tbar^T S^+ (t - tbar)
    otherwise; for samples WITH missing values the same formula is applied to the observed cells and that closure is not claimed
    (their scores come from the masked sequence, which is not linear in x).  cells=True adds "spe_cells" (the signed residual e)
    and "t2_cells" (d), shaped (n, *X.shape[1:]) per block, formed by torch ops: ValueError when n * prod(X.shape[1:]) exceeds
    2**28 in a block.  On the GPU every block's selected rows are read once (cmtfpls_contrib_rows_*); device=False, R > 16 or a
    first mode beyond the kernel's LDS takes torch ops instead.  Which form ran: ``contributions_report_`` (contributions.py)."""
    from .contributions import sample_contributions as _run

    return _run(pls_tensor, X, rows, cells, device)


def selectivity_ratio(pls_tensor, X=None, level: float = 0.95, cells: bool = True, device: bool = True) -> dict:
    """Which variables carry the prediction of a fitted tPLS or ctPLS: the selectivity ratio of every cell and of every slice of
    every mode, by target projection onto the fitted response tau = scores coef_ Q^T (I x M).  X=None: the training rows (fitted
    scores and ``original_X``; ValueError after a copy_X=False fit); otherwise new rows (a ctPLS: a list of blocks), scored as
    transform scores them.  With x = X - X_mean over its finite entries, per cell c and response m: a = sum_i x tau_im, d = sum_i
    tau_im^2 over the observed rows of c, s = sum_i x^2, n = the observed rows.
    Returns {"tp_loading": a / d, "explained": a^2 / d, "residual": max(s - explained, 0), "sr": explained / residual, each shaped
    (M, *X.shape[1:]) and left out with cells=False; "n_observed": X.shape[1:]; "sr_mode": one (M, J_k) array per mode k >= 1, the
    sum of explained over the sum of residual over the cells of slice j; "f_limit": F.ppf(level, I - 2, I - 3), I the training
    rows (NaN when I <= 3; nominal where values are missing: see n_observed); "level"}.  sr is NaN where d = 0 or n = 0 and inf where
    residual = 0 < explained; NaN cells are skipped in sr_mode.  A ctPLS gives every value but f_limit and level as a list over its
    blocks, which share tau.  Any order >= 2.  On the GPU every block is read once (cmtfpls_selectivity_cols_*); device=False takes
    torch ops instead.  Which form ran: ``importance_report_`` (importance.py)."""
    from .importance import selectivity_ratio as _run

    return _run(pls_tensor, X, level, cells, device)


def vip_scores(pls_tensor, per_component: bool = False) -> dict:
    """VIP (variable importance in projection) of every slice of every mode k >= 1 of a fitted tPLS or ctPLS, from the fitted factors
    alone: with s_r = max(R2Y[r] - R2Y[r - 1], 0) and unit-norm loadings W_k (J_k x R), vip[k][j] = sqrt(J_k sum_r s_r W_k[j, r]^2 /
    sum_r s_r), so that sum_j vip[k][j]^2 = J_k.  Returns {"vip": a list with one (J_k,) array per mode (per_component=True: (R,
    J_k), row p from the first p + 1 components; a ctPLS: such a list per block), "component_weights": s (R,), "clipped": the
    components whose R2Y increment was negative and taken as 0, "why": None, or why every value is NaN (sum s = 0)}; the last two
    also on the model (``vip_report_``)."""
    from .importance import vip_scores as _run

    return _run(pls_tensor, per_component)


def impute(pls_tensor, X=None, device: bool = True):
    """X with every missing (non-finite) entry filled from the fitted tPLS or ctPLS, X_mean + T W^T there, and every observed entry
    untouched.  X=None: the training rows (their fitted scores and ``original_X`` / ``original_Xs``; ValueError after a copy_X=False
    fit); otherwise new rows (a ctPLS: a list of blocks, ValueError for a wrong number of them), scored as transform scores them,
    rows with missing values included.  NumPy in: NumPy out in the input's dtype; a tensor in: a new tensor of the storage type on
    the input's device (a device tensor stays on the device, a host tensor comes back to the host), the caller's tensor only read
    (a ctPLS: the list of blocks).  On the GPU every block is read once and the
    reconstruction is never materialised (cmtfpls_impute_*; a block uploaded for the call is completed in place, only its gaps
    written); device=False, or R > 16, takes torch ops instead.  ``imputation_report_``: the form that ran, the number of imputed
    entries per block and the reads taken (imputation.py)."""
    from .imputation import impute as _run

    return _run(pls_tensor, X, device)


def get_q2x_heldout(pls_tensor, fraction: float = 0.1, n_repeats: int = 5, random_state=0, device: bool = True, tol: float = 1e-8,
                    max_iter: int = 100) -> dict:
    """Q2X by held-out entries, the X-side counterpart of the Q2Y family: repeat g hides the share `fraction` of the entries of every
    training block (i.i.d., the counter rule of include/cmtfpls.h keyed by seeds[g] =
    np.random.default_rng(random_state).integers(0, 2**63, n_repeats)[g], Philox stream 2 + block), refits a copy of the model
    (its dtype, device, backend, algorithm and options; tol, max_iter; Y = ``original_Y``) in place on the masked copies, and
    scores the refit on the hidden observed entries of the original blocks for every component count:
    Q2X_r = 1 - sum (x - xhat_r)^2 / sum (x - X_mean)^2, xhat_r = X_mean + the first r components, X_mean the refit's.
    Returns {"q2x": (n_repeats, n_blocks, R), "q2x_all": (n_repeats, R) with the blocks pooled by summing numerators and
    denominators, "mean" / "std" (ddof 1, NaN for one repeat) of q2x over the repeats and "mean_all" / "std_all" of q2x_all,
    "n_heldout": (n_repeats, n_blocks) hidden observed entries, "seeds", "report"}.  ValueError unless 0 < fraction < 1 and
    n_repeats >= 1, after a copy_X=False fit, and for a repeat whose masking leaves some sample without an observed entry in a
    block (the masked score divides by that count); NotImplementedError for a sharded model.  On the GPU a repeat reads the
    original blocks twice (cmtfpls_holdout_mask_*, cmtfpls_heldout_resid_*) and no mask tensor exists; device=False, or R > 16,
    takes torch ops with the same mask.  Which form ran is recorded on the model (``q2x_report_``; imputation.py)."""
    from .imputation import get_q2x_heldout as _run

    return _run(pls_tensor, fraction, n_repeats, random_state, device, tol, max_iter)
