"""Leave-one-out and K-fold cross-validation of a tPLS whose X has order 4 AND missing values, every fold refitted by one
512-thread workgroup (cmtfpls_cv_masked_tensor_f64, EngineOptions.masked_tensor_folds): against literal refits on the
regular engine with the option off, per component count, where the masked arithmetic switches on and off, on both sides of the
kernel's size switches, at the declared limits and just past them, in chunks of folds, for a float32 model, and with the option
off.  Every end-to-end test checks the report's form first, so a silent decline cannot compare refits with refits.  Refits are
compared with the regular engine, not the oracle: the oracle masks before centring where tpls.py:128-131 masks after.

Tolerances are those of test_gpu_kfold_order4.py for order 4: predictions 1e-7 relative, Q2Y 1e-8, identical NaN patterns, n_iter
equal to the refits'.  Seeds and shapes: the float64 oracle's inner loop converges below max_iter in every fold (a fold that stops
at 100 amplifies rounding differences); unless a test says otherwise every column is observed in every training part and no
training row is empty (_refit_kfold asserts both)."""
import ast
import functools

import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import (MASKED_FORM, MASKED_TENSOR_FORM, TENSOR_RANK1, fold_ids, masked_predictions, masked_tensor_lds_bytes,
                                masked_tensor_side)
from cmtf_pls_amd.validate import get_q2y, get_q2y_kfold, kfold_predictions, loo_predictions

pytestmark = pytest.mark.gpu

_DEV = "cuda:0"
ON = EngineOptions(small_fit=False, masked_tensor_folds=True)
REGULAR = EngineOptions(small_fit=False)
LDS_CAP = 150 * 1024
PRED_TOL, Q2Y_TOL = 1e-7, 1e-8


def _rel(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float(np.abs(got[ok] - want[ok]).max() / max(np.abs(want[ok]).max(), 1e-300))


def _data(shape, M, R, nan, seed):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=seed)
    if nan:
        x[np.random.default_rng(seed + 100).random(x.shape) < nan] = np.nan
    return x, y


def _model(x, y, R, dtype="float64", options=ON):
    m = tPLS(R, dtype=dtype, options=options)
    m.fit(x, y)
    return m


def _tensor(rep):
    assert MASKED_TENSOR_FORM in rep["form"] and rep["rank1"] == TENSOR_RANK1 and rep["launches"] >= 1, rep
    return rep


def _refit_kfold(x, y, ids, K, R, dtype="float64", columns_observed=True):
    """Literal per-fold refits on the regular engine with the option off, every component count: ((R, I, M), n_iter (K, R)).
    Asserts the data's two conditions: every column observed in every training part (unless the test is about one that is not),
    no training row empty."""
    want = np.zeros((R,) + y.shape)
    n_iter = []
    for k in range(K):
        test = ids == k
        seen = ~np.isnan(x[~test]).reshape(int((~test).sum()), -1)
        assert seen.any(axis=1).all() and (seen.any(axis=0).all() or not columns_observed), f"fold {k}"
        r = tPLS(R, dtype=dtype, options=REGULAR)
        r.fit(x[~test], y[~test])
        sc = r.transform(x[test])
        for c in range(1, R + 1):
            want[c - 1, test] = (sc[:, :c] @ r.coef_[:c, :c]) @ r.Y_factors[1][:, :c].T + r.Y_mean
        n_iter.append([int(v) for v in r.n_iter_])
    return want, n_iter


def _refit_loo(x, y, R, dtype="float64"):
    I = x.shape[0]
    return _refit_kfold(x, y, np.arange(I), I, R, dtype)


def _agree(what, pred, rep, want, n_iter):
    """The comparison of every end-to-end test: deviation printed, then predictions, NaN pattern and n_iter against the refits."""
    dev = _rel(pred, want)
    print(f"{what}: max relative deviation of the predictions {dev:.3e}")
    assert dev <= PRED_TOL
    assert rep["n_iter"] == n_iter


@functools.lru_cache(maxsize=None)
def _kfold40():
    """(40, 6, 5, 4), M 3, R 3, 10 % NaN, seed 40: the data and, per fold assignment, the refits (computed once)."""
    return _data((40, 6, 5, 4), 3, 3, 0.1, seed=40)


@functools.lru_cache(maxsize=None)
def _kfold40_refits(case):
    x, y = _kfold40()
    folds = None
    if case == "shuffled":
        folds = np.random.default_rng(3).permutation(np.arange(40) % 5)
        folds[:3] = 0                                          # unequal fold sizes
    ids, K = fold_ids(40, 40 if case == "loo" else 4, folds)
    return folds, ids, K, _refit_kfold(x, y, ids, K, 3)


# ---- 1. leave-one-out equals literal refits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 5, 7, 11])
def test_loo_equals_refits(seed):
    shape, M, R = (30, 5, 4, 3), 3, 2
    x, y = _data(shape, M, R, 0.1, seed=seed)
    m = _model(x, y, R)
    pred = loo_predictions(m)
    rep = _tensor(m.q2y_report_)
    assert rep["folds"] == 30 and np.asarray(rep["n_iter"]).shape == (30, R)
    want, n_iter = _refit_loo(x, y, R)
    _agree(f"leave-one-out, seed {seed}", pred, rep, want[-1], n_iter)
    q = get_q2y(m)
    _tensor(m.q2y_report_)
    q_ref = get_q2y(m, device_folds=False)
    assert m.q2y_report_["form"].startswith("one refit per fold")
    q_want = 1 - ((want[-1] - y) ** 2).sum() / (y ** 2).sum()
    print(f"Q2Y deviation {abs(q - q_ref):.3e} (get_q2y without device folds), {abs(q - q_want):.3e} (refits)")
    assert abs(q - q_ref) <= Q2Y_TOL and abs(q - q_want) <= Q2Y_TOL


# ---- 2. K-fold, every component count -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["k4", "shuffled", "loo"])
def test_kfold_every_component_equals_refits(case):
    x, y = _kfold40()
    R = 3
    folds, ids, K, (want, n_iter) = _kfold40_refits(case)
    m = _model(x, y, R)
    pred = kfold_predictions(m, n_splits=K, folds=folds)
    rep = _tensor(m.q2y_report_)
    assert rep["folds"] == K and np.asarray(rep["n_iter"]).shape == (K, R) and rep["masked_folds"] == K
    assert pred.shape == (R,) + y.shape
    _agree(f"K-fold {case}", pred, rep, want, n_iter)
    q = get_q2y_kfold(m, n_splits=K, folds=folds, per_component=True)
    q_want = 1 - ((want - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum()
    print(f"Q2Y deviation per component count {np.abs(q - q_want)}")
    assert np.abs(q - q_want).max() <= Q2Y_TOL
    if case == "loo":
        assert _rel(pred[-1], loo_predictions(m)) <= 1e-12


# ---- 3. unequal dims, a unit mode, A = 1 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,M,R,nan,K,seed", [((36, 6, 4, 3), 2, 3, 0.3, 6, 36), ((24, 4, 3, 2), 2, 2, 0.05, 4, 24),
                                                  ((24, 5, 4, 1), 2, 2, 0.1, 4, 24), ((24, 1, 5, 4), 2, 2, 0.1, 4, 27)])
def test_unequal_dims_and_unit_modes(shape, M, R, nan, K, seed):
    x, y = _data(shape, M, R, nan, seed=seed)
    assert len({d for d in shape[1:] if d > 1}) == sum(d > 1 for d in shape[1:])   # no two modes alike: a mix-up of modes shows
    m = _model(x, y, R)
    pred = kfold_predictions(m, n_splits=K)
    rep = _tensor(m.q2y_report_)
    ids, K = fold_ids(shape[0], K)
    _agree(f"{shape}", pred, rep, *_refit_kfold(x, y, ids, K, R))


# ---- 4. where the arithmetic switches -------------------------------------------------------------------------------------------
def test_nan_in_one_row_masks_all_folds_but_its_own():
    x, y = _data((24, 4, 3, 2), 2, 2, 0.0, seed=11)
    x[6, 1, 2, 0] = np.nan
    x[6, 3, 0, 1] = np.nan
    m = _model(x, y, 2)
    pred = loo_predictions(m)
    rep = _tensor(m.q2y_report_)
    assert rep["masked_folds"] == 23 and rep["masked_batches"] == 1     # only fold 6 trains unmasked and predicts masked
    want, n_iter = _refit_loo(x, y, 2)
    _agree("NaN in one row", pred, rep, want[-1], n_iter)


def _column_only_in_fold0(seed):
    """Column (2, 1, 1) observed only in fold 0's held-out rows (K = 4 contiguous folds of 24): c_p = 0 there (the one case whose
    columns are, on purpose, not all observed in every training part)."""
    x, y = _data((24, 4, 3, 2), 2, 2, 0.05, seed=seed)
    ids, K = fold_ids(24, 4)
    x[ids != 0, 2, 1, 1] = np.nan
    x[ids == 0, 2, 1, 1] = np.arange(6) + 0.5
    return x, y, ids, K


def test_column_observed_only_in_held_out_rows():
    x, y, ids, K = _column_only_in_fold0(seed=17)
    m = _model(x, y, 2)
    pred = kfold_predictions(m, n_splits=K)
    rep = _tensor(m.q2y_report_)
    assert rep["masked_folds"] == K and rep["masked_batches"] >= 1
    assert np.isfinite(pred).all()
    _agree("column observed only in held-out rows", pred, rep, *_refit_kfold(x, y, ids, K, 2, columns_observed=False))


def test_held_out_row_without_an_observed_entry_predicts_nan():
    x, y, ids, K = _column_only_in_fold0(seed=17)
    r0 = int(np.flatnonzero(ids == 0)[2])
    x[r0] = np.nan
    x[r0, 2, 1, 1] = 1.5                                       # its one entry is in the column fold 0 never trains on
    m = _model(x, y, 2)
    pred = kfold_predictions(m, n_splits=K)
    rep = _tensor(m.q2y_report_)
    want, n_iter = _refit_kfold(x, y, ids, K, 2, columns_observed=False)
    assert np.isnan(pred[:, r0]).all() and np.isnan(want[:, r0]).all()
    _agree("held-out row without a trained entry", pred, rep, want, n_iter)


def test_training_row_without_an_observed_entry_declines():
    x, y = _data((20, 4, 3, 2), 2, 2, 0.1, seed=19)
    m = _model(x, y, 2)                                        # (the reference's own fit would be NaN everywhere on x4)
    x4 = x.copy()
    x4[4] = np.nan
    ids, K = fold_ids(20, 4)
    pred, why = masked_predictions(m, x4, y, ids, K, 1e-8, 100)
    assert pred is None and why == "training rows without an observed entry of X in folds [1, 2, 3]", why
    pred, why = masked_predictions(m, x4, y, np.arange(20), 20, 1e-8, 100)
    assert pred is None and why.startswith("training rows without an observed entry of X in folds [")
    assert ast.literal_eval(why[why.index("["):]) == [f for f in range(20) if f != 4]       # every fold that trains on row 4


# ---- 5. both branches of each size switch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,K,seed", [((30, 5, 4, 3), 5, 1), ((12, 2, 32, 32), 3, 12)])
def test_both_sides_of_the_thread_count(shape, K, seed):
    """P = 60 < the 512 threads: mf_contract's partial rows and the CP's row groups of v.  P = 2048 with B1 B2 = 1024 >= the threads:
    a thread per column in both."""
    P, B = int(np.prod(shape[1:])), shape[2] * shape[3]
    assert (P < 512) != (B >= 1024)
    x, y = _data(shape, 2, 2, 0.1, seed=seed)
    m = _model(x, y, 2)
    pred = kfold_predictions(m, n_splits=K)
    rep = _tensor(m.q2y_report_)
    ids, K = fold_ids(shape[0], K)
    _agree(f"P = {P}", pred, rep, *_refit_kfold(x, y, ids, K, 2))


# ---- 6. declared limits ---------------------------------------------------------------------------------------------------------
def _lds_edge_rows(A, B1, B2, M, R):
    I = 2
    while masked_tensor_lds_bytes(I + 1, A, B1, B2, M, R) <= LDS_CAP:
        I += 1
    return I


_AT = {"side64": ((12, 64, 8, 8), 2, 2, 2, 23), "m64": ((40, 6, 5, 4), 64, 2, 3, 23), "r16": ((60, 6, 5, 4), 2, 16, 3, 49),
       "lds": (None, 2, 1, 2, 23), "all": (None, 64, 16, 2, 23)}     # all: short side 64, M = 64, R = 16 and the rows at the cap for them


@pytest.mark.parametrize("case", list(_AT))
def test_at_the_limits_runs_the_tensor_form(case):
    shape, M, R, K, seed = _AT[case]
    if case == "side64":
        assert masked_tensor_side(*shape[1:]) == 64
    if case in ("lds", "all"):
        shape = (_lds_edge_rows(64, 8, 8, M, R), 64, 8, 8)
        assert masked_tensor_lds_bytes(shape[0], 64, 8, 8, M, R) <= LDS_CAP < masked_tensor_lds_bytes(shape[0] + 1, 64, 8, 8, M, R)
    x, y = _data(shape, M, R, 0.05, seed)
    m = _model(x, y, R)
    pred = kfold_predictions(m, n_splits=K)
    rep = _tensor(m.q2y_report_)
    ids, K = fold_ids(shape[0], K)
    _agree(f"at the limit {case} {shape}", pred, rep, *_refit_kfold(x, y, ids, K, R))


@pytest.mark.parametrize("case", ["side65", "m65", "r17", "lds"])
def test_past_the_limits_declines_to_refits(case):
    shape, M, R = {"side65": ((8, 65, 13, 5), 2, 1), "m65": ((20, 6, 5, 4), 65, 2), "r17": ((40, 6, 5, 4), 2, 17),
                   "lds": ((_lds_edge_rows(64, 8, 8, 2, 1) + 1, 64, 8, 8), 2, 1)}[case]
    if case == "side65":
        assert masked_tensor_side(*shape[1:]) == 65
    x, y = _data(shape, M, R, 0.05, seed=29)
    m = _model(x, y, R)
    kfold_predictions(m, n_splits=2)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and MASKED_TENSOR_FORM in rep["why"] and "shape outside" in rep["why"], rep


# ---- 7. chunks of folds ---------------------------------------------------------------------------------------------------------
def test_chunked_launches_are_bit_identical():
    from cmtf_pls_amd.backend import HipBackend
    be = HipBackend(torch.device(_DEV))
    x, y = _data((36, 6, 4, 3), 2, 3, 0.3, seed=36)
    I, (A, B1, B2), M, R = 36, (6, 4, 3), 2, 3
    X2 = torch.from_numpy(x.reshape(I, -1)).to(_DEV)
    Y2 = torch.from_numpy(y.reshape(I, -1)).to(_DEV)
    ids, K = fold_ids(I, 9)
    fo = torch.from_numpy(ids.astype(np.int32)).to(_DEV)
    one = be.cv_masked_tensor(X2, Y2, fo, K, A, B1, B2, R, 1e-8, 100)
    assert one[4] == 1
    per = int(be.lib.cmtfpls_cv_masked_tensor_fold_workspace_bytes(I, A, B1, B2, M, R))
    for budget, launches in ((per, 9), (2 * per, 5), (4 * per + 7, 3)):
        many = be.cv_masked_tensor(X2, Y2, fo, K, A, B1, B2, R, 1e-8, 100, max_ws_bytes=budget)
        assert many[4] == launches
        for a, b in zip(one[:4], many[:4]):
            assert torch.equal(a, b)
    assert not one[2].any() and one[3][:, 0].all()


# ---- 8. float32 model -----------------------------------------------------------------------------------------------------------
def test_float32_model_computes_in_float64():
    x, y = _data((30, 5, 4, 3), 3, 2, 0.1, seed=1)
    m = _model(x, y, 2, dtype="float32")
    pred = loo_predictions(m)
    _tensor(m.q2y_report_)
    d64 = _rel(pred, _refit_loo(x, y, 2)[0][-1])
    d32 = _rel(pred, _refit_loo(x, y, 2, dtype="float32")[0][-1])
    print(f"float32 model: deviation from float64 refits {d64:.3e}, from float32 refits {d32:.3e}")
    assert d64 <= PRED_TOL and d32 <= 1e-5


# ---- 9. option off: every report and every bit as before ------------------------------------------------------------------------
@pytest.mark.parametrize("options,text", [
    (dict(masked_folds=True), f"the masked form ({MASKED_FORM}) declined: X of order 4 (the masked form takes order 2 and 3)"),
    (dict(tensor_folds=True), "missing values in X"),
    (dict(), "X of order 4 (the device form takes order 2 and 3)")])
def test_option_off_keeps_the_refits_and_their_reasons(options, text):
    x, y = _data((24, 4, 3, 2), 2, 2, 0.05, seed=24)
    m = _model(x, y, 2, options=EngineOptions(small_fit=False, **options))
    assert loo_predictions(m) is None
    kfold_predictions(m, n_splits=4)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and rep["why"] == text and "rank1" not in rep, rep
    get_q2y(m)
    assert m.q2y_report_["form"].startswith("one refit per fold") and "tensor" not in m.q2y_report_["why"], m.q2y_report_


@pytest.mark.parametrize("shape,nan,base", [((24, 4, 3, 2), 0.0, dict(tensor_folds=True)), ((24, 5, 4), 0.1, dict(masked_folds=True)),
                                            ((24, 5, 4), 0.1, dict())])
def test_option_on_leaves_other_inputs_alone(shape, nan, base):
    """Complete order-4 X, and order-3 X with NaN: the same routing and the same bits with and without masked_tensor_folds."""
    x, y = _data(shape, 2, 2, nan, seed=24)
    runs = []
    for extra in (dict(), dict(masked_tensor_folds=True)):
        m = _model(x, y, 2, options=EngineOptions(small_fit=False, **base, **extra))
        pred = kfold_predictions(m, n_splits=4)
        rep = dict(m.q2y_report_)
        loo = loo_predictions(m)
        runs.append((pred, rep, loo, dict(m.q2y_report_)))
    (p0, r0, l0, q0), (p1, r1, l1, q1) = runs
    assert r0 == r1 and q0 == q1 and MASKED_TENSOR_FORM not in r1["form"] and MASKED_TENSOR_FORM not in str(r1.get("why"))
    assert np.array_equal(p0, p1, equal_nan=True)
    assert (l0 is None and l1 is None) or np.array_equal(l0, l1, equal_nan=True)
    if base:
        assert not r1["form"].startswith("one refit per fold"), r1
