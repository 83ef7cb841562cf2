"""Leave-one-out and K-fold cross-validation of a tPLS whose X has missing values, every fold refitted by one workgroup in one
launch (cmtfpls_cv_masked_f64, EngineOptions.masked_folds): against literal refits on the regular engine, per component count,
where the masked arithmetic switches on and off, at the declared limits (min(A, B) <= 64, M <= 64, R <= 16, 150 KB of LDS) and
just past them, in chunks of folds, and for a float32 model.  Every end-to-end test checks the report's form, so a silent decline
cannot compare refits with refits.  Refits are compared with the regular engine, not the oracle: the oracle masks before centring
where tpls.py masks after."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import MASKED_FORM, fold_ids, masked_predictions
from cmtf_pls_amd.validate import get_q2y, get_q2y_kfold, kfold_predictions, loo_predictions

pytestmark = pytest.mark.gpu

_DEV = "cuda:0"
ON = EngineOptions(small_fit=False, masked_folds=True)
REGULAR = EngineOptions(small_fit=False)
LDS_CAP = 150 * 1024


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


def _model(x, y, R, dtype="float64"):
    m = tPLS(R, dtype=dtype, options=ON)
    m.fit(x, y)
    return m


def _masked(rep):
    assert MASKED_FORM in rep["form"], rep
    return rep


def _refit_loo(x, y, R, dtype="float64"):
    """Literal leave-one-out refits on the regular engine: tPLS.fit(X[keep]).predict(X[i:i+1])."""
    want = np.zeros(y.shape)
    keep = np.ones(x.shape[0], dtype=bool)
    for i in range(x.shape[0]):
        keep[i] = False
        r = tPLS(R, dtype=dtype, options=REGULAR)
        r.fit(x[keep], y[keep])
        want[i] = r.predict(x[i:i + 1]).reshape(want[i].shape)
        keep[i] = True
    return want


def _refit_kfold(x, y, ids, K, R, dtype="float64"):
    """Literal per-fold refits on the regular engine, every component count: (R, I, M)."""
    want = np.zeros((R,) + y.shape)
    for k in range(K):
        test = ids == k
        r = tPLS(R, dtype=dtype, options=REGULAR)
        r.fit(x[~test], y[~test])
        sc = r.transform(x[test])
        for c in range(1, R + 1):
            want[c - 1, test] = (sc[:, :c] @ r.coef_[:c, :c]) @ r.Y_factors[1][:, :c].T + r.Y_mean
    return want


def _lds(I, A, B, M, R):
    """cv_masked_lds_bytes (csrc/cv_masked.hip)."""
    n, k, P = min(A, B), max(A, B), A * B
    return 8 * (2 * I + P + A + B + 2 * M + 2 * n * n + n + k + M + R * R + R * (A + B) + R * M + R * R + 3 * R + 256 + 2 * I)


# ---- 1. leave-one-out equals literal refits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,M,R", [((30, 6, 5), 3, 2), ((28, 9), 2, 2), ((60, 10, 8), 4, 3)])
def test_loo_equals_refits(shape, M, R):
    x, y = _data(shape, M, R, 0.1, seed=shape[0])
    m = _model(x, y, R)
    pred = loo_predictions(m)
    rep = _masked(m.q2y_report_)
    assert rep["folds"] == shape[0] and np.asarray(rep["n_iter"]).shape == (shape[0], R)
    want = _refit_loo(x, y, R)
    assert _rel(pred, want) <= 1e-10
    q = get_q2y(m)
    _masked(m.q2y_report_)
    q_ref = get_q2y(m, device_folds=False)
    assert m.q2y_report_["form"].startswith("one refit per fold")
    assert abs(q - q_ref) <= 1e-10 and abs(q - (1 - ((want - y) ** 2).sum() / (y ** 2).sum())) <= 1e-10


def test_option_off_keeps_the_refits():
    x, y = _data((20, 5, 4), 2, 2, 0.1, seed=5)
    m = tPLS(2, dtype="float64", options=REGULAR)
    m.fit(x, y)
    assert loo_predictions(m) is None
    kfold_predictions(m, n_splits=4)
    assert m.q2y_report_["form"].startswith("one refit per fold") and "masked" not in m.q2y_report_["why"]


# ---- 2. K-fold, every component count -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["k4", "shuffled", "loo"])
def test_kfold_every_component_equals_refits(case):
    shape, M, R = (40, 6, 5), 3, 3
    x, y = _data(shape, M, R, 0.1, seed=7)
    I = shape[0]
    folds = None
    K = 4
    if case == "shuffled":
        folds = np.random.default_rng(3).permutation(np.arange(I) % 5)
        folds[:3] = 0                                          # unequal fold sizes
    if case == "loo":
        K = I
    m = _model(x, y, R)
    pred = kfold_predictions(m, n_splits=K, folds=folds)
    rep = _masked(m.q2y_report_)
    ids, K = fold_ids(I, K, folds)
    assert rep["folds"] == K and np.asarray(rep["n_iter"]).shape == (K, R) and rep["masked_folds"] == K
    want = _refit_kfold(x, y, ids, K, R)
    assert pred.shape == (R,) + y.shape
    assert _rel(pred, want) <= 1e-10
    q = get_q2y_kfold(m, n_splits=K, folds=folds, per_component=True)
    q_want = 1 - ((want - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum()
    assert np.abs(q - q_want).max() <= 1e-10
    if case == "loo":
        assert _rel(pred[-1], loo_predictions(m)) <= 1e-12


# ---- 3. where the arithmetic switches ------------------------------------------------------------------------------------------
def test_nan_in_one_row_masks_all_folds_but_its_own():
    x, y = _data((24, 5, 4), 2, 2, 0.0, seed=9)
    x[6, 1, 2] = np.nan
    x[6, 3, 0] = np.nan
    m = _model(x, y, 2)
    pred = loo_predictions(m)
    rep = _masked(m.q2y_report_)
    assert rep["masked_folds"] == 23 and rep["masked_batches"] == 1     # only fold 6 trains unmasked and predicts masked
    assert _rel(pred, _refit_loo(x, y, 2)) <= 1e-10


def _column_only_in_fold0(seed):
    """Column (2, 3) observed only in fold 0's held-out rows (K = 4 contiguous folds of 24): c_p = 0 there."""
    x, y = _data((24, 5, 4), 2, 2, 0.05, seed=seed)
    ids, K = fold_ids(24, 4)
    x[ids != 0, 2, 3] = np.nan
    x[ids == 0, 2, 3] = np.arange(6) + 0.5
    return x, y, ids, K


def test_column_observed_only_in_held_out_rows():
    x, y, ids, K = _column_only_in_fold0(seed=13)
    m = _model(x, y, 2)
    pred = kfold_predictions(m, n_splits=K)
    rep = _masked(m.q2y_report_)
    assert rep["masked_folds"] == K and rep["masked_batches"] >= 1
    assert np.isfinite(pred).all()
    assert _rel(pred, _refit_kfold(x, y, ids, K, 2)) <= 1e-10


def test_held_out_row_without_an_observed_entry_predicts_nan():
    x, y, ids, K = _column_only_in_fold0(seed=17)
    r0 = int(np.flatnonzero(ids == 0)[2])
    x[r0] = np.nan
    x[r0, 2, 3] = 1.5                                          # its one entry is in the column fold 0 never trains on
    m = _model(x, y, 2)
    pred = kfold_predictions(m, n_splits=K)
    _masked(m.q2y_report_)
    want = _refit_kfold(x, y, ids, K, 2)
    assert np.isnan(pred[:, r0]).all() and np.isnan(want[:, r0]).all()
    assert _rel(pred, want) <= 1e-10


def test_training_row_without_an_observed_entry_declines():
    x, y = _data((20, 5, 4), 2, 2, 0.1, seed=19)
    m = _model(x, y, 2)                                        # (the reference's own fit would be NaN everywhere on x4)
    x4 = x.copy()
    x4[4] = np.nan
    ids, K = fold_ids(20, 4)
    pred, why = masked_predictions(m, x4, y, ids, K, 1e-8, 100)
    assert pred is None and why == "training rows without an observed entry of X in folds [1, 2, 3]", why
    pred, why = masked_predictions(m, x4, y, np.arange(20), 20, 1e-8, 100)
    assert pred is None and why.startswith("training rows without an observed entry of X in folds [")
    assert eval(why[why.index("["):]) == [f for f in range(20) if f != 4]       # every fold that trains on row 4


# ---- 4. declared limits ---------------------------------------------------------------------------------------------------------
def _kfold_runs(shape, M, R, K, nan=0.05, seed=23):
    x, y = _data(shape, M, R, nan, seed)
    m = _model(x, y, R)
    pred = kfold_predictions(m, n_splits=K)
    return x, y, m, pred


def _lds_edge_rows(B, M, R):
    I = 2
    while _lds(I + 1, 1, B, M, R) <= LDS_CAP:
        I += 1
    return I


@pytest.mark.parametrize("case", ["side64", "m64", "r16", "lds"])
def test_at_the_limits_runs_the_masked_form(case):
    shape, M, R, K = {"side64": ((24, 64, 64), 2, 2, 2), "m64": ((40, 6, 5), 64, 2, 3), "r16": ((60, 6, 5), 2, 16, 3),
                      "lds": ((_lds_edge_rows(4000, 2, 1), 4000), 2, 1, 2)}[case]
    if case == "lds":
        assert _lds(shape[0], 1, 4000, M, R) <= LDS_CAP < _lds(shape[0] + 1, 1, 4000, M, R)
    x, y, m, pred = _kfold_runs(shape, M, R, K)
    _masked(m.q2y_report_)
    ids, K = fold_ids(shape[0], K)
    assert _rel(pred, _refit_kfold(x, y, ids, K, R)) <= 1e-10


@pytest.mark.parametrize("case", ["side65", "m65", "r17", "lds", "nan_y", "order4", "coupled"])
def test_past_the_limits_declines_to_refits(case):
    x, y = _data((12, 4, 3, 2) if case == "order4" else (20, 6, 5), 2, 2, 0.1, seed=29)
    R, K = 2, 2
    if case == "side65":
        x, y = _data((8, 65, 65), 2, 1, 0.05, seed=29)
        R = 1
    if case == "m65":
        x, y = _data((20, 6, 5), 65, 2, 0.1, seed=29)
    if case == "r17":
        x, y = _data((40, 6, 5), 2, 17, 0.1, seed=29)
        R = 17
    if case == "lds":
        x, y = _data((_lds_edge_rows(4000, 2, 1) + 1, 4000), 2, 1, 0.05, seed=29)
        R = 1
    if case == "nan_y":                                        # (a fit on it would be NaN: the decline itself)
        m = _model(x, y, R)
        y[3, 0] = np.nan
        pred, why = masked_predictions(m, x, y, *fold_ids(20, K), 1e-8, 100)
        assert pred is None and why == "missing values in Y"
        return
    if case == "coupled":
        m = ctPLS(R, dtype="float64", options=ON)
        m.fit([x, x[:, :, :3].copy()], y)
    else:
        m = _model(x, y, R)
    kfold_predictions(m, n_splits=K)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and rep.get("why"), rep
    if case not in ("coupled",):
        assert MASKED_FORM in rep["why"], rep
    if case in ("side65", "m65", "r17", "lds"):
        assert "shape outside" in rep["why"]


# ---- 5. chunks of folds ---------------------------------------------------------------------------------------------------------
def test_chunked_launches_are_bit_identical():
    from cmtf_pls_amd.backend import HipBackend
    be = HipBackend(torch.device(_DEV))
    x, y = _data((36, 7, 6), 3, 3, 0.1, seed=31)
    I, (A, B) = 36, (7, 6)
    X2 = torch.from_numpy(x.reshape(I, -1)).to(_DEV)
    Y2 = torch.from_numpy(y.reshape(I, -1)).to(_DEV)
    ids, K = fold_ids(I, 9)
    fo = torch.from_numpy(ids.astype(np.int32)).to(_DEV)
    one = be.cv_masked(X2, Y2, fo, K, A, B, 3, 1e-8, 100)
    per = int(be.lib.cmtfpls_cv_masked_fold_workspace_bytes(I, A, B, 3, 3))
    for budget in (per, 2 * per, 4 * per + 7):
        many = be.cv_masked(X2, Y2, fo, K, A, B, 3, 1e-8, 100, max_ws_bytes=budget)
        for a, b in zip(one, many):
            assert torch.equal(a, b)
    assert not one[2].any() and one[3][:, 0].all()


# ---- 6. float32 model ----------------------------------------------------------------------------------------------------------
def test_float32_model_computes_in_float64():
    x, y = _data((30, 6, 5), 3, 2, 0.1, seed=37)
    m = _model(x, y, 2, dtype="float32")
    pred = loo_predictions(m)
    _masked(m.q2y_report_)
    assert _rel(pred, _refit_loo(x, y, 2)) <= 1e-10
    assert _rel(pred, _refit_loo(x, y, 2, dtype="float32")) <= 1e-5
