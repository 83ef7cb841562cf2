"""Device cross-validation of a tPLS whose X has order 4 (EngineOptions.tensor_folds): K-fold, the permutation test,
repeated and nested K-fold take X as I x A x B1 B2 with the rank-1 CP of each fold's cross-covariance inside the fold loop
(cmtfpls_kfold_inner_tensor_f64), against literal refits on the regular engine (device_folds=False) and float64 oracle refits.
Tolerances: those test_gpu_kfold.py uses for order 3 (predictions 1e-7 relative, Q2Y 1e-8)."""
import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import TENSOR_RANK1, fold_ids
from cmtf_pls_amd.validate import (get_q2y_kfold, get_q2y_nested_kfold, get_q2y_repeated_kfold, kfold_predictions,
                                   permutation_test_q2y)

pytestmark = pytest.mark.gpu

SHAPE, M, R, K = (48, 6, 5, 4), 3, 3, 4
OPT = EngineOptions(small_fit=False, tensor_folds=True)
ENTRY = "cmtfpls_kfold_inner_tensor_f64"


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(np.abs(np.asarray(want)).max(), 1e-300))


def _data(dtype="float64", seed=7):
    x, y, _ = O.import_synthetic(SHAPE, M, R + 1, error=0.3, seed=seed)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)
    return x, y


def _fitted(x, y, dtype="float64", options=OPT):
    m = tPLS(R, dtype=dtype, options=options)
    m.fit(x, y)
    return m


def _device_report(rep):
    assert ENTRY in rep["form"] and rep.get("rank1") == TENSOR_RANK1 and "why" not in rep, rep


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_kfold_takes_order4_on_the_device(dtype):
    x, y = _data(dtype)
    m = _fitted(x, y, dtype)
    q = get_q2y_kfold(m, n_splits=K, per_component=True)
    rep = m.q2y_report_
    _device_report(rep)                                                              # (the parent commit refits here)
    assert "K folds from shared reads of X" in rep["form"] and rep["x_reads"] == 2 * R and rep["folds"] == K
    pred = kfold_predictions(m, n_splits=K)
    pred_ref = kfold_predictions(m, n_splits=K, device_folds=False)
    ref = m.q2y_report_
    assert ref["form"].startswith("one refit per fold") and "rank1" not in ref
    print("predictions against refits", _rel(pred, pred_ref))
    assert _rel(pred, pred_ref) <= 1e-7
    assert rep["n_iter"] == [list(v) for v in ref["n_iter"]]
    q_ref = get_q2y_kfold(m, n_splits=K, per_component=True, device_folds=False)
    assert q.shape == (R,) and np.abs(q - q_ref).max() <= 1e-8 * max(1.0, np.abs(q_ref).max()), (q, q_ref)
    ids, _ = fold_ids(SHAPE[0], K)                                                   # float64 oracle refits of every fold
    want = np.zeros_like(pred)
    for k in range(K):
        test = ids == k
        fit = O.fit_tpls(x[~test], y[~test], R)
        s = O.transform(fit, x[test])
        for r in range(1, R + 1):
            want[r - 1, test] = (s[:, :r] @ fit.coef[:r, :r]) @ fit.Q[:, :r].T + fit.y_mean
        assert rep["n_iter"][k] == fit.n_iter, (k, rep["n_iter"][k], fit.n_iter)
    print("predictions against the oracle", _rel(pred, want))
    assert _rel(pred, want) <= 1e-7
    q_or = 1 - ((want - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum()
    assert np.abs(q - q_or).max() <= 1e-8 * max(1.0, np.abs(q_or).max()), (q, q_or)


def test_permutation_test_takes_order4():
    x, y = _data()
    m = _fitted(x, y)
    res = permutation_test_q2y(m, n_permutations=7, n_splits=K, random_state=3, per_component=True)
    rep = m.q2y_report_
    _device_report(rep)
    assert rep["passes"] == 1 and rep["models_per_pass"] == 7 * K and "cmtfpls_kfold_wide_xcov" in rep["form"]
    _device_report(rep["observed"])
    ref = permutation_test_q2y(m, n_permutations=7, n_splits=K, random_state=3, per_component=True, device_folds=False)
    assert m.q2y_report_["passes"] == 0 and "rank1" not in m.q2y_report_
    assert np.array_equal(res["permutations"], ref["permutations"])
    assert np.abs(res["null"] - ref["null"]).max() <= 1e-8 * max(1.0, np.abs(ref["null"]).max())
    assert np.abs(res["q2y"] - ref["q2y"]).max() <= 1e-8
    assert rep["n_iter"] == m.q2y_report_["n_iter"]


def test_repeated_kfold_takes_order4():
    x, y = _data()
    m = _fitted(x, y)
    res = get_q2y_repeated_kfold(m, n_splits=K, n_repeats=3, per_component=True)
    rep = m.q2y_report_
    _device_report(rep)
    assert rep["passes"] == 1 and rep["splits_per_pass"] == 3 and "cmtfpls_kfold_epilogue_splits_f64" in rep["form"]
    ref = get_q2y_repeated_kfold(m, n_splits=K, n_repeats=3, per_component=True, device_folds=False)
    assert m.q2y_report_["passes"] == 0 and "rank1" not in m.q2y_report_
    assert np.array_equal(res["folds"], ref["folds"])
    assert np.abs(res["q2y"] - ref["q2y"]).max() <= 1e-8 * max(1.0, np.abs(ref["q2y"]).max())
    assert rep["n_iter"] == m.q2y_report_["n_iter"]


def test_nested_kfold_takes_order4():
    x, y = _data()
    m = _fitted(x, y)
    res = get_q2y_nested_kfold(m, n_outer=3, n_inner=3)
    rep = m.q2y_report_
    _device_report(rep)
    assert rep["passes"] == 1 and rep["models"] == 12 and "cmtfpls_kfold_epilogue_weighted_f64" in rep["form"]
    ref = get_q2y_nested_kfold(m, n_outer=3, n_inner=3, device_folds=False)
    assert m.q2y_report_["passes"] == 0 and "rank1" not in m.q2y_report_
    assert np.array_equal(res["selected"], ref["selected"])
    assert abs(res["q2y"] - ref["q2y"]) <= 1e-8 * max(1.0, abs(ref["q2y"]))
    for key in ("inner_q2y", "outer_q2y"):
        assert np.abs(res[key] - ref[key]).max() <= 1e-8 * max(1.0, np.abs(ref[key]).max()), key
    assert _rel(res["predictions"], ref["predictions"]) <= 1e-7


def test_missing_values_still_refit():
    x, y = _data()
    x[3, 1, 2, 0] = np.nan
    m = _fitted(x, y)
    get_q2y_kfold(m, n_splits=K)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and rep["why"] == "missing values in X" and "rank1" not in rep, rep


def test_coupled_block_of_order4_still_refits():
    x, y = _data()
    xm = np.random.default_rng(3).standard_normal((SHAPE[0], 7))
    m = ctPLS(2, dtype="float64", options=OPT)
    m.fit([x, xm], y)
    get_q2y_kfold(m, n_splits=K)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and rep["why"] == "block 0 of order 4 (the device form takes order 2 and 3)", rep


def test_shape_beyond_the_unfolding_limit_refits_with_the_new_reason():
    x, y, _ = O.import_synthetic((12, 257, 1, 257), 2, 2, error=0.3, seed=5)
    m = tPLS(1, dtype="float64", options=OPT)
    m.fit(x, y)
    pred = kfold_predictions(m, n_splits=3)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and rep["why"] == "mode-0 unfolding: min(257, 257) = 257 > 256", rep
    assert np.all(np.isfinite(pred))


def test_option_off_and_order3_reports_are_as_before():
    x, y = _data()
    m = _fitted(x, y, options=EngineOptions(small_fit=False))                        # the default: an order-4 X refits as it always did
    get_q2y_kfold(m, n_splits=K)
    assert m.q2y_report_["why"] == "X of order 4 (the device form takes order 2 and 3)"
    x3, y3, _ = O.import_synthetic((48, 6, 20), M, R + 1, error=0.3, seed=7)
    reps = []
    for opt in (EngineOptions(small_fit=False), OPT):
        m3 = _fitted(x3, y3, options=opt)
        q = get_q2y_kfold(m3, n_splits=K, per_component=True)
        reps.append((q, m3.q2y_report_))
    assert np.array_equal(reps[0][0], reps[1][0]) and reps[0][1] == reps[1][1]       # the same bits, the same report
    assert "rank1" not in reps[1][1] and "cmtfpls_kfold_inner_f64" in reps[1][1]["form"]
