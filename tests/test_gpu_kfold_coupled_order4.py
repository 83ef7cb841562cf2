"""Device cross-validation of a ctPLS with blocks of order 4 (EngineOptions.tensor_folds_coupled): K-fold, the permutation
test (with coupled_permutations), repeated and nested K-fold run the coupled passes with the rank-1 CP of every order-4 block's
cross-covariance inside the fold loop (cmtfpls_kfold_inner_coupled_tensor_f64), against literal refits on the regular engine
(device_folds=False) and float64 oracle.fit_ctpls refits.  Tolerances: those of test_gpu_kfold_order4.py (predictions 1e-7 relative,
Q2Y 1e-8, iteration counts and the nested selection identical)."""
import numpy as np
import pytest

from cmtf_pls_amd import ctPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import TENSOR_RANK1, fold_ids
from cmtf_pls_amd.validate import (bootstrap_factors, get_q2y_kfold, get_q2y_nested_kfold, get_q2y_repeated_kfold, kfold_predictions,
                                   permutation_test_q2y)
from kfold_coupled_order4_ref import coupled_data, oracle_fold_predictions

pytestmark = pytest.mark.gpu

SHAPES, M, R, K = [(48, 6, 5, 4), (48, 7)], 3, 3, 4
THREE = [(48, 6, 5, 4), (48, 8, 6), (48, 3, 4, 7)]
OPT = EngineOptions(small_fit=False, tensor_folds_coupled=True)
ENTRY = "cmtfpls_kfold_inner_coupled_tensor_f64"
OLD = "block 0 of order 4 (the device form takes order 2 and 3)"


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(np.abs(np.asarray(want)).max(), 1e-300))


def _data(shapes=SHAPES, dtype="float64", seed=7):
    Xs, y = coupled_data(shapes, M, R + 1, seed=seed)
    if dtype == "float32":
        Xs = [X.astype(np.float32).astype(np.float64) for X in Xs]
    return Xs, y


def _fitted(Xs, y, dtype="float64", options=OPT):
    m = ctPLS(R, dtype=dtype, options=options)
    m.fit(Xs, y)
    return m


def _device_report(rep):
    assert ENTRY in rep["form"] and rep.get("rank1") == TENSOR_RANK1 and "why" not in rep, rep
    assert "cmtfpls_kfold_inner_coupled_f64" not in rep["form"] and "cmtfpls_kfold_inner_coupled_grouped_f64" not in rep["form"]


def _kfold_against_refits_and_oracle(shapes, dtype):
    Xs, y = _data(shapes, dtype)
    m = _fitted(Xs, y, dtype)
    q = get_q2y_kfold(m, n_splits=K, per_component=True)
    rep = m.q2y_report_
    _device_report(rep)                                                              # (the parent commit refits here)
    assert "K folds from shared reads of every block" in rep["form"] and rep["x_reads"] == [2 * R] * len(shapes) and rep["folds"] == K
    pred = kfold_predictions(m, n_splits=K)
    pred_ref = kfold_predictions(m, n_splits=K, device_folds=False)
    ref = m.q2y_report_
    assert ref["form"].startswith("one refit per fold") and "rank1" not in ref
    print("predictions against refits", _rel(pred, pred_ref))
    assert _rel(pred, pred_ref) <= 1e-7
    assert rep["n_iter"] == [list(v) for v in ref["n_iter"]]
    q_ref = get_q2y_kfold(m, n_splits=K, per_component=True, device_folds=False)
    assert q.shape == (R,) and np.abs(q - q_ref).max() <= 1e-8 * max(1.0, np.abs(q_ref).max()), (q, q_ref)
    ids, _ = fold_ids(shapes[0][0], K)
    want, n_iter = oracle_fold_predictions(Xs, y, ids, K, R)                         # float64 oracle refits of every fold
    assert rep["n_iter"] == n_iter, (rep["n_iter"], n_iter)
    print("predictions against the oracle", _rel(pred, want))
    assert _rel(pred, want) <= 1e-7
    q_or = 1 - ((want - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum()
    assert np.abs(q - q_or).max() <= 1e-8 * max(1.0, np.abs(q_or).max()), (q, q_or)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_kfold_takes_a_block_of_order4_on_the_device(dtype):
    _kfold_against_refits_and_oracle(SHAPES, dtype)


def test_kfold_takes_three_blocks_two_of_order4():
    _kfold_against_refits_and_oracle(THREE, "float64")


def test_permutation_test_takes_a_block_of_order4():
    Xs, y = _data()
    m = _fitted(Xs, y, options=OPT.but(coupled_permutations=True))
    res = permutation_test_q2y(m, n_permutations=7, n_splits=K, random_state=3, per_component=True)
    rep = m.q2y_report_
    _device_report(rep)
    assert rep["passes"] == 1 and rep["models_per_pass"] == 7 * K and "cmtfpls_kfold_wide_xcov" in rep["form"]
    assert rep["x_reads"] == [2 * R] * 2
    _device_report(rep["observed"])
    ref = permutation_test_q2y(m, n_permutations=7, n_splits=K, random_state=3, per_component=True, device_folds=False)
    assert m.q2y_report_["passes"] == 0 and "rank1" not in m.q2y_report_
    assert np.array_equal(res["permutations"], ref["permutations"])
    assert np.abs(res["null"] - ref["null"]).max() <= 1e-8 * max(1.0, np.abs(ref["null"]).max())
    assert np.abs(res["q2y"] - ref["q2y"]).max() <= 1e-8
    assert rep["n_iter"] == m.q2y_report_["n_iter"]


def test_permutation_test_without_coupled_permutations_refits_as_before():
    Xs, y = _data()
    m = _fitted(Xs, y)
    permutation_test_q2y(m, n_permutations=2, n_splits=K, random_state=3)
    rep = m.q2y_report_
    assert rep["passes"] == 0 and rep["why"] == "coupled model: permutation device form not built" and "rank1" not in rep, rep
    _device_report(rep["observed"])


def test_repeated_kfold_takes_a_block_of_order4():
    Xs, y = _data()
    m = _fitted(Xs, y)
    res = get_q2y_repeated_kfold(m, n_splits=K, n_repeats=3, per_component=True)
    rep = m.q2y_report_
    _device_report(rep)
    assert rep["passes"] == 1 and rep["splits_per_pass"] == 3 and "cmtfpls_kfold_epilogue_splits_f64" in rep["form"]
    ref = get_q2y_repeated_kfold(m, n_splits=K, n_repeats=3, per_component=True, device_folds=False)
    assert m.q2y_report_["passes"] == 0 and "rank1" not in m.q2y_report_
    assert np.array_equal(res["folds"], ref["folds"])
    assert np.abs(res["q2y"] - ref["q2y"]).max() <= 1e-8 * max(1.0, np.abs(ref["q2y"]).max())
    assert rep["n_iter"] == m.q2y_report_["n_iter"]


def test_nested_kfold_takes_a_block_of_order4():
    Xs, y = _data()
    m = _fitted(Xs, y)
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


def test_option_off_refits_with_the_old_reason():
    Xs, y = _data()
    for opt in (EngineOptions(small_fit=False), EngineOptions(small_fit=False, tensor_folds=True)):
        m = _fitted(Xs, y, options=opt)
        get_q2y_kfold(m, n_splits=K)
        rep = m.q2y_report_
        assert rep["form"].startswith("one refit per fold") and rep["why"] == OLD and "rank1" not in rep, rep


def test_missing_values_in_a_block_still_refit():
    for b, at in ((0, (3, 1, 2, 0)), (1, (5, 2))):
        Xs, y = _data()
        Xs[b][at] = np.nan
        m = _fitted(Xs, y)
        get_q2y_kfold(m, n_splits=K)
        rep = m.q2y_report_
        assert rep["form"].startswith("one refit per fold") and rep["why"] == f"missing values in block {b}" and "rank1" not in rep, rep


def test_bootstrap_still_refits_with_its_reason():
    Xs, y = _data()
    m = _fitted(Xs, y)
    bootstrap_factors(m, n_resamples=3, random_state=1)
    rep = m.bootstrap_report_
    assert rep["form"] == "one refit per resample on the regular engine" and rep["passes"] == 0 and rep["why"] == OLD, rep


def test_order3_blocks_give_the_same_bits_and_report_with_the_option_on():
    Xs, y = _data([(48, 6, 20), (48, 7)])
    reps = []
    for opt in (EngineOptions(small_fit=False), OPT):
        m = _fitted(Xs, y, options=opt)
        q = get_q2y_kfold(m, n_splits=K, per_component=True)
        reps.append((q, m.q2y_report_))
    assert np.array_equal(reps[0][0], reps[1][0]) and reps[0][1] == reps[1][1]       # the same bits, the same report
    assert "rank1" not in reps[1][1] and "cmtfpls_kfold_inner_coupled_f64" in reps[1][1]["form"]
