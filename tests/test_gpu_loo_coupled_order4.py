"""Leave-one-out Q2Y of a ctPLS with blocks of order 4 on the device (EngineOptions.tensor_resamples_coupled): get_q2y and
loo_predictions through cmtfpls_loo_xcov_coupled_tensor_f64 against the per-fold refits on the regular engine (device_folds=False) and
float64 oracle refits (loo_coupled_ref.loo_literal), the unchanged routing with the option off and without an order-4 block, and the
declines.  Tolerances: test_gpu_loo_order4.py's (Q2Y 1e-8, predictions 1e-7 relative to max|Y|)."""
import numpy as np
import pytest

import loo_coupled_ref as C
from cmtf_pls_amd import ctPLS
from cmtf_pls_amd import validate as V
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import TENSOR_RANK1
from kfold_coupled_order4_ref import coupled_data

pytestmark = pytest.mark.gpu

R = 3
TWO = ([(24, 6, 5, 4), (24, 7)], 2)                         # (shapes, M)
THREE = ([(20, 6, 5, 4), (20, 8, 6), (20, 3, 4, 7)], 3)
OPT = EngineOptions(small_fit=False, tensor_resamples_coupled=True)
OFF = EngineOptions(small_fit=False)
ENTRY = "cmtfpls_loo_xcov_coupled_tensor_f64"
OLD_WHY = "block 0 of order 4 > 3 (cmtfpls_loo_xcov_coupled_f64)"
REFIT = "one refit per fold on the regular engine"


def _data(which):
    shapes, M = which
    return coupled_data(shapes, M, 4, seed=7)


def _fitted(Xs, y, options=OPT):
    m = ctPLS(R, dtype="float64", options=options)
    m.fit(Xs, y)
    return m


@pytest.fixture(scope="module", params=[TWO, THREE], ids=["two_blocks", "three_blocks"])
def case(request):
    """The data, and the Q2Y and report of the per-fold refit loop (computed once per data set)."""
    Xs, y = _data(request.param)
    m = _fitted(Xs, y)
    q = V.get_q2y(m, device_folds=False)
    return Xs, y, q, dict(m.q2y_report_)


def test_get_q2y_takes_order4_blocks_on_the_device(case):
    Xs, y, q_ref, rep_ref = case
    I = y.shape[0]
    m = _fitted(Xs, y)
    q = V.get_q2y(m)
    rep = m.q2y_report_
    assert rep["form"] == V.LOO_COUPLED_TENSOR_FORM and ENTRY in rep["form"], rep   # (the parent commit refits here)
    assert rep["rank1"] == TENSOR_RANK1 and rep["folds"] == I and rep["blocks"] == len(Xs) and "why" not in rep, rep
    assert rep["n_iter_total"] >= 2 * R * I                                          # at least two passes per fold and component
    assert rep_ref["form"] == REFIT and rep_ref["why"] == "device folds switched off" and "rank1" not in rep_ref
    print("Q2Y", q, "refits", q_ref, "difference", abs(q - q_ref))
    assert abs(q - q_ref) <= 1e-8
    pred = V.loo_predictions(m)
    assert pred.shape == y.shape and m.q2y_report_["form"] == V.LOO_COUPLED_TENSOR_FORM
    oracle = C.loo_literal(Xs, y, R)["pred"].reshape(y.shape)
    err = float(np.abs(pred - oracle).max() / np.abs(y).max())
    print("predictions against oracle refits", err)
    assert err <= 1e-7
    assert abs(C.q2y(pred, y) - q) <= 1e-12                                          # the predictions get_q2y scored


def test_option_off_refits_with_the_report_it_always_had(case):
    Xs, y, q_ref, _ = case
    for opt in (OFF, EngineOptions(small_fit=False, tensor_folds_coupled=True, tensor_folds=True)):   # neither of the siblings switches it on
        m = _fitted(Xs, y, opt)
        assert V.loo_predictions(m) is None
    q = V.get_q2y(m)
    rep = m.q2y_report_
    assert rep["form"] == REFIT and rep["why"] == OLD_WHY and rep["folds"] == y.shape[0] and rep["blocks"] == len(Xs) and "rank1" not in rep
    assert abs(q - q_ref) <= 1e-8


def test_without_an_order4_block_the_option_changes_nothing():
    Xs, y = coupled_data([(24, 6, 20), (24, 7)], 2, 4, seed=7)
    got = []
    for opt in (OFF, OPT):
        m = _fitted(Xs, y, opt)
        q = V.get_q2y(m)
        got.append((q, V.loo_predictions(m), dict(m.q2y_report_)))
    assert got[0][2]["form"] == V.LOO_COUPLED_FORM and got[0][2] == got[1][2]
    assert got[0][0] == got[1][0] and np.array_equal(got[0][1], got[1][1])


def test_a_missing_value_refits_and_names_its_block():
    Xs, y = _data(TWO)
    Xs = [X.copy() for X in Xs]
    Xs[1][3, 2] = np.nan
    m = _fitted(Xs, y)
    assert V.loo_predictions(m) is None
    q = V.get_q2y(m)
    rep = m.q2y_report_
    assert rep["form"] == REFIT and rep["why"] == f"missing values in block 1 ({ENTRY} is the complete-data form)", rep
    assert np.isfinite(q)


def test_get_q2y_reports_the_decline(monkeypatch):
    """A declined shape refits with the why of the limit (the decline forced on the small model: no large block is built)."""
    Xs, y = _data(TWO)
    m = _fitted(Xs, y)
    monkeypatch.setattr(V, "MAX_SIDE", 4)
    q = V.get_q2y(m)
    rep = m.q2y_report_
    assert rep["form"] == REFIT and rep["why"] == f"block 0: mode-0 unfolding: min(6, 20) = 6 > 4 ({ENTRY})", rep
    assert np.isfinite(q)
