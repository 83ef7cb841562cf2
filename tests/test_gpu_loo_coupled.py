"""validate.get_q2y / loo_predictions of a fitted ctPLS: the leave-one-out kernel of coupled models (cmtfpls_loo_xcov_coupled_f64,
DESIGN 8r) through the public interface, its routing and its reports.  Reference: loo_coupled_ref.loo_literal (literal refits over
the float64 oracle) on every fold of the first two cases of tests/test_gpu_loo_coupled_kernel.py; bound: that file's, normwise <=
max(1e-8, 10 x condition_probe).  Every test checks the report's form, so a silent refit cannot compare refits with refits."""
import numpy as np
import pytest

import loo_coupled_ref as C
import loo_xcov_ref as L
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import COUPLED_FORM
from cmtf_pls_amd.validate import LOO_COUPLED_FORM, LOO_REFIT_FORM, get_q2y, loo_predictions

pytestmark = pytest.mark.gpu

OFF = EngineOptions(small_fit=False)
ON = EngineOptions(small_fit=False, masked_folds_coupled=True)
CASES = C.BASIC_CASES[:2]


def _fit(case, options=OFF, xs=None):
    data, y = C._data(case)
    xs = [np.array(x) for x in (data if xs is None else xs)]
    m = ctPLS(case[3], dtype="float64", options=options)
    m.fit(xs, np.array(y))
    return m, xs, np.array(y)


def _device_report(rep, case):
    assert rep["form"] == LOO_COUPLED_FORM and "why" not in rep, rep
    assert rep["folds"] == case[0] and rep["blocks"] == len(case[1]), rep
    assert isinstance(rep["n_iter_total"], int) and rep["n_iter_total"] >= 2 * case[0] * case[3], rep


@pytest.mark.parametrize("case", CASES, ids=[C.case_id(c) for c in CASES])
def test_q2y_and_predictions_equal_the_literal_refits(case):
    m, xs, y = _fit(case)
    ref = C.reference(case, C.TOL, C.MAX_ITER)
    bound = C.case_bound(case, C.TOL, C.MAX_ITER)
    q = get_q2y(m)
    _device_report(m.q2y_report_, case)
    firm = ~C.on_threshold(ref, C.TOL)
    if firm.all():
        assert m.q2y_report_["n_iter_total"] == int(ref["n_iter"].sum())
    pred = loo_predictions(m)
    _device_report(m.q2y_report_, case)
    assert pred.shape == y.shape
    err = C.normwise(pred, ref["pred"])
    want = C.q2y(ref["pred"], y)
    print(f"{C.case_id(case)}: predictions normwise {err:.2e} (bound {bound:.2e}); Q2Y {q:.12f} literal {want:.12f}")
    assert err <= bound
    assert abs(q - C.q2y(pred, y)) <= 1e-12                                         # validate.py:35-37 on those predictions (a second run)
    assert C.normwise(q, want) <= bound


@pytest.mark.parametrize("case", CASES, ids=[C.case_id(c) for c in CASES])
def test_device_folds_off_refits_to_the_same_q2y(case):
    m, xs, y = _fit(case)
    ref = C.reference(case, C.TOL, C.MAX_ITER)
    bound = C.case_bound(case, C.TOL, C.MAX_ITER)
    q_dev = get_q2y(m)
    _device_report(m.q2y_report_, case)
    q_refit = get_q2y(m, device_folds=False)
    rep = m.q2y_report_
    assert rep["form"] == LOO_REFIT_FORM and rep["why"] == "device folds switched off", rep
    assert rep["folds"] == case[0] and rep["blocks"] == len(case[1]) and rep["n_iter_total"] >= 2 * case[0] * case[3], rep
    want = C.q2y(ref["pred"], y)
    print(f"{C.case_id(case)}: Q2Y device {q_dev:.12f} refit {q_refit:.12f} literal {want:.12f}")
    assert C.normwise(q_refit, want) <= bound and C.normwise(q_dev, want) <= bound


def _refits_with(m, I, nb, needle):
    q = get_q2y(m)
    rep = m.q2y_report_
    assert np.isfinite(q)
    assert rep["form"] == LOO_REFIT_FORM and needle in rep["why"], rep
    assert rep["folds"] == I and rep["blocks"] == nb and rep["n_iter_total"] >= I, rep
    assert loo_predictions(m) is None


def test_an_order_4_block_refits_and_says_why():
    rng = np.random.default_rng(3)
    T = rng.standard_normal((7, 2))
    xs = [np.einsum("ir,ar,br,cr->iabc", T, *(rng.standard_normal((d, 2)) for d in (3, 2, 4))) + 0.1 * rng.standard_normal((7, 3, 2, 4)),
          T @ rng.standard_normal((2, 5)) + 0.1 * rng.standard_normal((7, 5))]
    y = T @ rng.standard_normal((2, 2)) + 0.1 * rng.standard_normal((7, 2))
    m = ctPLS(2, dtype="float64", options=OFF)
    m.fit(xs, y)
    _refits_with(m, 7, 2, "block 0 of order 4 > 3")


def test_a_nan_block_without_the_option_refits_and_with_it_takes_the_masked_form():
    case = CASES[0]
    data, _ = C._data(case)
    xs = [np.array(x) for x in data]
    xs[1][2, 3] = np.nan
    m, _, y = _fit(case, OFF, xs)
    _refits_with(m, case[0], 2, "missing values in block 1")
    on, _, _ = _fit(case, ON, xs)
    q = get_q2y(on)
    rep = on.q2y_report_
    assert COUPLED_FORM in rep["form"] and rep["refitted"] == [] and "why" not in rep, rep
    assert rep["folds"] == case[0] and rep["blocks"] == 2 and rep["n_iter_total"] == int(np.sum(rep["n_iter"])), rep
    assert np.isfinite(q)
    assert loo_predictions(on).shape == y.shape


def test_nine_blocks_refit_and_say_why():
    rng = np.random.default_rng(5)
    T = rng.standard_normal((6, 2))
    xs = [T @ rng.standard_normal((2, 3)) + 0.1 * rng.standard_normal((6, 3)) for _ in range(9)]
    y = T @ rng.standard_normal((2, 2)) + 0.1 * rng.standard_normal((6, 2))
    m = ctPLS(2, dtype="float64", options=OFF)
    m.fit(xs, y)
    _refits_with(m, 6, 9, "9 blocks > 8")


def test_a_tpls_keeps_its_value_and_its_reports():
    """The tPLS paths of get_q2y: the report strings below are the ones validate.py has always written."""
    x, y = L.case_data((12, 5, 7), 3, 4, 0.3, 14)
    ref = L.loo_literal(x, y, 2)
    want = C.q2y(ref["pred"], y)
    m = tPLS(2, dtype="float64", options=OFF)
    m.fit(np.array(x), np.array(y))
    q = get_q2y(m)
    rep = m.q2y_report_
    assert set(rep) == {"form", "folds", "n_iter_total"} and rep["folds"] == 12
    assert rep["form"] == "all folds in one launch, a workgroup per fold, vectors in LDS (cmtfpls_loo_tpls_f64)"
    assert abs(q - want) <= 1e-8 and C.normwise(loo_predictions(m), ref["pred"]) <= 1e-8
    q_refit = get_q2y(m, device_folds=False)
    assert m.q2y_report_ == {"form": "one refit per fold on the regular engine", "folds": 12, "why": "device folds switched off"}
    assert abs(q_refit - want) <= 1e-8
    xl, yl = L.case_data((6, 65, 66), 2, 5, 0.3, 284)                               # beyond the LDS form: the xcov kernel
    big = tPLS(2, dtype="float64", options=OFF)
    big.fit(np.array(xl), np.array(yl))
    qb = get_q2y(big)
    assert big.q2y_report_["form"] == "a workgroup per fold on the fold's cross-covariance (cmtfpls_loo_xcov_f64)"
    assert set(big.q2y_report_) == {"form", "folds", "n_iter_total"} and big.q2y_report_["folds"] == 6
    assert np.isfinite(qb)
