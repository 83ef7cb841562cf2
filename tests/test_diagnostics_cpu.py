"""CPU-only: sample diagnostics (validate.sample_diagnostics) on the NumPy test backend, i.e. the torch form of the residual pass,
against a float64 NumPy restatement (tests/diagnostics_ref.py), the identities of DESIGN 8g, the limits and the argument errors."""
import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.diagnostics import spe_limit, t2_limit
from cmtf_pls_amd.validate import sample_diagnostics
from diagnostics_ref import check_against_restatement
from numpy_backend import NumpyBackend


def _data(shape, nan, seed):
    x, y, cp = O.import_synthetic(shape, 3, 3, error=0.3, seed=seed)
    if nan:
        x[np.random.default_rng(seed).random(x.shape) < nan] = np.nan
    return x, y, cp


@pytest.mark.parametrize("shape", [(30, 9), (28, 6, 5), (26, 4, 3, 5)])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("nan", [0.0, 0.1])
def test_tpls_against_restatement(shape, R, nan):
    x, y, _ = _data(shape, nan, 3)
    m = tPLS(R, backend=NumpyBackend())
    m.fit(x, y)
    d = sample_diagnostics(m)
    check_against_restatement(m, x, y, d, 1e-10, new=False)
    assert m.diagnostics_report_["form"] == "torch fallback" and m.diagnostics_report_["x_reads"] == [1]
    xn, yn, _ = _data((12,) + shape[1:], nan, 8)
    dn = sample_diagnostics(m, xn, yn)
    check_against_restatement(m, x, y, dn, 1e-10, new=True, Xn=xn, yn=yn)
    assert np.array_equal(dn["scores"], m.transform(xn))
    assert m.diagnostics_report_["training_stats"] == "cached"


@pytest.mark.parametrize("nan", [0.0, 0.1])
def test_ctpls_against_restatement(nan):
    x, y, cp = _data((30, 6, 5), nan, 4)
    xm = cp.factors[0] @ np.random.default_rng(1).normal(size=(7, 3)).T + 0.2 * np.random.default_rng(2).normal(size=(30, 7))
    m = ctPLS(3, backend=NumpyBackend())
    m.fit([x, xm], y)
    d = sample_diagnostics(m)
    check_against_restatement(m, [x, xm], y, d, 1e-10, new=False)
    for b in range(2):
        np.testing.assert_allclose(d["spe"][b].sum() / d["ssq"][b].sum(), 1 - m.R2Xs[b][-1], rtol=1e-10)
    xn = x[:10] + 0.1
    dn = sample_diagnostics(m, [xn, xm[:10] - 0.1], y[:10])
    check_against_restatement(m, [x, xm], y, dn, 1e-10, new=True, Xn=[xn, xm[:10] - 0.1], yn=y[:10])
    assert len(m.diagnostics_report_["x_reads"]) == 2


@pytest.mark.parametrize("nan", [0.0, 0.1])
def test_identities_on_training_rows(nan):
    x, y, _ = _data((35, 7, 6), nan, 5)
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    d = sample_diagnostics(m)
    ratio = d["spe"].sum() / d["ssq"].sum()
    np.testing.assert_allclose(ratio, 1 - m.R2X[-1], rtol=1e-10)
    np.testing.assert_allclose(ratio, 1 - m.R2X_literal(x), rtol=1e-10)
    np.testing.assert_allclose(d["t2"].sum(), 3 * 34, rtol=1e-10)
    again = sample_diagnostics(m, x)            # the training rows diagnosed as new data: projected, not fitted, scores
    np.testing.assert_allclose(again["scores"], d["scores"], rtol=1e-9, atol=1e-12 * np.abs(d["scores"]).max())
    np.testing.assert_allclose(again["spe"], d["spe"], rtol=1e-8)


def test_cache_dropped_by_refit_and_copy_x_false():
    x, y, _ = _data((30, 6, 5), 0.0, 6)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    sample_diagnostics(m, x[:5])
    assert m.diagnostics_report_["training_stats"] == "computed" and m.diagnostics_report_["x_reads"] == [3]
    sample_diagnostics(m, x[:5])
    assert m.diagnostics_report_["training_stats"] == "cached" and m.diagnostics_report_["x_reads"] == [2]
    m.fit(x[:25], y[:25])
    sample_diagnostics(m, x[:5])
    assert m.diagnostics_report_["training_stats"] == "computed"
    import torch
    k = tPLS(2, backend=NumpyBackend(), copy_X=False)
    k.fit(torch.from_numpy(x.copy()), y)
    with pytest.raises(ValueError, match="copy_X=False"):
        sample_diagnostics(k)
    d = sample_diagnostics(k, x[:5])
    assert np.isnan(d["spe_limit"]) and "copy_X=False" in k.diagnostics_report_["spe_limit_why"]
    assert np.isfinite(d["t2_limit"])


def test_limits_against_scipy_and_nan_cases():
    from scipy import stats

    I, R, lv = 40, 3, 0.9
    assert t2_limit(I, R, lv, True)[0] == pytest.approx((I - 1) ** 2 / I * stats.beta.ppf(lv, R / 2, (I - R - 1) / 2), rel=1e-14)
    assert t2_limit(I, R, lv, False)[0] == pytest.approx(R * (I - 1) * (I + 1) / (I * (I - R)) * stats.f.ppf(lv, R, I - R), rel=1e-14)
    m, v = 2.0, 0.5
    assert spe_limit(m, v, I, R, lv)[0] == pytest.approx(v / (2 * m) * stats.chi2.ppf(lv, 2 * m * m / v), rel=1e-14)
    assert np.isnan(t2_limit(4, 3, lv, True)[0]) and t2_limit(4, 3, lv, True)[1]
    assert np.isnan(spe_limit(m, 0.0, I, R, lv)[0]) and "v = 0" in spe_limit(m, 0.0, I, R, lv)[1]
    x, y, _ = _data((5, 4, 3), 0.0, 7)
    k = tPLS(4, backend=NumpyBackend())
    k.fit(x, y)
    d = sample_diagnostics(k)
    assert np.isnan(d["t2_limit"]) and np.isnan(d["spe_limit"]) and k.diagnostics_report_["t2_limit_why"]


def test_argument_errors():
    x, y, _ = _data((20, 5, 4), 0.0, 9)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    for lv in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="level"):
            sample_diagnostics(m, level=lv)
    with pytest.raises(ValueError, match=r"Training X has shape \(20, 5, 4\), while the new X has shape \(3, 4, 5\)"):
        sample_diagnostics(m, np.zeros((3, 4, 5)))
    with pytest.raises(ValueError, match="fitted"):
        sample_diagnostics(tPLS(2, backend=NumpyBackend()))
