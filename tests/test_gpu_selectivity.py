"""Variable importance on the device (validate.selectivity_ratio / vip_scores, cmtf_pls_amd/importance.py): the estimator on the
HIP backend against the float64 NumPy restatement (tests/selectivity_ref.py) evaluated on the GPU-fitted model's own factors, for
training rows and new rows, with and without missing values, a tPLS of order 3 and 4 and a ctPLS; its report; device=False against
device=True within the kernel's tolerances; the VIP identities on the GPU model.

Tolerances: explained and residual |got - want| <= rtol s_c with the project's estimator rtol (1e-9 for float64 storage, 1e-5 for
float32), scaled by the column's sum of squares because sr amplifies error where the residual is small; sr_mode to the same rtol."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.validate import selectivity_ratio, vip_scores
from selectivity_ref import check, selectivity, vip

pytestmark = pytest.mark.gpu

KERNEL = "selectivity pass (cmtfpls_selectivity_cols)"


def _fit(shape, dtype, nan, coupled, seed=1):
    x, y, cp = O.import_synthetic(shape, 2, 3, error=0.2, seed=seed)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)
    if nan:
        x[np.random.default_rng(seed).random(x.shape) < nan] = np.nan
    if not coupled:
        m = tPLS(3, dtype=dtype)
        m.fit(x, y)
        return m, x
    xm = cp.factors[0] @ np.random.default_rng(seed + 1).normal(size=(7, 3)).T + 0.1 * np.random.default_rng(seed + 2).normal(size=(shape[0], 7))
    if dtype == "float32":
        xm = xm.astype(np.float32).astype(np.float64)
    if nan:
        xm[np.random.default_rng(seed + 3).random(xm.shape) < nan] = np.nan
    m = ctPLS(3, dtype=dtype)
    m.fit([x, xm], y)
    return m, [x, xm]


@pytest.mark.parametrize("dtype,rtol", [("float64", 1e-9), ("float32", 1e-5)])
@pytest.mark.parametrize("shape,nan,coupled", [
    ((40, 6, 5), 0.0, False),
    ((40, 6, 5), 0.1, False),
    ((64, 5, 4, 3), 0.0, False),
    ((64, 5, 4, 3), 0.1, False),
    ((40, 6, 5), 0.0, True),
    ((40, 6, 5), 0.1, True),
])
def test_estimator_against_restatement(dtype, rtol, shape, nan, coupled):
    m, X = _fit(shape, dtype, nan, coupled)
    nb = 2 if coupled else 1
    assert m.Y_factors[1].shape[0] == 2                     # M = 2
    g = selectivity_ratio(m)
    rep = m.importance_report_
    assert rep["form"] == [KERNEL] * nb and rep["why"] is None and rep["x_reads"] == [1] * nb, rep
    assert rep["masked"] == ["masked" if nan else "complete"] * nb and rep["projection"] is None, rep
    check(g, selectivity(m, train=X), coupled, rtol)
    # new rows
    xn = O.import_synthetic((shape[0] // 2,) + shape[1:], 2, 3, error=0.2, seed=9)[0]
    if dtype == "float32":
        xn = xn.astype(np.float32).astype(np.float64)
    if nan:
        xn[np.random.default_rng(5).random(xn.shape) < nan] = np.nan
    Xn = [xn, X[1][: xn.shape[0]] + 0.05] if coupled else xn
    gn = selectivity_ratio(m, Xn)
    rep = m.importance_report_
    assert rep["form"] == [KERNEL] * nb and rep["training_rows"] == shape[0] and rep["rows"] == xn.shape[0], rep
    if not nan:
        assert rep["x_reads"] == [2] * nb and rep["masked"] == ["complete"] * nb, rep
    else:
        assert rep["masked"] == ["masked"] * nb, rep
    check(gn, selectivity(m, Xn), coupled, rtol)
    # the torch form of the same call: the kernel's tolerances (sums of squares rtol 1e-11 of s_c; a cancels: estimator bound)
    gt = selectivity_ratio(m, Xn, device=False)
    rep = m.importance_report_
    assert rep["form"] == ["torch fallback"] * nb and "switched off" in rep["why"], rep
    lst = (lambda v: v) if coupled else (lambda v: [v])
    want = selectivity(m, Xn)
    for b in range(nb):
        s = lst(want["s"])[b]
        np.testing.assert_array_equal(lst(gn["n_observed"])[b], lst(gt["n_observed"])[b])
        for key in ("explained", "residual"):
            a, t = lst(gn[key])[b], lst(gt[key])[b]
            assert np.array_equal(np.isnan(a), np.isnan(t))
            assert (np.abs(np.nan_to_num(a - t)) <= 1e-11 * s + 1e-300).all(), key


def test_cells_false_and_read_only_device_tensor():
    x, y, _ = O.import_synthetic((300, 16, 12), 2, 3, error=0.2, seed=4)
    xd = torch.from_numpy(x).float().cuda()
    m = tPLS(4, dtype="float32")
    m.fit(xd, y)
    before = xd.clone()
    g = selectivity_ratio(m, cells=False)
    assert sorted(g) == ["f_limit", "level", "n_observed", "sr_mode"] and torch.equal(xd, before)
    assert [a.shape for a in g["sr_mode"]] == [(2, 16), (2, 12)] and m.importance_report_["x_reads"] == [1]
    full = selectivity_ratio(m)
    assert full["sr"].shape == (2, 16, 12) and all(np.array_equal(a, b) for a, b in zip(full["sr_mode"], g["sr_mode"]))


@pytest.mark.parametrize("coupled", [False, True])
def test_vip_identities_on_the_gpu_model(coupled):
    m, _ = _fit((40, 6, 5), "float64", 0.0, coupled)
    v = vip_scores(m, per_component=True)
    want, w = vip(m, per_component=True)
    np.testing.assert_allclose(v["component_weights"], w, rtol=0, atol=0)
    blocks = v["vip"] if coupled else [v["vip"]]
    for got_b, want_b in zip(blocks, want if coupled else [want]):
        for a, b in zip(got_b, want_b):
            assert a.shape == b.shape == (3, a.shape[1])
            np.testing.assert_allclose(a, b, rtol=1e-12)
            np.testing.assert_allclose((a * a).sum(axis=1), a.shape[1], rtol=1e-12)
    last = vip_scores(m)["vip"]
    for a, b in zip(last if not coupled else last[0], blocks[0]):
        np.testing.assert_array_equal(a, b[-1])
