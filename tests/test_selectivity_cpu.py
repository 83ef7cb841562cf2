"""CPU-only: variable importance (validate.selectivity_ratio, validate.vip_scores) on the NumPy test backend, i.e. the torch form
of the target-projection pass, against a float64 NumPy restatement (tests/selectivity_ref.py); the identities of DESIGN 8q, the
edge cases (a column without observations, a constant response), a planted case, cells=False, per_component, clipped increments
and the argument errors."""
import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.validate import sample_diagnostics, selectivity_ratio, vip_scores
from numpy_backend import NumpyBackend
from selectivity_ref import check, f_limit, selectivity, vip

RTOL = 1e-10


def _data(shape, nan, seed):
    x, y, cp = O.import_synthetic(shape, 3, 3, error=0.3, seed=seed)
    if nan:
        x[np.random.default_rng(seed).random(x.shape) < nan] = np.nan
    return x, y, cp


def _coupled(nan, seed=4):
    x, y, cp = _data((30, 6, 5), nan, seed)
    xm = cp.factors[0] @ np.random.default_rng(1).normal(size=(7, 3)).T + 0.2 * np.random.default_rng(2).normal(size=(30, 7))
    if nan:
        xm[np.random.default_rng(seed + 1).random(xm.shape) < nan] = np.nan
    m = ctPLS(3, backend=NumpyBackend())
    m.fit([x, xm], y)
    return m, [x, xm], y


@pytest.mark.parametrize("shape,nan", [((30, 9), 0.0), ((30, 9), 0.15), ((28, 6, 5), 0.0), ((28, 6, 5), 0.15),
                                       ((26, 4, 3, 5), 0.0), ((26, 4, 3, 5), 0.15)])
def test_tpls_against_restatement(shape, nan):
    x, y, _ = _data(shape, nan, 3)
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    g = selectivity_ratio(m)
    check(g, selectivity(m, train=x), False, RTOL)
    rep = m.importance_report_
    assert rep["form"] == ["torch fallback"] and "no selectivity_cols kernel" in rep["why"] and rep["x_reads"] == [1], rep
    assert rep["masked"] == ["masked" if nan else "complete"] and rep["rows"] == shape[0] and rep["projection"] is None, rep
    M = y.shape[1]
    assert g["sr"].shape == (M,) + shape[1:] and g["n_observed"].shape == shape[1:] and g["level"] == 0.95
    assert [a.shape for a in g["sr_mode"]] == [(M, d) for d in shape[1:]]
    assert (g["residual"][~np.isnan(g["residual"])] >= 0).all()
    xn, _, _ = _data((12,) + shape[1:], nan, 8)
    gn = selectivity_ratio(m, xn, level=0.9)
    check(gn, selectivity(m, xn, level=0.9), False, RTOL)
    rep = m.importance_report_
    assert rep["training_rows"] == shape[0] and rep["rows"] == 12 and rep["projection"], rep
    assert gn["f_limit"] == f_limit(shape[0], 0.9)
    if not nan:
        assert rep["x_reads"] == [2] and rep["masked"] == ["complete"], rep


@pytest.mark.parametrize("nan", [0.0, 0.15])
def test_ctpls_against_restatement(nan):
    m, Xs, y = _coupled(nan)
    g = selectivity_ratio(m)
    check(g, selectivity(m, train=Xs), True, RTOL)
    assert len(g["sr"]) == 2 and g["sr"][0].shape == (3, 6, 5) and g["sr"][1].shape == (3, 7)
    assert len(g["sr_mode"][0]) == 2 and len(g["sr_mode"][1]) == 1 and m.importance_report_["x_reads"] == [1, 1]
    Xn = [Xs[0][:10] + 0.1, Xs[1][:10] - 0.1]
    check(selectivity_ratio(m, Xn), selectivity(m, Xn), True, RTOL)


@pytest.mark.parametrize("shape,coupled", [((30, 9), False), ((28, 6, 5), False), ((26, 4, 3, 5), False), ((30, 6, 5), True)])
def test_explained_and_residual_close_to_the_total_sum_of_squares(shape, coupled):
    """Complete data: for every response, sum_c explained + sum_c residual = sum_c s_c = the total ssq of sample_diagnostics."""
    if coupled:
        m, X, _ = _coupled(0.0)
    else:
        X, y, _ = _data(shape, 0.0, 5)
        m = tPLS(3, backend=NumpyBackend())
        m.fit(X, y)
    g, diag = selectivity_ratio(m), sample_diagnostics(m)
    lst = (lambda v: v) if coupled else (lambda v: [v])
    for ex, rs, ssq in zip(lst(g["explained"]), lst(g["residual"]), lst(diag["ssq"])):
        M = ex.shape[0]
        assert (rs >= 0).all()
        np.testing.assert_allclose(ex.reshape(M, -1).sum(axis=1) + rs.reshape(M, -1).sum(axis=1), ssq.sum(), rtol=1e-10)


@pytest.mark.parametrize("coupled", [False, True])
def test_vip_identity_per_component_and_restatement(coupled):
    if coupled:
        m, _, _ = _coupled(0.1)
    else:
        x, y, _ = _data((28, 6, 5), 0.0, 3)
        m = tPLS(3, backend=NumpyBackend())
        m.fit(x, y)
    v, vp = vip_scores(m), vip_scores(m, per_component=True)
    want, w = vip(m, per_component=True)
    np.testing.assert_allclose(v["component_weights"], w, rtol=0, atol=0)
    assert v["why"] is None and m.vip_report_["per_component"] is True
    lst = (lambda t: t) if coupled else (lambda t: [t])
    for last_b, all_b, want_b in zip(lst(v["vip"]), lst(vp["vip"]), lst(want)):
        for last, every, ref in zip(last_b, all_b, want_b):
            J = last.shape[0]
            assert every.shape == (3, J)
            np.testing.assert_allclose((last * last).sum(), J, rtol=1e-12)                    # sum_j vip^2 = J_k
            np.testing.assert_allclose((every * every).sum(axis=1), J, rtol=1e-12)            # ... for every prefix
            np.testing.assert_array_equal(every[-1], last)
            np.testing.assert_allclose(every, ref, rtol=1e-12)


def test_clipped_increments_and_no_explained_response():
    x, y, _ = _data((28, 6, 5), 0.0, 3)
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    m.R2Y = np.array([0.5, 0.4, 0.7])                        # a decreasing step: clipped to 0, and listed
    v = vip_scores(m, per_component=True)
    assert v["clipped"] == [{"component": 1, "increment": pytest.approx(-0.1)}] and m.vip_report_["clipped"] == v["clipped"]
    np.testing.assert_allclose(v["component_weights"], [0.5, 0.0, 0.3])
    np.testing.assert_array_equal(v["vip"][0][0], v["vip"][0][1])                              # a zero weight adds nothing
    np.testing.assert_allclose(v["vip"][0], vip(m, per_component=True)[0][0], rtol=1e-12)
    m.R2Y = np.array([0.0, -0.1, -0.2])
    v = vip_scores(m)
    assert v["why"] and "R2Y" in v["why"] and all(np.isnan(a).all() for a in v["vip"]) and len(v["clipped"]) == 2


def test_column_without_observations_and_constant_response():
    x, y, _ = _data((28, 6, 5), 0.1, 3)
    x[:, 2, 3] = np.nan                                       # a column nobody observed
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    g = selectivity_ratio(m)
    check(g, selectivity(m, train=x), False, RTOL)
    assert g["n_observed"][2, 3] == 0
    for key in ("sr", "explained", "residual", "tp_loading"):
        assert np.isnan(g[key][:, 2, 3]).all() and not np.isnan(g[key][:, 0, 0]).any(), key
    assert not np.isnan(g["sr_mode"][0]).any() and not np.isnan(g["sr_mode"][1]).any()        # NaN cells are skipped
    # a constant response: Y_mean takes it, its column of Q is zero, so is its column of tau
    x2, y2, _ = _data((28, 6, 5), 0.0, 3)
    y2 = y2.copy()
    y2[:, 1] = 4.0
    k = tPLS(2, backend=NumpyBackend())
    k.fit(x2, y2)
    g = selectivity_ratio(k)
    assert np.isnan(g["sr"][1]).all() and np.isnan(g["sr_mode"][0][1]).all() and np.isnan(g["sr_mode"][1][1]).all()
    assert not np.isnan(g["sr"][0]).any()
    check(g, selectivity(k, train=x2), False, RTOL)


def _planted():
    """X = y (x) a (x) b + noise with a zero on half of its entries: mode 1 slices on the support of a predict y, the others are
    noise.  Sizes, seed and noise chosen so that the float64 restatement itself separates the two groups with room (asserted)."""
    rng = np.random.default_rng(12)
    I, J, K = 60, 8, 5
    yv = rng.normal(size=I)
    a = np.array([1.0, 0.0, 1.2, 0.0, 0.8, 0.0, 1.1, 0.0])
    b = np.array([1.0, 0.9, 1.1, 1.2, 0.8])
    x = np.einsum("i,j,k->ijk", yv, a, b) + 0.3 * rng.normal(size=(I, J, K))
    return x, yv.reshape(-1, 1) + 0.05 * rng.normal(size=(I, 1)), a != 0


def test_planted_support_is_above_the_limit_and_the_rest_below():
    x, y, on = _planted()
    m = tPLS(1, backend=NumpyBackend())
    m.fit(x, y)
    ref = selectivity(m, train=x)
    lim = ref["f_limit"]
    assert ref["sr_mode"][0][0][on].min() > 3 * lim and ref["sr_mode"][0][0][~on].max() < lim / 3      # the restatement, with room
    g = selectivity_ratio(m)
    assert g["f_limit"] == lim == f_limit(60)
    assert (g["sr_mode"][0][0][on] > lim).all() and (g["sr_mode"][0][0][~on] < lim).all()
    assert (g["sr"][0][on] > lim).all() and (g["sr"][0][~on] < lim).mean() > 0.9
    v = vip_scores(m)["vip"][0]
    assert v[on].min() > 1.0 > v[~on].max()


def test_cells_false_levels_and_limit_without_enough_rows():
    x, y, _ = _data((28, 6, 5), 0.1, 3)
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    full, lean = selectivity_ratio(m), selectivity_ratio(m, cells=False)
    assert sorted(lean) == ["f_limit", "level", "n_observed", "sr_mode"]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(full["sr_mode"], lean["sr_mode"]))
    assert m.importance_report_["f_limit_nominal"] is True and m.importance_report_["f_limit_why"] is None
    xs, ys, _ = _data((3, 6, 5), 0.0, 3)
    k = tPLS(1, backend=NumpyBackend())
    k.fit(xs, ys)
    g = selectivity_ratio(k)
    assert np.isnan(g["f_limit"]) and "3" in k.importance_report_["f_limit_why"]


def test_argument_errors():
    import torch

    x, y, _ = _data((20, 5, 4), 0.0, 9)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    with pytest.raises(ValueError, match=r"Training X has shape \(20, 5, 4\), while the new X has shape \(3, 4, 5\)"):
        selectivity_ratio(m, np.zeros((3, 4, 5)))
    for bad in (0.0, 1.0, -1, 2):
        with pytest.raises(ValueError, match="level"):
            selectivity_ratio(m, level=bad)
    with pytest.raises(ValueError, match="fitted"):
        selectivity_ratio(tPLS(2, backend=NumpyBackend()))
    with pytest.raises(ValueError, match="fitted"):
        vip_scores(tPLS(2, backend=NumpyBackend()))
    k = tPLS(2, backend=NumpyBackend(), copy_X=False)
    k.fit(torch.from_numpy(x.copy()), y)
    with pytest.raises(ValueError, match="copy_X=False"):
        selectivity_ratio(k)
    assert selectivity_ratio(k, x[:6])["sr"].shape == (3, 5, 4)
    mc, Xs, _ = _coupled(0.0)
    with pytest.raises(ValueError, match="2 blocks, while the new Xs has 1"):
        selectivity_ratio(mc, [Xs[0]])
    with pytest.raises(ValueError, match="shape"):
        selectivity_ratio(mc, [Xs[0], Xs[1][:, :5]])
