"""CPU-only: the bootstrap of the factors (validate.bootstrap_factors) on the NumPy backend, i.e. the refit path: the default draws,
argument validation, the alignment rule, the spread of the stacks and every resample against literal oracle fits."""
import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.bootstrap import align_factors, model_factors
from cmtf_pls_amd.validate import bootstrap_factors
from numpy_backend import NumpyBackend


def _fitted(R=2, shape=(23, 5, 4), M=2, seed=11):
    x, y, _ = O.import_synthetic(shape, M, 3, error=0.3, seed=seed)
    m = tPLS(R, backend=NumpyBackend())
    m.fit(x, y)
    return m, x, y


def _colwise(a, b):
    """max over columns of |a - b| / |b|, columns on the last axis but one (dim x R per model)."""
    return float((np.linalg.norm(a - b, axis=-2) / np.maximum(np.linalg.norm(b, axis=-2), 1e-300)).max())


@pytest.mark.parametrize("B,seed", [(5, 0), (3, 17)])
def test_default_draws_are_one_default_rng_call(B, seed):
    m, x, y = _fitted()
    res = bootstrap_factors(m, n_resamples=B, random_state=seed)
    assert np.array_equal(res["resamples"], np.random.default_rng(seed).integers(0, 23, (B, 23)))
    rep = m.bootstrap_report_
    assert rep["resamples"] == B and rep["passes"] == 0 and rep["x_reads"] is None and "why" in rep and len(rep["n_iter"]) == B


@pytest.mark.parametrize("kwargs,msg", [
    ({"n_resamples": 1}, "at least 2"),
    ({"resamples": np.zeros((1, 23), dtype=int)}, "at least two"),
    ({"resamples": np.zeros((3, 22), dtype=int)}, "shape"),
    ({"resamples": np.zeros(23, dtype=int)}, "shape"),
    ({"resamples": np.full((3, 23), 23)}, "out of range"),
    ({"resamples": np.full((3, 23), -1)}, "out of range"),
    ({"resamples": np.zeros((3, 23))}, "integer"),
    ({"level": 0.0}, "level"),
    ({"level": 1.0}, "level"),
    ({"level": 1.5}, "level"),
])
def test_argument_errors(kwargs, msg):
    m, _, _ = _fitted()
    with pytest.raises(ValueError, match=msg):
        bootstrap_factors(m, **kwargs)


def test_alignment_flips_signs_and_leaves_predict_unchanged():
    m, x, y = _fitted(R=3)
    idx = np.random.default_rng(4).integers(0, 23, 23)
    r = tPLS(3, backend=NumpyBackend())
    r.fit(x[idx], y[idx])
    blocks, Q, coef = model_factors(r)
    ref = [[L * np.array([-1.0, 1.0, 1.0]) for L in blocks[0][:1]] + [L * np.array([1.0, -1.0, 1.0]) for L in blocks[0][1:]]]
    (al,), Qa, ca = align_factors(ref, blocks, Q, coef)
    d = np.array([-1.0, -1.0, 1.0])                                   # product of the two modes' flips per component
    assert np.array_equal(al[0], blocks[0][0] * [-1.0, 1.0, 1.0]) and np.array_equal(al[1], blocks[0][1] * [1.0, -1.0, 1.0])
    assert np.array_equal(Qa, Q * d) and np.array_equal(ca, coef * np.outer(d, d))
    np.testing.assert_allclose((r.transform(x) * d) @ ca @ Qa.T + r.Y_mean, r.predict(x), rtol=1e-12, atol=1e-12)
    (same,), Qs, cs = align_factors(blocks, blocks, Q, coef)           # aligned to itself: unchanged
    assert all(np.array_equal(a, b) for a, b in zip(same, blocks[0])) and np.array_equal(Qs, Q) and np.array_equal(cs, coef)


def test_zero_inner_product_counts_as_plus_one():
    L = np.array([[1.0, 0.0], [0.0, 1.0]])
    ref = [[np.array([[0.0, 0.0], [1.0, -1.0]])]]                     # column 0 orthogonal to L's, column 1 opposite
    (al,), Qa, ca = align_factors(ref, [[L]], np.ones((3, 2)), np.eye(2))
    assert np.array_equal(al[0], L * [1.0, -1.0]) and np.array_equal(Qa, np.ones((3, 2)) * [1.0, -1.0])


@pytest.mark.parametrize("level", [0.95, 0.5])
def test_se_and_ci_are_numpy_std_and_percentile(level):
    m, _, _ = _fitted()
    res = bootstrap_factors(m, n_resamples=6, random_state=3, level=level)
    lo, hi = 100 * (1 - level) / 2, 100 * (1 + level) / 2
    for key in ("Y_loadings", "coef"):
        assert np.array_equal(res["se"][key], res[key].std(axis=0, ddof=1))
        assert np.array_equal(res["ci"][key], np.percentile(res[key], [lo, hi], axis=0))
    for j, st in enumerate(res["X_factors"]):
        assert np.array_equal(res["se"]["X_factors"][j], st.std(axis=0, ddof=1))
        assert np.array_equal(res["ci"]["X_factors"][j], np.percentile(st, [lo, hi], axis=0))
        assert res["ci"]["X_factors"][j].shape == (2,) + st.shape[1:]


def _oracle_aligned(ref_blocks, f):
    return align_factors(ref_blocks, [list(b) for b in f.loadings], f.Q, f.coef)


@pytest.mark.parametrize("coupled", [False, True])
def test_refit_path_matches_oracle_fits(coupled):
    m, x, y = _fitted(R=2)
    R, I, B = 2, 23, 4
    if coupled:
        xm = np.random.default_rng(3).standard_normal((I, 6)) + x[:, :, 0] @ np.ones((5, 6)) * 0.1
        m = ctPLS(R, backend=NumpyBackend())
        m.fit([x, xm], y)
    res = bootstrap_factors(m, n_resamples=B, random_state=9)
    ref, _, _ = model_factors(m)
    num = np.zeros((R, I, y.shape[1]))
    seen = np.zeros(I)
    for b, idx in enumerate(res["resamples"]):
        f = O.fit_ctpls([x[idx], xm[idx]], y[idx], R) if coupled else O.fit_tpls(x[idx], y[idx], R)
        blocks, Q, coef = _oracle_aligned(ref, f)
        got = res["X_factors"] if coupled else [res["X_factors"]]
        for bi, modes in enumerate(blocks):
            for j, L in enumerate(modes):
                assert _colwise(got[bi][j][b], L) <= 1e-8, (b, bi, j)
        assert _colwise(res["Y_loadings"][b], Q) <= 1e-8 and np.abs(res["coef"][b] - coef).max() <= 1e-8 * np.abs(coef).max()
        oob = np.setdiff1d(np.arange(I), idx)
        for r in range(1, R + 1):
            g = O.fit_ctpls([x[idx], xm[idx]], y[idx], r) if coupled else O.fit_tpls(x[idx], y[idx], r)
            num[r - 1, oob] += O.predict(g, [x[oob], xm[oob]] if coupled else x[oob])
        seen[oob] += 1
    rows = seen > 0
    pred = num[:, rows] / seen[rows][None, :, None]
    want = 1 - ((pred - y[rows]) ** 2).reshape(R, -1).sum(axis=1) / (y[rows] ** 2).sum()
    assert res["oob_rows"] == int(rows.sum())
    np.testing.assert_allclose(res["oob_q2y"], want, rtol=0, atol=1e-9)
    rep = m.bootstrap_report_
    assert rep["form"] == "one refit per resample on the regular engine" and "K-fold kernels" in rep["why"]
