"""CPU-only: the response-permutation test of K-fold Q2Y (validate.permutation_test_q2y) on the NumPy backend, i.e. the refit path:
null entries against literal per-fold oracle fits on Y[pi_p], the p-value, the permutation draws and argument validation."""
import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.kfold import fold_ids
from cmtf_pls_amd.validate import get_q2y_kfold, permutation_test_q2y
from numpy_backend import NumpyBackend


def _oracle_q2y(x, y, ids, K, R):
    """Q2Y of every component count from literal per-fold oracle fits."""
    pred = np.zeros((R,) + y.shape)
    for k in range(K):
        test = ids == k
        for r in range(1, R + 1):
            pred[r - 1, test] = O.predict(O.fit_tpls(x[~test], y[~test], r), x[test])
    return 1 - ((pred - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum()


def _model(shape=(23, 5, 4), M=2, R=2, seed=11):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=seed)
    m = tPLS(R, backend=NumpyBackend())
    m.fit(x, y)
    return m, x, y


@pytest.mark.parametrize("shape,M,R,folds", [((23, 5, 4), 2, 2, None), ((20, 6), 3, 2, None), ((18, 4, 5), 2, 2, "shuffled")])
def test_null_equals_literal_oracle_fits(shape, M, R, folds):
    m, x, y = _model(shape, M, R)
    if folds == "shuffled":
        folds = np.random.default_rng(2).permutation(np.arange(shape[0]) % 3)
        folds[:2] = 0                                            # unequal fold sizes
    res = permutation_test_q2y(m, n_permutations=4, n_splits=4, folds=folds, per_component=True)
    ids, K = fold_ids(shape[0], 4, folds)
    assert res["null"].shape == (4, R) and res["permutations"].shape == (4, shape[0])
    for p, pi in enumerate(res["permutations"]):
        np.testing.assert_allclose(res["null"][p], _oracle_q2y(x, y[pi], ids, K, R), rtol=1e-8, atol=1e-8)
    rep = m.q2y_report_
    np.testing.assert_allclose(res["q2y"], get_q2y_kfold(m, n_splits=4, folds=folds, per_component=True), rtol=0, atol=0)
    assert rep["form"].startswith("one refit per fold") and "K-fold kernels" in rep["why"]
    assert rep["permutations"] == 4 and rep["passes"] == 0 and rep["x_reads"] is None
    assert len(rep["n_iter"]) == 4 and np.array(rep["n_iter"][0]).shape == (K, R)


def test_identity_permutation_gives_the_observed_q2y():
    m, x, y = _model()
    I = y.shape[0]
    perms = np.stack([np.arange(I), np.random.default_rng(5).permutation(I)])
    res = permutation_test_q2y(m, permutations=perms)
    assert res["q2y"] == get_q2y_kfold(m)
    assert res["null"][0] == pytest.approx(res["q2y"], rel=1e-12, abs=1e-12)
    assert np.array_equal(res["permutations"], perms)


def test_p_value_formula_with_ties():
    m, x, y = _model()
    I = y.shape[0]
    rng = np.random.default_rng(8)
    perms = np.stack([np.arange(I), np.arange(I)] + [rng.permutation(I) for _ in range(5)])
    res = permutation_test_q2y(m, permutations=perms, per_component=True)
    null, q = res["null"], res["q2y"]
    np.testing.assert_array_equal(null[:2], np.broadcast_to(q, (2, q.size)))      # the identity rows tie with the observed value
    want = (1 + (null >= q).sum(axis=0)) / (perms.shape[0] + 1)
    np.testing.assert_array_equal(res["p_value"], want)
    assert np.all(res["p_value"] >= 3 / 8)                                        # ties count as >=
    last = permutation_test_q2y(m, permutations=perms)
    assert last["p_value"] == (1 + np.sum(last["null"] >= last["q2y"])) / (perms.shape[0] + 1)


def test_random_state_reproducible_and_in_order():
    m, x, y = _model()
    I = y.shape[0]
    a = permutation_test_q2y(m, n_permutations=3, random_state=7)
    b = permutation_test_q2y(m, n_permutations=3, random_state=7)
    assert np.array_equal(a["permutations"], b["permutations"])
    np.testing.assert_array_equal(a["null"], b["null"])
    rng = np.random.default_rng(7)
    assert np.array_equal(a["permutations"], np.stack([rng.permutation(I) for _ in range(3)]))
    c = permutation_test_q2y(m, n_permutations=3, random_state=8)
    assert not np.array_equal(a["permutations"], c["permutations"])


def test_shapes():
    m, x, y = _model(R=3)
    r = permutation_test_q2y(m, n_permutations=5, per_component=True)
    assert r["null"].shape == (5, 3) and r["p_value"].shape == (3,) and r["q2y"].shape == (3,)
    s = permutation_test_q2y(m, n_permutations=5)
    assert s["null"].shape == (5,) and isinstance(s["p_value"], float) and isinstance(s["q2y"], float)
    np.testing.assert_allclose(s["null"], r["null"][:, -1], rtol=0, atol=0)


def test_argument_validation():
    m, x, y = _model()
    I = y.shape[0]
    bad = [{"n_permutations": 0}, {"n_permutations": -3},
           {"permutations": np.zeros((2, I), dtype=int)},                      # not a permutation
           {"permutations": np.arange(I)},                                      # 1-d
           {"permutations": np.stack([np.arange(I - 1)])},                      # wrong length
           {"permutations": np.stack([np.arange(I) + 1])},                      # out of range
           {"permutations": np.stack([np.arange(I).astype(float)])}]            # not integers
    for kw in bad:
        with pytest.raises(ValueError):
            permutation_test_q2y(m, **kw)
    n = tPLS(2, backend=NumpyBackend(), copy_X=False)
    n.fit(x, y)
    with pytest.raises(AssertionError):
        permutation_test_q2y(n)


def test_coupled_model_refits():
    x, y, _ = O.import_synthetic((21, 5, 4), 2, 3, error=0.3, seed=13)
    xm = np.random.default_rng(3).standard_normal((21, 6)) + x[:, :, 0] @ np.ones((5, 6)) * 0.1
    m = ctPLS(2, backend=NumpyBackend())
    m.fit([x, xm], y)
    res = permutation_test_q2y(m, n_permutations=2, n_splits=3, per_component=True)
    ids, K = fold_ids(21, 3)
    for p, pi in enumerate(res["permutations"]):
        want = np.zeros((2,) + y.shape)
        for k in range(K):
            test = ids == k
            for r in (1, 2):
                fit = O.fit_ctpls([x[~test], xm[~test]], y[pi][~test], r)
                want[r - 1, test] = O.predict(fit, [x[test], xm[test]])
        q = 1 - ((want - y[pi]) ** 2).reshape(2, -1).sum(axis=1) / (y ** 2).sum()
        np.testing.assert_allclose(res["null"][p], q, rtol=1e-8, atol=1e-8)
    rep = m.q2y_report_
    assert rep["why"] == "coupled model: permutation device form not built"
    assert rep["passes"] == 0 and rep["x_reads"] is None
