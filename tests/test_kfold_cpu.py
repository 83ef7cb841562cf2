"""CPU-only: K-fold cross-validation (validate.kfold_predictions / get_q2y_kfold) on the NumPy backend, i.e. the literal
refit-per-fold path: fold splitting, per-component predictions against the oracle, argument validation."""
import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import tPLS
from cmtf_pls_amd.kfold import fold_ids
from cmtf_pls_amd.validate import get_q2y_kfold, kfold_predictions
from numpy_backend import NumpyBackend


@pytest.mark.parametrize("n,k", [(10, 2), (17, 5), (30, 30), (101, 7), (64, 4)])
def test_fold_sizes_match_sklearn_kfold(n, k):
    skl = pytest.importorskip("sklearn.model_selection")
    ids, K = fold_ids(n, k)
    assert K == k
    want = np.empty(n, dtype=np.int64)
    for f, (_, test) in enumerate(skl.KFold(n_splits=k, shuffle=False).split(np.zeros((n, 1)))):
        want[test] = f
    assert np.array_equal(ids, want)


def test_fold_sizes_without_sklearn():
    ids, K = fold_ids(17, 5)
    assert K == 5 and np.bincount(ids).tolist() == [4, 4, 3, 3, 3] and np.all(np.diff(ids) >= 0)


def _literal(x, y, ids, K, R):
    pred = np.zeros((R,) + y.shape)
    for k in range(K):
        test = ids == k
        for r in range(1, R + 1):
            pred[r - 1, test] = O.predict(O.fit_tpls(x[~test], y[~test], r), x[test])
    return pred


@pytest.mark.parametrize("shape,M,R,folds", [((23, 5, 4), 2, 3, None), ((20, 6), 3, 2, None), ((18, 4, 5), 2, 2, "shuffled")])
def test_per_component_predictions_equal_the_oracle(shape, M, R, folds):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=11)
    if folds == "shuffled":
        folds = np.random.default_rng(2).permutation(np.arange(shape[0]) % 3)
        folds[:2] = 0                                       # unequal fold sizes
    m = tPLS(R, backend=NumpyBackend())
    m.fit(x, y)
    pred = kfold_predictions(m, n_splits=4, folds=folds)
    ids, K = fold_ids(shape[0], 4, folds)
    want = _literal(x, y, ids, K, R)
    assert pred.shape == (R,) + y.shape
    np.testing.assert_allclose(pred, want, rtol=1e-8, atol=1e-10)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and "K-fold kernels" in rep["why"] and rep["folds"] == K
    assert np.array(rep["n_iter"]).shape == (K, R)
    q = get_q2y_kfold(m, n_splits=4, folds=folds, per_component=True)
    q_want = 1 - ((want - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum()
    np.testing.assert_allclose(q, q_want, rtol=1e-9)
    assert get_q2y_kfold(m, n_splits=4, folds=folds) == pytest.approx(q_want[-1], rel=1e-9)


def test_argument_validation():
    x, y, _ = O.import_synthetic((12, 4, 3), 2, 2, error=0.3, seed=3)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    for kw in ({"n_splits": 1}, {"n_splits": 13}, {"folds": np.zeros(12, dtype=int)}, {"folds": np.arange(11) % 3},
               {"folds": np.r_[-1, np.arange(11) % 3]}, {"folds": np.r_[np.zeros(6, int), np.full(6, 2)]},
               {"folds": np.full(12, 0.5)}, {"folds": (np.arange(12) % 2).reshape(3, 4)}):
        with pytest.raises(ValueError):
            kfold_predictions(m, **kw)
    n = tPLS(2, backend=NumpyBackend(), copy_X=False)
    n.fit(x, y)
    with pytest.raises(AssertionError):
        get_q2y_kfold(n)
