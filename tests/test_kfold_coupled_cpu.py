"""CPU-only: K-fold cross-validation of a coupled model (validate.kfold_predictions / get_q2y_kfold on a ctPLS) on the NumPy
backend, i.e. the literal refit-per-fold path: per-component predictions against the oracle, the training data the estimator
keeps, argument validation."""
import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import ctPLS
from cmtf_pls_amd.kfold import fold_ids
from cmtf_pls_amd.validate import get_q2y_kfold, kfold_predictions
from numpy_backend import NumpyBackend


def _coupled_data(shapes, M, L, seed):
    """Blocks with the given shapes (rows first, shared) driven by one latent score, and a Y of M responses."""
    rng = np.random.default_rng(seed)
    I = shapes[0][0]
    T = rng.standard_normal((I, L))
    Xs = []
    for shape in shapes:
        X = O.cp_factors_to_tensor([T] + [rng.standard_normal((d, L)) for d in shape[1:]])
        Xs.append(X + 0.3 * rng.standard_normal(shape))
    Y = T @ rng.standard_normal((L, M)) + 0.3 * rng.standard_normal((I, M))
    return Xs, Y


def _literal(Xs, y, ids, K, R):
    pred = np.zeros((R,) + y.shape)
    for k in range(K):
        test = ids == k
        for r in range(1, R + 1):
            fit = O.fit_ctpls([X[~test] for X in Xs], y[~test], r)
            pred[r - 1, test] = O.predict(fit, [X[test] for X in Xs]).reshape((int(test.sum()),) + y.shape[1:])
    return pred


@pytest.mark.parametrize("shapes,M,R,folds", [
    ([(23, 5, 4), (23, 7)], 2, 3, None),                    # tensor + matrix
    ([(21, 6), (21, 4, 3)], 3, 2, None),                    # matrix + tensor
    ([(20, 4, 5), (20, 6), (20, 3, 3)], 2, 2, "shuffled"),  # three blocks, shuffled unequal folds
])
def test_per_component_predictions_equal_the_oracle(shapes, M, R, folds):
    Xs, y = _coupled_data(shapes, M, R + 1, seed=11)
    I = shapes[0][0]
    if folds == "shuffled":
        folds = np.random.default_rng(2).permutation(np.arange(I) % 3)
        folds[:3] = 0                                       # unequal fold sizes
    m = ctPLS(R, backend=NumpyBackend())
    m.fit(Xs, y)
    pred = kfold_predictions(m, n_splits=4, folds=folds)
    ids, K = fold_ids(I, 4, folds)
    want = _literal(Xs, y, ids, K, R)
    assert pred.shape == (R,) + y.shape
    np.testing.assert_allclose(pred, want, rtol=1e-8, atol=1e-10)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and "K-fold kernels" in rep["why"] and rep["folds"] == K
    assert rep["x_reads"] is None and np.array(rep["n_iter"]).shape == (K, R)
    q = get_q2y_kfold(m, n_splits=4, folds=folds, per_component=True)
    q_want = 1 - ((want - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum()
    np.testing.assert_allclose(q, q_want, rtol=1e-9)
    assert get_q2y_kfold(m, n_splits=4, folds=folds) == pytest.approx(q_want[-1], rel=1e-9)


def test_one_response_vector_y():
    Xs, y = _coupled_data([(18, 4, 3), (18, 5)], 1, 2, seed=5)
    y = y[:, 0]
    m = ctPLS(2, backend=NumpyBackend())
    m.fit(Xs, y)
    pred = kfold_predictions(m, n_splits=3)
    ids, K = fold_ids(18, 3)
    want = _literal(Xs, y.reshape(-1, 1), ids, K, 2).reshape(pred.shape)
    assert pred.shape == (2, 18)
    np.testing.assert_allclose(pred, want, rtol=1e-8, atol=1e-10)


def test_training_data_is_kept_by_reference():
    Xs, y = _coupled_data([(12, 4, 3), (12, 5)], 2, 2, seed=3)
    m = ctPLS(2, backend=NumpyBackend())
    m.fit(Xs, y)
    assert m.original_Xs is Xs and m.original_Y is y
    assert all(a is b for a, b in zip(m.original_Xs, Xs))
    n = ctPLS(2, backend=NumpyBackend(), copy_X=False)
    n.fit([X.copy() for X in Xs], y)
    assert n.original_Xs is None and n.original_Y is None
    with pytest.raises(AssertionError):
        get_q2y_kfold(n)
    with pytest.raises(AssertionError):
        kfold_predictions(n)


def test_fit_outputs_unchanged_by_the_kept_data():
    Xs, y = _coupled_data([(16, 4, 3), (16, 5)], 2, 2, seed=4)
    ref = O.fit_ctpls(Xs, y, 2)
    m = ctPLS(2, backend=NumpyBackend())
    m.fit(Xs, y)
    np.testing.assert_allclose(m.predict(Xs), O.predict(ref, Xs), rtol=1e-8, atol=1e-10)


def test_argument_validation():
    Xs, y = _coupled_data([(12, 4, 3), (12, 5)], 2, 2, seed=3)
    m = ctPLS(2, backend=NumpyBackend())
    m.fit(Xs, y)
    for kw in ({"n_splits": 1}, {"n_splits": 13}, {"folds": np.zeros(12, dtype=int)}, {"folds": np.arange(11) % 3},
               {"folds": np.r_[-1, np.arange(11) % 3]}, {"folds": np.r_[np.zeros(6, int), np.full(6, 2)]},
               {"folds": np.full(12, 0.5)}, {"folds": (np.arange(12) % 2).reshape(3, 4)}):
        with pytest.raises(ValueError):
            kfold_predictions(m, **kw)
        with pytest.raises(ValueError):
            get_q2y_kfold(m, **kw)
