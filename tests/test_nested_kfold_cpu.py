"""CPU-only: nested K-fold Q2Y (validate.get_q2y_nested_kfold) on the NumPy backend, i.e. the refit path: the splits against
sklearn's KFold, inner_q2y / outer_q2y against get_q2y_kfold and literal oracle fits, the selection and the nested estimate
recomputed from oracle fits, given splits, the report and argument validation."""
import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.nested import model_rows, nested_fold_ids
from cmtf_pls_amd.validate import get_q2y_kfold, get_q2y_nested_kfold
from numpy_backend import NumpyBackend


@pytest.mark.parametrize("I,Ko,Ki,seed", [(23, 5, 4, 7), (20, 5, 5, 0), (24, 4, 3, 11), (11, 2, 2, 3), (33, 4, 7, 9)])
def test_default_splits(I, Ko, Ki, seed):
    outer, Ko2, inner, Ki2 = nested_fold_ids(I, Ko, Ki, random_state=seed)
    assert (Ko2, Ki2) == (Ko, Ki) and outer.shape == (I,) and inner.shape == (Ko, I)
    for o in range(Ko):
        held = outer == o
        assert np.array_equal(inner[o] == -1, held)
        sizes = np.bincount(inner[o][~held], minlength=Ki)
        assert sizes.shape == (Ki,) and sizes.min() >= 1 and sizes.max() - sizes.min() <= 1, (o, sizes)
    sk = pytest.importorskip("sklearn.model_selection")
    tests = [t for _, t in sk.KFold(n_splits=Ko, shuffle=True, random_state=seed).split(np.zeros((I, 1)))]
    for o in range(Ko):
        assert np.array_equal(np.flatnonzero(outer == o), np.sort(tests[o])), o
        train = np.flatnonzero(outer != o)                       # ascending rows, split with random_state + 1 + o
        itests = [t for _, t in sk.KFold(n_splits=Ki, shuffle=True, random_state=seed + 1 + o).split(np.zeros((train.size, 1)))]
        for i in range(Ki):
            assert np.array_equal(np.flatnonzero(inner[o] == i), train[np.sort(itests[i])]), (o, i)


def test_splits_are_reproducible_and_differ_between_seeds():
    a = nested_fold_ids(30, 3, 4, random_state=5)
    b = nested_fold_ids(30, 3, 4, random_state=5)
    c = nested_fold_ids(30, 3, 4, random_state=6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[2], c[2])


def test_model_rows_partition_the_scored_rows():
    outer, Ko, inner, Ki = nested_fold_ids(26, 3, 4, random_state=1)
    counts, ev = model_rows(outer, Ko, inner, Ki)
    assert counts.shape == ev.shape == (Ko * (Ki + 1), 26)
    assert not np.any((counts > 0) & (ev > 0))                    # no model scores a row it trained on
    assert np.array_equal((ev == 2).sum(axis=0), np.ones(26))     # every row predicted by exactly one outer model
    for o in range(Ko):
        e = o * (Ki + 1)
        assert np.array_equal(ev[e + 1:e + 1 + Ki].sum(axis=0), (outer != o).astype(int))


def _fit(fit, Xs, y, r):
    return fit(Xs if len(Xs) > 1 else Xs[0], y, r)


def _oracle_pred(fit, Xs, y, train, test, R):
    """(R, n_test, M): the rows `test` predicted by literal oracle fits on the rows `train` with r = 1..R components."""
    return np.stack([O.predict(_fit(fit, [X[train] for X in Xs], y[train], r), [X[test] for X in Xs] if len(Xs) > 1 else Xs[0][test])
                     for r in range(1, R + 1)])


def _oracle_q2y(fit, Xs, y, ids, K, R):
    pred = np.zeros((R,) + y.shape)
    for k in range(K):
        pred[:, ids == k] = _oracle_pred(fit, Xs, y, ids != k, ids == k, R)
    return 1 - ((pred - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum()


def _models(coupled, R=3):
    x, y, _ = O.import_synthetic((26, 5, 4), 2, 3, error=0.3, seed=11)
    if coupled:
        xm = np.random.default_rng(3).standard_normal((26, 6)) + x[:, :, 0] @ np.ones((5, 6)) * 0.1
        return [x, xm], y, lambda: ctPLS(R, backend=NumpyBackend()), O.fit_ctpls
    return [x], y, lambda: tPLS(R, backend=NumpyBackend()), O.fit_tpls


@pytest.mark.parametrize("coupled", [False, True])
def test_inner_and_outer_q2y_equal_get_q2y_kfold_and_oracle_fits(coupled):
    R, Ko, Ki = 3, 3, 4
    Xs, y, make, fit = _models(coupled, R)
    m = make()
    m.fit(Xs if coupled else Xs[0], y)
    res = get_q2y_nested_kfold(m, n_outer=Ko, n_inner=Ki, random_state=2)
    rep = m.q2y_report_
    outer, inner = res["outer_folds"], res["inner_folds"]
    ref = nested_fold_ids(26, Ko, Ki, random_state=2)
    assert np.array_equal(outer, ref[0]) and np.array_equal(inner, ref[2])
    assert res["inner_q2y"].shape == (Ko, R) and res["outer_q2y"].shape == (R,) and res["selected"].shape == (Ko,)
    assert res["predictions"].shape == y.shape and isinstance(res["q2y"], float)
    np.testing.assert_array_equal(res["outer_q2y"], get_q2y_kfold(m, folds=outer, per_component=True))   # the same refits
    np.testing.assert_allclose(res["outer_q2y"], _oracle_q2y(fit, Xs, y, outer, Ko, R), rtol=1e-8, atol=1e-8)
    for o in range(Ko):
        tr = outer != o
        sub = make()
        sub.fit([X[tr] for X in Xs] if coupled else Xs[0][tr], y[tr])
        # the same refits, their squared errors added fold by fold instead of in one sum: < 100 terms, far inside 1e-12
        np.testing.assert_allclose(res["inner_q2y"][o], get_q2y_kfold(sub, folds=inner[o][tr], per_component=True), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(res["inner_q2y"][o], _oracle_q2y(fit, [X[tr] for X in Xs], y[tr], inner[o][tr], Ki, R),
                                   rtol=1e-8, atol=1e-8)
    assert rep["models"] == Ko * (Ki + 1) and len(rep["n_iter"]) == Ko * (Ki + 1) and np.array(rep["n_iter"]).shape == (Ko * (Ki + 1), R)


@pytest.mark.parametrize("coupled", [False, True])
def test_selection_predictions_and_q2y_from_oracle_fits(coupled):
    R, Ko, Ki = 3, 3, 4
    Xs, y, make, fit = _models(coupled, R)
    m = make()
    m.fit(Xs if coupled else Xs[0], y)
    res = get_q2y_nested_kfold(m, n_outer=Ko, n_inner=Ki, random_state=2)
    outer = res["outer_folds"]
    sel = np.argmax(res["inner_q2y"], axis=1) + 1                 # the first maximum: the smallest r on a tie
    assert np.array_equal(res["selected"], sel) and sel.min() >= 1 and sel.max() <= R
    pred = np.zeros(y.shape)
    for o in range(Ko):
        pred[outer == o] = _oracle_pred(fit, Xs, y, outer != o, outer == o, R)[sel[o] - 1]
    np.testing.assert_allclose(res["predictions"], pred, rtol=1e-8, atol=1e-8)
    assert res["q2y"] == pytest.approx(1 - ((pred - y) ** 2).sum() / (y ** 2).sum(), rel=1e-8, abs=1e-8)
    assert res["q2y"] == 1 - ((res["predictions"] - y) ** 2).sum() / (y ** 2).sum()


def test_given_folds_are_used_as_given():
    x, y, _ = O.import_synthetic((20, 6), 3, 3, error=0.3, seed=4)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    outer = np.arange(20) % 4
    inner = np.full((4, 20), -1)
    for o in range(4):
        tr = np.flatnonzero(outer != o)
        inner[o, tr] = np.random.default_rng(o).permutation(np.arange(tr.size) % 3)
    res = get_q2y_nested_kfold(m, n_outer=9, n_inner=9, outer_folds=outer, inner_folds=inner, random_state="ignored")
    assert np.array_equal(res["outer_folds"], outer) and np.array_equal(res["inner_folds"], inner)
    assert res["inner_q2y"].shape == (4, 2) and m.q2y_report_["models"] == 16
    np.testing.assert_array_equal(res["outer_q2y"], get_q2y_kfold(m, folds=outer, per_component=True))
    only_outer = get_q2y_nested_kfold(m, n_inner=3, outer_folds=outer, random_state=5)    # inner drawn per outer fold
    assert np.array_equal(only_outer["outer_folds"], outer)
    assert np.array_equal(only_outer["inner_folds"], nested_fold_ids(20, 5, 3, outer_folds=outer, random_state=5)[2])
    only_inner = get_q2y_nested_kfold(m, n_outer=4, inner_folds=nested_fold_ids(20, 4, 3, random_state=7)[2], random_state=7)
    assert np.array_equal(only_inner["outer_folds"], nested_fold_ids(20, 4, 3, random_state=7)[0])


def test_argument_validation():
    x, y, _ = O.import_synthetic((20, 5, 4), 2, 3, error=0.3, seed=8)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    outer = np.arange(20) % 4
    inner = np.stack([np.where(outer == o, -1, (np.arange(20) // 4) % 3) for o in range(4)])
    get_q2y_nested_kfold(m, outer_folds=outer, inner_folds=inner)                       # (well formed)

    def changed(o, rows, value):
        f = inner.copy()
        f[o, rows] = value
        return f
    bad = [{"random_state": None}, {"random_state": 1.0}, {"random_state": True}, {"random_state": np.random.RandomState(0)},
           {"outer_folds": outer, "random_state": None},                            # inner still drawn
           {"n_outer": 1}, {"n_outer": 21}, {"n_inner": 1}, {"n_inner": 17},            # 16 training rows per outer fold of 5
           {"outer_folds": outer[:-1]}, {"outer_folds": np.stack([outer, outer])}, {"outer_folds": outer + 0.5},
           {"outer_folds": outer - 1}, {"outer_folds": np.where(outer == 2, 3, outer)},  # fold 2 empty
           {"outer_folds": np.zeros(20, dtype=int)},                                    # one fold
           {"outer_folds": outer, "inner_folds": inner[0]},                             # 1-d
           {"outer_folds": outer, "inner_folds": inner[:3]},                            # a row per outer fold
           {"outer_folds": outer, "inner_folds": inner[:, :-1]},                        # wrong length
           {"outer_folds": outer, "inner_folds": inner + 0.5},                          # not integers
           {"outer_folds": outer, "inner_folds": changed(1, 0, -1)},                    # -1 on a training row
           {"outer_folds": outer, "inner_folds": changed(0, 0, 1)},                     # an id on a held-out row
           {"outer_folds": outer, "inner_folds": changed(2, 0, -2)},                    # negative id
           {"outer_folds": outer, "inner_folds": np.where(inner == 1, 3, inner)},       # inner fold 1 empty
           {"outer_folds": outer, "inner_folds": np.where(inner >= 0, 0, inner)},       # one inner fold
           {"outer_folds": outer, "inner_folds": changed(3, inner[3] == 2, 1)},         # K_i = 2 in row 3, 3 elsewhere
           {"inner_folds": inner}]                                                      # drawn outer folds do not match it
    for kw in bad:
        with pytest.raises(ValueError):
            get_q2y_nested_kfold(m, **kw)
    n = tPLS(2, backend=NumpyBackend())
    with pytest.raises(AssertionError):
        get_q2y_nested_kfold(n)                                                         # not fitted
    c = tPLS(2, backend=NumpyBackend(), copy_X=False)
    c.fit(x, y)
    with pytest.raises(AssertionError):
        get_q2y_nested_kfold(c)


def test_report_keys_and_why_names_the_backend():
    x, y, _ = O.import_synthetic((20, 5, 4), 2, 3, error=0.3, seed=8)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    get_q2y_nested_kfold(m, n_outer=4, n_inner=3)
    rep = m.q2y_report_
    assert set(rep) == {"form", "models", "outer_folds", "inner_folds", "passes", "models_per_pass", "x_reads", "n_iter", "why"}
    assert rep["form"].startswith("one refit per model") and rep["models"] == 16 and rep["passes"] == 0
    assert rep["models_per_pass"] is None and rep["x_reads"] is None
    assert "numpy" in rep["why"] and "K-fold kernels" in rep["why"], rep["why"]
    get_q2y_nested_kfold(m, n_outer=4, n_inner=3, device_folds=False)
    assert m.q2y_report_["why"] == "device folds switched off"
