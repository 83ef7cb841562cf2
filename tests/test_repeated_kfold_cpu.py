"""CPU-only: repeated K-fold Q2Y (validate.get_q2y_repeated_kfold) on the NumPy backend, i.e. the refit path: the splits against
sklearn's RepeatedKFold, each split against get_q2y_kfold and literal oracle fits, the summary, the report and argument validation."""
import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.kfold import repeated_fold_ids
from cmtf_pls_amd.repeated import summary
from cmtf_pls_amd.validate import get_q2y_kfold, get_q2y_repeated_kfold
from numpy_backend import NumpyBackend


@pytest.mark.parametrize("I,K,S,seed", [(23, 5, 4, 7), (20, 5, 3, 0), (24, 4, 3, 11), (11, 2, 5, 3), (40, 2, 2, 123), (33, 32, 2, 9)])
def test_splits_equal_sklearn_repeated_kfold(I, K, S, seed):
    sk = pytest.importorskip("sklearn.model_selection")
    ids, K2 = repeated_fold_ids(I, K, S, seed)
    assert K2 == K and ids.shape == (S, I)
    tests = [t for _, t in sk.RepeatedKFold(n_splits=K, n_repeats=S, random_state=seed).split(np.zeros((I, 1)))]
    assert len(tests) == S * K
    for g in range(S):
        for k in range(K):
            assert np.array_equal(np.flatnonzero(ids[g] == k), np.sort(tests[g * K + k])), (g, k)


def test_splits_are_reproducible_and_differ_between_seeds():
    a, _ = repeated_fold_ids(30, 3, 4, 5)
    b, _ = repeated_fold_ids(30, 3, 4, 5)
    c, _ = repeated_fold_ids(30, 3, 4, 6)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert not np.array_equal(a[0], a[1])                         # every repeat draws a new shuffle
    assert all(np.array_equal(np.bincount(r), [10, 10, 10]) for r in a)


def _oracle_q2y(fit, Xs, y, ids, K, R):
    pred = np.zeros((R,) + y.shape)
    for k in range(K):
        test = ids == k
        for r in range(1, R + 1):
            f = fit([X[~test] for X in Xs] if len(Xs) > 1 else Xs[0][~test], y[~test], r)
            pred[r - 1, test] = O.predict(f, [X[test] for X in Xs] if len(Xs) > 1 else Xs[0][test])
    return 1 - ((pred - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum()


@pytest.mark.parametrize("coupled", [False, True])
def test_each_split_equals_get_q2y_kfold_and_oracle_fits(coupled):
    x, y, _ = O.import_synthetic((23, 5, 4), 2, 3, error=0.3, seed=11)
    R = 2
    if coupled:
        xm = np.random.default_rng(3).standard_normal((23, 6)) + x[:, :, 0] @ np.ones((5, 6)) * 0.1
        Xs, m, fit = [x, xm], ctPLS(R, backend=NumpyBackend()), O.fit_ctpls
        m.fit(Xs, y)
    else:
        Xs, m, fit = [x], tPLS(R, backend=NumpyBackend()), O.fit_tpls
        m.fit(x, y)
    res = get_q2y_repeated_kfold(m, n_splits=4, n_repeats=3, random_state=2, per_component=True)
    rep = m.q2y_report_
    assert res["q2y"].shape == (3, R) and res["folds"].shape == (3, 23)
    assert np.array_equal(res["folds"], repeated_fold_ids(23, 4, 3, 2)[0])
    for g in range(3):
        np.testing.assert_array_equal(res["q2y"][g], get_q2y_kfold(m, folds=res["folds"][g], per_component=True))
        np.testing.assert_allclose(res["q2y"][g], _oracle_q2y(fit, Xs, y, res["folds"][g], 4, R), rtol=1e-8, atol=1e-8)
    assert len(rep["n_iter"]) == 3 and np.array(rep["n_iter"][0]).shape == (4, R)
    last = get_q2y_repeated_kfold(m, n_splits=4, n_repeats=3, random_state=2)
    np.testing.assert_array_equal(last["q2y"], res["q2y"][:, -1])
    assert last["mean"] == pytest.approx(res["mean"][-1], rel=0, abs=0) and "one_se" not in last


def test_given_folds_are_used_and_other_arguments_ignored():
    x, y, _ = O.import_synthetic((20, 6), 3, 3, error=0.3, seed=4)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    folds = np.stack([np.arange(20) % 3, np.random.default_rng(1).permutation(np.arange(20) % 3)])
    res = get_q2y_repeated_kfold(m, n_splits=7, n_repeats=9, folds=folds, random_state="ignored")
    assert np.array_equal(res["folds"], folds) and res["q2y"].shape == (2,) and m.q2y_report_["splits"] == 2
    assert res["q2y"][1] == get_q2y_kfold(m, folds=folds[1])


def test_summary_on_a_hand_made_example():
    q = np.array([[0.1, 0.50, 0.52],
                  [0.2, 0.60, 0.58],
                  [0.3, 0.55, 0.60]])
    s = summary(q)
    np.testing.assert_allclose(s["mean"], [0.2, 0.55, 0.17 / 0.3], rtol=1e-14)
    np.testing.assert_allclose(s["std"], [np.sqrt(0.02 / 3), np.sqrt(0.005 / 3), np.sqrt(0.0104 / 9)], rtol=1e-12)   # ddof = 0
    # max mean 0.5667 at r = 3, std 0.0340 there: threshold 0.5667 - 0.0340 / sqrt(3) = 0.5470 <= 0.55, the mean at r = 2
    assert s["one_se"] == 2
    s2 = summary(np.array([[0.1, 0.3], [0.2, 0.5]]))             # threshold 0.4 - 0.1 / sqrt(2) = 0.329 > 0.15: r = 2
    assert s2["one_se"] == 2 and s2["std"][1] == pytest.approx(0.1)
    s3 = summary(np.array([[0.5, 0.4], [0.5, 0.45]]))            # the best is r = 1 itself
    assert s3["one_se"] == 1
    s4 = summary(np.array([0.2, 0.4]))
    assert s4["mean"] == pytest.approx(0.3) and s4["std"] == pytest.approx(0.1) and "one_se" not in s4


def test_result_summary_matches_numpy():
    x, y, _ = O.import_synthetic((18, 4, 5), 2, 3, error=0.3, seed=6)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    res = get_q2y_repeated_kfold(m, n_splits=3, n_repeats=4, per_component=True)
    np.testing.assert_array_equal(res["mean"], res["q2y"].mean(axis=0))
    np.testing.assert_array_equal(res["std"], np.std(res["q2y"], axis=0))
    best = int(np.argmax(res["mean"]))
    ok = res["mean"] >= res["mean"][best] - res["std"][best] / 2.0
    assert res["one_se"] == int(np.flatnonzero(ok)[0]) + 1


def test_argument_validation():
    x, y, _ = O.import_synthetic((20, 5, 4), 2, 3, error=0.3, seed=8)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    good = np.arange(20) % 4
    bad = [{"random_state": None}, {"random_state": 1.0}, {"random_state": np.random.RandomState(0)}, {"random_state": True},
           {"n_repeats": 0}, {"n_repeats": -2}, {"n_splits": 1}, {"n_splits": 21},
           {"folds": good},                                                         # 1-d
           {"folds": np.stack([good[:-1]])},                                        # wrong length
           {"folds": np.zeros((0, 20), dtype=int)},                                 # no split
           {"folds": np.stack([good, np.where(good == 2, 3, good)])},               # fold 2 empty in row 1
           {"folds": np.stack([good, np.arange(20) % 3])},                          # K = 4 and K = 3
           {"folds": np.stack([good + 0.5])},                                       # not integers
           {"folds": np.stack([good - 1])}]                                         # negative ids
    for kw in bad:
        with pytest.raises(ValueError):
            get_q2y_repeated_kfold(m, **kw)
    n = tPLS(2, backend=NumpyBackend())
    with pytest.raises(AssertionError):
        get_q2y_repeated_kfold(n)                                                   # not fitted
    c = tPLS(2, backend=NumpyBackend(), copy_X=False)
    c.fit(x, y)
    with pytest.raises(AssertionError):
        get_q2y_repeated_kfold(c)
    cc = ctPLS(2, backend=NumpyBackend(), copy_X=False)
    cc.fit([x, x[:, :, 0]], y)
    with pytest.raises(AssertionError):
        get_q2y_repeated_kfold(cc)


def test_report_keys_and_why_names_the_backend():
    x, y, _ = O.import_synthetic((20, 5, 4), 2, 3, error=0.3, seed=8)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    get_q2y_repeated_kfold(m, n_splits=4, n_repeats=2)
    rep = m.q2y_report_
    assert set(rep) == {"form", "splits", "passes", "splits_per_pass", "x_reads", "n_iter", "why"}
    assert rep["form"].startswith("one refit per fold") and rep["splits"] == 2 and rep["passes"] == 0
    assert rep["splits_per_pass"] is None and rep["x_reads"] is None
    assert "numpy" in rep["why"] and "K-fold kernels" in rep["why"], rep["why"]
    get_q2y_repeated_kfold(m, n_splits=4, n_repeats=2, device_folds=False)
    assert m.q2y_report_["why"] == "device folds switched off"
