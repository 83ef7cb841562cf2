"""K-fold cross-validation of a coupled model on the device (validate.kfold_predictions / get_q2y_kfold on a ctPLS,
cmtf_pls_amd/kfold.py): every fold served by the same reads of every block (cmtfpls_kfold_xcov_* per block,
cmtfpls_kfold_inner_coupled_f64, cmtfpls_mttkrp_* per block, cmtfpls_kfold_combine_scores_f64, cmtfpls_kfold_epilogue_f64,
cmtfpls_xcov_* per block), against literal ctPLS refits of each fold on the regular engine."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.kfold import fold_ids
from cmtf_pls_amd.validate import get_q2y_kfold, kfold_predictions

pytestmark = pytest.mark.gpu

_TOL = {"float64": 1e-8, "float32": 1e-7}


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(np.abs(np.asarray(want)).max(), 1e-300))


def _coupled_data(shapes, M, L, seed, error=0.3):
    rng = np.random.default_rng(seed)
    I = shapes[0][0]
    T = rng.standard_normal((I, L))
    Xs = [O.cp_factors_to_tensor([T] + [rng.standard_normal((d, L)) for d in shape[1:]]) + error * rng.standard_normal(shape)
          for shape in shapes]
    Y = T @ rng.standard_normal((L, M)) + error * rng.standard_normal((I, M))
    return Xs, Y


def _refit(Xs, y, train, test, R, dtype):
    """A literal ctPLS refit of one fold: (predictions of the test rows with the first r components for r = 1..R, n_iter_)."""
    m = ctPLS(R, dtype=dtype)
    m.fit([X[train] for X in Xs], y[train])
    s = m.transform([X[test] for X in Xs])
    Qr = m.Y_factors[1].T
    preds = [(s[:, :r] @ m.coef_[:r, :r]) @ Qr[:r] + m.Y_mean for r in range(1, R + 1)]
    np.testing.assert_allclose(preds[-1], m.predict([X[test] for X in Xs]).reshape(preds[-1].shape), rtol=1e-10, atol=1e-12)
    return np.stack(preds), list(m.n_iter_)


def _literal_all(Xs, y, ids, K, R, dtype):
    out = np.zeros((R,) + y.shape)
    for k in range(K):
        test = ids == k
        out[:, test] = _refit(Xs, y, ~test, test, R, dtype)[0].reshape((R, int(test.sum())) + y.shape[1:])
    return out


CASES = [
    ("tensor+matrix", [(60, 10, 8), (60, 12)], 4, 3, 5, None),
    ("two tensors", [(50, 10, 8), (50, 24, 16)], 3, 3, 4, None),
    ("three blocks", [(48, 8, 6), (48, 10), (48, 5, 7)], 3, 3, 3, None),
    ("side 256", [(36, 256, 260), (36, 20)], 3, 2, 3, None),
    ("M 16", [(40, 12, 10), (40, 15)], 16, 4, 4, None),
    ("shuffled", [(60, 10, 8), (60, 12)], 4, 3, 4, "shuffled"),
]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name,shapes,M,R,K,folds", CASES, ids=[c[0] for c in CASES])
def test_device_form_equals_literal_refits(name, shapes, M, R, K, folds, dtype):
    Xs, y = _coupled_data(shapes, M, R + 1, seed=7)
    if dtype == "float32":
        Xs = [X.astype(np.float32).astype(np.float64) for X in Xs]
    I = shapes[0][0]
    if folds == "shuffled":
        folds = np.random.default_rng(4).permutation(np.arange(I) % K)
        folds[:5] = 1                                           # unequal folds
    m = ctPLS(R, dtype=dtype)
    m.fit(Xs, y)
    pred = kfold_predictions(m, n_splits=K, folds=folds)
    rep = m.q2y_report_
    assert "cmtfpls_kfold_inner_coupled_f64" in rep["form"], rep
    assert rep["x_reads"] == [2 * R] * len(Xs) and rep["folds"] == K
    assert np.array(rep["n_iter"]).shape == (K, R)
    ids, K = fold_ids(I, K, folds)
    tol = _TOL[dtype]
    for k in range(K):
        test = ids == k
        want, n_iter = _refit(Xs, y, ~test, test, R, dtype)
        got = pred.reshape(R, I, -1)[:, test]
        assert _rel(got, want.reshape(got.shape)) <= tol, (k, _rel(got, want.reshape(got.shape)))
        assert rep["n_iter"][k] == n_iter, (k, rep["n_iter"][k], n_iter)
    q = get_q2y_kfold(m, n_splits=K, folds=folds)
    q_ref = get_q2y_kfold(m, n_splits=K, folds=folds, device_folds=False)
    assert m.q2y_report_["form"].startswith("one refit per fold")
    assert abs(q - q_ref) <= 1e-8 * max(1.0, abs(q_ref)), (q, q_ref)


@pytest.mark.parametrize("shape", [(60, 10, 8), (50, 30)])
def test_single_block_equals_tpls(shape):
    x, y, _ = O.import_synthetic(shape, 4, 4, error=0.3, seed=8)
    c = ctPLS(3, dtype="float64")
    c.fit([x], y)
    t = tPLS(3, dtype="float64")
    t.fit(x, y)
    pc = kfold_predictions(c, n_splits=5)
    assert "cmtfpls_kfold_inner_coupled_f64" in c.q2y_report_["form"] and c.q2y_report_["x_reads"] == [6]
    pt = kfold_predictions(t, n_splits=5)
    assert "cmtfpls_kfold_inner_f64" in t.q2y_report_["form"]
    assert _rel(pc, pt) <= 1e-12, _rel(pc, pt)
    assert c.q2y_report_["n_iter"] == t.q2y_report_["n_iter"]


def test_per_component_q2y_equals_smaller_models():
    Xs, y = _coupled_data([(60, 10, 8), (60, 12)], 4, 4, seed=9)
    R = 3
    m = ctPLS(R, dtype="float64")
    m.fit(Xs, y)
    q = get_q2y_kfold(m, per_component=True)
    assert q.shape == (R,) and "coupled" in m.q2y_report_["form"]
    for r in range(1, R + 1):
        mr = ctPLS(r, dtype="float64")
        mr.fit(Xs, y)
        q_r = get_q2y_kfold(mr)
        assert "coupled" in mr.q2y_report_["form"]
        assert abs(q_r - q[r - 1]) <= 1e-8, (r, q_r, q[r - 1])


def test_callers_device_blocks_are_only_read():
    I, M, R, L = 16384, 4, 3, 3
    g = torch.Generator(device="cuda:0").manual_seed(5)
    T = torch.randn(I, L, device="cuda:0", dtype=torch.float64, generator=g)
    X0 = torch.einsum("il,jl,kl->ijk", T, torch.randn(32, L, device="cuda:0", dtype=torch.float64, generator=g),
                      torch.randn(24, L, device="cuda:0", dtype=torch.float64, generator=g)).to(torch.float32)
    X0 += 0.5 * torch.randn(X0.shape, device="cuda:0", dtype=torch.float32, generator=g)
    X1 = (T @ torch.randn(L, 200, device="cuda:0", dtype=torch.float64, generator=g)).to(torch.float32)
    X1 += 0.5 * torch.randn(X1.shape, device="cuda:0", dtype=torch.float32, generator=g)
    Y = T @ torch.randn(L, M, device="cuda:0", dtype=torch.float64, generator=g) + 0.3 * torch.randn(I, M, device="cuda:0",
                                                                                                      dtype=torch.float64, generator=g)
    m = ctPLS(R, dtype="float32")
    m.fit([X0, X1], Y)
    before = [X0.clone(), X1.clone()]
    pred = kfold_predictions(m)
    torch.cuda.synchronize()
    assert "coupled" in m.q2y_report_["form"], m.q2y_report_
    assert torch.equal(X0, before[0]) and torch.equal(X1, before[1])
    ids, _ = fold_ids(I, 5)
    for k in (0, 3):
        test = ids == k
        tr = torch.from_numpy(np.flatnonzero(~test)).cuda()
        te = torch.from_numpy(np.flatnonzero(test)).cuda()
        r = ctPLS(R, dtype="float32")
        r.fit([X0.index_select(0, tr), X1.index_select(0, tr)], Y.index_select(0, tr))
        want = r.predict([X0.index_select(0, te), X1.index_select(0, te)])
        assert _rel(pred[-1][test], want) <= 1e-7, (k, _rel(pred[-1][test], want))
        assert m.q2y_report_["n_iter"][k] == list(r.n_iter_)


@pytest.mark.parametrize("case,why", [("nan", "missing values in block 1"), ("order4", "block 1 of order 4"), ("k33", "K = 33"),
                                      ("m65", "M = 65")])
def test_declines_refit_per_fold(case, why):
    shapes, M, R, K = [(40, 6, 5), (40, 7)], 3, 2, 4
    if case == "order4":
        shapes = [(40, 6, 5), (40, 4, 3, 5)]
    if case == "k33":
        K = 33
    if case == "m65":
        M = 65
    Xs, y = _coupled_data(shapes, M, R + 1, seed=12)
    if case == "nan":
        Xs[1][3, 2] = np.nan
        Xs[1][7, 0] = np.nan
    m = ctPLS(R, dtype="float64")
    m.fit(Xs, y)
    q = get_q2y_kfold(m, n_splits=K, per_component=True)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and why in rep["why"], rep
    q_ref = get_q2y_kfold(m, n_splits=K, per_component=True, device_folds=False)
    np.testing.assert_allclose(q, q_ref, rtol=0, atol=1e-12)
    if case != "nan":
        pred = kfold_predictions(m, n_splits=K)
        ids, K = fold_ids(40, K)
        assert _rel(pred, _literal_all(Xs, y, ids, K, R, "float64")) <= 1e-10


def test_nan_in_a_device_block_declines():
    """A device block is not scanned on the host: NaN shows up in the column sums of its first pass (kfold_xcov)."""
    Xs, y = _coupled_data([(40, 6, 5), (40, 7)], 3, 3, seed=13)
    xd = [torch.from_numpy(X).cuda() for X in Xs]
    m = ctPLS(2, dtype="float64")
    m.fit(xd, y)
    xd[1][5, 2] = float("nan")                          # (after the fit: only the cross-validation sees it)
    pred = kfold_predictions(m, n_splits=4)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and "non-finite" in rep["why"] and "block 1" in rep["why"], rep
    assert pred.shape == (2,) + y.shape


def test_copy_x_false_raises():
    Xs, y = _coupled_data([(30, 6, 5), (30, 7)], 2, 2, seed=1)
    n = ctPLS(2, dtype="float64", copy_X=False)
    n.fit([torch.from_numpy(X).cuda() for X in Xs], y)
    assert n.original_Xs is None
    with pytest.raises(AssertionError):
        get_q2y_kfold(n)
