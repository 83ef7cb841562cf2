"""K-fold cross-validation on the device (validate.kfold_predictions / get_q2y_kfold, cmtf_pls_amd/kfold.py): every fold served by
the same reads of X (cmtfpls_kfold_xcov_* / kfold_inner_f64 / kfold_epilogue_f64 with the MTTKRP and the contraction), against
literal refits of each fold on the regular engine."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import tPLS
from cmtf_pls_amd.kfold import fold_ids
from cmtf_pls_amd.validate import get_q2y, get_q2y_kfold, kfold_predictions

pytestmark = pytest.mark.gpu

_TOL = {"float64": 1e-8, "float32": 1e-7}


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(np.abs(np.asarray(want)).max(), 1e-300))


def _refit(x, y, train, test, R, dtype, algorithm="direct"):
    """A literal refit of one fold: (predictions of the test rows with the first r components for r = 1..R, n_iter_)."""
    m = tPLS(R, dtype=dtype, algorithm=algorithm)
    m.fit(x[train], y[train])
    s = m.transform(x[test])
    Qr = m.Y_factors[1].T
    preds = [(s[:, :r] @ m.coef_[:r, :r]) @ Qr[:r] + m.Y_mean for r in range(1, R + 1)]
    np.testing.assert_allclose(preds[-1], m.predict(x[test]).reshape(preds[-1].shape), rtol=1e-10, atol=1e-12)
    return np.stack(preds), list(m.n_iter_)


def _check_against_refits(m, x, y, pred, ids, K, R, dtype, folds_to_check=None):
    tol = _TOL[dtype]
    for k in (range(K) if folds_to_check is None else folds_to_check):
        test = ids == k
        want, n_iter = _refit(x, y, ~test, test, R, dtype)
        got = pred.reshape(R, y.shape[0], -1)[:, test]
        assert _rel(got, want.reshape(got.shape)) <= tol, (k, _rel(got, want.reshape(got.shape)))
        assert m.q2y_report_["n_iter"][k] == n_iter, (k, m.q2y_report_["n_iter"][k], n_iter)


CASES = [((60, 10, 8), 4, 3, 5, None), ((50, 30), 3, 3, 4, None), ((48, 80, 96), 3, 3, 3, None), ((36, 128, 128), 16, 4, 6, None),
         ((44, 72, 80), 3, 20, 4, None), ((60, 10, 8), 4, 3, 4, "shuffled")]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape,M,R,K,folds", CASES)
def test_device_form_equals_literal_refits(shape, M, R, K, folds, dtype):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=7)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)
    if folds == "shuffled":
        folds = np.random.default_rng(4).permutation(np.arange(shape[0]) % K)
        folds[:5] = 1                                           # unequal folds
    m = tPLS(R, dtype=dtype)
    m.fit(x, y)
    pred = kfold_predictions(m, n_splits=K, folds=folds)
    rep = m.q2y_report_
    assert "cmtfpls_kfold_inner_f64" in rep["form"], rep
    assert rep["x_reads"] == 2 * R and rep["folds"] == K
    assert np.array(rep["n_iter"]).shape == (K, R)
    ids, K = fold_ids(shape[0], K, folds)
    _check_against_refits(m, x, y, pred, ids, K, R, dtype)
    q = get_q2y_kfold(m, n_splits=K, folds=folds)
    q_ref = get_q2y_kfold(m, n_splits=K, folds=folds, device_folds=False)
    assert m.q2y_report_["form"].startswith("one refit per fold")
    assert abs(q - q_ref) <= 1e-8 * max(1.0, abs(q_ref)), (q, q_ref)


def test_per_component_q2y_equals_smaller_models():
    x, y, _ = O.import_synthetic((60, 10, 8), 4, 4, error=0.3, seed=8)
    R = 3
    m = tPLS(R, dtype="float64")
    m.fit(x, y)
    q = get_q2y_kfold(m, per_component=True)
    assert q.shape == (R,) and "kfold" in m.q2y_report_["form"]
    for r in range(1, R + 1):
        mr = tPLS(r, dtype="float64")
        mr.fit(x, y)
        assert abs(get_q2y_kfold(mr) - q[r - 1]) <= 1e-8, (r, get_q2y_kfold(mr), q[r - 1])


def test_k_equal_to_n_is_leave_one_out():
    x, y, _ = O.import_synthetic((30, 10, 8), 3, 3, error=0.3, seed=9)
    m = tPLS(2, dtype="float64")
    m.fit(x, y)
    q_k = get_q2y_kfold(m, n_splits=30)
    assert "kfold" in m.q2y_report_["form"]
    q_loo = get_q2y(m)
    assert "loo" in m.q2y_report_["form"]
    assert abs(q_k - q_loo) <= 1e-8, (q_k, q_loo)


def _device_data(I, J, K, M, L, seed):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    T = torch.randn(I, L, device="cuda:0", dtype=torch.float64, generator=g)
    Fa = torch.randn(J, L, device="cuda:0", dtype=torch.float64, generator=g)
    Fb = torch.randn(K, L, device="cuda:0", dtype=torch.float64, generator=g)
    Qy = torch.randn(M, L, device="cuda:0", dtype=torch.float64, generator=g)
    X = torch.einsum("il,jl,kl->ijk", T, Fa, Fb).to(torch.float32)
    X += 0.5 * torch.randn(I, J, K, device="cuda:0", dtype=torch.float32, generator=g)
    Y = T @ Qy.T + 0.3 * torch.randn(I, M, device="cuda:0", dtype=torch.float64, generator=g)
    return X, Y


@pytest.mark.parametrize("offset", [0.0, 1e3])
def test_callers_device_tensor_is_only_read(offset):
    I, J, K, M, R = 65536, 32, 32, 4, 3
    X, Y = _device_data(I, J, K, M, R, seed=3)
    if offset:
        spread = float(X.float().std())
        X += offset * spread * (1.0 + torch.arange(J * K, device="cuda:0", dtype=torch.float32).reshape(J, K) / (J * K))
    m = tPLS(R, dtype="float32")
    m.fit(X, Y)
    before = X.clone()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    pred = kfold_predictions(m)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert "kfold" in m.q2y_report_["form"], m.q2y_report_
    assert torch.equal(X, before)
    assert extra < 0.25 * X.numel() * X.element_size(), (extra, X.numel() * X.element_size())
    ids, Kf = fold_ids(I, 5)
    for k in (0, 3):
        test = ids == k
        r = tPLS(R, dtype="float32")
        tr = torch.from_numpy(np.flatnonzero(~test)).cuda()
        te = torch.from_numpy(np.flatnonzero(test)).cuda()
        r.fit(X.index_select(0, tr), Y.index_select(0, tr))
        want = r.predict(X.index_select(0, te))
        assert _rel(pred[-1][test], want) <= 1e-7, (k, _rel(pred[-1][test], want))
        assert m.q2y_report_["n_iter"][k] == list(r.n_iter_)


def _literal_all(x, y, ids, K, R, dtype):
    out = np.zeros((R,) + y.shape)
    for k in range(K):
        test = ids == k
        out[:, test] = _refit(x, y, ~test, test, R, dtype)[0].reshape((R, int(test.sum())) + y.shape[1:])
    return out


@pytest.mark.parametrize("case", ["nan", "order4", "k33", "m65"])
def test_declines_refit_per_fold(case):
    shape, M, R, K = (40, 6, 5), 3, 2, 4
    if case == "order4":
        shape = (24, 4, 3, 5)
    if case == "k33":
        shape, K = (40, 6, 5), 33
    if case == "m65":
        M = 65
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=12)
    if case == "nan":
        x[3, 1, 2] = np.nan
        x[7, 0, 0] = np.nan
    m = tPLS(R, dtype="float64")
    m.fit(x, y)
    pred = kfold_predictions(m, n_splits=K)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and rep.get("why"), rep
    ids, K = fold_ids(shape[0], K)
    want = _literal_all(x, y, ids, K, R, "float64")
    assert _rel(pred, want) <= 1e-10


def test_copy_x_false_and_malformed_folds():
    x, y, _ = O.import_synthetic((30, 6, 5), 2, 2, error=0.3, seed=1)
    n = tPLS(2, dtype="float64", copy_X=False)
    n.fit(torch.from_numpy(x).cuda(), y)
    with pytest.raises(AssertionError):
        get_q2y_kfold(n)
    m = tPLS(2, dtype="float64")
    m.fit(x, y)
    for kw in ({"n_splits": 1}, {"folds": np.arange(29) % 3}, {"folds": np.r_[-1, np.arange(29) % 3]},
               {"folds": np.r_[np.zeros(15, int), np.full(15, 2)]}):
        with pytest.raises(ValueError):
            get_q2y_kfold(m, **kw)


def test_full_size_cfg2_two_folds_against_refits():
    from cmtf_pls_amd.synthetic import synthetic_shard_device
    I, J, K, M, R = 65536, 128, 128, 16, 10
    X, Y = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=215, device="cuda:0")
    m = tPLS(R, dtype="float32")
    m.fit(X, Y)
    pred = kfold_predictions(m)
    assert "kfold" in m.q2y_report_["form"] and m.q2y_report_["x_reads"] == 2 * R
    ids, _ = fold_ids(I, 5)
    for k in (0, 4):
        test = ids == k
        tr = torch.from_numpy(np.flatnonzero(~test)).cuda()
        te = torch.from_numpy(np.flatnonzero(test)).cuda()
        r = tPLS(R, dtype="float32")
        r.fit(X.index_select(0, tr), Y.index_select(0, tr))
        want = r.predict(X.index_select(0, te))
        del tr
        assert _rel(pred[-1][test], want) <= 1e-7, (k, _rel(pred[-1][test], want))


def test_declines_on_the_device_tensor_route():
    """A device tensor is not scanned on the host: NaN shows up in the column sums of the first pass (kfold_xcov), and an offset
    beyond EngineOptions.xcov_raw_max_offset in its statistics; both decline to the refits with a why."""
    from cmtf_pls_amd.engine import EngineOptions
    x, y, _ = O.import_synthetic((40, 6, 5), 3, 3, error=0.3, seed=13)
    ids, K = fold_ids(40, 4)
    want = _literal_all(x, y, ids, K, 2, "float64")
    xd = torch.from_numpy(x).cuda()
    m = tPLS(2, dtype="float64")
    m.fit(xd, y)
    xd[5, 2, 1] = float("nan")                          # (after the fit: only the cross-validation sees it)
    pred = kfold_predictions(m, n_splits=4)
    assert m.q2y_report_["form"].startswith("one refit per fold") and "non-finite" in m.q2y_report_["why"], m.q2y_report_
    assert pred.shape == (2,) + y.shape
    xd[5, 2, 1] = float(x[5, 2, 1])
    strict = tPLS(2, dtype="float64", options=EngineOptions(small_fit=False, xcov_raw_max_offset=1e-3))
    strict.fit(xd, y)
    pred = kfold_predictions(strict, n_splits=4)
    assert strict.q2y_report_["form"].startswith("one refit per fold") and "spread" in strict.q2y_report_["why"], strict.q2y_report_
    assert _rel(pred, want) <= 1e-10
