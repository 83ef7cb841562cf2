"""Response-permutation test of K-fold Q2Y on the device (validate.permutation_test_q2y, cmtf_pls_amd/permutation.py): G permutations
x K folds per pass from shared reads of X (cmtfpls_kfold_wide_xcov_* / kfold_inner_grouped_f64 / kfold_epilogue_grouped_f64 with the
MTTKRP and the contraction), against literal refits of every fold on Y[pi_p]; and the wide build against float64 torch."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd import kfold
from cmtf_pls_amd.kfold import fold_ids
from cmtf_pls_amd.validate import get_q2y_kfold, kfold_predictions, permutation_test_q2y

pytestmark = pytest.mark.gpu

_TOL = {"float64": 1e-8, "float32": 1e-7}


def _refit_q2y(x, y, ids, K, R, dtype):
    """(Q2Y of every component count, n_iter per fold) from one literal refit per fold."""
    pred = np.zeros((R,) + y.shape)
    n_iter = []
    for k in range(K):
        test = ids == k
        m = tPLS(R, dtype=dtype)
        m.fit(x[~test], y[~test])
        s = m.transform(x[test])
        Qr = m.Y_factors[1].T
        for r in range(1, R + 1):
            pred[r - 1, test] = ((s[:, :r] @ m.coef_[:r, :r]) @ Qr[:r] + m.Y_mean).reshape(pred[r - 1, test].shape)
        n_iter.append(list(m.n_iter_))
    return 1 - ((pred - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum(), n_iter


CASES = [((60, 10, 8), 4, 3, 5, None), ((50, 30), 3, 3, 4, None), ((48, 80, 96), 3, 3, 3, None), ((36, 128, 128), 16, 4, 6, None),
         ((44, 72, 80), 3, 20, 4, None), ((60, 10, 8), 4, 3, 4, "shuffled")]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape,M,R,K,folds", CASES)
def test_device_null_equals_literal_refits(shape, M, R, K, folds, dtype):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=7)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)
    if folds == "shuffled":
        folds = np.random.default_rng(4).permutation(np.arange(shape[0]) % K)
        folds[:5] = 1                                           # unequal folds
    m = tPLS(R, dtype=dtype)
    m.fit(x, y)
    G = 32 // K
    P = 2 * G + 1                                               # three passes, the last one partial
    res = permutation_test_q2y(m, n_permutations=P, n_splits=K, folds=folds, random_state=3, per_component=True)
    rep = m.q2y_report_
    assert "cmtfpls_kfold_wide_xcov" in rep["form"] and "why" not in rep, rep
    assert rep["passes"] == 3 and rep["models_per_pass"] == K * G and rep["permutations"] == P
    assert rep["x_reads"] == 2 * R * rep["passes"]
    assert res["null"].shape == (P, R) and np.all(np.isfinite(res["null"]))
    ids, K = fold_ids(shape[0], K, folds)
    for p in (0, G + 1, P - 1):                                 # one permutation of every pass
        pi = res["permutations"][p]
        want, n_iter = _refit_q2y(x, y[pi], ids, K, R, dtype)
        err = np.abs(res["null"][p] - want).max() / max(1.0, np.abs(want).max())
        assert err <= _TOL[dtype], (p, err, res["null"][p], want)
        assert rep["n_iter"][p] == n_iter, (p, rep["n_iter"][p], n_iter)
    q = get_q2y_kfold(m, n_splits=K, folds=folds, per_component=True)
    np.testing.assert_array_equal(res["q2y"], q)
    np.testing.assert_array_equal(res["p_value"], (1 + (res["null"] >= q).sum(axis=0)) / (P + 1))


@pytest.mark.parametrize("shape,M,R,K,folds", CASES)
def test_grouped_run_with_identity_map_is_bitwise_kfold(shape, M, R, K, folds):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=9)
    if folds == "shuffled":
        folds = np.random.default_rng(4).permutation(np.arange(shape[0]) % K)
        folds[:5] = 1
    m = tPLS(R, dtype="float64")
    m.fit(x, y)
    want = kfold_predictions(m, n_splits=K, folds=folds)
    assert "cmtfpls_kfold_inner_f64" in m.q2y_report_["form"]
    ids, K = fold_ids(shape[0], K, folds)
    be = m._get_engine().be                                     # the K-fold device form with model k = fold k in one group
    I = shape[0]
    A, B = kfold._dims(x)
    Yh = y.reshape(I, -1).astype(np.float64)
    order, off, ybar, nu, Yk = kfold._fold_y(Yh, ids, K)
    t = lambda a, dt=torch.float64: kfold._to_dev(a, be.device, dt)
    X2 = t(x.reshape(I, A * B))
    S, mean = be.empty(K, M, A * B), be.empty(K, A * B)
    assert be.kfold_xcov(X2, A, B, t(Yh - ybar), t(order, torch.int32), t(off, torch.int32), K, t(nu - ybar), S, mean) is not None
    st, shared, own = kfold._state(be, t(ids, torch.int32), t(Yk), [(A, B, S, mean)], R, 1)
    mf = torch.arange(K, dtype=torch.int32, device=be.device)
    assert kfold._components(be, [X2], st, shared, own, R, 1e-8, 100, False, grouped=(mf, 1)) is None
    assert not shared["status"].any()
    got = kfold._held_out_predictions(shared["Tout"][0].cpu().numpy(), shared["coef"].cpu().numpy(), shared["Q"].cpu().numpy(), nu,
                                      ids, K, R, M)
    assert np.array_equal(got.reshape(want.shape), want)
    assert shared["n_iter"].cpu().numpy().tolist() == m.q2y_report_["n_iter"]


def test_identity_permutation_equals_observed():
    x, y, _ = O.import_synthetic((60, 10, 8), 4, 4, error=0.3, seed=5)
    m = tPLS(3, dtype="float64")
    m.fit(x, y)
    perms = np.stack([np.random.default_rng(1).permutation(60), np.arange(60), np.random.default_rng(2).permutation(60)])
    res = permutation_test_q2y(m, permutations=perms, per_component=True)
    assert "cmtfpls_kfold_wide_xcov" in m.q2y_report_["form"]
    assert np.abs(res["null"][1] - res["q2y"]).max() <= 1e-10, (res["null"][1], res["q2y"])


def test_callers_device_tensor_is_only_read():
    I, J, K, M, R = 4096, 24, 20, 4, 3
    g = torch.Generator(device="cuda:0").manual_seed(3)
    T = torch.randn(I, R, device="cuda:0", dtype=torch.float64, generator=g)
    X = torch.einsum("il,jl,kl->ijk", T, torch.randn(J, R, device="cuda:0", dtype=torch.float64, generator=g),
                     torch.randn(K, R, device="cuda:0", dtype=torch.float64, generator=g)).to(torch.float32)
    X += 0.5 * torch.randn(I, J, K, device="cuda:0", dtype=torch.float32, generator=g)
    Y = T @ torch.randn(M, R, device="cuda:0", dtype=torch.float64, generator=g).T
    m = tPLS(R, dtype="float32")
    m.fit(X, Y)
    before = X.clone()
    res = permutation_test_q2y(m, n_permutations=8)
    assert "cmtfpls_kfold_wide_xcov" in m.q2y_report_["form"], m.q2y_report_
    assert torch.equal(X, before)
    assert res["p_value"] == pytest.approx(1 / 9)                 # a strong signal beats every permutation


@pytest.mark.parametrize("case", ["nan", "order4", "m65"])
def test_fallbacks_refit_with_why(case):
    shape, M, R, K = (40, 6, 5), 3, 2, 4
    if case == "order4":
        shape = (24, 4, 3, 5)
    if case == "m65":
        M = 65
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=12)
    if case == "nan":
        x[3, 1, 2] = np.nan
    m = tPLS(R, dtype="float64")
    m.fit(x, y)
    res = permutation_test_q2y(m, n_permutations=2, n_splits=K, per_component=True)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and rep.get("why") and rep["passes"] == 0, rep
    assert res["null"].shape == (2, R)
    if case != "nan":
        ids, K = fold_ids(shape[0], K)
        want, _ = _refit_q2y(x, y[res["permutations"][1]], ids, K, R, "float64")
        assert np.abs(res["null"][1] - want).max() <= 1e-8


def test_device_nan_declines_after_the_first_pass_statistics():
    x, y, _ = O.import_synthetic((40, 6, 5), 3, 3, error=0.3, seed=13)
    xd = torch.from_numpy(x).cuda()
    m = tPLS(2, dtype="float64")
    m.fit(xd, y)
    xd[5, 2, 1] = float("nan")                                  # (after the fit: only the permutation test sees it)
    permutation_test_q2y(m, n_permutations=2, n_splits=4)
    assert m.q2y_report_["form"].startswith("one refit per fold") and "non-finite" in m.q2y_report_["why"], m.q2y_report_


def test_coupled_model_refits_with_why():
    x, y, _ = O.import_synthetic((30, 6, 5), 2, 3, error=0.3, seed=13)
    xm = np.random.default_rng(3).standard_normal((30, 7))
    m = ctPLS(2, dtype="float64")
    m.fit([x, xm], y)
    res = permutation_test_q2y(m, n_permutations=2, n_splits=3)
    rep = m.q2y_report_
    assert rep["why"] == "coupled model: permutation device form not built" and rep["passes"] == 0
    assert res["q2y"] == get_q2y_kfold(m, n_splits=3) and np.all(np.isfinite(res["null"]))


# ---- the wide build on its own ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("I,A,B,W,K", [(300, 7, 9, 5, 2), (300, 16, 32, 96, 2), (517, 1, 130, 37, 32), (400, 12, 20, 1024, 2),
                                       (2000, 8, 8, 200, 32), (5000, 33, 40, 64, 5)])
def test_wide_build_against_float64_torch(I, A, B, W, K, xdtype):
    _check_wide_build(I, A, B, W, K, xdtype)


@pytest.mark.parametrize("xdtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("I,A,B,W,K", [(300, 16, 32, 96, 2), (2000, 8, 8, 200, 32)])
def test_wide_build_of_a_misaligned_view_against_float64_torch(I, A, B, W, K, xdtype):
    """X a view one element into its storage: P % 4 == 0, but the rows are not aligned to the vector loads of the VEC instance."""
    _check_wide_build(I, A, B, W, K, xdtype, base=1)


def _check_wide_build(I, A, B, W, K, xdtype, base=0):
    from cmtf_pls_amd.backend import HipBackend
    be = HipBackend(torch.device("cuda:0"))
    g = torch.Generator(device="cuda:0").manual_seed(I + W)
    P = A * B
    X = (torch.randn(I, P, device="cuda:0", dtype=torch.float64, generator=g) + 0.3).to(xdtype)
    if base:
        buf = torch.zeros(base + I * P, device="cuda:0", dtype=xdtype)
        buf[base:].view(I, P).copy_(X)
        X = buf[base:].view(I, P)
        assert X.is_contiguous() and X.data_ptr() % 16 != 0
    before = X.clone()
    Yw = torch.randn(I, W, device="cuda:0", dtype=torch.float64, generator=g)
    ids = np.random.default_rng(W).permutation(np.arange(I) % K)
    counts = np.bincount(ids, minlength=K)
    order = torch.from_numpy(np.argsort(ids, kind="stable").astype(np.int32)).cuda()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
    ydev = torch.randn(K, W, device="cuda:0", dtype=torch.float64, generator=g)
    S = torch.empty(K, W, P, device="cuda:0", dtype=torch.float64)
    mean = torch.empty(K, P, device="cuda:0", dtype=torch.float64)
    stats = be.kfold_wide_xcov(X, A, B, Yw, order, off, K, ydev, S, mean)
    S2, mean2 = torch.empty_like(S), torch.empty_like(mean)
    stats2 = be.kfold_wide_xcov(X, A, B, Yw, order, off, K, ydev, S2, mean2)
    assert torch.equal(S, S2) and torch.equal(mean, mean2) and torch.equal(stats, stats2)    # the same bits on every run
    assert torch.equal(X, before)
    X64 = X.to(torch.float64)
    idt = torch.from_numpy(ids).cuda()
    Sf = torch.stack([X64[idt == f].T @ Yw[idt == f] for f in range(K)])                     # P x W per fold group
    for k in range(K):
        ntr = I - int(counts[k])
        mu = X64[idt != k].sum(0) / ntr
        want = (Sf.sum(0) - Sf[k]).T - ntr * ydev[k][:, None] * mu[None, :]
        scale = float(want.abs().max())
        assert float((S[k] - want).abs().max()) <= 1e-12 * scale, k
        assert float((mean[k] - mu).abs().max()) <= 1e-13 * float(mu.abs().max())
    assert float((stats[:P] - X64.sum(0)).abs().max()) <= 1e-12 * float(X64.sum(0).abs().max())
    assert float((stats[P:] - (X64 * X64).sum(0)).abs().max()) <= 1e-12 * float((X64 * X64).sum(0).max())
