"""Repeated K-fold Q2Y on the device (validate.get_q2y_repeated_kfold, cmtf_pls_amd/repeated.py): G shuffled splits x K folds per
pass, split-major, sharing every MTTKRP and contraction of X (cmtfpls_kfold_xcov_* per split, cmtfpls_kfold_inner_f64 or
cmtfpls_kfold_inner_coupled_f64, cmtfpls_kfold_epilogue_splits_f64), against the device get_q2y_kfold of every split; the new
epilogue entry against cmtfpls_kfold_epilogue_f64; the fallbacks against literal refits."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, kfold, tPLS
from cmtf_pls_amd.kfold import fold_ids
from cmtf_pls_amd.validate import get_q2y_kfold, get_q2y_repeated_kfold

pytestmark = pytest.mark.gpu

_TOL = {"float64": 1e-12, "float32": 1e-9}


def _check_against_kfold(m, res, K, dtype):
    """Every split's per-component Q2Y and n_iter against the device get_q2y_kfold of that split."""
    rep = m.q2y_report_
    for g, ids in enumerate(res["folds"]):
        want = get_q2y_kfold(m, folds=ids, per_component=True)
        assert "cmtfpls_kfold_inner" in m.q2y_report_["form"] and "why" not in m.q2y_report_, m.q2y_report_
        err = np.abs(res["q2y"][g] - want).max() / max(1.0, np.abs(want).max())
        assert err <= _TOL[dtype], (g, err, res["q2y"][g], want)
        assert rep["n_iter"][g] == m.q2y_report_["n_iter"], (g, rep["n_iter"][g], m.q2y_report_["n_iter"])


# name, shape, M, R, K, S, splits per pass
CASES = [
    ("order 2", (50, 30), 3, 3, 4, 10, 8),
    ("I % K != 0, partial last pass", (62, 10, 8), 4, 3, 5, 8, 6),
    ("K 2", (40, 6, 5), 3, 2, 2, 17, 16),
    ("K 32", (70, 12, 9), 2, 2, 32, 2, 1),
    ("M 1", (45, 9, 7), 1, 3, 3, 4, 4),
    ("I sets G", (21, 6, 5), 2, 2, 3, 12, 7),
    ("M 16 wide", (36, 64, 48), 16, 4, 4, 3, 3),
]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name,shape,M,R,K,S,G", CASES, ids=[c[0] for c in CASES])
def test_device_splits_equal_kfold_per_split(name, shape, M, R, K, S, G, dtype):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=7)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)
    m = tPLS(R, dtype=dtype)
    m.fit(x, y)
    res = get_q2y_repeated_kfold(m, n_splits=K, n_repeats=S, random_state=5, per_component=True)
    rep = m.q2y_report_
    assert "cmtfpls_kfold_epilogue_splits_f64" in rep["form"] and "why" not in rep, rep
    passes = -(-S // G)
    assert rep["splits_per_pass"] == G and rep["passes"] == passes and rep["splits"] == S
    assert rep["x_reads"] == S + passes * (2 * R - 1)
    assert res["q2y"].shape == (S, R) and np.all(np.isfinite(res["q2y"]))
    np.testing.assert_array_equal(res["mean"], res["q2y"].mean(axis=0))
    _check_against_kfold(m, res, K, dtype)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_coupled_tensor_and_matrix_blocks(dtype):
    rng = np.random.default_rng(3)
    I, L, M, R, K, S = 61, 4, 4, 3, 5, 8
    T = rng.standard_normal((I, L))
    Xs = [O.cp_factors_to_tensor([T, rng.standard_normal((10, L)), rng.standard_normal((8, L))]) + 0.3 * rng.standard_normal((I, 10, 8)),
          T @ rng.standard_normal((L, 12)) + 0.3 * rng.standard_normal((I, 12))]
    if dtype == "float32":
        Xs = [X.astype(np.float32).astype(np.float64) for X in Xs]
    y = T @ rng.standard_normal((L, M)) + 0.3 * rng.standard_normal((I, M))
    m = ctPLS(R, dtype=dtype)
    m.fit(Xs, y)
    res = get_q2y_repeated_kfold(m, n_splits=K, n_repeats=S, random_state=1, per_component=True)
    rep = m.q2y_report_
    assert "cmtfpls_kfold_inner_coupled_f64" in rep["form"] and "cmtfpls_kfold_epilogue_splits_f64" in rep["form"], rep
    assert "why" not in rep and rep["splits_per_pass"] == 6 and rep["passes"] == 2
    assert rep["x_reads"] == [S + 2 * (2 * R - 1)] * 2
    _check_against_kfold(m, res, K, dtype)


def test_one_block_ctpls_is_bitwise_tpls():
    x, y, _ = O.import_synthetic((50, 10, 8), 3, 4, error=0.3, seed=9)
    t = tPLS(3, dtype="float64")
    t.fit(x, y)
    c = ctPLS(3, dtype="float64")
    c.fit([x], y)
    a = get_q2y_repeated_kfold(t, n_splits=4, n_repeats=9, random_state=2, per_component=True)
    b = get_q2y_repeated_kfold(c, n_splits=4, n_repeats=9, random_state=2, per_component=True)
    assert "cmtfpls_kfold_inner_coupled_f64" in c.q2y_report_["form"] and "why" not in c.q2y_report_
    assert np.array_equal(a["q2y"], b["q2y"])
    assert t.q2y_report_["n_iter"] == c.q2y_report_["n_iter"]


def _kfold_buffers(m, K, splits):
    """Run the tPLS K-fold device form through kfold._state and kfold._components (kfold_epilogue; with splits > 0
    kfold_epilogue_splits with that many splits) and return its buffers after the last component."""
    be = m._get_engine().be
    X, Y = m.original_X, m.original_Y
    R = m.n_components
    I = X.shape[0]
    A, B = kfold._dims(X)
    P = A * B
    ids, K = fold_ids(I, K)
    Yh = Y.reshape(I, -1).astype(np.float64)
    M = Yh.shape[1]
    order, off, ybar, nu, Yk = kfold._fold_y(Yh, ids, K)
    t = lambda a, dt=torch.float64: kfold._to_dev(a, be.device, dt)
    X2 = t(X.reshape(I, P))
    S, mean = be.empty(K, M, P), be.empty(K, P)
    assert be.kfold_xcov(X2, A, B, t(Yh - ybar), t(order, torch.int32), t(off, torch.int32), K, t(nu - ybar), S, mean) is not None
    st, shared, own = kfold._state(be, t(ids, torch.int32), t(Yk), [(A, B, S, mean)], R, 1)
    assert kfold._components(be, [X2], st, shared, own, R, 1e-8, 100, False, splits=splits) is None
    torch.cuda.synchronize()
    return {**shared, **own[0]}


@pytest.mark.parametrize("shape,M,R,K", [((60, 10, 8), 4, 3, 5), ((37, 30), 2, 4, 3), ((40, 6, 5), 16, 2, 2)])
def test_splits_entry_with_one_split_is_bitwise_kfold_epilogue(shape, M, R, K):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=4)
    m = tPLS(R, dtype="float64")
    m.fit(x, y)
    want = _kfold_buffers(m, K, 0)
    got = _kfold_buffers(m, K, 1)
    for f in ("Tout", "coef", "Q", "S", "Yk", "T", "n_iter", "status"):
        assert torch.equal(got[f], want[f]), f


def test_callers_device_tensors_are_only_read():
    I, J, K, M, R = 4096, 24, 20, 4, 3
    g = torch.Generator(device="cuda:0").manual_seed(3)
    T = torch.randn(I, R, device="cuda:0", dtype=torch.float64, generator=g)
    X = torch.einsum("il,jl,kl->ijk", T, torch.randn(J, R, device="cuda:0", dtype=torch.float64, generator=g),
                     torch.randn(K, R, device="cuda:0", dtype=torch.float64, generator=g)).to(torch.float32)
    X += 0.5 * torch.randn(I, J, K, device="cuda:0", dtype=torch.float32, generator=g)
    Xm = (T @ torch.randn(R, 30, device="cuda:0", dtype=torch.float64, generator=g)).to(torch.float32)
    Y = T @ torch.randn(M, R, device="cuda:0", dtype=torch.float64, generator=g).T
    before, before_m = X.clone(), Xm.clone()
    m = tPLS(R, dtype="float32")
    m.fit(X, Y)
    res = get_q2y_repeated_kfold(m, n_splits=5, n_repeats=7, random_state=0)
    rep = m.q2y_report_
    assert "cmtfpls_kfold_epilogue_splits_f64" in rep["form"] and "why" not in rep, rep
    assert rep["passes"] == 2 and rep["splits_per_pass"] == 6 and rep["x_reads"] == 7 + 2 * (2 * R - 1)
    assert torch.equal(X, before) and res["mean"] > 0.9
    c = ctPLS(R, dtype="float32")
    c.fit([X, Xm], Y)
    get_q2y_repeated_kfold(c, n_splits=5, n_repeats=3)
    assert "why" not in c.q2y_report_ and c.q2y_report_["x_reads"] == [3 + 2 * R - 1] * 2, c.q2y_report_
    assert torch.equal(X, before) and torch.equal(Xm, before_m)


def _refit_q2y(x, y, ids, K, R):
    """Q2Y of every component count from one literal tPLS refit per fold."""
    pred = np.zeros((R,) + y.shape)
    for k in range(K):
        test = ids == k
        m = tPLS(R, dtype="float64")
        m.fit(x[~test], y[~test])
        s = m.transform(x[test])
        Qr = m.Y_factors[1].T
        for r in range(1, R + 1):
            pred[r - 1, test] = ((s[:, :r] @ m.coef_[:r, :r]) @ Qr[:r] + m.Y_mean).reshape(pred[r - 1, test].shape)
    return 1 - ((pred - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum()


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
    res = get_q2y_repeated_kfold(m, n_splits=K, n_repeats=2, per_component=True)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and rep.get("why") and rep["passes"] == 0 and rep["x_reads"] is None, rep
    assert res["q2y"].shape == (2, R)
    if case != "nan":
        for g in range(2):
            want = _refit_q2y(x, y, res["folds"][g], K, R)
            assert np.abs(res["q2y"][g] - want).max() <= 1e-8


def test_device_nan_declines_after_the_first_build_statistics():
    x, y, _ = O.import_synthetic((40, 6, 5), 3, 3, error=0.3, seed=13)
    xd = torch.from_numpy(x).cuda()
    m = tPLS(2, dtype="float64")
    m.fit(xd, y)
    xd[5, 2, 1] = float("nan")                                  # (after the fit: only the cross-validation sees it)
    get_q2y_repeated_kfold(m, n_splits=4, n_repeats=3)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and "non-finite" in rep["why"], rep
