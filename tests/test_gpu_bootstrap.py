"""Bootstrap of the factors on the device (validate.bootstrap_factors, cmtf_pls_amd/bootstrap.py): up to 32 resamples per pass as
count-weighted models sharing every read of X (cmtfpls_kfold_weighted_xcov_*, cmtfpls_kfold_inner_f64 or
cmtfpls_kfold_inner_coupled_f64, cmtfpls_kfold_epilogue_weighted_f64), against aligned literal refits on X[idx_b]; the weighted
epilogue entry against cmtfpls_kfold_epilogue_f64; the fallbacks."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, kfold, tPLS
from cmtf_pls_amd.bootstrap import aligned_factors
from cmtf_pls_amd.kfold import _from_scores, fold_ids
from cmtf_pls_amd.validate import bootstrap_factors

pytestmark = pytest.mark.gpu

_TOL = {"float64": 1e-8, "float32": 1e-5}


def _colwise(a, b):
    """max over columns of |a - b| / |b| (columns on the last axis)."""
    return float((np.linalg.norm(a - b, axis=-2) / np.maximum(np.linalg.norm(b, axis=-2), 1e-300)).max())


def _literal(m, Xs, y, idx):
    """The float64 literal refit of resample idx (a ctPLS when Xs is a list) with the fitted model's algorithm."""
    coupled = isinstance(Xs, list)
    r = (ctPLS if coupled else tPLS)(m.n_components, dtype="float64", algorithm=m._algorithm)
    r.fit([X[idx] for X in Xs] if coupled else Xs[idx], y[idx])
    return r


def _check_against_literal(m, Xs, y, res, tol):
    coupled = isinstance(Xs, list)
    for b, idx in enumerate(res["resamples"]):
        blocks, Q, coef = aligned_factors(m, _literal(m, Xs, y, idx))
        got = res["X_factors"] if coupled else [res["X_factors"]]
        for bi, modes in enumerate(blocks if coupled else [blocks]):
            for j, L in enumerate(modes):
                assert _colwise(got[bi][j][b], L) <= tol, (b, bi, j, _colwise(got[bi][j][b], L))
        assert _colwise(res["Y_loadings"][b], Q) <= tol, (b, _colwise(res["Y_loadings"][b], Q))
        assert _colwise(res["coef"][b], coef) <= tol, (b, _colwise(res["coef"][b], coef))


def _check_device_report(m, R, B, G, nb=None):
    rep = m.bootstrap_report_
    assert "cmtfpls_kfold_weighted_xcov_*" in rep["form"] and "cmtfpls_kfold_epilogue_weighted_f64" in rep["form"], rep
    assert "why" not in rep, rep
    passes = -(-B // G)
    assert rep["models_per_pass"] == G and rep["passes"] == passes and rep["resamples"] == B and len(rep["n_iter"]) == B
    assert rep["x_reads"] == (passes * 2 * R if nb is None else [passes * 2 * R] * nb)


# name, shape, M, R, B, resamples per pass
CASES = [
    ("order 2", (50, 30), 3, 3, 10, 10),
    ("order 3", (40, 10, 8), 4, 3, 12, 12),
    ("partial one-model pass", (60, 6, 5), 2, 2, 33, 32),
    ("M 1", (45, 9, 7), 1, 3, 6, 6),
    ("M 16 wide", (36, 64, 48), 16, 4, 5, 5),
]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name,shape,M,R,B,G", CASES, ids=[c[0] for c in CASES])
def test_device_resamples_equal_literal_refits(name, shape, M, R, B, G, dtype):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=7)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)
    m = tPLS(R, dtype=dtype)
    m.fit(x, y)
    res = bootstrap_factors(m, n_resamples=B, random_state=5)
    _check_device_report(m, R, B, G)
    assert res["coef"].shape == (B, R, R) and res["Y_loadings"].shape == (B, M, R) and np.all(np.isfinite(res["oob_q2y"]))
    _check_against_literal(m, x, y, res, _TOL[dtype])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_all_ones_counts_reproduce_the_fitted_model(dtype):
    x, y, _ = O.import_synthetic((48, 9, 7), 3, 4, error=0.3, seed=2)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)
    m = tPLS(3, dtype=dtype)
    m.fit(x, y)
    res = bootstrap_factors(m, resamples=np.tile(np.arange(48), (2, 1)))
    _check_device_report(m, 3, 2, 2)
    modes, Q, coef = aligned_factors(m, m)
    for b in range(2):
        for j, L in enumerate(modes):
            assert _colwise(res["X_factors"][j][b], L) <= _TOL[dtype]
        assert _colwise(res["Y_loadings"][b], Q) <= _TOL[dtype] and _colwise(res["coef"][b], coef) <= _TOL[dtype]
    assert res["oob_rows"] == 0 and np.all(np.isnan(res["oob_q2y"]))


def test_oob_q2y_equals_literal_refits_predictions():
    x, y, _ = O.import_synthetic((40, 8, 6), 3, 4, error=0.3, seed=3)
    R, I = 3, 40
    m = tPLS(R, dtype="float64")
    m.fit(x, y)
    res = bootstrap_factors(m, n_resamples=20, random_state=1)
    num, seen = np.zeros((R, I, 3)), np.zeros(I)
    for idx in res["resamples"]:
        oob = np.setdiff1d(np.arange(I), idx)
        if oob.size == 0:
            continue
        lit = _literal(m, x, y, idx)
        sc = lit.transform(x[oob])
        for r in range(1, R + 1):
            num[r - 1, oob] += _from_scores(sc, lit.coef_, lit.Y_factors[1].T, lit.Y_mean, r)
        seen[oob] += 1
    rows = seen > 0
    pred = num[:, rows] / seen[rows][None, :, None]
    want = 1 - ((pred - y[rows]) ** 2).reshape(R, -1).sum(axis=1) / (y[rows] ** 2).sum()
    assert res["oob_rows"] == int(rows.sum())
    np.testing.assert_allclose(res["oob_q2y"], want, rtol=0, atol=1e-10)


def _kfold_buffers(m, K, weighted):
    """The tPLS K-fold device form through kfold._state / kfold._components with kfold_epilogue, or (weighted) with
    kfold_epilogue_weighted on counts = the 0/1 training indicator of each fold; its buffers after the last component."""
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
    fold_of = (ids[None, :] != np.arange(K)[:, None]).astype(np.int32) if weighted else ids
    st, shared, own = kfold._state(be, t(fold_of, torch.int32), t(Yk), [(A, B, S, mean)], R, 1)
    assert kfold._components(be, [X2], st, shared, own, R, 1e-8, 100, False, weighted=weighted) is None
    torch.cuda.synchronize()
    return {**shared, **own[0]}


@pytest.mark.parametrize("shape,M,R,K", [((60, 10, 8), 4, 3, 5), ((37, 30), 2, 4, 3), ((40, 6, 5), 16, 2, 2)])
def test_weighted_epilogue_with_training_indicator_is_bitwise_kfold_epilogue(shape, M, R, K):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=4)
    m = tPLS(R, dtype="float64")
    m.fit(x, y)
    want = _kfold_buffers(m, K, False)
    got = _kfold_buffers(m, K, True)
    for f in ("T", "coef", "Q", "Gy", "vec", "S", "Yk", "n_iter", "status"):
        assert torch.equal(got[f], want[f]), f


def _coupled_data(dtype, I=61, seed=3):
    rng = np.random.default_rng(seed)
    L, M = 4, 4
    T = rng.standard_normal((I, L))
    Xs = [O.cp_factors_to_tensor([T, rng.standard_normal((10, L)), rng.standard_normal((8, L))]) + 0.3 * rng.standard_normal((I, 10, 8)),
          T @ rng.standard_normal((L, 12)) + 0.3 * rng.standard_normal((I, 12))]
    if dtype == "float32":
        Xs = [X.astype(np.float32).astype(np.float64) for X in Xs]
    return Xs, T @ rng.standard_normal((L, M)) + 0.3 * rng.standard_normal((I, M))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_coupled_tensor_and_matrix_blocks_equal_literal_refits(dtype):
    Xs, y = _coupled_data(dtype)
    R, B = 3, 9
    m = ctPLS(R, dtype=dtype)
    m.fit(Xs, y)
    res = bootstrap_factors(m, n_resamples=B, random_state=2)
    assert "cmtfpls_kfold_inner_coupled_f64" in m.bootstrap_report_["form"]
    _check_device_report(m, R, B, B, nb=2)
    assert [len(b) for b in res["X_factors"]] == [2, 1] and res["X_factors"][1][0].shape == (B, 12, R)
    _check_against_literal(m, Xs, y, res, _TOL[dtype])


def test_one_block_ctpls_is_bitwise_tpls():
    x, y, _ = O.import_synthetic((50, 9, 7), 3, 4, error=0.3, seed=8)
    t, c = tPLS(3, dtype="float64"), ctPLS(3, dtype="float64")
    t.fit(x, y)
    c.fit([x], y)
    a = bootstrap_factors(t, n_resamples=35, random_state=4)
    b = bootstrap_factors(c, n_resamples=35, random_state=4)
    assert "cmtfpls_kfold_inner_coupled_f64" in c.bootstrap_report_["form"] and "why" not in c.bootstrap_report_
    assert all(np.array_equal(p, q) for p, q in zip(a["X_factors"], b["X_factors"][0]))
    for key in ("Y_loadings", "coef", "oob_q2y"):
        assert np.array_equal(a[key], b[key]), key
    assert t.bootstrap_report_["n_iter"] == c.bootstrap_report_["n_iter"]


@pytest.mark.parametrize("case", ["nan", "order 4", "M 65", "switched off"])
def test_fallbacks_refit_with_a_reason(case):
    rng = np.random.default_rng(6)
    shape, M = {"order 4": ((30, 4, 3, 3), 2), "M 65": ((30, 5, 4), 65)}.get(case, ((30, 5, 4), 2))
    x = rng.standard_normal(shape)
    y = x.reshape(30, -1)[:, :M] @ np.eye(M) + 0.1 * rng.standard_normal((30, M)) if M <= x[0].size else rng.standard_normal((30, M))
    if case == "nan":
        x[3, 1, 2] = np.nan
    m = tPLS(2, dtype="float64")
    m.fit(x, y)
    res = bootstrap_factors(m, n_resamples=3, random_state=0, device_folds=case != "switched off")
    rep = m.bootstrap_report_
    assert rep["form"] == "one refit per resample on the regular engine" and rep["passes"] == 0 and rep["why"], rep
    if case != "nan":
        assert np.all(np.isfinite(res["coef"]))
    if case == "switched off":
        dev = bootstrap_factors(m, n_resamples=3, random_state=0)
        assert "why" not in m.bootstrap_report_
        for key in ("Y_loadings", "coef"):
            assert _colwise(dev[key], res[key]) <= 1e-8, key
        for p, q in zip(dev["X_factors"], res["X_factors"]):
            assert _colwise(p, q) <= 1e-8
        np.testing.assert_allclose(dev["oob_q2y"], res["oob_q2y"], rtol=0, atol=1e-8)


def test_callers_device_tensor_is_only_read():
    I, J, K, M, R = 2048, 24, 20, 4, 3
    g = torch.Generator(device="cuda:0").manual_seed(3)
    T = torch.randn(I, R, device="cuda:0", dtype=torch.float64, generator=g)
    X = torch.einsum("il,jl,kl->ijk", T, torch.randn(J, R, device="cuda:0", dtype=torch.float64, generator=g),
                     torch.randn(K, R, device="cuda:0", dtype=torch.float64, generator=g)).to(torch.float32)
    X += 0.5 * torch.randn(I, J, K, device="cuda:0", dtype=torch.float32, generator=g)
    Y = T @ torch.randn(M, R, device="cuda:0", dtype=torch.float64, generator=g).T
    before = X.clone()
    m = tPLS(R, dtype="float32")
    m.fit(X, Y)
    res = bootstrap_factors(m, n_resamples=40, random_state=0)
    torch.cuda.synchronize()
    assert "why" not in m.bootstrap_report_ and m.bootstrap_report_["passes"] == 2
    assert torch.equal(X, before)
    assert res["X_factors"][0].shape == (40, J, R) and np.all(np.isfinite(res["oob_q2y"]))
