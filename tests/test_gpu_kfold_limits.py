"""The device cross-validation family at the limits it declares (kfold.MAX_FOLDS, MAX_RESPONSES, MAX_COMPONENTS, MAX_SIDE = 32, 64,
64, 256; W = 1024 columns of the wide and weighted builds): the first-pass kernels (cmtfpls_kfold_xcov_*,
cmtfpls_kfold_weighted_xcov_*) against float64 torch at every template instance and on both sides of each boundary, then K-fold,
coupled K-fold, the permutation test, repeated K-fold and the bootstrap at those sizes against literal refits on the regular engine,
and the declines just past each limit.  Every end-to-end test also checks that the device form ran (its report), so a silent
decline cannot turn it into refits compared with refits."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, kfold, tPLS
from cmtf_pls_amd.bootstrap import aligned_factors
from cmtf_pls_amd.kfold import fold_ids
from cmtf_pls_amd.validate import bootstrap_factors, get_q2y_kfold, get_q2y_repeated_kfold, kfold_predictions, permutation_test_q2y

pytestmark = pytest.mark.gpu

_TOL = {"float64": 1e-8, "float32": 1e-7}                     # test_gpu_kfold.py, test_gpu_permutation.py
_TOL_BOOT = {"float64": 1e-8, "float32": 1e-5}                # test_gpu_bootstrap.py
_DEV = "cuda:0"


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(np.abs(np.asarray(want)).max(), 1e-300))


def _backend():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(_DEV))


def _as_view(X, base):
    """X itself (base 0), or a copy of it `base` elements into a larger buffer: contiguous, but its data pointer is not aligned
    to the 16 bytes of a four-element vector load."""
    if not base:
        return X
    I, P = X.shape
    buf = torch.zeros(base + I * P, device=X.device, dtype=X.dtype)
    buf[base:].view(I, P).copy_(X)
    V = buf[base:].view(I, P)
    assert V.is_contiguous() and V.data_ptr() % 16 != 0
    return V


# ---- first pass: cmtfpls_kfold_xcov_* ---------------------------------------------------------------------------------------
# (I, A, B, M, K, folds): every instance of kfold_partials_kernel (M <= 8, 16, 32, 64) on both sides of each boundary; K 2, 5 and
# 32 with uneven and shuffled folds; one row chunk (I / K < 128) and the cap of 64 (I / K >= 4096, P <= 256, K = 2); fold
# lengths neither multiples of 4 nor of the chunk count; P < 256, P = 256 and a partial 256-column block (33 x 40)
XCOV_CASES = [
    (70, 1, 30, 1, 2, "contiguous"),          # one chunk, order 2
    (203, 7, 9, 8, 5, "shuffled"),
    (517, 33, 40, 9, 5, "shuffled"),          # P = 1320: five 256-column blocks and a partial one
    (301, 16, 16, 16, 32, "uneven"),          # P = 256
    (8195, 16, 16, 17, 2, "contiguous"),      # 64 chunks of folds of 4098 and 4097 rows
    (999, 5, 20, 32, 32, "shuffled"),
    (1234, 12, 11, 33, 5, "uneven"),
    (600, 9, 8, 64, 3, "shuffled"),
]


def _fold_split(I, K, kind, seed):
    if kind == "contiguous":
        return fold_ids(I, K)
    ids = np.arange(I) % K
    if kind == "uneven":                     # fold 0 takes a run of extra rows from the others; no fold empties
        ids[: I // 3] = np.where(np.arange(I // 3) % 3 == 0, ids[: I // 3], 0)
    return fold_ids(I, folds=np.random.default_rng(seed).permutation(ids))


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("xdtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("I,A,B,M,K,kind", XCOV_CASES)
def test_kfold_xcov_against_float64_torch(I, A, B, M, K, kind, xdtype, base):
    be = _backend()
    g = torch.Generator(device=_DEV).manual_seed(I + M)
    P = A * B
    X = _as_view((torch.randn(I, P, device=_DEV, dtype=torch.float64, generator=g) + 0.3).to(xdtype), base)
    Y = torch.randn(I, M, device=_DEV, dtype=torch.float64, generator=g)
    ydev = torch.randn(K, M, device=_DEV, dtype=torch.float64, generator=g)
    ids, K = _fold_split(I, K, kind, I)
    counts = np.bincount(ids, minlength=K)
    assert counts.min() >= 1
    order = torch.from_numpy(np.argsort(ids, kind="stable").astype(np.int32)).to(_DEV)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(_DEV)
    before = X.clone()
    S, mean = torch.empty(K, M, P, device=_DEV, dtype=torch.float64), torch.empty(K, P, device=_DEV, dtype=torch.float64)
    stats = be.kfold_xcov(X, A, B, Y, order, off, K, ydev, S, mean)
    assert stats is not None
    S2, mean2 = torch.empty_like(S), torch.empty_like(mean)
    stats2 = be.kfold_xcov(X, A, B, Y, order, off, K, ydev, S2, mean2)
    assert torch.equal(S, S2) and torch.equal(mean, mean2) and torch.equal(stats, stats2)    # the same bits on every run
    assert torch.equal(X, before)
    X64 = X.to(torch.float64)
    idt = torch.from_numpy(ids).to(_DEV)
    Sf = torch.stack([X64[idt == f].T @ Y[idt == f] for f in range(K)])                      # P x M per fold
    for k in range(K):
        ntr = I - int(counts[k])
        mu = X64[idt != k].sum(0) / ntr
        want = (Sf.sum(0) - Sf[k]).T - ntr * ydev[k][:, None] * mu[None, :]
        assert float((S[k] - want).abs().max()) <= 1e-12 * float(want.abs().max()), k
        assert float((mean[k] - mu).abs().max()) <= 1e-13 * float(mu.abs().max()), k
    assert float((stats[:P] - X64.sum(0)).abs().max()) <= 1e-12 * float(X64.sum(0).abs().max())
    assert float((stats[P:] - (X64 * X64).sum(0)).abs().max()) <= 1e-12 * float((X64 * X64).sum(0).max())


# ---- first pass of the bootstrap: cmtfpls_kfold_weighted_xcov_* --------------------------------------------------------------
# (I, A, B, M, n): W = n (M + 1) over every MFMA tile count mt = 1..4 of kfold_wide_kernel, more than one 64-column block of Y''
# (nyb > 1), W = 975 (n = 15, M = 64: bootstrap.py's pass at M = 64) and W = 1024 (n = 32, M = 31); P % 4 != 0 (the scalar
# instance) and P % 4 == 0 (VEC); I large enough for several row chunks
WEIGHTED_CASES = [
    (300, 7, 9, 3, 2),                        # W = 8: mt 1, P = 63
    (300, 4, 8, 6, 4),                        # W = 28: mt 2, P = 32
    (517, 1, 130, 8, 5),                      # W = 45: mt 3, P = 130
    (2000, 8, 8, 9, 6),                       # W = 60: mt 4, P = 64
    (700, 12, 20, 16, 5),                     # W = 85: two Y'' blocks, P = 240
    (2000, 33, 40, 64, 15),                   # W = 975, P = 1320
    (1500, 7, 13, 31, 32),                    # W = 1024, P = 91
    (1500, 8, 16, 31, 32),                    # W = 1024, P = 128
]


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("xdtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("I,A,B,M,n", WEIGHTED_CASES)
def test_kfold_weighted_xcov_against_float64_torch(I, A, B, M, n, xdtype, base):
    be = _backend()
    g = torch.Generator(device=_DEV).manual_seed(I + n * M)
    P = A * B
    X = _as_view((torch.randn(I, P, device=_DEV, dtype=torch.float64, generator=g) + 0.3).to(xdtype), base)
    Yd = torch.randn(I, M, device=_DEV, dtype=torch.float64, generator=g)
    idx = np.random.default_rng(n * M).integers(0, I, size=(n, I))                            # real bootstrap draws
    counts = np.stack([np.bincount(r, minlength=I) for r in idx])
    assert (counts == 0).any() and (counts == 1).any() and (counts >= 2).any()
    C = torch.from_numpy(counts.astype(np.int32)).to(_DEV)
    Cf = C.to(torch.float64)
    nu = (Cf @ Yd) / I                                                                         # Y'' as bootstrap.py builds it
    Yc = Yd.unsqueeze(0) - nu.unsqueeze(1)
    Yw = torch.cat([(Cf.unsqueeze(2) * Yc).permute(1, 0, 2).reshape(I, n * M), Cf.t()], dim=1).contiguous()
    before = X.clone()
    S, mean = torch.empty(n, M, P, device=_DEV, dtype=torch.float64), torch.empty(n, P, device=_DEV, dtype=torch.float64)
    stats = be.kfold_weighted_xcov(X, A, B, Yw, n, M, S, mean)
    assert stats is not None
    S2, mean2 = torch.empty_like(S), torch.empty_like(mean)
    stats2 = be.kfold_weighted_xcov(X, A, B, Yw, n, M, S2, mean2)
    assert torch.equal(S, S2) and torch.equal(mean, mean2) and torch.equal(stats, stats2)
    assert torch.equal(X, before)
    X64 = X.to(torch.float64)
    for b in range(n):
        want = (Cf[b].unsqueeze(1) * (Yd - nu[b])).T @ X64                                    # S_b = X^T (c_b * (Y - nu_b))
        assert float((S[b] - want).abs().max()) <= 1e-12 * float(want.abs().max()), b
        mu = X64.T @ Cf[b] / I
        assert float((mean[b] - mu).abs().max()) <= 1e-13 * float(mu.abs().max()), b
    assert float((stats[:P] - X64.sum(0)).abs().max()) <= 1e-12 * float(X64.sum(0).abs().max())
    assert float((stats[P:] - (X64 * X64).sum(0)).abs().max()) <= 1e-12 * float((X64 * X64).sum(0).max())


# ---- K-fold tPLS at the limits ----------------------------------------------------------------------------------------------
def _refit(x, y, train, test, R, dtype):
    """A literal refit of one fold: (predictions of the test rows with the first r components for r = 1..R, n_iter_)."""
    m = tPLS(R, dtype=dtype)
    m.fit(x[train], y[train])
    s = m.transform(x[test])
    Qr = m.Y_factors[1].T
    preds = [(s[:, :r] @ m.coef_[:r, :r]) @ Qr[:r] + m.Y_mean for r in range(1, R + 1)]
    return np.stack(preds), list(m.n_iter_)


def _check_against_refits(rep, x, y, pred, ids, R, dtype, folds_to_check, refit_dtype):
    for k in folds_to_check:
        test = ids == k
        want, n_iter = _refit(x, y, ~test, test, R, refit_dtype)
        got = pred.reshape(R, y.shape[0], -1)[:, test]
        assert _rel(got, want.reshape(got.shape)) <= _TOL[dtype], (k, _rel(got, want.reshape(got.shape)))
        assert rep["n_iter"][k] == n_iter, (k, rep["n_iter"][k], n_iter)


# name, shape, M, R, K, folds checked against refits (None: all).  The refits have the model's storage type, but at R = 64 a
# float32 model is checked against the float64 refit of the same (float32-representable) data: the float32 refit deflates X in
# its float32 storage after every component, and over 64 components, the late ones fitted to noise with small gaps between
# singular values, that rounding moves its predictions by ~4e-5 relative.  The device form never writes X and works in float64
# throughout, which is what the float64 refit of the same data computes.
KFOLD_CASES = [
    ("M 17", (60, 10, 8), 17, 3, 4, None),
    ("M 33", (50, 30), 33, 3, 5, None),
    ("M 64", (60, 10, 8), 64, 4, 3, None),
    ("R 64", (200, 10, 12), 4, 64, 3, (0,)),                   # 133 training rows, P = 120: T_train of rank 64
    ("R 32 M 64 row tiles", (3001, 6, 8), 64, 32, 5, (2,)),    # 12 row tiles of 251 rows, 9 row chunks per fold
    ("K 32 uneven", (70, 12, 9), 5, 4, 32, (0, 5, 6, 31)),     # six folds of 3 rows, 26 of 2
    ("side 256", (40, 256, 260), 3, 2, 3, (1,)),
]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name,shape,M,R,K,check", KFOLD_CASES, ids=[c[0] for c in KFOLD_CASES])
def test_kfold_at_the_limits_equals_literal_refits(name, shape, M, R, K, check, dtype):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=7)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)
    m = tPLS(R, dtype=dtype)
    m.fit(x, y)
    pred = kfold_predictions(m, n_splits=K)
    rep = m.q2y_report_
    assert "cmtfpls_kfold_inner_f64" in rep["form"] and "why" not in rep, rep
    assert rep["x_reads"] == 2 * R and rep["folds"] == K and np.array(rep["n_iter"]).shape == (K, R)
    ids, K = fold_ids(shape[0], K)
    refit_dtype = "float64" if R == kfold.MAX_COMPONENTS else dtype
    _check_against_refits(rep, x, y, pred, ids, R, dtype, range(K) if check is None else check, refit_dtype)


@pytest.mark.parametrize("case,why", [("R 65", "R = 65 components > 64"), ("side 257", "min(J, K) = 257 > 256")])
def test_kfold_declines_just_past_the_limits(case, why):
    shape, M, R, K = ((160, 10, 12), 4, 65, 2) if case == "R 65" else ((30, 257, 258), 3, 2, 2)
    x, y, _ = O.import_synthetic(shape, M, min(R + 1, 8), error=0.3, seed=12)
    m = tPLS(R, dtype="float64")
    m.fit(x, y)
    pred = kfold_predictions(m, n_splits=K)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and rep.get("why") == why, rep
    ids, K = fold_ids(shape[0], K)
    want = np.zeros((R,) + y.shape)
    for k in range(K):
        test = ids == k
        want[:, test] = _refit(x, y, ~test, test, R, "float64")[0].reshape((R, int(test.sum())) + y.shape[1:])
    assert _rel(pred, want) <= 1e-10


# ---- coupled K-fold at M = 64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_coupled_kfold_at_64_responses_equals_literal_refits(dtype):
    rng = np.random.default_rng(7)
    I, M, R, K = 90, 64, 24, 3
    L = R + 1
    T = rng.standard_normal((I, L))
    Xs = [O.cp_factors_to_tensor([T, rng.standard_normal((10, L)), rng.standard_normal((8, L))]) + 0.3 * rng.standard_normal((I, 10, 8)),
          T @ rng.standard_normal((L, 40)) + 0.3 * rng.standard_normal((I, 40))]     # both blocks of rank >= R on 60 training rows
    if dtype == "float32":
        Xs = [X.astype(np.float32).astype(np.float64) for X in Xs]
    y = T @ rng.standard_normal((L, M)) + 0.3 * rng.standard_normal((I, M))
    m = ctPLS(R, dtype=dtype)
    m.fit(Xs, y)
    pred = kfold_predictions(m, n_splits=K)
    rep = m.q2y_report_
    assert "cmtfpls_kfold_inner_coupled_f64" in rep["form"] and "why" not in rep, rep
    assert rep["x_reads"] == [2 * R] * 2 and rep["folds"] == K
    ids, K = fold_ids(I, K)
    test = ids == 1
    r = ctPLS(R, dtype=dtype)
    r.fit([X[~test] for X in Xs], y[~test])
    s = r.transform([X[test] for X in Xs])
    want = np.stack([(s[:, :c] @ r.coef_[:c, :c]) @ r.Y_factors[1].T[:c] + r.Y_mean for c in range(1, R + 1)])
    assert _rel(pred[:, test], want) <= _TOL[dtype], _rel(pred[:, test], want)
    assert rep["n_iter"][1] == list(r.n_iter_), (rep["n_iter"][1], list(r.n_iter_))


# ---- permutation test: 16 permutations x 2 folds, W = 16 x 64 = 1024 ------------------------------------------------------------
def _refit_q2y(x, y, ids, K, R, dtype):
    """(Q2Y of every component count, n_iter per fold) from one literal refit per fold."""
    pred = np.zeros((R,) + y.shape)
    n_iter = []
    for k in range(K):
        test = ids == k
        p, it = _refit(x, y, ~test, test, R, dtype)
        pred[:, test] = p.reshape((R, int(test.sum())) + y.shape[1:])
        n_iter.append(it)
    return 1 - ((pred - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum(), n_iter


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_permutation_null_at_1024_columns_equals_literal_refits(dtype):
    x, y, _ = O.import_synthetic((60, 10, 8), 64, 4, error=0.3, seed=7)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)
    R, K, NP = 3, 2, 16
    m = tPLS(R, dtype=dtype)
    m.fit(x, y)
    res = permutation_test_q2y(m, n_permutations=NP, n_splits=K, random_state=3, per_component=True)
    rep = m.q2y_report_
    assert "cmtfpls_kfold_wide_xcov" in rep["form"] and "why" not in rep, rep
    assert rep["passes"] == 1 and rep["models_per_pass"] == 32 and rep["permutations"] == NP and rep["x_reads"] == 2 * R
    ids, K = fold_ids(60, K)
    for p in (0, NP - 1):                                       # the first and the last 64 columns of Y'
        pi = res["permutations"][p]
        want, n_iter = _refit_q2y(x, y[pi], ids, K, R, dtype)
        err = np.abs(res["null"][p] - want).max() / max(1.0, np.abs(want).max())
        assert err <= _TOL[dtype], (p, err, res["null"][p], want)
        assert rep["n_iter"][p] == n_iter, (p, rep["n_iter"][p], n_iter)


# ---- repeated K-fold: 16 splits x 2 folds = 32 models per pass at M = 33 ------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_repeated_kfold_with_32_models_per_pass(dtype):
    x, y, _ = O.import_synthetic((48, 9, 7), 33, 4, error=0.3, seed=7)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)
    R, K, S = 3, 2, 16
    m = tPLS(R, dtype=dtype)
    m.fit(x, y)
    res = get_q2y_repeated_kfold(m, n_splits=K, n_repeats=S, random_state=5, per_component=True)
    rep = m.q2y_report_
    assert "cmtfpls_kfold_epilogue_splits_f64" in rep["form"] and "why" not in rep, rep
    assert rep["splits_per_pass"] == 16 and rep["passes"] == 1 and rep["x_reads"] == S + 2 * R - 1
    for g in (0, S - 1):
        want, n_iter = _refit_q2y(x, y, res["folds"][g], K, R, dtype)
        err = np.abs(res["q2y"][g] - want).max() / max(1.0, np.abs(want).max())
        assert err <= _TOL[dtype], (g, err, res["q2y"][g], want)
        assert rep["n_iter"][g] == n_iter, (g, rep["n_iter"][g], n_iter)
    for g in range(S):                                          # every split against the device K-fold of that split
        q = get_q2y_kfold(m, folds=res["folds"][g], per_component=True)
        assert "cmtfpls_kfold_inner_f64" in m.q2y_report_["form"] and "why" not in m.q2y_report_
        assert np.abs(res["q2y"][g] - q).max() <= 1e-12 * max(1.0, np.abs(q).max()), g


# ---- bootstrap: M = 64 (15 resamples, W = 975) and M = 31 (32 resamples, W = 1024) ------------------------------------------------
def _colwise(a, b):
    """max over columns of |a - b| / |b| (columns on the last axis)."""
    return float((np.linalg.norm(a - b, axis=-2) / np.maximum(np.linalg.norm(b, axis=-2), 1e-300)).max())


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape,M,G", [((40, 9, 7), 64, 15), ((50, 9, 7), 31, 32)], ids=["M 64", "M 31"])
def test_bootstrap_at_1024_columns_equals_literal_refits(shape, M, G, dtype):
    x, y, _ = O.import_synthetic(shape, M, 4, error=0.3, seed=7)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)
    R = 3
    m = tPLS(R, dtype=dtype)
    m.fit(x, y)
    res = bootstrap_factors(m, n_resamples=G, random_state=5)
    rep = m.bootstrap_report_
    assert "cmtfpls_kfold_weighted_xcov_*" in rep["form"] and "cmtfpls_kfold_epilogue_weighted_f64" in rep["form"], rep
    assert "why" not in rep and rep["models_per_pass"] == G and rep["passes"] == 1 and rep["x_reads"] == 2 * R, rep
    tol = _TOL_BOOT[dtype]
    for b, idx in enumerate(res["resamples"]):
        r = tPLS(R, dtype="float64")
        r.fit(x[idx], y[idx])
        modes, Q, coef = aligned_factors(m, r)
        for j, L in enumerate(modes):
            assert _colwise(res["X_factors"][j][b], L) <= tol, (b, j, _colwise(res["X_factors"][j][b], L))
        assert _colwise(res["Y_loadings"][b], Q) <= tol, (b, _colwise(res["Y_loadings"][b], Q))
        assert _colwise(res["coef"][b], coef) <= tol, (b, _colwise(res["coef"][b], coef))
