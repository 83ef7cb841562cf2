"""Cross-validation of a ctPLS whose blocks have missing values, every model refitted by one workgroup
(cmtfpls_cv_masked_coupled_f64, EngineOptions.masked_folds_coupled): one model against the NumPy restatement (coupled_masked_ref),
one block equal to cmtfpls_cv_masked_models_f64, chunks of models; then K-fold, leave-one-out, the permutation test, repeated K-fold
and the bootstrap against literal refits on the regular engine, where the per-block masked arithmetic switches on and off, the
status paths, the declared limits and one step past them, the declines, and a float32 model.  Every end-to-end test checks the
report's form and that nothing was refitted, so a silent decline cannot compare refits with refits.  The bound is the family's:
1e-10 relative (tests/test_gpu_cv_masked.py).  In the parity cases every row keeps an observed entry in every block (asserted by
_coupled_data), so the data alone gives no model a status."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import (COUPLED_FORM, coupled_lds_bytes, fold_ids, masked_coupled_report, masked_fold_numerators,
                                masked_models_coupled, masked_predictions_coupled, refit_fold, refit_predictions)
from cmtf_pls_amd.validate import bootstrap_factors, get_q2y_kfold, get_q2y_repeated_kfold, kfold_predictions, permutation_test_q2y
from coupled_masked_ref import coupled_masked_fit

pytestmark = pytest.mark.gpu

_DEV = "cuda:0"
ON = EngineOptions(small_fit=False, masked_folds_coupled=True)
OFF = EngineOptions(small_fit=False)
LDS_CAP = 150 * 1024
BOUND = 1e-10

TM = [(6, 5), (7,)]                    # tensor + matrix
TT = [(6, 5), (4, 7)]                  # tensor + tensor
TMT = [(4, 5), (6,), (3, 3)]           # three blocks


def _coupled_data(I, trailing, M, L, seed, nan=(0.1,)):
    """Blocks (I, *trailing[b]) driven by one latent score and a Y of M responses; nan[b] of block b's entries missing (the last
    value repeats).  Every row keeps an observed entry in every block: asserted."""
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((I, L))
    Xs = []
    for b, tr in enumerate(trailing):
        shape = (I,) + tuple(tr)
        X = O.cp_factors_to_tensor([T] + [rng.standard_normal((d, L)) for d in tr]) + 0.3 * rng.standard_normal(shape)
        frac = nan[min(b, len(nan) - 1)]
        if frac:
            hole = rng.random(shape) < frac
            hole.reshape(I, -1)[:, b % int(np.prod(tr))] = False
            X[hole] = np.nan
        assert (~np.isnan(X).reshape(I, -1)).sum(axis=1).min() >= 1
        Xs.append(X)
    Y = T @ rng.standard_normal((L, M)) + 0.3 * rng.standard_normal((I, M))
    return Xs, Y


def _pair(Xs, y, R, dtype="float64"):
    on, off = ctPLS(R, dtype=dtype, options=ON), ctPLS(R, dtype="float64", options=OFF)
    on.fit(Xs, y)
    off.fit(Xs, y)
    return on, off


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float(np.abs(got[ok] - want[ok]).max() / max(np.abs(want[ok]).max(), 1e-300)) if ok.any() else 0.0


def _col_rel(got, want):
    """Normwise relative error of the worst column (last axis) of a stack."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    g, w = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    return float(max(np.linalg.norm(g[:, j] - w[:, j]) / max(np.linalg.norm(w[:, j]), 1e-300) for j in range(w.shape[1])))


def _coupled(rep, models=None):
    """The report of a run that the coupled masked form took whole."""
    assert COUPLED_FORM in rep["form"], rep
    assert rep["refitted"] == [] and "why" not in rep, rep
    assert rep["x_reads"] is None and rep["launches"] >= 1, rep
    if models is not None:
        assert rep["models"] == models, rep
    return rep


def _leaves(tree):
    return [a for t in tree for a in _leaves(t)] if isinstance(tree, (list, tuple)) else [tree]


def _refit_kfold(Xs, y, ids, K, R):
    """Literal per-fold refits on the regular engine, every component count: (R, I, M)."""
    want = np.zeros((R,) + y.shape)
    for k in range(K):
        test = ids == k
        r = ctPLS(R, dtype="float64", options=OFF)
        r.fit([X[~test] for X in Xs], y[~test])
        sc = r.transform([X[test] for X in Xs])
        for c in range(1, R + 1):
            want[c - 1, test] = (sc[:, :c] @ r.coef_[:c, :c]) @ r.Y_factors[1][:, :c].T + r.Y_mean
    return want


def _backend():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(_DEV))


def _dev(a, dt=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=_DEV, dtype=dt)


def _kernel(be, Xs, y, counts, yrow, R, **kw):
    I = y.shape[0]
    dims = [(X.ndim, 1, X.shape[1]) if X.ndim == 2 else (3, X.shape[1], X.shape[2]) for X in Xs]
    return be.cv_masked_coupled([_dev(X.reshape(I, -1)) for X in Xs], dims, _dev(y.reshape(I, -1)), _dev(counts, torch.int32),
                                None if yrow is None else _dev(yrow, torch.int32), R, 1e-8, 100, **kw)


# ---- 1. kernel level -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trailing,nan", [(TM, (0.1,)), (TT, (0.1, 0.0)), (TMT, (0.0, 0.1, 0.1)), (TM, (0.0,))])
def test_one_model_equals_the_numpy_restatement(trailing, nan):
    I, M, R = 30, 2, 3
    Xs, y = _coupled_data(I, trailing, M, R + 1, seed=30, nan=nan)
    rng = np.random.default_rng(31)
    counts = rng.integers(0, 4, size=(3, I)).astype(np.int32)
    counts[:, :3] = 0
    counts[2] = (counts[2] > 0)                                            # a 0/1 model
    yrow = np.stack([np.arange(I), rng.permutation(I), np.arange(I)]).astype(np.int32)
    got = _kernel(_backend(), Xs, y, counts, yrow, R, factors=True)
    assert got["launches"] == 1 and not got["status"].any()
    for j in range(3):
        loadings, Q, coef, pred, n_iter, info = coupled_masked_fit(Xs, y, counts[j], R, yrow[j])
        assert got["n_iter"][j].tolist() == n_iter and got["info"][j].tolist() == list(info)
        held = counts[j] == 0
        print("model", j, "Ypred", _rel(got["Ypred"][j][:, held].cpu(), pred), "Q", _col_rel(got["Q"][j].cpu().numpy().T, Q))
        assert _rel(got["Ypred"][j][:, held].cpu(), pred) <= BOUND
        assert not got["Ypred"][j][:, ~held].any()                         # written at held-out rows only
        assert _col_rel(got["Q"][j].cpu().numpy().T, Q) <= BOUND
        assert np.abs(got["coef"][j].cpu().numpy() - coef).max() <= BOUND * np.abs(coef).max()
        for b, X in enumerate(Xs):
            modes = [got["Wb"][b][j]] if X.ndim == 2 else [got["Wa"][b][j], got["Wb"][b][j]]
            for L, Lw in zip(modes, loadings[b]):
                assert _col_rel(L.cpu().numpy().T, Lw) <= BOUND, (j, b)


@pytest.mark.parametrize("shape", [(26, 6, 5), (26, 9)])
def test_one_block_equals_the_tpls_kernel(shape):
    be = _backend()
    I, M, R = shape[0], 3, 3
    (x,), y = _coupled_data(I, [shape[1:]], M, R + 1, seed=47)
    ids, K = fold_ids(I, 4)
    counts = (ids[None, :] != np.arange(K)[:, None]).astype(np.int32)
    A, B = (1, shape[1]) if len(shape) == 2 else shape[1:]
    want = be.cv_masked_models(_dev(x.reshape(I, -1)), _dev(y), _dev(counts, torch.int32), None, A, B, R, 1e-8, 100, factors=True)
    got = _kernel(be, [x], y, counts, None, R, factors=True)
    assert not got["status"].any() and torch.equal(got["status"], want["status"])
    assert torch.equal(got["n_iter"], want["n_iter"]) and torch.equal(got["info"], want["info"])
    # the two kernels run the same steps (csrc/masked_fold.hpp); what one block adds, 0.0 + s and * 1.0, is exact
    for key, g in (("Ypred", got["Ypred"]), ("Wa", got["Wa"][0]), ("Wb", got["Wb"][0]), ("coef", got["coef"]), ("Q", got["Q"])):
        g, w = g.cpu().numpy(), want[key].cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g, w, equal_nan=True), key


def test_chunked_launches_are_bit_identical():
    be = _backend()
    I, M, R = 36, 3, 3
    Xs, y = _coupled_data(I, TMT, M, R + 1, seed=79)
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 3, size=(9, I)).astype(np.int32)
    yrow = np.stack([rng.permutation(I) for _ in range(9)]).astype(np.int32)
    one = _kernel(be, Xs, y, counts, yrow, R, factors=True)
    assert one["launches"] == 1
    from cmtf_pls_amd import _lib
    blocks = (_lib.CvCoupledBlock * 3)(*[_lib.CvCoupledBlock(None, X.ndim, 1 if X.ndim == 2 else X.shape[1], X.shape[-1]) for X in Xs])
    per = int(be.lib.cmtfpls_cv_masked_coupled_workspace_bytes(blocks, 3, I, M, R))
    assert per == 8 * (sum((I + 2) * int(np.prod(X.shape[1:])) for X in Xs) + I * M + I * R)
    per += R * I * M * 8
    for budget, launches in ((per, 9), (2 * per, 5), (4 * per + 7, 3)):
        many = _kernel(be, Xs, y, counts, yrow, R, factors=True, max_ws_bytes=budget)
        assert many["launches"] == launches
        for key, v in one.items():
            for a, b in zip(_leaves(v), _leaves(many[key])):
                if isinstance(a, torch.Tensor):
                    assert torch.equal(a, b), key


# ---- 2. K-fold and leave-one-out -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trailing,folds", [(TM, None), (TT, "shuffled"), (TMT, None)])
def test_kfold_equals_refits_for_every_component_count(trailing, folds):
    I, M, R, K = 30, 2, 3, 4
    Xs, y = _coupled_data(I, trailing, M, R + 1, seed=I + len(trailing))
    if folds == "shuffled":
        folds = np.random.default_rng(2).permutation(np.arange(I) % K)
        folds[:3] = 0                                                      # unequal fold sizes
    on, _ = _pair(Xs, y, R)
    pred = kfold_predictions(on, n_splits=K, folds=folds)
    rep = _coupled(on.q2y_report_, models=K)
    assert rep["folds"] == K and np.asarray(rep["n_iter"]).shape == (K, R)
    assert rep["masked_blocks"] == [K] * len(Xs) and rep["masked_batches"] == [K] * len(Xs), rep
    ids, _ = fold_ids(I, K, folds)
    want = _refit_kfold(Xs, y, ids, K, R)
    assert np.isfinite(want).all()
    print("kfold", _rel(pred, want))
    assert _rel(pred, want) <= BOUND


def test_leave_one_out_equals_refits():
    I, M, R = 24, 2, 3
    Xs, y = _coupled_data(I, TM, M, R + 1, seed=24)
    on, off = _pair(Xs, y, R)
    got = get_q2y_kfold(on, n_splits=I, per_component=True)
    _coupled(on.q2y_report_, models=I)
    want = get_q2y_kfold(off, n_splits=I, per_component=True)
    assert off.q2y_report_["form"] == "one refit per fold on the regular engine"
    assert np.isfinite(want).all()
    print("loo", _rel(got, want))
    assert _rel(got, want) <= BOUND
    assert _rel(kfold_predictions(on, n_splits=I), _refit_kfold(Xs, y, np.arange(I), I, R)) <= BOUND


def test_nan_in_one_block_only_keeps_the_other_unmasked():
    I, M, R, K = 28, 2, 3, 4
    Xs, y = _coupled_data(I, TM, M, R + 1, seed=28, nan=(0.0, 0.1))
    on, _ = _pair(Xs, y, R)
    pred = kfold_predictions(on, n_splits=K)
    rep = _coupled(on.q2y_report_, models=K)
    assert rep["masked_blocks"] == [0, K] and rep["masked_batches"] == [0, K], rep
    assert _rel(pred, _refit_kfold(Xs, y, fold_ids(I, K)[0], K, R)) <= BOUND


def test_nan_only_in_rows_a_fold_holds_out():
    I, M, R, K = 24, 2, 2, 4
    Xs, y = _coupled_data(I, TM, M, R + 1, seed=61, nan=(0.0,))
    Xs[0][1, 2, 2] = np.nan                                               # fold 0 holds out rows 0..5
    Xs[1][3, 4] = np.nan
    on, _ = _pair(Xs, y, R)
    out, why = masked_models_coupled(on, Xs, y, (fold_ids(I, K)[0][None, :] != np.arange(K)[:, None]).astype(np.int32), None, 1e-8, 100)
    assert why is None and out["info"].tolist() == [[0, 3], [3, 0], [3, 0], [3, 0]]
    pred = kfold_predictions(on, n_splits=K)
    rep = _coupled(on.q2y_report_, models=K)
    assert rep["masked_blocks"] == [K - 1, K - 1] and rep["masked_batches"] == [1, 1], rep
    assert _rel(pred, _refit_kfold(Xs, y, fold_ids(I, K)[0], K, R)) <= BOUND


# ---- 3. permutation test, repeated K-fold, bootstrap ----------------------------------------------------------------------------
@pytest.mark.parametrize("trailing", [TM, TMT])
def test_permutation_test_equals_refits(trailing):
    I, M, R = 30, 2, 3
    Xs, y = _coupled_data(I, trailing, M, R + 1, seed=33)
    on, off = _pair(Xs, y, R)
    got = permutation_test_q2y(on, n_permutations=5, n_splits=4, per_component=True)
    rep = _coupled(on.q2y_report_, models=20)
    assert rep["permutations"] == 5 and np.asarray(rep["n_iter"]).shape == (5, 4, 3)
    _coupled(rep["observed"], models=4)
    want = permutation_test_q2y(off, n_permutations=5, n_splits=4, per_component=True)
    assert off.q2y_report_["form"] == "one refit per fold and permutation on the regular engine"
    assert np.isfinite(want["null"]).all() and np.isfinite(want["q2y"]).all()
    print("perm", _rel(got["null"], want["null"]), _rel(got["q2y"], want["q2y"]))
    assert _rel(got["q2y"], want["q2y"]) <= BOUND
    assert _rel(got["null"], want["null"]) <= BOUND
    np.testing.assert_array_equal(got["p_value"], want["p_value"])
    np.testing.assert_array_equal(got["permutations"], want["permutations"])


@pytest.mark.parametrize("trailing", [TM, TT])
def test_repeated_kfold_equals_refits(trailing):
    I, M, R = 28, 2, 3
    Xs, y = _coupled_data(I, trailing, M, R + 1, seed=35)
    on, off = _pair(Xs, y, R)
    got = get_q2y_repeated_kfold(on, n_splits=4, n_repeats=3, per_component=True)
    rep = _coupled(on.q2y_report_, models=12)
    assert rep["splits"] == 3
    want = get_q2y_repeated_kfold(off, n_splits=4, n_repeats=3, per_component=True)
    assert off.q2y_report_["form"] == "one refit per fold and split on the regular engine"
    for key in ("q2y", "mean", "std"):
        assert _rel(got[key], want[key]) <= BOUND, key
    assert got["one_se"] == want["one_se"]
    np.testing.assert_array_equal(got["folds"], want["folds"])


@pytest.mark.parametrize("trailing", [TM, TMT])
def test_bootstrap_equals_refits(trailing):
    I, M, R = 30, 2, 3
    Xs, y = _coupled_data(I, trailing, M, R + 1, seed=41)
    nan_row = int(np.flatnonzero(np.isnan(Xs[-1]).reshape(I, -1).any(axis=1))[0])
    idx = np.random.default_rng(5).integers(0, I, size=(8, I))
    idx[0, :3] = nan_row                                                  # a resample that repeats a row holding NaN
    on, off = _pair(Xs, y, R)
    got = bootstrap_factors(on, resamples=idx)
    rep = _coupled(on.bootstrap_report_, models=8)
    assert rep["resamples"] == 8
    want = bootstrap_factors(off, resamples=idx)
    assert off.bootstrap_report_["form"] == "one refit per resample on the regular engine"
    assert len(_leaves(got["X_factors"])) == len(_leaves(want["X_factors"])) == sum(len(t) for t in trailing)
    for a, b in zip(_leaves(got["X_factors"]), _leaves(want["X_factors"])):
        assert _col_rel(a, b) <= BOUND
    for key in ("Y_loadings", "coef"):
        assert _col_rel(got[key], want[key]) <= BOUND, key
    for part in ("se", "ci"):
        for key in ("Y_loadings", "coef"):
            assert _col_rel(got[part][key], want[part][key]) <= BOUND, (part, key)
        for a, b in zip(_leaves(got[part]["X_factors"]), _leaves(want[part]["X_factors"])):
            assert _col_rel(a, b) <= BOUND, part
    assert _rel(got["oob_q2y"], want["oob_q2y"]) <= BOUND and got["oob_rows"] == want["oob_rows"]


def test_float32_model_computes_in_float64():
    I, M, R = 30, 2, 2
    Xs, y = _coupled_data(I, TM, M, R + 1, seed=83)
    on, off = _pair(Xs, y, R, dtype="float32")
    got = get_q2y_repeated_kfold(on, n_splits=3, n_repeats=2, per_component=True)
    _coupled(on.q2y_report_, models=6)
    want = get_q2y_repeated_kfold(off, n_splits=3, n_repeats=2, per_component=True)
    assert _rel(got["q2y"], want["q2y"]) <= BOUND


# ---- 4. the status paths and the empty held-out row -------------------------------------------------------------------------------
def test_held_out_row_empty_in_one_block_predicts_nan():
    I, M, R = 24, 2, 2
    Xs, y = _coupled_data(I, TM, M, R + 1, seed=59)
    Xs[1][2] = np.nan                                                     # row 2 has nothing observed in the matrix block
    counts = np.ones((2, I), np.int32)
    counts[0, :5] = 0
    counts[1, [2, 15, 16, 17, 18]] = 0                                    # row 2 is held out by both models
    good = [X.copy() for X in Xs]
    good[1][2] = 0.5
    m, ref = _pair(good, y, R)
    out, why = masked_models_coupled(m, Xs, y, counts, None, 1e-8, 100)
    assert why is None and not out["status"].any()
    for j in range(2):
        test = counts[j] == 0
        want, _ = refit_fold(ref, Xs, y, test, 1e-8, 100)
        assert np.isnan(want[:, list(np.flatnonzero(test)).index(2)]).all()          # from the first component on
        assert _rel(out["Ypred"][j][:, test], want) <= BOUND
    assert np.isnan(out["Ypred"][:, :, 2]).all() and np.isfinite(out["Ypred"][0, :, 3]).all() and np.isfinite(out["Ypred"][1, :, 15]).all()


def test_training_row_empty_in_one_block_refits_those_folds_alone():
    I, M, R, K = 24, 2, 2, 3
    Xs, y = _coupled_data(I, TM, M, R + 1, seed=67)
    m, ref = _pair(Xs, y, R)                                              # (a fit on the data below would be NaN everywhere)
    bad = [X.copy() for X in Xs]
    bad[0][4] = np.nan                                                    # row 4 is in fold 0: folds 1 and 2 train on it
    ids, _ = fold_ids(I, K)
    pred, rep = masked_predictions_coupled(m, bad, y, ids, K, 1e-8, 100)
    assert COUPLED_FORM in rep["form"] and rep["refitted"] == [1, 2] and rep["models"] == K, rep
    assert rep["why"] == "a training row without an observed entry in some block in folds [1, 2]", rep
    want, want_iter = refit_predictions(ref, bad, y, ids, K, 1e-8, 100)
    assert _rel(pred, want) <= BOUND and rep["n_iter"][1] == want_iter[1]
    perm = np.random.default_rng(9).permutation(I)
    nums, n_iter, rep = masked_fold_numerators(m, bad, y, ids[None], K, perm[None], 1e-8, 100, coupled=True)
    assert COUPLED_FORM in rep["form"] and rep["refitted"] == [1, 2], rep
    assert rep["why"] == "a training row without an observed entry in some block in models [1, 2]" and nums.shape == (1, R)


def test_too_few_training_rows_and_bad_counts_set_a_status_and_write_nothing():
    I, M, R = 20, 2, 2
    Xs, y = _coupled_data(I, TM, M, R + 1, seed=71)
    m, _ = _pair(Xs, y, R)
    counts = np.ones((5, I), np.int32)
    counts[:, :4] = 0
    counts[1] = 0
    counts[1, 7] = 1                                                      # n = 1
    counts[2] = 0                                                         # n = 0
    counts[3, 9] = -1                                                     # a negative count
    out, why = masked_models_coupled(m, Xs, y, counts, None, 1e-8, 100, factors=True)
    assert why is None and out["status"].tolist() == [0, 2, 2, 3, 0]
    for j in (1, 2, 3):
        assert not out["Ypred"][j].any() and not out["info"][j].any() and not out["coef"][j].any() and not out["n_iter"][j].any()
    np.testing.assert_array_equal(out["Ypred"][0], out["Ypred"][4])        # the healthy models are untouched by their neighbours
    rep = masked_coupled_report(out, np.flatnonzero(out["status"]), "models")
    assert rep["refitted"] == [1, 2, 3] and rep["masked_blocks"] == [2, 2], rep
    assert rep["why"] == "fewer than 2 training rows in models [1, 2]; bad counts or Y rows in models [3]", rep
    yrow = np.tile(np.arange(I, dtype=np.int32), (5, 1))
    yrow[4, 0] = I                                                        # a Y row out of range
    out, _ = masked_models_coupled(m, Xs, y, np.abs(counts), yrow, 1e-8, 100)
    assert out["status"].tolist() == [0, 2, 2, 0, 3]


# ---- 5. limits -------------------------------------------------------------------------------------------------------------------
def _lds_edge_rows(trailing, M, R):
    dims = [(1, t[0]) if len(t) == 1 else tuple(t) for t in trailing]
    I = 2
    while coupled_lds_bytes(dims, I + 1, M, R) <= LDS_CAP:
        I += 1
    return I


_LDS_TRAILING = [(4000,), (6, 5)]


def _limit_case(case):
    if case in ("side64", "side65"):
        s = 64 if case == "side64" else 65
        return _coupled_data(24 if s == 64 else 8, [(s, s), (7,)], 2, 3, seed=71, nan=(0.05,)), (2 if s == 64 else 1)
    if case in ("m64", "m65"):
        return _coupled_data(40, TM, 64 if case == "m64" else 65, 3, seed=72), 2
    if case in ("r16", "r17"):
        R = 16 if case == "r16" else 17
        return _coupled_data(60, [(6, 5), (20,)], 2, R + 1, seed=73, nan=(0.05,)), R
    if case in ("nb8", "nb9"):
        return _coupled_data(30, [(3, 4), (5,)] * 4 + ([(4,)] if case == "nb9" else []), 2, 3, seed=74), 2
    I = _lds_edge_rows(_LDS_TRAILING, 2, 1) + (1 if case == "lds+1" else 0)
    return _coupled_data(I, _LDS_TRAILING, 2, 2, seed=75, nan=(0.02,)), 1


@pytest.mark.parametrize("case", ["side64", "m64", "r16", "nb8", "lds"])
def test_at_the_limits_runs_on_the_device(case):
    (Xs, y), R = _limit_case(case)
    if case == "lds":
        dims = [(1, 4000), (6, 5)]
        assert coupled_lds_bytes(dims, y.shape[0], 2, 1) <= LDS_CAP < coupled_lds_bytes(dims, y.shape[0] + 1, 2, 1)
    on, off = _pair(Xs, y, R)
    got = get_q2y_kfold(on, n_splits=3, per_component=True)
    _coupled(on.q2y_report_, models=3)
    want = get_q2y_kfold(off, n_splits=3, per_component=True)
    assert off.q2y_report_["form"] == "one refit per fold on the regular engine"
    assert np.isfinite(want).all()
    print(case, _rel(got, want))
    assert _rel(got, want) <= BOUND


@pytest.mark.parametrize("case", ["side65", "m65", "r17", "nb9", "lds+1"])
def test_past_the_limits_declines_to_refits(case):
    (Xs, y), R = _limit_case(case)
    on, off = _pair(Xs, y, R)
    got = get_q2y_kfold(on, n_splits=2, per_component=True)
    rep = on.q2y_report_
    assert rep["form"] == "one refit per fold on the regular engine", rep
    assert rep["why"].startswith(f"the masked form ({COUPLED_FORM}) declined: shape outside"), rep
    want = get_q2y_kfold(off, n_splits=2, per_component=True)
    np.testing.assert_array_equal(got, want)


# ---- 6. declines -----------------------------------------------------------------------------------------------------------------
def test_an_order_four_block_declines_to_refits():
    I, R = 20, 2
    Xs, y = _coupled_data(I, [(3, 2, 2), (5,)], 2, R + 1, seed=91)
    on, off = _pair(Xs, y, R)
    got = get_q2y_repeated_kfold(on, n_splits=2, n_repeats=2, per_component=True)
    rep = on.q2y_report_
    assert rep["form"] == "one refit per fold and split on the regular engine", rep
    assert rep["why"] == f"the masked form ({COUPLED_FORM}) declined: block 0 of order 4 (the masked form takes order 2 and 3)", rep
    want = get_q2y_repeated_kfold(off, n_splits=2, n_repeats=2, per_component=True)
    np.testing.assert_array_equal(got["q2y"], want["q2y"])


def test_nan_in_y_and_a_sharded_model_decline():
    I, R = 20, 2
    Xs, y = _coupled_data(I, TM, 2, R + 1, seed=93)
    m, _ = _pair(Xs, y, R)
    counts = np.ones((2, I), np.int32)
    counts[0, :5] = counts[1, 5:10] = 0
    ybad = y.copy()
    ybad[3, 0] = np.nan                                                   # (a fit on it would be NaN: the decline itself)
    assert masked_models_coupled(m, Xs, ybad, counts, None, 1e-8, 100) == (None, "missing values in Y")
    assert masked_predictions_coupled(m, Xs, ybad, *fold_ids(I, 4), 1e-8, 100) == (None, "missing values in Y")
    m._comm = object()                                                    # a sharded model: declined before anything is used
    try:
        assert masked_models_coupled(m, Xs, y, counts, None, 1e-8, 100) == (None, "sharded model (comm)")
    finally:
        m._comm = None


def test_option_off_or_complete_blocks_keep_todays_forms():
    I, R = 30, 2
    Xs, y = _coupled_data(I, TM, 2, R + 1, seed=89)
    off = ctPLS(R, dtype="float64", options=OFF)
    off.fit(Xs, y)
    also = ctPLS(R, dtype="float64", options=EngineOptions(small_fit=False, masked_folds=True))      # the tPLS option alone
    also.fit(Xs, y)
    for m in (off, also):
        a = kfold_predictions(m, n_splits=3)
        assert m.q2y_report_["form"] == "one refit per fold on the regular engine" and COUPLED_FORM not in m.q2y_report_["why"]
        permutation_test_q2y(m, n_permutations=2, n_splits=3)
        assert m.q2y_report_["why"] == "coupled model: permutation device form not built"
        get_q2y_repeated_kfold(m, n_splits=3, n_repeats=2)
        assert COUPLED_FORM not in str(m.q2y_report_)
        bootstrap_factors(m, n_resamples=2)
        assert COUPLED_FORM not in str(m.bootstrap_report_)
    np.testing.assert_array_equal(kfold_predictions(also, n_splits=3), a)
    Xc, yc = _coupled_data(I, TM, 2, R + 1, seed=89, nan=(0.0,))          # no NaN: the shared-read forms, option or not
    full = ctPLS(R, dtype="float64", options=ON)
    full.fit(Xc, yc)
    kfold_predictions(full, n_splits=3)
    assert "from shared reads of every block" in full.q2y_report_["form"], full.q2y_report_
    permutation_test_q2y(full, n_permutations=2, n_splits=3)
    assert full.q2y_report_["why"] == "coupled model: permutation device form not built"
    get_q2y_repeated_kfold(full, n_splits=3, n_repeats=2)
    assert "from shared reads of every block" in full.q2y_report_["form"], full.q2y_report_
    bootstrap_factors(full, n_resamples=2)
    assert "from shared reads of every block" in full.bootstrap_report_["form"], full.bootstrap_report_
