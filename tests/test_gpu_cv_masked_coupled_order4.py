"""Cross-validation of a ctPLS with a block of order 4 AND missing values, every model refitted by one 512-thread workgroup with the
rank-1 CP of every order-4 block's contraction inside it (cmtfpls_cv_masked_coupled_tensor_f64, EngineOptions.masked_tensor_folds_coupled,
DESIGN 8v).  Kernel level: one model against the NumPy restatement (coupled_masked_order4_ref), a single order-4 block bit for bit
against cmtfpls_cv_masked_tensor_models_f64, a B2 = 1 block, unit modes, chunks of models.  End to end, against literal refits on the
regular engine with the option off: K-fold, leave-one-out, the permutation test, repeated K-fold, the bootstrap, a float32 model, the
empty held-out and training rows, the statuses, the declared limits and one step past them.  Every end-to-end test checks the
report's form first, so a silent decline cannot compare refits with refits.

Tolerances are the order-4 family's (test_gpu_cv_masked_order4.py, test_gpu_kfold_order4.py): predictions 1e-7 relative, Q2Y and null
values 1e-8, NaN patterns and n_iter equal; the kernel against the NumPy restatement takes the 1e-7 of the kernel-level comparison of
test_gpu_cv_masked_order4_models.py (predictions and factors, normwise per component): what widens it from the order-3 form's 1e-10 is
the CP's stopping rule alone.  Every deviation is printed.  Input condition: in every parity case every row keeps an observed entry
in every block (asserted by _coupled_data) and every model's inner loop stops below max_iter (asserted through n_iter)."""
import functools

import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import (COUPLED_FORM, COUPLED_TENSOR_FORM, TENSOR_RANK1, coupled_tensor_masked_lds_bytes,
                                coupled_tensor_masked_workspace_bytes, fold_ids, masked_coupled_report, masked_fold_numerators,
                                masked_models_coupled, masked_predictions_coupled, masked_tensor_side, refit_fold, refit_predictions)
from cmtf_pls_amd.validate import (bootstrap_factors, get_q2y, get_q2y_kfold, get_q2y_repeated_kfold, kfold_predictions,
                                   loo_predictions, permutation_test_q2y)
from coupled_masked_order4_ref import coupled_masked_order4_fit

pytestmark = pytest.mark.gpu

_DEV = "cuda:0"
ON = EngineOptions(small_fit=False, masked_tensor_folds_coupled=True)
OFF = EngineOptions(small_fit=False)
LDS_CAP = 150 * 1024
PRED_TOL, Q2Y_TOL = 1e-7, 1e-8
BOUND = 1e-7                           # kernel against the NumPy restatement
MAX_ITER = 100

QM = [(3, 2, 2), (5,)]                 # order 4 + matrix
QT = [(4, 3, 2), (4, 5)]               # order 4 + order 3
TMQ = [(4, 5), (6,), (3, 3, 2)]        # order 3, matrix, order 4


def _nan_where(trailing, where):
    """The NaN fraction per block: in the blocks of order 4 only, in the others only, or in all."""
    return tuple(0.1 if where == "all" or (where == "tensor") == (len(t) == 3) else 0.0 for t in trailing)


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


def _converged(n_iter):
    """The input condition: every inner loop stopped below max_iter."""
    assert np.asarray(n_iter).size and np.asarray(n_iter).max() < MAX_ITER, np.asarray(n_iter).max()


def _same_iters(a, b):
    """n_iter of the device form and of the refits: equal."""
    return np.array_equal(np.asarray(a), np.asarray(b))


def _tensor(rep, models=None):
    """The report of a run that the coupled masked order-4 form took whole."""
    assert COUPLED_TENSOR_FORM in rep["form"] and COUPLED_FORM not in rep["form"], rep
    assert rep["refitted"] == [] and "why" not in rep, rep
    assert rep["rank1"] == TENSOR_RANK1 and rep["x_reads"] is None and rep["launches"] >= 1, rep
    if models is not None:
        assert rep["models"] == models, rep
    _converged(rep["n_iter"])
    return rep


def _leaves(tree):
    return [a for t in tree for a in _leaves(t)] if isinstance(tree, (list, tuple)) else [tree]


def _refit_kfold(Xs, y, ids, K, R):
    """Literal per-fold refits on the regular engine, every component count: ((R, I, M), n_iter K x R)."""
    want = np.zeros((R,) + y.shape)
    n_iter = []
    for k in range(K):
        test = ids == k
        r = ctPLS(R, dtype="float64", options=OFF)
        r.fit([X[~test] for X in Xs], y[~test])
        sc = r.transform([X[test] for X in Xs])
        for c in range(1, R + 1):
            want[c - 1, test] = (sc[:, :c] @ r.coef_[:c, :c]) @ r.Y_factors[1][:, :c].T + r.Y_mean
        n_iter.append([int(v) for v in r.n_iter_])
    return want, n_iter


def _backend():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(_DEV))


def _dev(a, dt=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=_DEV, dtype=dt)


def _descr(Xs):
    """(dims, tensor) of the backend call: (order, A, B) and (B1, B2) per block."""
    dims = [(2, 1, X.shape[1]) if X.ndim == 2 else (X.ndim, X.shape[1], int(np.prod(X.shape[2:]))) for X in Xs]
    return dims, [(X.shape[2], X.shape[3]) if X.ndim == 4 else (0, 0) for X in Xs]


def _kernel(be, Xs, y, counts, yrow, R, **kw):
    I = y.shape[0]
    return be.cv_masked_coupled_tensor([_dev(X.reshape(I, -1)) for X in Xs], *_descr(Xs), _dev(y.reshape(I, -1)), _dev(counts, torch.int32),
                                       None if yrow is None else _dev(yrow, torch.int32), R, 1e-8, MAX_ITER, **kw)


def _against_the_restatement(Xs, y, counts, yrow, R, what):
    got = _kernel(_backend(), Xs, y, counts, yrow, R, factors=True)
    assert got["launches"] == 1 and not got["status"].any()
    for j in range(counts.shape[0]):
        factors, Q, coef, pred, n_iter, info = coupled_masked_order4_fit(Xs, y, counts[j], R, None if yrow is None else yrow[j])
        _converged(n_iter)
        assert got["n_iter"][j].tolist() == n_iter and got["info"][j].tolist() == list(info), (j, got["n_iter"][j].tolist(), n_iter)
        held = counts[j] == 0
        devs = {"Ypred": _rel(got["Ypred"][j][:, held].cpu(), pred), "Q": _col_rel(got["Q"][j].cpu().numpy().T, Q),
                "coef": float(np.abs(got["coef"][j].cpu().numpy() - coef).max() / np.abs(coef).max())}
        assert not got["Ypred"][j][:, ~held].any()                         # written at held-out rows only
        for b, f in enumerate(factors):
            for key, want in f.items():
                assert got[key][b] is not None, (b, key)
                devs[f"{key}[{b}]"] = _col_rel(got[key][b][j].cpu().numpy().T, want)
            for key in ("Wk", "Wl"):
                assert (got[key][b] is None) == (key not in f)
        print(what, "model", j, " ".join(f"{k} {v:.3e}" for k, v in devs.items()))
        assert max(devs.values()) <= BOUND, devs
    return got


# ---- 1. kernel level -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["tensor", "matrix", "all"])
@pytest.mark.parametrize("trailing", [QM, QT, TMQ])
def test_one_model_equals_the_numpy_restatement(trailing, where):
    I, M, R = 30, 2, 3
    Xs, y = _coupled_data(I, trailing, M, R + 1, seed=31, nan=_nan_where(trailing, where))
    rng = np.random.default_rng(31)
    counts = rng.integers(0, 4, size=(3, I)).astype(np.int32)
    counts[:, :3] = 0
    counts[2] = (counts[2] > 0)                                            # a 0/1 model
    yrow = np.stack([np.arange(I), rng.permutation(I), np.arange(I)]).astype(np.int32)
    got = _against_the_restatement(Xs, y, counts, yrow, R, f"{trailing} NaN in {where}")
    masked = sum(1 << b for b, f in enumerate(_nan_where(trailing, where)) if f)
    assert (got["info"][:, 0].cpu().numpy() & ~masked == 0).all()          # a complete block never takes the masked arithmetic


def test_single_order4_block_equals_the_tpls_tensor_kernel_bit_for_bit():
    be = _backend()
    I, M, R, (A, B1, B2) = 26, 3, 3, (4, 3, 2)
    (x,), y = _coupled_data(I, [(A, B1, B2)], M, R + 1, seed=48)
    ids, K = fold_ids(I, 4)
    counts = (ids[None, :] != np.arange(K)[:, None]).astype(np.int32)
    want = be.cv_masked_tensor_models(_dev(x.reshape(I, -1)), _dev(y), _dev(counts, torch.int32), None, A, B1, B2, R, 1e-8, MAX_ITER,
                                      factors=True)
    got = _kernel(be, [x], y, counts, None, R, factors=True)
    assert not got["status"].any() and torch.equal(got["status"], want["status"])
    _converged(got["n_iter"].cpu().numpy())
    assert torch.equal(got["n_iter"], want["n_iter"]) and torch.equal(got["info"], want["info"])
    # the two kernels run the same steps at the same 512 threads (csrc/masked_fold.hpp, lx_cp3); what one block adds, 0.0 + s and
    # * 1.0, is exact
    for key, g in (("Ypred", got["Ypred"]), ("Wa", got["Wa"][0]), ("Wk", got["Wk"][0]), ("Wl", got["Wl"][0]), ("coef", got["coef"]),
                   ("Q", got["Q"])):
        g, w = g.cpu().numpy(), want[key].cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g, w, equal_nan=True), key
    wb = torch.einsum("mrk,mrl->mrkl", got["Wk"][0], got["Wl"][0]).reshape(K, R, B1 * B2)
    assert torch.equal(got["Wb"][0], wb)                                   # Wb of a tensor block is wK (x) wL in C order


@pytest.mark.parametrize("trailing", [[(4, 3, 1), (5,)], [(1, 3, 2), (5,)], [(3, 1, 2), (4, 3)]])
def test_b2_of_one_runs_the_cp_and_unit_modes_are_accepted(trailing):
    I, M, R = 24, 2, 2
    Xs, y = _coupled_data(I, trailing, M, R + 1, seed=52)
    counts = np.ones((2, I), np.int32)
    counts[0, :6] = 0
    counts[1, 6:12] = 0
    got = _against_the_restatement(Xs, y, counts, None, R, f"{trailing}")
    b = next(b for b, t in enumerate(trailing) if len(t) == 3)
    assert tuple(got["Wk"][b].shape) == (2, R, trailing[b][1]) and tuple(got["Wl"][b].shape) == (2, R, trailing[b][2])
    assert got["Wk"][b].any() and got["Wl"][b].any()                       # the CP's own factors, compared with the restatement's above


def test_chunked_launches_are_bit_identical():
    be = _backend()
    I, M, R = 36, 3, 3
    Xs, y = _coupled_data(I, TMQ, M, R + 1, seed=79)
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 3, size=(9, I)).astype(np.int32)
    yrow = np.stack([rng.permutation(I) for _ in range(9)]).astype(np.int32)
    one = _kernel(be, Xs, y, counts, yrow, R, factors=True)
    assert one["launches"] == 1
    dims, tensor = _descr(Xs)
    per = coupled_tensor_masked_workspace_bytes([(A, B) for _, A, B in dims], tensor, I, M, R)
    assert per == 8 * (sum((I + 2) * int(np.prod(X.shape[1:])) for X in Xs) + I * M + I * R + 4 * 18)
    per += R * I * M * 8
    for budget, launches in ((per, 9), (2 * per, 5), (4 * per + 7, 3)):
        many = _kernel(be, Xs, y, counts, yrow, R, factors=True, max_ws_bytes=budget)
        assert many["launches"] == launches
        for key, v in one.items():
            for a, b in zip(_leaves(v), _leaves(many[key])):
                if isinstance(a, torch.Tensor):
                    assert torch.equal(a, b), key


# ---- 2. K-fold and leave-one-out -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trailing,folds", [(QM, None), (QT, "shuffled"), (TMQ, None)])
def test_kfold_equals_refits_for_every_component_count(trailing, folds):
    I, M, R, K = 30, 2, 3, 4
    Xs, y = _coupled_data(I, trailing, M, R + 1, seed=I + len(trailing))
    if folds == "shuffled":
        folds = np.random.default_rng(2).permutation(np.arange(I) % K)
        folds[:3] = 0                                                      # unequal fold sizes
    on, _ = _pair(Xs, y, R)
    pred = kfold_predictions(on, n_splits=K, folds=folds)
    rep = _tensor(on.q2y_report_, models=K)
    assert rep["folds"] == K and np.asarray(rep["n_iter"]).shape == (K, R)
    ids, _ = fold_ids(I, K, folds)
    batches = [sum(bool(np.isnan(X[ids == k]).any()) for k in range(K)) for X in Xs]     # a held-out batch is masked when it holds a NaN
    assert rep["masked_blocks"] == [K] * len(Xs) and rep["masked_batches"] == batches, rep
    want, n_iter = _refit_kfold(Xs, y, ids, K, R)
    assert np.isfinite(want).all()
    print("kfold", trailing, _rel(pred, want))
    assert _rel(pred, want) <= PRED_TOL and _same_iters(rep["n_iter"], n_iter)
    q = get_q2y_kfold(on, n_splits=K, folds=folds, per_component=True)
    _tensor(on.q2y_report_, models=K)
    q_want = 1.0 - ((want - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum()
    print("kfold q2y", np.abs(q - q_want).max())
    assert np.abs(q - q_want).max() <= Q2Y_TOL


def test_leave_one_out_equals_refits():
    I, M, R = 24, 2, 3
    Xs, y = _coupled_data(I, QM, M, R + 1, seed=24)
    on, off = _pair(Xs, y, R)
    q = get_q2y(on)
    rep = _tensor(on.q2y_report_, models=I)
    assert rep["blocks"] == 2 and rep["n_iter_total"] == int(np.sum(rep["n_iter"]))
    q_want = get_q2y(off)
    assert off.q2y_report_["form"] == "one refit per fold on the regular engine"
    print("loo q2y", abs(q - q_want))
    assert abs(q - q_want) <= Q2Y_TOL
    want, n_iter = _refit_kfold(Xs, y, np.arange(I), I, R)
    pred = loo_predictions(on)
    assert _same_iters(_tensor(on.q2y_report_, models=I)["n_iter"], n_iter)
    print("loo", _rel(pred, want[-1]))
    assert _rel(pred, want[-1]) <= PRED_TOL
    assert _rel(kfold_predictions(on, n_splits=I), want) <= PRED_TOL


def test_nan_in_the_matrix_block_only_keeps_the_tensor_block_unmasked():
    I, M, R, K = 28, 2, 3, 4
    Xs, y = _coupled_data(I, QM, M, R + 1, seed=28, nan=(0.0, 0.1))
    on, _ = _pair(Xs, y, R)
    pred = kfold_predictions(on, n_splits=K)
    rep = _tensor(on.q2y_report_, models=K)
    assert rep["masked_blocks"] == [0, K] and rep["masked_batches"] == [0, K], rep
    want, n_iter = _refit_kfold(Xs, y, fold_ids(I, K)[0], K, R)
    assert _rel(pred, want) <= PRED_TOL and _same_iters(rep["n_iter"], n_iter)


# ---- 3. permutation test, repeated K-fold, bootstrap ----------------------------------------------------------------------------
@pytest.mark.parametrize("trailing", [QM, TMQ])
def test_permutation_test_equals_refits(trailing):
    I, M, R = 30, 2, 3
    Xs, y = _coupled_data(I, trailing, M, R + 1, seed=44)
    on, off = _pair(Xs, y, R)
    got = permutation_test_q2y(on, n_permutations=5, n_splits=4, per_component=True)
    rep = _tensor(on.q2y_report_, models=20)
    assert rep["permutations"] == 5 and np.asarray(rep["n_iter"]).shape == (5, 4, 3)
    _tensor(rep["observed"], models=4)
    want = permutation_test_q2y(off, n_permutations=5, n_splits=4, per_component=True)
    assert off.q2y_report_["form"] == "one refit per fold and permutation on the regular engine"
    assert np.isfinite(want["null"]).all() and np.isfinite(want["q2y"]).all()
    print("perm", np.abs(got["null"] - want["null"]).max(), np.abs(got["q2y"] - want["q2y"]).max())
    assert np.abs(got["q2y"] - want["q2y"]).max() <= Q2Y_TOL
    assert np.abs(got["null"] - want["null"]).max() <= Q2Y_TOL
    assert _same_iters(rep["n_iter"], off.q2y_report_["n_iter"])
    np.testing.assert_array_equal(got["p_value"], want["p_value"])
    np.testing.assert_array_equal(got["permutations"], want["permutations"])


@pytest.mark.parametrize("trailing", [QM, QT])
def test_repeated_kfold_equals_refits(trailing):
    I, M, R = 28, 2, 3
    Xs, y = _coupled_data(I, trailing, M, R + 1, seed=36)
    on, off = _pair(Xs, y, R)
    got = get_q2y_repeated_kfold(on, n_splits=4, n_repeats=3, per_component=True)
    rep = _tensor(on.q2y_report_, models=12)
    assert rep["splits"] == 3
    want = get_q2y_repeated_kfold(off, n_splits=4, n_repeats=3, per_component=True)
    assert off.q2y_report_["form"] == "one refit per fold and split on the regular engine"
    for key in ("q2y", "mean", "std"):
        print("repeated", key, np.abs(np.asarray(got[key]) - np.asarray(want[key])).max())
        assert np.abs(np.asarray(got[key]) - np.asarray(want[key])).max() <= Q2Y_TOL, key
    assert got["one_se"] == want["one_se"] and _same_iters(rep["n_iter"], off.q2y_report_["n_iter"])
    np.testing.assert_array_equal(got["folds"], want["folds"])


@pytest.mark.parametrize("trailing", [QM, TMQ])
def test_bootstrap_equals_refits(trailing):
    I, M, R = 30, 2, 3
    Xs, y = _coupled_data(I, trailing, M, R + 1, seed=41)
    nan_row = int(np.flatnonzero(np.isnan(Xs[-1]).reshape(I, -1).any(axis=1))[0])
    idx = np.random.default_rng(5).integers(0, I, size=(8, I))
    idx[0, :3] = nan_row                                                  # a resample that repeats a row holding NaN
    on, off = _pair(Xs, y, R)
    got = bootstrap_factors(on, resamples=idx)
    rep = _tensor(on.bootstrap_report_, models=8)
    assert rep["resamples"] == 8
    want = bootstrap_factors(off, resamples=idx)
    assert off.bootstrap_report_["form"] == "one refit per resample on the regular engine"
    assert _same_iters(rep["n_iter"], off.bootstrap_report_["n_iter"])
    assert len(_leaves(got["X_factors"])) == len(_leaves(want["X_factors"])) == sum(len(t) for t in trailing)   # per mode: [wA, wK, wL]
    for b, t in enumerate(trailing):
        assert [f.shape[1] for f in got["X_factors"][b]] == list(t)
    devs = [_col_rel(a, b) for a, b in zip(_leaves(got["X_factors"]), _leaves(want["X_factors"]))]
    devs += [_col_rel(got[key], want[key]) for key in ("Y_loadings", "coef")]
    for part in ("se", "ci"):
        devs += [_col_rel(got[part][key], want[part][key]) for key in ("Y_loadings", "coef")]
        devs += [_col_rel(a, b) for a, b in zip(_leaves(got[part]["X_factors"]), _leaves(want[part]["X_factors"]))]
    print("bootstrap", trailing, "stacks, se, ci", max(devs), "oob_q2y", np.abs(got["oob_q2y"] - want["oob_q2y"]).max())
    assert max(devs) <= PRED_TOL
    assert np.abs(got["oob_q2y"] - want["oob_q2y"]).max() <= Q2Y_TOL and got["oob_rows"] == want["oob_rows"]


def test_float32_model_computes_in_float64():
    I, M, R = 30, 2, 2
    Xs, y = _coupled_data(I, QM, M, R + 1, seed=83)
    on, off = _pair(Xs, y, R, dtype="float32")
    got = get_q2y_repeated_kfold(on, n_splits=3, n_repeats=2, per_component=True)
    _tensor(on.q2y_report_, models=6)
    want = get_q2y_repeated_kfold(off, n_splits=3, n_repeats=2, per_component=True)
    print("float32 model", np.abs(got["q2y"] - want["q2y"]).max())
    assert np.abs(got["q2y"] - want["q2y"]).max() <= Q2Y_TOL


# ---- 4. the status paths and the empty held-out row -------------------------------------------------------------------------------
def test_held_out_row_empty_in_the_tensor_block_predicts_nan():
    I, M, R = 24, 2, 2
    Xs, y = _coupled_data(I, QM, M, R + 1, seed=59)
    Xs[0][2] = np.nan                                                     # row 2 has nothing observed in the tensor block
    counts = np.ones((2, I), np.int32)
    counts[0, :5] = 0
    counts[1, [2, 15, 16, 17, 18]] = 0                                    # row 2 is held out by both models
    good = [X.copy() for X in Xs]
    good[0][2] = 0.5
    m, ref = _pair(good, y, R)
    out, why = masked_models_coupled(m, Xs, y, counts, None, 1e-8, MAX_ITER)
    assert why is None and not out["status"].any() and out["tensor"] == [(2, 2), (0, 0)]
    _converged(out["n_iter"])
    for j in range(2):
        test = counts[j] == 0
        want, n_iter = refit_fold(ref, Xs, y, test, 1e-8, MAX_ITER)
        assert np.isnan(want[:, list(np.flatnonzero(test)).index(2)]).all()          # from the first component on, on both sides
        assert _rel(out["Ypred"][j][:, test], want) <= PRED_TOL and out["n_iter"][j].tolist() == n_iter
    assert np.isnan(out["Ypred"][:, :, 2]).all() and np.isfinite(out["Ypred"][0, :, 3]).all() and np.isfinite(out["Ypred"][1, :, 15]).all()


def test_training_row_empty_in_one_block_refits_those_folds_alone():
    I, M, R, K = 24, 2, 2, 3
    Xs, y = _coupled_data(I, QM, M, R + 1, seed=67)
    m, ref = _pair(Xs, y, R)                                              # (a fit on the data below would be NaN everywhere)
    bad = [X.copy() for X in Xs]
    bad[0][4] = np.nan                                                    # row 4 is in fold 0: folds 1 and 2 train on it
    ids, _ = fold_ids(I, K)
    pred, rep = masked_predictions_coupled(m, bad, y, ids, K, 1e-8, MAX_ITER)
    assert COUPLED_TENSOR_FORM in rep["form"] and rep["rank1"] == TENSOR_RANK1 and rep["refitted"] == [1, 2] and rep["models"] == K, rep
    assert rep["why"] == "a training row without an observed entry in some block in folds [1, 2]", rep
    want, want_iter = refit_predictions(ref, bad, y, ids, K, 1e-8, MAX_ITER)
    assert _rel(pred, want) <= PRED_TOL and _same_iters(rep["n_iter"], want_iter)
    perm = np.random.default_rng(9).permutation(I)
    nums, n_iter, rep = masked_fold_numerators(m, bad, y, ids[None], K, perm[None], 1e-8, MAX_ITER, coupled=True)
    assert COUPLED_TENSOR_FORM in rep["form"] and rep["refitted"] == [1, 2], rep
    assert rep["why"] == "a training row without an observed entry in some block in models [1, 2]" and nums.shape == (1, R)


def test_too_few_training_rows_and_bad_counts_set_a_status_and_write_nothing():
    I, M, R = 20, 2, 2
    Xs, y = _coupled_data(I, QM, M, R + 1, seed=71)
    m, _ = _pair(Xs, y, R)
    counts = np.ones((5, I), np.int32)
    counts[:, :4] = 0
    counts[1] = 0
    counts[1, 7] = 1                                                      # n = 1
    counts[2] = 0                                                         # n = 0
    counts[3, 9] = -1                                                     # a negative count
    out, why = masked_models_coupled(m, Xs, y, counts, None, 1e-8, MAX_ITER, factors=True)
    assert why is None and out["status"].tolist() == [0, 2, 2, 3, 0]
    for j in (1, 2, 3):
        assert not out["Ypred"][j].any() and not out["info"][j].any() and not out["coef"][j].any() and not out["n_iter"][j].any()
        assert not out["Wk"][0][j].any() and not out["Wl"][0][j].any() and not out["Wa"][0][j].any() and not out["Wb"][1][j].any()
    np.testing.assert_array_equal(out["Ypred"][0], out["Ypred"][4])        # the healthy models are untouched by their neighbours
    np.testing.assert_array_equal(out["Wk"][0][0], out["Wk"][0][4])
    assert out["Wk"][0][0].any() and out["Wk"][1] is None
    rep = masked_coupled_report(out, np.flatnonzero(out["status"]), "models")
    assert rep["refitted"] == [1, 2, 3] and rep["masked_blocks"] == [2, 2] and COUPLED_TENSOR_FORM in rep["form"], rep
    assert rep["why"] == "fewer than 2 training rows in models [1, 2]; bad counts or Y rows in models [3]", rep
    yrow = np.tile(np.arange(I, dtype=np.int32), (5, 1))
    yrow[4, 0] = I                                                        # a Y row out of range
    out, _ = masked_models_coupled(m, Xs, y, np.abs(counts), yrow, 1e-8, MAX_ITER)
    assert out["status"].tolist() == [0, 2, 2, 0, 3]


# ---- 5. limits -------------------------------------------------------------------------------------------------------------------
def _mirror_args(trailing):
    dims = [(1, t[0]) if len(t) == 1 else (t[0], int(np.prod(t[1:]))) for t in trailing]
    return dims, [(t[1], t[2]) if len(t) == 3 else (0, 0) for t in trailing]


def _lds_edge_rows(trailing, M, R):
    I = 2
    while coupled_tensor_masked_lds_bytes(*_mirror_args(trailing), I + 1, M, R) <= LDS_CAP:
        I += 1
    return I


_LDS_TRAILING = [(4000,), (3, 2, 2)]


@functools.lru_cache(maxsize=None)
def _limit_case(case):
    """((blocks, Y), R) at a declared limit or one step past it."""
    if case in ("side64", "side65"):
        t = (64, 8, 8) if case == "side64" else (65, 13, 5)
        assert masked_tensor_side(*t) == int(case[4:])
        return _coupled_data(12 if case == "side64" else 8, [t, (7,)], 2, 3, seed=71, nan=(0.05,)), (2 if case == "side64" else 1)
    if case in ("mat64", "mat65"):
        s = int(case[3:])
        return _coupled_data(24 if s == 64 else 8, [(3, 2, 2), (s, s)], 2, 3, seed=76, nan=(0.05,)), (2 if s == 64 else 1)
    if case in ("m64", "m65"):
        return _coupled_data(40, QM, int(case[1:]), 3, seed=72), 2
    if case in ("r16", "r17"):
        R = int(case[1:])
        return _coupled_data(60, [(6, 5, 4), (20,)], 2, R + 1, seed=82, nan=(0.05,)), R
    if case in ("nb8", "nb9"):
        return _coupled_data(30, [(3, 2, 2)] + [(3, 4), (5,)] * 3 + [(4,)] + ([(3,)] if case == "nb9" else []), 2, 3, seed=74), 2
    I = _lds_edge_rows(_LDS_TRAILING, 2, 1) + (1 if case == "lds+1" else 0)
    return _coupled_data(I, _LDS_TRAILING, 2, 2, seed=75, nan=(0.02,)), 1


@pytest.mark.parametrize("case", ["side64", "mat64", "m64", "r16", "nb8", "lds"])
def test_at_the_limits_runs_on_the_device(case):
    (Xs, y), R = _limit_case(case)
    if case == "lds":
        args = _mirror_args(_LDS_TRAILING)
        assert coupled_tensor_masked_lds_bytes(*args, y.shape[0], 2, 1) <= LDS_CAP < coupled_tensor_masked_lds_bytes(*args, y.shape[0] + 1, 2, 1)
    if case == "nb8":
        assert len(Xs) == 8 and sum(X.ndim == 4 for X in Xs) == 1
    on, off = _pair(Xs, y, R)
    got = get_q2y_kfold(on, n_splits=3, per_component=True)
    rep = _tensor(on.q2y_report_, models=3)
    want = get_q2y_kfold(off, n_splits=3, per_component=True)
    assert off.q2y_report_["form"] == "one refit per fold on the regular engine"
    assert np.isfinite(want).all() and _same_iters(rep["n_iter"], off.q2y_report_["n_iter"])
    print(case, np.abs(got - want).max())
    assert np.abs(got - want).max() <= Q2Y_TOL


@pytest.mark.parametrize("case", ["side65", "mat65", "m65", "r17", "nb9", "lds+1"])
def test_past_the_limits_declines_to_refits(case):
    (Xs, y), R = _limit_case(case)
    on, off = _pair(Xs, y, R)
    got = get_q2y_kfold(on, n_splits=2, per_component=True)
    rep = on.q2y_report_
    assert rep["form"] == "one refit per fold on the regular engine", rep
    assert rep["why"].startswith(f"the masked form ({COUPLED_TENSOR_FORM}) declined: shape outside"), rep
    for number in ("largest short side = [", f"M = {y.shape[1]}", f"R = {R}", "LDS = "):
        assert number in rep["why"], rep
    want = get_q2y_kfold(off, n_splits=2, per_component=True)
    np.testing.assert_array_equal(got, want)


# ---- 6. declines and what stays ---------------------------------------------------------------------------------------------------
def test_nan_in_y_a_sharded_model_and_an_order_five_block_decline():
    I, R = 20, 2
    Xs, y = _coupled_data(I, QM, 2, R + 1, seed=93)
    m, _ = _pair(Xs, y, R)
    counts = np.ones((2, I), np.int32)
    counts[0, :5] = counts[1, 5:10] = 0
    ybad = y.copy()
    ybad[3, 0] = np.nan                                                   # (a fit on it would be NaN: the decline itself)
    assert masked_models_coupled(m, Xs, ybad, counts, None, 1e-8, MAX_ITER) == (None, "missing values in Y")
    five = Xs + [np.random.default_rng(1).standard_normal((I, 2, 2, 2, 2))]
    assert masked_models_coupled(m, five, y, counts, None, 1e-8, MAX_ITER) == (None, "block 2 of order 5 (the masked form takes order 2, 3 and 4)")
    m._comm = object()                                                    # a sharded model: declined before anything is used
    try:
        assert masked_models_coupled(m, Xs, y, counts, None, 1e-8, MAX_ITER) == (None, "sharded model (comm)")
    finally:
        m._comm = None


def test_option_off_or_complete_data_keep_todays_forms_and_bits():
    I, R = 30, 2
    Xs, y = _coupled_data(I, QM, 2, R + 1, seed=89)
    off = ctPLS(R, dtype="float64", options=OFF)
    off.fit(Xs, y)
    old = ctPLS(R, dtype="float64", options=EngineOptions(small_fit=False, masked_folds_coupled=True))   # the order-2/3 option alone
    old.fit(Xs, y)
    a = kfold_predictions(off, n_splits=3)
    assert off.q2y_report_["form"] == "one refit per fold on the regular engine" and "masked form" not in off.q2y_report_["why"]
    np.testing.assert_array_equal(kfold_predictions(old, n_splits=3), a)
    assert old.q2y_report_["why"] == f"the masked form ({COUPLED_FORM}) declined: block 0 of order 4 (the masked form takes order 2 and 3)"
    for m in (off, old):
        get_q2y_repeated_kfold(m, n_splits=3, n_repeats=2)
        assert COUPLED_TENSOR_FORM not in str(m.q2y_report_)
        bootstrap_factors(m, n_resamples=2)
        assert COUPLED_TENSOR_FORM not in str(m.bootstrap_report_)
    Xc, yc = _coupled_data(I, QM, 2, R + 1, seed=89, nan=(0.0,))          # no NaN: today's routes, option or not
    full, plain = ctPLS(R, dtype="float64", options=ON), ctPLS(R, dtype="float64", options=OFF)
    full.fit(Xc, yc)
    plain.fit(Xc, yc)
    np.testing.assert_array_equal(kfold_predictions(full, n_splits=3), kfold_predictions(plain, n_splits=3))
    assert full.q2y_report_ == plain.q2y_report_ and COUPLED_TENSOR_FORM not in str(full.q2y_report_)
    X3, y3 = _coupled_data(I, [(4, 5), (6,)], 2, R + 1, seed=90)          # NaN but no block of order 4: the option does not govern it
    no4, plain = ctPLS(R, dtype="float64", options=ON), ctPLS(R, dtype="float64", options=OFF)
    no4.fit(X3, y3)
    plain.fit(X3, y3)
    np.testing.assert_array_equal(kfold_predictions(no4, n_splits=3), kfold_predictions(plain, n_splits=3))
    assert no4.q2y_report_ == plain.q2y_report_
