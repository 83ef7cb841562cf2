"""The permutation test, repeated K-fold and the bootstrap of a tPLS whose X has missing values, every model refitted by one
workgroup (cmtfpls_cv_masked_models_f64, EngineOptions.masked_folds): each tool against the same call with the option off, which
refits every model literally on the regular engine; the weights against literally duplicated rows; 0/1 counts against
cmtfpls_cv_masked_f64; the edges of the masked arithmetic, the declared limits and one step past them, chunks of models, a float32
model, and that nothing changes with the option off, without NaN or for a ctPLS."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import MODELS_FORM, _refit_numerators, fold_ids, masked_fold_numerators, masked_models, refit_fold
from cmtf_pls_amd.validate import bootstrap_factors, get_q2y_repeated_kfold, permutation_test_q2y

pytestmark = pytest.mark.gpu

_DEV = "cuda:0"
ON = EngineOptions(small_fit=False, masked_folds=True)
OFF = EngineOptions(small_fit=False)


def _data(shape, M, R, nan, seed):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=seed)
    if nan:
        x[np.random.default_rng(seed + 100).random(x.shape) < nan] = np.nan
    return x, y


def _pair(x, y, R, dtype="float64"):
    on, off = tPLS(R, dtype=dtype, options=ON), tPLS(R, dtype="float64", options=OFF)
    on.fit(x, y)
    off.fit(x, y)
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


def _masked(rep):
    assert MODELS_FORM in rep["form"], rep
    assert rep["x_reads"] is None and rep["models"] >= 1 and rep["launches"] >= 1, rep
    return rep


def _leaves(tree):
    return [a for t in tree for a in _leaves(t)] if isinstance(tree, (list, tuple)) else [tree]


# ---- 1. permutation test ---------------------------------------------------------------------------------------------------------
def test_permutation_test_equals_refits():
    x, y = _data((30, 6, 5), 2, 3, 0.1, seed=30)
    on, off = _pair(x, y, 3)
    got = permutation_test_q2y(on, n_permutations=6, n_splits=4, per_component=True)
    rep = _masked(on.q2y_report_)
    assert rep["models"] == 24 and rep["permutations"] == 6 and np.asarray(rep["n_iter"]).shape == (6, 4, 3)
    assert rep["masked_models"] == 24 and "refitted" not in rep
    want = permutation_test_q2y(off, n_permutations=6, n_splits=4, per_component=True)
    assert off.q2y_report_["form"] == "one refit per fold and permutation on the regular engine"
    assert _rel(got["null"], want["null"]) <= 1e-10
    np.testing.assert_array_equal(got["p_value"], want["p_value"])
    np.testing.assert_array_equal(got["permutations"], want["permutations"])


# ---- 2. repeated K-fold ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,M", [((28, 9), 2), ((60, 10, 8), 4)])
def test_repeated_kfold_equals_refits(shape, M):
    R = 3
    x, y = _data(shape, M, R, 0.1, seed=shape[0])
    on, off = _pair(x, y, R)
    got = get_q2y_repeated_kfold(on, n_splits=4, n_repeats=3, per_component=True)
    rep = _masked(on.q2y_report_)
    assert rep["models"] == 12 and rep["splits"] == 3
    want = get_q2y_repeated_kfold(off, n_splits=4, n_repeats=3, per_component=True)
    assert off.q2y_report_["form"] == "one refit per fold and split on the regular engine"
    for key in ("q2y", "mean", "std"):
        assert _rel(got[key], want[key]) <= 1e-10, key
    assert got["one_se"] == want["one_se"]
    np.testing.assert_array_equal(got["folds"], want["folds"])


# ---- 3. bootstrap ----------------------------------------------------------------------------------------------------------------
def _check_bootstrap(got, want, skip=()):
    keep = [b for b in range(got["coef"].shape[0]) if b not in skip]
    for a, b in zip(_leaves(got["X_factors"]), _leaves(want["X_factors"])):
        assert _col_rel(a[keep], b[keep]) <= 1e-10
    assert _col_rel(got["Y_loadings"][keep], want["Y_loadings"][keep]) <= 1e-10
    assert _col_rel(got["coef"][keep], want["coef"][keep]) <= 1e-10
    if not skip:
        for part in ("se", "ci"):
            for key in ("Y_loadings", "coef"):
                assert _col_rel(got[part][key], want[part][key]) <= 1e-10
            for a, b in zip(_leaves(got[part]["X_factors"]), _leaves(want[part]["X_factors"])):
                assert _col_rel(a, b) <= 1e-10
        assert _rel(got["oob_q2y"], want["oob_q2y"]) <= 1e-10 and got["oob_rows"] == want["oob_rows"]


def test_bootstrap_equals_refits():
    x, y = _data((30, 6, 5), 2, 3, 0.1, seed=41)
    I = 30
    nan_row = int(np.flatnonzero(np.isnan(x).reshape(I, -1).any(axis=1))[0])
    idx = np.random.default_rng(5).integers(0, I, size=(10, I))
    idx[0, :3] = nan_row                                                  # a resample that repeats a row holding NaN
    on, off = _pair(x, y, 3)
    got = bootstrap_factors(on, resamples=idx)
    rep = _masked(on.bootstrap_report_)
    assert rep["models"] == 10 and rep["resamples"] == 10 and "refitted" not in rep
    want = bootstrap_factors(off, resamples=idx)
    assert off.bootstrap_report_["form"] == "one refit per resample on the regular engine"
    _check_bootstrap(got, want)


# ---- 4. weights mean duplication -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,M", [((24, 6, 5), 3), ((22, 11), 2)])
def test_weights_equal_duplicated_rows(shape, M):
    from cmtf_pls_amd.backend import HipBackend
    be = HipBackend(torch.device(_DEV))
    R = 3
    x, y = _data(shape, M, R, 0.1, seed=43)
    I = shape[0]
    A, B = (1, shape[1]) if len(shape) == 2 else shape[1:]
    rng = np.random.default_rng(7)
    c = rng.integers(0, 4, size=(3, I))
    c[:, :4] = 0
    c[:, 5] = 3
    dev = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(device=_DEV, dtype=dt)
    X2, Y2 = x.reshape(I, -1), y.reshape(I, -1)
    got = be.cv_masked_models(dev(X2), dev(Y2), dev(c, torch.int32), None, A, B, R, 1e-8, 100, factors=True)
    assert not got["status"].any()
    for j in range(3):
        held = np.flatnonzero(c[j] == 0)
        rows = np.concatenate([np.repeat(np.arange(I), c[j]), held])       # the duplicated rows, then the held-out ones
        cd = np.concatenate([np.ones(rows.size - held.size, np.int32), np.zeros(held.size, np.int32)])[None]
        dup = be.cv_masked_models(dev(X2[rows]), dev(Y2[rows]), dev(cd, torch.int32), None, A, B, R, 1e-8, 100, factors=True)
        assert not dup["status"].any()
        n_tr = rows.size - held.size
        assert _rel(got["Ypred"][j][:, held].cpu(), dup["Ypred"][0][:, n_tr:].cpu()) <= 1e-12
        for key in ("Wa", "Wb", "coef", "Q"):
            assert _rel(got[key][j].cpu(), dup[key][0].cpu()) <= 1e-12, key
        assert torch.equal(got["info"][j], dup["info"][0])


# ---- 5. 0/1 counts are cmtfpls_cv_masked_f64's folds -----------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, None])
def test_zero_one_counts_equal_the_fold_kernel(K):
    from cmtf_pls_amd.backend import HipBackend
    be = HipBackend(torch.device(_DEV))
    x, y = _data((26, 6, 5), 3, 3, 0.1, seed=47)
    I, (A, B) = 26, (6, 5)
    ids, K = (np.arange(I), I) if K is None else fold_ids(I, K)
    X2 = torch.from_numpy(x.reshape(I, -1)).to(_DEV)
    Y2 = torch.from_numpy(y.reshape(I, -1)).to(_DEV)
    folds = be.cv_masked(X2, Y2, torch.from_numpy(ids.astype(np.int32)).to(_DEV), K, A, B, 3, 1e-8, 100)
    counts = (ids[None, :] != np.arange(K)[:, None]).astype(np.int32)
    got = be.cv_masked_models(X2, Y2, torch.from_numpy(counts).to(_DEV), None, A, B, 3, 1e-8, 100)
    pred = sum(got["Ypred"][k] for k in range(K))                        # each model writes only its own fold's rows
    assert _rel(pred.cpu(), folds[0].cpu()) <= 1e-12
    assert torch.equal(got["n_iter"], folds[1]) and torch.equal(got["info"], folds[3])


# ---- 6. edges --------------------------------------------------------------------------------------------------------------------
def _direct_vs_refits(x, y, counts, R=2):
    """masked_models on the given counts, each model against refit_fold of its held-out rows."""
    m = tPLS(R, dtype="float64", options=ON)
    m.fit(x, y)
    out, why = masked_models(m, x, y, counts, None, 1e-8, 100)
    assert why is None and not out["status"].any()
    ref = tPLS(R, dtype="float64", options=OFF)
    ref.fit(x, y)
    for j in range(counts.shape[0]):
        test = counts[j] == 0
        want, _ = refit_fold(ref, x, y, test, 1e-8, 100)
        assert _rel(out["Ypred"][j][:, test], want) <= 1e-10
    return out


def test_column_unobserved_in_the_training_rows():
    x, y = _data((24, 5, 4), 2, 2, 0.05, seed=53)
    counts = np.ones((2, 24), np.int32)
    counts[:, :6] = 0
    x[6:, 2, 3] = np.nan                                                  # column (2, 3): observed only in the held-out rows
    x[:6, 2, 3] = np.arange(6) + 0.5
    out = _direct_vs_refits(x, y, counts)
    assert out["info"][:, 0].all() and out["info"][:, 1].all()


def test_held_out_row_without_an_observed_entry_predicts_nan():
    x, y = _data((24, 5, 4), 2, 2, 0.05, seed=59)
    x[2] = np.nan
    counts = np.ones((2, 24), np.int32)
    counts[0, :5] = 0
    counts[1, [2, 15, 16, 17, 18]] = 0
    out = _direct_vs_refits(x, y, counts)
    assert np.isnan(out["Ypred"][:, :, 2]).all() and np.isfinite(out["Ypred"][0, :, 3]).all() and np.isfinite(out["Ypred"][1, :, 15]).all()


def test_nan_only_in_held_out_rows_takes_the_unmasked_arithmetic():
    x, y = _data((24, 5, 4), 2, 2, 0.0, seed=61)
    x[1, 2, 2] = np.nan
    x[3, 0, 1] = np.nan
    counts = np.ones((2, 24), np.int32)
    counts[0, :5] = 0                                                      # model 0 holds out both NaN rows
    counts[1, 20:] = 0                                                     # model 1 trains on them
    out = _direct_vs_refits(x, y, counts)
    assert out["info"].tolist() == [[0, 1], [1, 0]]


def test_training_row_without_an_observed_entry_refits_that_model_alone():
    x, y = _data((24, 5, 4), 2, 2, 0.1, seed=67)
    m = tPLS(2, dtype="float64", options=ON)
    m.fit(x, y)                                                            # (a fit on x4 itself would be NaN everywhere)
    x4 = x.copy()
    x4[4] = np.nan
    ids, K = fold_ids(24, 2)                                               # row 4 is in fold 0: only model 1 trains on it
    perm = np.random.default_rng(9).permutation(24)
    nums, n_iter, rep = masked_fold_numerators(m, x4, y, ids[None], K, perm[None], 1e-8, 100)
    assert MODELS_FORM in rep["form"] and rep["refitted"] == [1], rep
    assert rep["why"] == "a training row without an observed entry of X in models [1]", rep
    ref = tPLS(2, dtype="float64", options=OFF)
    ref.fit(x, y)
    want, want_iter = _refit_numerators(ref, x4, y, ids, K, perm, 1e-8, 100)
    assert _rel(nums[0], want) <= 1e-10 and n_iter[0][1] == want_iter[1]


# ---- 7. limits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["side64", "m64", "r16"])
def test_at_the_limits_runs_on_the_device(case):
    shape, M, R = {"side64": ((24, 64, 64), 2, 2), "m64": ((40, 6, 5), 64, 2), "r16": ((60, 6, 5), 2, 16)}[case]
    x, y = _data(shape, M, R, 0.05, seed=71)
    on, off = _pair(x, y, R)
    got = get_q2y_repeated_kfold(on, n_splits=3, n_repeats=1, per_component=True)
    _masked(on.q2y_report_)
    want = get_q2y_repeated_kfold(off, n_splits=3, n_repeats=1, per_component=True)
    assert _rel(got["q2y"], want["q2y"]) <= 1e-10


@pytest.mark.parametrize("case", ["side65", "m65", "r17"])
def test_past_the_limits_declines_to_refits(case):
    shape, M, R = {"side65": ((8, 65, 65), 2, 1), "m65": ((20, 6, 5), 65, 2), "r17": ((40, 6, 5), 2, 17)}[case]
    x, y = _data(shape, M, R, 0.05, seed=73)
    on, off = _pair(x, y, R)
    got = get_q2y_repeated_kfold(on, n_splits=2, n_repeats=1, per_component=True)
    rep = on.q2y_report_
    assert rep["form"] == "one refit per fold and split on the regular engine", rep
    assert rep["why"].startswith(f"the masked form ({MODELS_FORM}) declined: shape outside"), rep
    want = get_q2y_repeated_kfold(off, n_splits=2, n_repeats=1, per_component=True)
    np.testing.assert_array_equal(got["q2y"], want["q2y"])


# ---- 8. chunks -------------------------------------------------------------------------------------------------------------------
def test_chunked_launches_are_bit_identical():
    from cmtf_pls_amd.backend import HipBackend
    be = HipBackend(torch.device(_DEV))
    x, y = _data((36, 7, 6), 3, 3, 0.1, seed=79)
    I, (A, B), R, M = 36, (7, 6), 3, 3
    X2 = torch.from_numpy(x.reshape(I, -1)).to(_DEV)
    Y2 = torch.from_numpy(y.reshape(I, -1)).to(_DEV)
    rng = np.random.default_rng(11)
    counts = torch.from_numpy(rng.integers(0, 3, size=(9, I)).astype(np.int32)).to(_DEV)
    yrow = torch.from_numpy(np.stack([rng.permutation(I) for _ in range(9)]).astype(np.int32)).to(_DEV)
    one = be.cv_masked_models(X2, Y2, counts, yrow, A, B, R, 1e-8, 100, factors=True)
    assert one["launches"] == 1
    per = int(be.lib.cmtfpls_cv_masked_model_workspace_bytes(I, A, B, M, R)) + R * I * M * 8
    for budget, launches in ((per, 9), (2 * per, 5), (4 * per + 7, 3)):
        many = be.cv_masked_models(X2, Y2, counts, yrow, A, B, R, 1e-8, 100, factors=True, max_ws_bytes=budget)
        assert many["launches"] == launches
        for key, v in one.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v, many[key]), key


# ---- 9. float32 model ------------------------------------------------------------------------------------------------------------
def test_float32_model_computes_in_float64():
    x, y = _data((30, 6, 5), 2, 2, 0.1, seed=83)
    on, off = _pair(x, y, 2, dtype="float32")
    got = permutation_test_q2y(on, n_permutations=3, n_splits=3, per_component=True)
    _masked(on.q2y_report_)
    want = permutation_test_q2y(off, n_permutations=3, n_splits=3, per_component=True)
    assert _rel(got["null"], want["null"]) <= 1e-10


# ---- 10. no behaviour change -----------------------------------------------------------------------------------------------------
def test_option_off_without_nan_or_coupled_keeps_todays_forms():
    x, y = _data((30, 6, 5), 2, 2, 0.1, seed=89)
    off = tPLS(2, dtype="float64", options=OFF)
    off.fit(x, y)
    permutation_test_q2y(off, n_permutations=2, n_splits=3)
    assert off.q2y_report_["form"] == "one refit per fold and permutation on the regular engine"
    assert MODELS_FORM not in off.q2y_report_["why"]
    get_q2y_repeated_kfold(off, n_splits=3, n_repeats=2)
    assert off.q2y_report_["form"] == "one refit per fold and split on the regular engine"
    bootstrap_factors(off, n_resamples=2)
    assert off.bootstrap_report_["form"] == "one refit per resample on the regular engine"

    xc, _ = _data((30, 6, 5), 2, 2, 0.0, seed=89)                      # no NaN: today's shared-read device forms
    full = tPLS(2, dtype="float64", options=ON)
    full.fit(xc, y)
    permutation_test_q2y(full, n_permutations=2, n_splits=3)
    assert full.q2y_report_["form"].startswith("6 models per pass (2 permutations x 3 folds)"), full.q2y_report_
    get_q2y_repeated_kfold(full, n_splits=3, n_repeats=2)
    assert "splits x 3 folds) from shared reads of X" in full.q2y_report_["form"], full.q2y_report_
    bootstrap_factors(full, n_resamples=2)
    assert full.bootstrap_report_["form"].startswith("2 resamples per pass from shared reads of X"), full.bootstrap_report_

    cm = ctPLS(2, dtype="float64", options=ON)                           # coupled: today's routing
    cm.fit([x, x[:, :, :3].copy()], y)
    permutation_test_q2y(cm, n_permutations=2, n_splits=3)
    assert cm.q2y_report_["form"] == "one refit per fold and permutation on the regular engine"
    assert cm.q2y_report_["why"] == "coupled model: permutation device form not built"
    get_q2y_repeated_kfold(cm, n_splits=3, n_repeats=2)
    assert MODELS_FORM not in cm.q2y_report_["form"] and MODELS_FORM not in cm.q2y_report_.get("why", "")
    bootstrap_factors(cm, n_resamples=2)
    assert MODELS_FORM not in cm.bootstrap_report_["form"] and MODELS_FORM not in cm.bootstrap_report_.get("why", "")
