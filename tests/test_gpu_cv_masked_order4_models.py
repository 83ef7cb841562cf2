"""The count-weighted models of a tPLS whose X has order 4 AND missing values, every model refitted by one 512-thread workgroup
(cmtfpls_cv_masked_tensor_models_f64, EngineOptions.masked_tensor_folds): 0/1 counts against the fold entry, counts > 1
against a refit on the literally repeated rows (predictions and factors), a permuted yrow against a refit on the permuted Y, the
statuses, and the permutation test, repeated K-fold and the bootstrap against the same call with device_folds=False, which refits
every model on the regular engine.  Every end-to-end test checks the report's form first.

Tolerances are those of test_gpu_kfold_order4.py for order 4: predictions 1e-7 relative, Q2Y 1e-8; the factors, from which the
predictions are formed, take the predictions' 1e-7 (normwise per component).  Data: (40, 6, 5, 4), M 3, R 3, 10 % NaN, seed 40; for
every model below the float64 oracle's inner loop converges below max_iter (at most 35 passes), every column is observed in
every training part and no training row is empty."""
import functools

import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import MODELS_TENSOR_FORM, TENSOR_RANK1, fold_ids, masked_models, refit_fold
from cmtf_pls_amd.validate import bootstrap_factors, get_q2y_repeated_kfold, permutation_test_q2y

pytestmark = pytest.mark.gpu

_DEV = "cuda:0"
ON = EngineOptions(small_fit=False, masked_tensor_folds=True)
REGULAR = EngineOptions(small_fit=False)
SHAPE, M, R = (40, 6, 5, 4), 3, 3
I, (A, B1, B2) = SHAPE[0], SHAPE[1:]
PRED_TOL, Q2Y_TOL = 1e-7, 1e-8


@functools.lru_cache(maxsize=None)
def _data():
    x, y, _ = O.import_synthetic(SHAPE, M, R + 1, error=0.3, seed=40)
    x[np.random.default_rng(140).random(x.shape) < 0.1] = np.nan
    return x, y


@functools.lru_cache(maxsize=None)
def _model():
    x, y = _data()
    m = tPLS(R, dtype="float64", options=ON)
    m.fit(x, y)
    return m


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float(np.abs(got[ok] - want[ok]).max() / max(np.abs(want[ok]).max(), 1e-300)) if ok.any() else 0.0


def _tensor(rep):
    assert MODELS_TENSOR_FORM in rep["form"] and rep["rank1"] == TENSOR_RANK1, rep
    assert rep["x_reads"] is None and rep["models"] >= 1 and rep["launches"] >= 1 and "masked_models" in rep and "masked_batches" in rep, rep
    return rep


def _dev(a, dt=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=_DEV, dtype=dt)


def _backend():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(_DEV))


# ---- 1. 0/1 counts are the fold entry's folds -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, None])
def test_zero_one_counts_equal_the_fold_entry(K):
    be = _backend()
    x, y = _data()
    ids, K = (np.arange(I), I) if K is None else fold_ids(I, K)
    X2, Y2 = _dev(x.reshape(I, -1)), _dev(y.reshape(I, -1))
    folds = be.cv_masked_tensor(X2, Y2, _dev(ids, torch.int32), K, A, B1, B2, R, 1e-8, 100)
    counts = (ids[None, :] != np.arange(K)[:, None]).astype(np.int32)
    got = be.cv_masked_tensor_models(X2, Y2, _dev(counts, torch.int32), None, A, B1, B2, R, 1e-8, 100)
    assert not got["status"].any() and not folds[2].any()
    pred = sum(got["Ypred"][k] for k in range(K))                        # each model writes only its own fold's rows
    dev = _rel(pred.cpu(), folds[0].cpu())
    print(f"models entry against the fold entry, K = {K}: {dev:.3e}")
    assert dev <= 1e-12
    assert torch.equal(got["n_iter"], folds[1]) and torch.equal(got["info"], folds[3])


# ---- 2. counts > 1 are literally repeated rows ----------------------------------------------------------------------------------
def test_counts_equal_a_refit_on_repeated_rows():
    be = _backend()
    x, y = _data()
    c = np.random.default_rng(7).integers(0, 4, size=(3, I))
    c[:, :4] = 0
    c[:, 5] = 3
    got = be.cv_masked_tensor_models(_dev(x.reshape(I, -1)), _dev(y.reshape(I, -1)), _dev(c, torch.int32), None, A, B1, B2, R, 1e-8, 100,
                                     factors=True)
    got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}
    assert not got["status"].any() and got["info"][:, 0].all()
    for j in range(3):
        idx, held = np.repeat(np.arange(I), c[j]), np.flatnonzero(c[j] == 0)
        ref = tPLS(R, dtype="float64", options=REGULAR)
        ref.fit(x[idx], y[idx])
        sc = ref.transform(x[held])
        for r in range(1, R + 1):
            want = (sc[:, :r] @ ref.coef_[:r, :r]) @ ref.Y_factors[1][:, :r].T + ref.Y_mean
            dev = _rel(got["Ypred"][j, r - 1][held], want.reshape(len(held), M))
            print(f"model {j}, {r} components: predictions {dev:.3e}")
            assert dev <= PRED_TOL
        assert not got["Ypred"][j][:, c[j] > 0].any()                     # nothing written where the model trained
        assert got["n_iter"][j].tolist() == [int(v) for v in ref.n_iter_]
        d = np.ones(R)                                                    # the refit's sign: per component, the product over the modes
        for key, f in (("Wa", ref.X_factors[1]), ("Wk", ref.X_factors[2]), ("Wl", ref.X_factors[3])):
            w = got[key][j].T                                             # dim x R, as the refit's
            assert w.shape == np.asarray(f).shape
            s = np.where((w * f).sum(axis=0) < 0, -1.0, 1.0)
            d *= s
            dev = max(np.linalg.norm(w[:, a] * s[a] - f[:, a]) / np.linalg.norm(f[:, a]) for a in range(R))
            print(f"model {j}: {key} {dev:.3e}")
            assert dev <= PRED_TOL
        q_dev = max(np.linalg.norm(got["Q"][j][a] * d[a] - ref.Y_factors[1][:, a]) / np.linalg.norm(ref.Y_factors[1][:, a]) for a in range(R))
        coef = got["coef"][j] * d[:, None] * d[None, :]
        c_dev = np.abs(coef - ref.coef_).max() / np.abs(ref.coef_).max()
        print(f"model {j}: Q {q_dev:.3e}, coef {c_dev:.3e}")
        assert q_dev <= PRED_TOL and c_dev <= PRED_TOL


# ---- 3. a permuted yrow is a refit on the permuted Y ----------------------------------------------------------------------------
def test_permuted_yrow_equals_a_refit_on_permuted_y():
    x, y = _data()
    m = _model()
    ids, K = fold_ids(I, 4)
    perm = np.random.default_rng(9).permutation(I)
    counts = (ids[None, :] != np.arange(K)[:, None]).astype(np.int32)
    out, why = masked_models(m, x, y, counts, np.broadcast_to(perm.astype(np.int32), (K, I)).copy(), 1e-8, 100)
    assert why is None and not out["status"].any() and out["tensor"] == (B1, B2)
    ref = tPLS(R, dtype="float64", options=REGULAR)
    ref.fit(x, y)
    for k in range(K):
        test = ids == k
        want, n_iter = refit_fold(ref, x, y[perm], test, 1e-8, 100)
        dev = _rel(out["Ypred"][k][:, test], want)
        print(f"permuted Y, fold {k}: {dev:.3e}")
        assert dev <= PRED_TOL and out["n_iter"][k].tolist() == n_iter


# ---- 4. statuses ----------------------------------------------------------------------------------------------------------------
def test_statuses():
    be = _backend()
    x, y = _data()
    c = np.ones((4, I), np.int32)
    c[:, :5] = 0
    c[1, 7] = -1                                                          # a negative count
    c[2] = 0
    c[2, 9] = 1                                                           # one training row
    yrow = np.broadcast_to(np.arange(I, dtype=np.int32), (4, I)).copy()
    yrow[3, 0] = I                                                        # a Y row outside 0..I-1
    got = be.cv_masked_tensor_models(_dev(x.reshape(I, -1)), _dev(y.reshape(I, -1)), _dev(c, torch.int32), _dev(yrow, torch.int32),
                                     A, B1, B2, R, 1e-8, 100, factors=True)
    assert got["status"].tolist() == [0, 3, 2, 3]
    for key in ("Ypred", "Wa", "Wk", "Wl", "coef", "Q"):                  # a model with a status writes nothing else
        assert got[key][0].any() and not got[key][1:].any(), key


# ---- 5. permutation test ----------------------------------------------------------------------------------------------------------
def test_permutation_test_equals_refits():
    m = _model()
    got = permutation_test_q2y(m, n_permutations=7, n_splits=4, per_component=True)
    rep = _tensor(m.q2y_report_)
    assert rep["models"] == 28 and rep["permutations"] == 7 and np.asarray(rep["n_iter"]).shape == (7, 4, R)
    assert rep["masked_models"] == 28 and "refitted" not in rep
    assert MODELS_TENSOR_FORM.replace("_models", "") in rep["observed"]["form"]         # the observed value: the fold entry
    want = permutation_test_q2y(m, n_permutations=7, n_splits=4, per_component=True, device_folds=False)
    assert m.q2y_report_["form"] == "one refit per fold and permutation on the regular engine"
    dev = np.abs(got["null"] - want["null"]).max()
    print(f"permutation null: largest deviation {dev:.3e}; observed {np.abs(got['q2y'] - want['q2y']).max():.3e}")
    assert dev <= Q2Y_TOL and np.abs(got["q2y"] - want["q2y"]).max() <= Q2Y_TOL
    assert rep["n_iter"] == m.q2y_report_["n_iter"]
    np.testing.assert_array_equal(got["permutations"], want["permutations"])


# ---- 6. repeated K-fold -----------------------------------------------------------------------------------------------------------
def test_repeated_kfold_equals_refits():
    m = _model()
    got = get_q2y_repeated_kfold(m, n_splits=4, n_repeats=3, per_component=True)
    rep = _tensor(m.q2y_report_)
    assert rep["models"] == 12 and rep["splits"] == 3
    want = get_q2y_repeated_kfold(m, n_splits=4, n_repeats=3, per_component=True, device_folds=False)
    assert m.q2y_report_["form"] == "one refit per fold and split on the regular engine"
    for key in ("q2y", "mean", "std"):
        dev = np.abs(got[key] - want[key]).max()
        print(f"repeated K-fold {key}: {dev:.3e}")
        assert dev <= Q2Y_TOL, key
    assert rep["n_iter"] == m.q2y_report_["n_iter"]
    np.testing.assert_array_equal(got["folds"], want["folds"])


# ---- 7. bootstrap -----------------------------------------------------------------------------------------------------------------
def test_bootstrap_equals_refits():
    m = _model()
    got = bootstrap_factors(m, n_resamples=8, random_state=0)
    rep = _tensor(m.bootstrap_report_)
    assert rep["models"] == 8 and rep["resamples"] == 8 and "refitted" not in rep and np.asarray(rep["n_iter"]).shape == (8, R)
    want = bootstrap_factors(m, n_resamples=8, random_state=0, device_folds=False)
    assert m.bootstrap_report_["form"] == "one refit per resample on the regular engine"
    assert rep["n_iter"] == m.bootstrap_report_["n_iter"]
    np.testing.assert_array_equal(got["resamples"], want["resamples"])
    assert [s.shape for s in got["se"]["X_factors"]] == [(A, R), (B1, R), (B2, R)]      # a per-mode std for three modes
    for mode, (a, b) in enumerate(zip(got["X_factors"], want["X_factors"])):
        assert a.shape == b.shape == (8, (A, B1, B2)[mode], R)
        dev = max(np.linalg.norm(a[e][:, c] - b[e][:, c]) / np.linalg.norm(b[e][:, c]) for e in range(8) for c in range(R))
        print(f"bootstrap mode {mode + 1}: {dev:.3e}")
        assert dev <= PRED_TOL
    for a, b in zip(got["se"]["X_factors"], want["se"]["X_factors"]):
        assert np.abs(a - b).max() <= PRED_TOL * max(np.abs(b).max(), 1.0)
    dev = np.abs(got["oob_q2y"] - want["oob_q2y"]).max()
    print(f"out-of-bag Q2Y: {dev:.3e}")
    assert dev <= Q2Y_TOL and got["oob_rows"] == want["oob_rows"]
