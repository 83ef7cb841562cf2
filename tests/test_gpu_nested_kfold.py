"""Nested K-fold Q2Y on the device (validate.get_q2y_nested_kfold, cmtf_pls_amd/nested.py): cmtfpls_press_rows_f64 alone against a
float64 NumPy restatement of its formula at the corners of its limits; the device form (0/1-weighted models of the bootstrap's
pass, scored by that kernel) against the device K-fold paths that already exist and against its own refit path; the report."""
import math

import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.backend import HipBackend
from cmtf_pls_amd.nested import torch_press
from cmtf_pls_amd.validate import get_q2y_kfold, get_q2y_nested_kfold

pytestmark = pytest.mark.gpu

_TOL = {"float64": 1e-8, "float32": 1e-5}          # tests/test_gpu_bootstrap.py's: the weighted form against literal refits
_U = 2.0 ** -53


def _kernel_inputs(n, I, R, M, seed):
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((n, I, R))
    coef = np.triu(rng.standard_normal((n, R, R)))
    Q = rng.standard_normal((n, R, M))
    nu = rng.standard_normal((n, M))
    Y = rng.standard_normal((I, M))
    ev = rng.choice([0, 1], size=(n, I), p=[0.6, 0.4]).astype(np.int32)
    owner = rng.integers(-1, n, size=I)                          # the one model that may write a row's predictions; -1: none
    ev[owner[owner >= 0], np.flatnonzero(owner >= 0)] = 2
    ev[1] = 0                                                    # a model with no evaluated row
    if I > 1024:
        ev[0, :1024] = 0                                         # and a model with none in a whole row tile
    T[ev == 0] = np.nan                                          # skipped rows never enter a sum
    return T, coef, Q, nu, Y, ev


def _reference(T, coef, Q, nu, Y, ev):
    """The formula of include/cmtfpls.h restated in float64 NumPy: (press (n, R), pred (R, I, M) with NaN where no model writes,
    mag (n, R): per entry of press the sum over its rows and responses of A^2, apred (R, I, M): A per entry of pred), A = |nu| +
    sum_c sum_k |t_k coef_kc q_cm| (+ |y| for press) the sum of the magnitudes of the terms of one prediction error."""
    n, I, R = T.shape
    M = Y.shape[1]
    press, mag = np.zeros((n, R)), np.zeros((n, R))
    pred, apred = np.full((R, I, M), np.nan), np.zeros((R, I, M))
    for j in range(n):
        rows = np.flatnonzero(ev[j] > 0)
        if not rows.size:
            continue
        C = np.cumsum((T[j, rows] @ coef[j])[:, :, None] * Q[j][None], axis=1) + nu[j]                       # rows x R x M
        A = np.cumsum((np.abs(T[j, rows]) @ np.abs(coef[j]))[:, :, None] * np.abs(Q[j])[None], axis=1) + np.abs(nu[j])
        press[j] = ((C - Y[rows][:, None, :]) ** 2).sum(axis=(0, 2))
        mag[j] = ((A + np.abs(Y[rows])[:, None, :]) ** 2).sum(axis=(0, 2))
        w = ev[j, rows] == 2
        pred[:, rows[w]] = C[w].transpose(1, 0, 2)
        apred[:, rows[w]] = A[w].transpose(1, 0, 2)
    return press, pred, mag, apred


@pytest.mark.parametrize("n,I", [(2, 2500), (32, 1100)])
@pytest.mark.parametrize("M", [1, 16, 64])
@pytest.mark.parametrize("R", [1, 16, 64])
def test_press_rows_kernel_against_numpy(R, M, n, I):
    """Tolerance, from the operation count.  One prediction error e = nu + sum_c h_c q_cm - y, h_c = sum_k t_k coef_kc, is a sum of
    at most R products into h, R fused multiply-adds and one subtraction: |de| <= (2R + 2) u A with u = 2^-53 and A the sum of the
    magnitudes of its terms, so |d(e^2)| <= 2 A |de| <= (4R + 4) u A^2.  An entry of press adds I M such squares; added pairwise or
    in short chains (what both NumPy and a tiled kernel do) that costs about log2(I M) u times their sum, which is <= sum A^2.
    Kernel and reference each carry that error: |press - ref| <= 2 (4R + 4 + log2(I M)) u sum A^2 <= 8 (R + log2(I M)) u sum A^2
    once log2(I M) >= 2: a small multiple of (R + log2 I) 2^-53 relative to the sum of the terms' magnitudes.  A
    prediction is the same sum without the subtraction and the square: |pred - ref| <= 2 (2R + 1) u A."""
    be = HipBackend(torch.device("cuda:0"))
    T, coef, Q, nu, Y, ev = _kernel_inputs(n, I, R, M, seed=1000 * R + 10 * M + n)
    want, want_pred, mag, apred = _reference(T, coef, Q, nu, Y, ev)
    dev = [torch.from_numpy(a).to(be.device) for a in (T, coef, Q, nu, Y, ev)]
    sentinel = -7.0
    pred = torch.full((R, I, M), sentinel, dtype=torch.float64, device=be.device)
    press = be.press_rows(*dev, pred)
    assert press is not None and press.shape == (n, R)
    got, got_pred = press.cpu().numpy(), pred.cpu().numpy()
    bound = 8.0 * (R + math.log2(I * M)) * _U * mag
    err = np.abs(got - want)
    print(f"R={R} M={M} n={n} I={I}: max |press - ref| / bound = {float((err[mag > 0] / bound[mag > 0]).max()):.3g}")
    assert np.all(np.isfinite(got)) and np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    assert np.array_equal(got[1], np.zeros(R))                   # no evaluated row: exactly 0
    written = ~np.isnan(want_pred)
    assert np.array_equal(got_pred[~written], np.full((~written).sum(), sentinel))       # rows without eval == 2 are left alone
    perr = np.abs(got_pred[written] - want_pred[written])
    assert np.all(perr <= 2.0 * (2 * R + 1) * _U * apred[written]), float(perr.max())
    again = be.press_rows(*dev, torch.full_like(pred, sentinel))
    assert torch.equal(again, press)                             # a fixed order of sums: the same bits
    assert torch.equal(be.press_rows(*dev, None), press)         # pred is optional


def test_press_rows_declines_shapes_outside_its_limits_and_torch_ops_agree():
    be = HipBackend(torch.device("cuda:0"))
    for R, M in ((65, 3), (3, 65)):
        T, coef, Q, nu, Y, ev = _kernel_inputs(2, 70, R, M, seed=5)
        dev = [torch.from_numpy(a).to(be.device) for a in (T, coef, Q, nu, Y, ev)]
        assert be.press_rows(*dev, None) is None
        want, want_pred, _, _ = _reference(T, coef, Q, nu, Y, ev)
        pred = torch.full((R, 70, M), np.nan, dtype=torch.float64, device=be.device)
        got = torch_press(*dev, pred)                            # what nested.py scores such a shape with
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-11, atol=0)
        np.testing.assert_allclose(pred.cpu().numpy(), want_pred, rtol=1e-11, atol=1e-12, equal_nan=True)


# name, block shapes, M, R, K_o, K_i, models per pass, passes: seed 1 leaves a gap of > 3e-2 between the best and the second-best
# inner_q2y of every outer fold on the refit path (found on the CPU with the NumPy backend; asserted below before selected is compared)
CASES = [
    ("order 2", [(60, 30)], 3, 3, 3, 4, 15, 1),
    ("order 3", [(50, 10, 8)], 4, 3, 5, 5, 30, 1),
    ("M 1", [(45, 9, 7)], 1, 3, 3, 3, 12, 1),
    ("two passes", [(72, 6, 5)], 2, 2, 6, 5, 30, 2),
    ("32 models", [(64, 8, 6)], 2, 3, 4, 7, 32, 1),
    ("coupled", [(50, 6, 5), (50, 7)], 3, 3, 3, 4, 15, 1),
]
_SEED = 1


def _data(shapes, M, R, dtype):
    x, y, _ = O.import_synthetic(shapes[0], M, R + 1, error=0.3, seed=_SEED)
    Xs = [x]
    for b, s in enumerate(shapes[1:]):
        Xs.append(np.random.default_rng(_SEED + 1 + b).standard_normal(s) + 0.1 * x.reshape(s[0], -1)[:, :1])
    if dtype == "float32":
        Xs = [X.astype(np.float32).astype(np.float64) for X in Xs]
    return Xs, y


def _fit(Xs, y, R, dtype):
    coupled = len(Xs) > 1
    m = (ctPLS if coupled else tPLS)(R, dtype=dtype)
    m.fit(Xs if coupled else Xs[0], y)
    return m


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(np.abs(np.asarray(want)).max(), 1e-300))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name,shapes,M,R,Ko,Ki,G,passes", CASES, ids=[c[0] for c in CASES])
def test_device_form_against_device_kfold_and_refits(name, shapes, M, R, Ko, Ki, G, passes, dtype):
    Xs, y = _data(shapes, M, R, dtype)
    coupled = len(Xs) > 1
    m = _fit(Xs, y, R, dtype)
    res = get_q2y_nested_kfold(m, n_outer=Ko, n_inner=Ki, random_state=_SEED)
    rep = m.q2y_report_
    n = Ko * (Ki + 1)
    assert "cmtfpls_press_rows_f64" in rep["form"] and "cmtfpls_kfold_weighted_xcov_*" in rep["form"], rep
    assert "cmtfpls_kfold_epilogue_weighted_f64" in rep["form"] and "torch ops" not in rep["form"] and "why" not in rep, rep
    assert ("cmtfpls_kfold_inner_coupled_f64" if coupled else "cmtfpls_kfold_inner_f64") in rep["form"], rep
    assert rep["models"] == n and rep["models_per_pass"] == G and rep["passes"] == passes, rep
    assert rep["x_reads"] == ([passes * 2 * R] * len(Xs) if coupled else passes * 2 * R)
    assert np.array(rep["n_iter"]).shape == (n, R)
    outer, inner = res["outer_folds"], res["inner_folds"]

    # the weighted build against the all-minus-own build of the device K-fold (both on the device, independent code paths)
    q_outer = get_q2y_kfold(m, folds=outer, per_component=True)
    assert "cmtfpls_kfold_xcov_*" in m.q2y_report_["form"], m.q2y_report_
    print(f"{name} {dtype}: max |outer_q2y - kfold| = {np.abs(res['outer_q2y'] - q_outer).max():.3g}")
    np.testing.assert_allclose(res["outer_q2y"], q_outer, rtol=0, atol=1e-8)
    for o in range(Ko):
        tr = outer != o
        sub = _fit([X[tr] for X in Xs], y[tr], R, dtype)
        q_inner = get_q2y_kfold(sub, folds=inner[o][tr], per_component=True)
        assert "cmtfpls_kfold_xcov_*" in sub.q2y_report_["form"], sub.q2y_report_
        print(f"{name} {dtype}: outer fold {o} max |inner_q2y - kfold| = {np.abs(res['inner_q2y'][o] - q_inner).max():.3g}")
        np.testing.assert_allclose(res["inner_q2y"][o], q_inner, rtol=0, atol=1e-8)

    # selection, predictions and the nested estimate against the refit path on the same model
    ref = get_q2y_nested_kfold(m, n_outer=Ko, n_inner=Ki, random_state=_SEED, device_folds=False)
    assert m.q2y_report_["form"].startswith("one refit per model") and m.q2y_report_["why"] == "device folds switched off"
    top = np.sort(ref["inner_q2y"], axis=1)
    assert np.all(top[:, -1] - top[:, -2] > 1e-4), top              # a condition on the inputs: no near tie to flip the argmax
    assert np.array_equal(res["selected"], ref["selected"]), (res["selected"], ref["selected"])
    assert np.array_equal(res["selected"], np.argmax(res["inner_q2y"], axis=1) + 1)
    print(f"{name} {dtype}: predictions rel {_rel(res['predictions'], ref['predictions']):.3g}, |q2y - refit| = {abs(res['q2y'] - ref['q2y']):.3g}")
    assert _rel(res["predictions"], ref["predictions"]) <= _TOL[dtype]
    assert abs(res["q2y"] - ref["q2y"]) <= 1e-8 * max(1.0, abs(ref["q2y"]))
    if dtype == "float64":      # (float32 storage: a refit centres its own float32 copy of X[train], a rounding the device form lacks)
        np.testing.assert_allclose(res["inner_q2y"], ref["inner_q2y"], rtol=0, atol=1e-8)
        np.testing.assert_allclose(res["outer_q2y"], ref["outer_q2y"], rtol=0, atol=1e-8)
    assert res["q2y"] == 1 - ((res["predictions"] - y) ** 2).sum() / (y ** 2).sum()


def test_given_splits_and_device_tensors():
    """Given outer and inner splits with unequal folds, on a model fitted to device tensors (the caller's X is never copied)."""
    x, y, _ = O.import_synthetic((54, 7, 6), 2, 3, error=0.3, seed=3)
    rng = np.random.default_rng(0)
    outer = rng.permutation(np.arange(54) % 3)
    outer[:4] = 0
    inner = np.full((3, 54), -1)
    for o in range(3):
        tr = np.flatnonzero(outer != o)
        inner[o, tr] = rng.permutation(np.arange(tr.size) % 4)
    m = tPLS(2, dtype="float64")
    m.fit(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    res = get_q2y_nested_kfold(m, outer_folds=outer, inner_folds=inner)
    assert "cmtfpls_press_rows_f64" in m.q2y_report_["form"] and "why" not in m.q2y_report_, m.q2y_report_
    assert np.array_equal(res["outer_folds"], outer) and np.array_equal(res["inner_folds"], inner)
    ref = get_q2y_nested_kfold(m, outer_folds=outer, inner_folds=inner, device_folds=False)
    np.testing.assert_allclose(res["inner_q2y"], ref["inner_q2y"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(res["outer_q2y"], ref["outer_q2y"], rtol=0, atol=1e-8)


def test_missing_values_refit_and_say_so():
    x, y, _ = O.import_synthetic((40, 6, 5), 2, 3, error=0.3, seed=2)
    x[3, 1, 2] = np.nan
    m = tPLS(2, dtype="float64")
    m.fit(x, y)
    res = get_q2y_nested_kfold(m, n_outer=3, n_inner=3)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per model") and "missing" in rep["why"] and rep["passes"] == 0, rep
    assert np.all(np.isfinite(res["inner_q2y"])) and np.isfinite(res["q2y"])
