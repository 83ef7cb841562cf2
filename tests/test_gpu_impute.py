"""GPU: validate.impute and validate.get_q2x_heldout on the HIP backend (cmtfpls_impute_*, cmtfpls_holdout_mask_*,
cmtfpls_heldout_resid_*) against X_reconstructed, transform and the literal host loop of tests/impute_ref.py."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.validate import get_q2x_heldout, impute
from impute_ref import literal_q2x, masked_copy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 3


def _tensor(nan, seed, f32):
    x, y, cp = O.import_synthetic((60, 8, 6), 3, R, error=0.3, seed=seed)
    if f32:
        x = x.astype(np.float32).astype(np.float64)                     # representable in the storage type
    x[np.random.default_rng(seed).random(x.shape) < nan] = np.nan
    return x, y, cp


def _coupled(nan, seed):
    x, y, cp = _tensor(nan, seed, False)
    rng = np.random.default_rng(seed + 1)
    xm = cp.factors[0] @ rng.normal(size=(5, R)).T + 0.2 * rng.normal(size=(60, 5))
    x4 = np.einsum("ir,jr,kr,lr->ijkl", cp.factors[0], *(rng.normal(size=(d, R)) for d in (3, 2, 4))) + 0.2 * rng.normal(size=(60, 3, 2, 4))
    xm[rng.random(xm.shape) < nan] = np.nan
    x4[rng.random(x4.shape) < nan] = np.nan
    return [x, xm, x4], y


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_impute_training_rows(dtype):
    f32 = dtype == "float32"
    x, y, _ = _tensor(0.15, 3, f32)
    m = tPLS(R, dtype=dtype, device=DEV)
    m.fit(x, y)
    gap = np.isnan(x)
    filled = impute(m)
    assert isinstance(filled, np.ndarray) and filled.dtype == x.dtype
    assert np.array_equal(filled[~gap], x[~gap]) and np.isfinite(filled).all()
    np.testing.assert_allclose(filled[gap], m.X_reconstructed()[gap], rtol=1e-6 if f32 else 1e-12, atol=0 if f32 else 1e-12)
    rep = m.imputation_report_
    assert rep["form"] == "fitted scores + imputation pass" and rep["why"] is None
    assert rep["imputed"] == [int(gap.sum())] and rep["x_reads"] == [1] and rep["in_place_on_private_copy"] == [True]
    off = impute(m, device=False)
    assert m.imputation_report_["form"] == "torch fallback" and np.array_equal(off[~gap], x[~gap])
    np.testing.assert_allclose(off[gap], filled[gap], rtol=1e-6 if f32 else 1e-12, atol=0 if f32 else 1e-12)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_impute_new_rows_and_device_tensor(dtype, monkeypatch):
    f32 = dtype == "float32"
    x, y, _ = _tensor(0.1, 4, f32)
    m = tPLS(R, dtype=dtype, device=DEV)
    m.fit(x, y)
    xn, _, _ = _tensor(0.2, 9, f32)
    xn = xn[:17]
    td = torch.float32 if f32 else torch.float64
    xt = torch.from_numpy(xn).to(device=DEV, dtype=td)
    before = xt.clone()
    eng = m._get_engine()
    handed = []
    inner = eng.impute_rows
    monkeypatch.setattr(eng, "impute_rows", lambda st, Xs, T, **kw: (handed.append(T.clone()), inner(st, Xs, T, **kw))[1])
    ft = impute(m, xt)
    assert isinstance(ft, torch.Tensor) and ft.is_cuda and ft.dtype == td and ft.data_ptr() != xt.data_ptr()
    assert torch.equal(xt.view(torch.int32 if f32 else torch.int64), before.view(torch.int32 if f32 else torch.int64))   # caller's tensor untouched
    T = m.transform(xt)                                                  # rows with missing values: the masked sequence
    assert len(handed) == 1 and np.isnan(xn).any(axis=(1, 2)).any()
    assert np.array_equal(handed[0].cpu().numpy().view(np.int64), T.view(np.int64))        # the scores impute used: bitwise transform's
    gap = np.isnan(xn)
    fh = ft.cpu().numpy()
    assert np.array_equal(fh[~gap], xt.cpu().numpy()[~gap])
    W = m.X_factors[1][:, None, :] * m.X_factors[2][None, :, :]
    want = np.einsum("ir,jkr->ijk", T, W) + m.X_mean
    np.testing.assert_allclose(fh[gap], want[gap], rtol=1e-6 if f32 else 1e-12, atol=0 if f32 else 1e-12)
    assert m.imputation_report_["rows"] == 17 and m.imputation_report_["in_place_on_private_copy"] == [False]
    fc = impute(m, xt.cpu())                                             # a host tensor comes back on the host, the same fill
    assert isinstance(fc, torch.Tensor) and fc.device.type == "cpu" and fc.dtype == td and torch.equal(fc, ft.cpu())
    fn = impute(m, xn)                                                   # NumPy in, NumPy out, the same fill
    assert isinstance(fn, np.ndarray) and fn.dtype == xn.dtype and np.array_equal(fn[~gap], xn[~gap])
    assert np.array_equal(fn[gap], fh.astype(np.float64)[gap])


def test_impute_ctpls():
    Xs, y = _coupled(0.15, 5)
    m = ctPLS(R, device=DEV)
    m.fit(Xs, y)
    filled = impute(m)
    rec = m.Xs_reconstructed()
    assert m.imputation_report_["imputed"] == [int(np.isnan(x).sum()) for x in Xs] and m.imputation_report_["why"] is None
    for x, f, r in zip(Xs, filled, rec):
        gap = np.isnan(x)
        assert np.array_equal(f[~gap], x[~gap])
        np.testing.assert_allclose(f[gap], r[gap], rtol=1e-12, atol=1e-12)


def _model_bits(m):
    fs = m.Xs_factors if isinstance(m, ctPLS) else [m.X_factors]
    return [a.copy() for f in fs for a in f] + [m.Y_factors[1].copy(), np.asarray(m.coef_).copy(), m._state.T.clone().cpu().numpy()]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_q2x_tpls_against_the_literal_loop(dtype):
    x, y, _ = _tensor(0.1, 6, dtype == "float32")
    m = tPLS(R, dtype=dtype, device=DEV)
    m.fit(x, y)
    bits, x0 = _model_bits(m), x.copy()
    out = get_q2x_heldout(m, fraction=0.2, n_repeats=3, random_state=7)
    assert m.q2x_report_["why"] is None and m.q2x_report_["mask"] == "cmtfpls_holdout_mask"
    sums, q2x, q2x_all, bounds = literal_q2x(lambda: tPLS(R, dtype=dtype, device=DEV), x, y, R, 0.2, out["seeds"])
    print(f"q2x tPLS {dtype}: max |device - literal loop| = {np.abs(out['q2x'] - q2x).max():.3g}")
    np.testing.assert_allclose(out["q2x"], q2x, rtol=0, atol=1e-8)
    np.testing.assert_allclose(out["q2x_all"], q2x_all, rtol=0, atol=1e-8)
    assert np.array_equal(out["n_heldout"][:, 0], [masked_copy(x, 0.2, int(s))[1][0] for s in out["seeds"]])
    again = get_q2x_heldout(m, fraction=0.2, n_repeats=3, random_state=7)
    assert np.array_equal(again["q2x"], out["q2x"]) and np.array_equal(again["n_heldout"], out["n_heldout"])
    other = get_q2x_heldout(m, fraction=0.2, n_repeats=3, random_state=8)
    assert not np.array_equal(other["n_heldout"], out["n_heldout"]) and not np.array_equal(other["q2x"], out["q2x"])
    host = get_q2x_heldout(m, fraction=0.2, n_repeats=3, random_state=7, device=False)
    assert m.q2x_report_["form"] == "torch fallback" and np.array_equal(host["n_heldout"], out["n_heldout"])
    # the two forms see the same masked bits and the same refit, and each form's sums lie within the bound of kernel check 2 of
    # the exact sums: with num_r and den off by at most `bound` each, Q2X_r = 1 - num_r / den moves by at most
    # bound / den (1 + num_r / den) per form (first order), twice that between the two forms
    den = sums[:, :, R:R + 1]
    q_tol = 2.0 * bounds[:, :, None] / den * (1.0 + sums[:, :, :R] / den)
    diff = np.abs(host["q2x"] - out["q2x"])
    print(f"q2x tPLS {dtype}: device=False against device=True, max difference / bound = {(diff / q_tol).max():.3g}")
    assert (diff <= q_tol).all()
    assert all(np.array_equal(a, b) for a, b in zip(_model_bits(m), bits))
    assert m.original_X is x and np.array_equal(np.nan_to_num(x, nan=7.5), np.nan_to_num(x0, nan=7.5))


def test_q2x_ctpls_against_the_literal_loop():
    Xs, y = _coupled(0.1, 8)
    m = ctPLS(R, device=DEV)
    m.fit(Xs, y)
    bits = _model_bits(m)
    out = get_q2x_heldout(m, fraction=0.1, n_repeats=2, random_state=3)
    assert out["q2x"].shape == (2, 3, R) and m.q2x_report_["why"] is None
    sums, q2x, q2x_all, _ = literal_q2x(lambda: ctPLS(R, device=DEV), Xs, y, R, 0.1, out["seeds"])
    print(f"q2x ctPLS: max |device - literal loop| = {np.abs(out['q2x'] - q2x).max():.3g}")
    np.testing.assert_allclose(out["q2x"], q2x, rtol=0, atol=1e-8)
    np.testing.assert_allclose(out["q2x_all"], q2x_all, rtol=0, atol=1e-8)
    assert np.array_equal(out["n_heldout"], sums[:, :, -1].astype(np.int64))
    assert all(np.array_equal(a, b) for a, b in zip(_model_bits(m), bits))
