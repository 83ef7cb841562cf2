"""Sample diagnostics on the device (validate.sample_diagnostics, cmtf_pls_amd/diagnostics.py): cmtfpls_resid_rows_* against a
float64 torch formula (storage types, unaligned shapes, many row blocks, R 1 / 10 / 16, a NaN score row, bit-identical repeats,
the R = 17 decline), then the estimator on the HIP backend against a float64 NumPy restatement, its read-only behaviour and its
read counts.  Every kernel shape here plans to 8 rows per block; tests/test_gpu_resid_rows_forms.py runs the taller plans, and
the last estimator case runs one of them end to end."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.backend import HipBackend
from cmtf_pls_amd.validate import sample_diagnostics
from diagnostics_ref import check_against_restatement
from resid_rows_ref import resid_plan

pytestmark = pytest.mark.gpu


def _formula(X2, T, WA, WB, mean):
    x = X2.double() - mean
    W = (WA[:, None, :] * WB[None, :, :]).reshape(x.shape[1], -1)
    fin = torch.isfinite(x)
    e = torch.where(fin, x - T @ W.T, 0.0)
    x = torch.where(fin, x, 0.0)
    return (torch.stack([(e * e).sum(1), (x * x).sum(1), fin.sum(1).double()], dim=1),
            torch.stack([(e * e).sum(0), (x * x).sum(0)], dim=1))


def _operands(I, A, B, R, dtype, seed, offset=0, nan_frac=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    P = A * B
    flat = torch.randn(I * P + offset, generator=g, dtype=torch.float64)
    if nan_frac:
        flat[torch.rand(flat.shape, generator=g) < nan_frac] = float("nan")
    X2 = flat.to("cuda", dtype)[offset:].view(I, P)
    T = torch.randn(I, R + 3, generator=g, dtype=torch.float64).cuda()[:, :R]       # a row stride > R
    WA = torch.randn(A, R, generator=g, dtype=torch.float64).cuda()
    WB = torch.randn(B, R, generator=g, dtype=torch.float64).cuda()
    mean = torch.randn(P, generator=g, dtype=torch.float64).cuda()
    return X2, T, WA, WB, mean


RESID_KERNEL_CASES = [
    (1, 3, 8, 1, 0, 0.0),                  # one row
    (5000, 4, 12, 10, 0, 0.1),             # many row blocks, missing values
    (300, 5, 7, 16, 0, 0.0),               # B % 4 != 0: one element per thread
    (257, 6, 8, 10, 1, 0.05),              # a view one element into its storage: misaligned base
    (64, 1, 1030, 10, 0, 0.0),             # a matrix block, columns past a whole tile
    (3000, 8, 160, 10, 0, 0.02),           # two column tiles, the second part dead lanes
    # the shapes of tests/test_gpu_workspace_contract.py, each at R = 1, 5 and 16: B % 4 != 0 with 65 row blocks and a short last
    # one; the vector form, also misaligned; P = 1320: five column tiles and a partial one
    (517, 7, 9, 1, 0, 0.1), (517, 7, 9, 5, 0, 0.1), (517, 7, 9, 16, 0, 0.1),
    (517, 12, 20, 1, 0, 0.1), (517, 12, 20, 5, 0, 0.1), (517, 12, 20, 16, 0, 0.1),
    (517, 12, 20, 1, 1, 0.1), (517, 12, 20, 5, 1, 0.1), (517, 12, 20, 16, 1, 0.1),
    (2100, 33, 40, 1, 0, 0.1), (2100, 33, 40, 5, 0, 0.1), (2100, 33, 40, 16, 0, 0.1),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("I,A,B,R,offset,nan", RESID_KERNEL_CASES)
def test_recon_r2_kernel_against_formula(dtype, I, A, B, R, offset, nan):
    """cmtfpls_recon_r2_*: calcR2X's two sums are the column sums of resid_rows' first two columns (sums of non-negative terms)."""
    be = HipBackend()
    X2, T, WA, WB, mean = _operands(I, A, B, R, dtype, seed=I + R, offset=offset, nan_frac=nan)
    before = X2.clone()
    got = be.recon_r2(X2, T, WA, WB, mean)
    want_r, _ = _formula(X2, T, WA, WB, mean)
    torch.testing.assert_close(got, want_r[:, :2].sum(0), rtol=1e-11, atol=1e-9)
    assert torch.equal(got, be.recon_r2(X2, T, WA, WB, mean))                             # deterministic: the same bits
    bits = torch.int32 if dtype == torch.float32 else torch.int64
    assert torch.equal(X2.view(bits), before.view(bits))                                   # read only


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("I,A,B,R,offset,nan", RESID_KERNEL_CASES)
def test_resid_rows_kernel_against_formula(dtype, I, A, B, R, offset, nan):
    be = HipBackend()
    X2, T, WA, WB, mean = _operands(I, A, B, R, dtype, seed=I + R, offset=offset, nan_frac=nan)
    before = X2.clone()
    rows, cols = be.resid_rows(X2, T, WA, WB, mean, True)
    want_r, want_c = _formula(X2, T, WA, WB, mean)
    torch.testing.assert_close(rows, want_r, rtol=1e-11, atol=1e-9)
    torch.testing.assert_close(cols, want_c, rtol=1e-11, atol=1e-9)
    rows2, cols2 = be.resid_rows(X2, T, WA, WB, mean, True)
    assert torch.equal(rows, rows2) and torch.equal(cols, cols2)                          # deterministic: the same bits
    rows3, none = be.resid_rows(X2, T, WA, WB, mean, False)
    assert none is None and torch.equal(rows3, rows)
    bits = torch.int32 if dtype == torch.float32 else torch.int64
    assert torch.equal(X2.view(bits), before.view(bits))                                   # read only


def test_resid_rows_nan_score_row_and_decline():
    be = HipBackend()
    X2, T, WA, WB, mean = _operands(40, 4, 8, 10, torch.float32, seed=3)
    T = T.contiguous()
    T[7] = float("nan")
    rows, _ = be.resid_rows(X2, T, WA, WB, mean, False)
    assert torch.isnan(rows[7, 0]) and not torch.isnan(rows[:, 0][torch.arange(40, device="cuda") != 7]).any()
    assert rows[7, 1] > 0 and rows[7, 2] == 32
    X2, T, WA, WB, mean = _operands(40, 4, 8, 17, torch.float32, seed=4)
    assert be.resid_rows(X2, T, WA, WB, mean, True) is None


def _fit(shape, R, dtype, nan=0.0, seed=1, coupled=False):
    x, y, cp = O.import_synthetic(shape, 3, 3, error=0.2, seed=seed)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)
    if nan:
        x[np.random.default_rng(seed).random(x.shape) < nan] = np.nan
    if coupled:
        xm = cp.factors[0] @ np.random.default_rng(seed + 1).normal(size=(9, 3)).T + 0.1 * np.random.default_rng(seed + 2).normal(size=(shape[0], 9))
        if dtype == "float32":
            xm = xm.astype(np.float32).astype(np.float64)
        m = ctPLS(R, dtype=dtype)
        m.fit([x, xm], y)
        return m, [x, xm], y
    m = tPLS(R, dtype=dtype)
    m.fit(x, y)
    return m, x, y


@pytest.mark.parametrize("dtype,rtol", [("float64", 1e-9), ("float32", 1e-5)])
@pytest.mark.parametrize("shape,R,nan,coupled", [
    ((60, 12), 3, 0.0, False),
    ((50, 8, 6), 1, 0.0, False),
    ((50, 8, 6), 3, 0.1, False),
    ((40, 5, 4, 3), 3, 0.0, False),
    ((45, 7, 6), 3, 0.1, True),
    ((143357, 2, 4), 3, 0.1, False),       # 70 rows per block in the residual pass: two 64-row chunks, the second of 6 rows
])
def test_estimator_against_restatement(dtype, rtol, shape, R, nan, coupled):
    if shape[0] > 100000:
        assert resid_plan(shape[0], int(np.prod(shape[1:])), 4 if dtype == "float32" else 2) == (1, 2048, 70, 67)
    m, X, y = _fit(shape, R, dtype, nan, coupled=coupled)
    d = sample_diagnostics(m)
    assert m.diagnostics_report_["form"] == "fitted scores + residual pass" and m.diagnostics_report_["x_reads"] == [1] * (2 if coupled else 1)
    check_against_restatement(m, X, y, d, rtol, new=False)
    xn, yn, _ = O.import_synthetic((shape[0] // 2,) + shape[1:], 3, 3, error=0.2, seed=9)
    if dtype == "float32":
        xn = xn.astype(np.float32).astype(np.float64)
    if nan:
        xn[np.random.default_rng(5).random(xn.shape) < nan] = np.nan
    Xn = [xn, (X[1][: xn.shape[0]] + 0.05)] if coupled else xn
    dn = sample_diagnostics(m, Xn, yn)
    assert np.array_equal(dn["scores"], m.transform(Xn))
    check_against_restatement(m, X, y, dn, rtol, new=True, Xn=Xn, yn=yn)


def test_read_only_and_read_counts():
    x, y, _ = O.import_synthetic((300, 16, 12), 3, 3, error=0.2, seed=4)
    xd = torch.from_numpy(x).float().cuda()
    m = tPLS(4, dtype="float32")
    m.fit(xd, y)
    before = xd.clone()
    d = sample_diagnostics(m)
    assert m.diagnostics_report_["x_reads"] == [1] and m.diagnostics_report_["training_stats"] == "computed"
    xn = torch.from_numpy(O.import_synthetic((100, 16, 12), 3, 3, error=0.2, seed=5)[0]).float().cuda()
    xn_before = xn.clone()
    m2 = tPLS(4, dtype="float32")
    m2.fit(xd, y)
    sample_diagnostics(m2, xn)
    assert m2.diagnostics_report_["x_reads"] == [3] and m2.diagnostics_report_["training_stats"] == "computed"
    dn = sample_diagnostics(m2, xn)
    rep = m2.diagnostics_report_
    assert rep["x_reads"] == [2] and rep["training_stats"] == "cached", rep
    assert rep["form"] == "projection (one-pass MTTKRP (one read, nothing written)) + residual pass", rep
    assert torch.equal(xd, before) and torch.equal(xn, xn_before)
    assert np.array_equal(dn["scores"], m2.transform(xn))
    np.testing.assert_allclose(d["t2"].sum(), 4 * 299, rtol=1e-9)


def test_more_than_16_components_fall_back_with_a_reason():
    x, y, _ = O.import_synthetic((80, 9, 8), 3, 3, error=0.2, seed=6)
    m = tPLS(17, dtype="float64")
    m.fit(x, y)
    d = sample_diagnostics(m)
    rep = m.diagnostics_report_
    assert rep["form"] == "torch fallback" and "16" in rep["why"], rep
    ref = sample_diagnostics(m, device=False)
    np.testing.assert_allclose(d["spe"], ref["spe"], rtol=1e-12)
    np.testing.assert_allclose(d["spe"].sum() / d["ssq"].sum(), 1 - m.R2X[-1], rtol=1e-9)
