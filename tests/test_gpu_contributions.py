"""Contribution plots on the device (validate.sample_contributions, cmtf_pls_amd/contributions.py): cmtfpls_contrib_rows_* against
a float64 torch formula (storage types, unaligned shapes, many rows, R 1 / 10 / 16, a row list, the LDS limit, a NaN score row,
bit-identical repeats, X untouched, the R = 17 and LDS declines; both sides of every register-chunk boundary, mean = NULL and a
misaligned mean, row indices outside X, the rows per workgroup halved by LDS pressure and five rows per workgroup, each with the
plan restated in tests/resid_rows_ref.py asserted), then the estimator on the HIP backend against the float64 NumPy
restatement (tests/contributions_ref.py), its report and its agreement with the torch form.

Tolerances.  The squared sums (speA, speB) are sums of non-negative terms: the project's rtol=1e-11, atol=1e-9 for such sums
(test_gpu_diagnostics.py).  The signed T^2 sums cancel, so they are held to the float64 accumulation bound instead:
|got - want| <= 1e-11 |want| + n_terms 2^-53 sum|d_ic|, sum|d_ic| over the cells of that sum taken from the formula, and n_terms =
the cells in the sum + R + 2 (every d is itself an R-term dot product, a centring and a product)."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.backend import HipBackend
from cmtf_pls_amd.validate import sample_contributions
from contributions_ref import check, contributions
from resid_rows_ref import CONTRIB_LDS_CASES, CONTRIB_ODD_G, contrib_g_start, contrib_plan, vec_width

pytestmark = pytest.mark.gpu


def _formula(X2, T, H, WA, WB, mean, rows=None):
    A, B = WA.shape[0], WB.shape[0]
    x = (X2 if rows is None else X2[rows]).double() - mean
    W = (WA[:, None, :] * WB[None, :, :]).reshape(A * B, -1)
    fin = torch.isfinite(x)
    e2 = torch.where(fin, x - T @ W.T, 0.0).square().view(-1, A, B)
    d = torch.where(fin, x * (H @ W.T), 0.0).view(-1, A, B)
    return e2.sum(2), e2.sum(1), d.sum(2), d.sum(1), d.abs().sum(2), d.abs().sum(1)


def _operands(I, A, B, R, dtype, seed, offset=0, nan_frac=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    P = A * B
    flat = torch.randn(I * P + offset, generator=g, dtype=torch.float64)
    if nan_frac:
        flat[torch.rand(flat.shape, generator=g) < nan_frac] = float("nan")
    X2 = flat.to("cuda", dtype)[offset:].view(I, P)
    T = torch.randn(I, R + 3, generator=g, dtype=torch.float64).cuda()[:, :R]       # a row stride > R
    H = torch.randn(I, R, generator=g, dtype=torch.float64).cuda()
    WA = torch.randn(A, R, generator=g, dtype=torch.float64).cuda()
    WB = torch.randn(B, R, generator=g, dtype=torch.float64).cuda()
    mean = torch.randn(P, generator=g, dtype=torch.float64).cuda()
    return X2, T, H, WA, WB, mean


def _check_kernel(got, want, A, B, R, label):
    speA, speB, t2A, t2B = got
    wA, wB, dA, dB, absA, absB = want
    if A == 1:
        assert speA is None and t2A is None
    else:
        torch.testing.assert_close(speA, wA, rtol=1e-11, atol=1e-9)
    torch.testing.assert_close(speB, wB, rtol=1e-11, atol=1e-9)
    for name, g, w, ab, cells in (("t2A", t2A, dA, absA, B), ("t2B", t2B, dB, absB, A)):
        if g is None:
            continue
        bound = 1e-11 * w.abs() + (cells + R + 2) * 2.0 ** -53 * ab
        err = (g - w).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{label} {name}: worst |got - want| / bound = {worst:.3g}")
        assert bool((err <= bound).all()), (label, name, worst)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("I,A,B,R,offset,nan", [
    (1, 3, 8, 1, 0, 0.0),                  # one row, R = 1
    (5000, 4, 12, 10, 0, 0.1),             # many row groups of 3 rows, missing values
    (300, 5, 7, 16, 0, 0.0),               # B % 4 != 0: one element per thread; R = 16
    (257, 6, 8, 10, 1, 0.05),              # a view one element into its storage: misaligned base
    (64, 1, 1030, 10, 0, 0.0),             # a matrix block, columns past a whole tile
    (3000, 8, 160, 10, 0, 0.02),           # 40 / 80 vectors per slice: dead lanes in the slice of 64
    (70, 9, 520, 10, 0, 0.02),             # B past one chunk of 64 vectors: the A sums accumulate over chunks
    (40, 300, 4, 5, 0, 0.0),               # a long first mode, one vector per slice
    (20003, 16, 16, 10, 0, 0.0),           # 8 rows per workgroup, a ragged last group
])
def test_contrib_rows_kernel_against_formula(dtype, I, A, B, R, offset, nan):
    be = HipBackend()
    X2, T, H, WA, WB, mean = _operands(I, A, B, R, dtype, seed=I + R, offset=offset, nan_frac=nan)
    before = X2.clone()
    got = be.contrib_rows(X2, T, H, WA, WB, mean)
    _check_kernel(got, _formula(X2, T, H, WA, WB, mean), A, B, R, f"{dtype} {(I, A, B, R)}")
    again = be.contrib_rows(X2, T, H, WA, WB, mean)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, again))      # deterministic: the same bits
    bits = torch.int32 if dtype == torch.float32 else torch.int64
    assert torch.equal(X2.view(bits), before.view(bits))                                       # read only


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_contrib_rows_row_list(dtype):
    be = HipBackend()
    X2, T, H, WA, WB, mean = _operands(500, 6, 20, 10, dtype, seed=11, nan_frac=0.05)
    rows = torch.randperm(500, generator=torch.Generator().manual_seed(2))[:77].cuda()
    Ts, Hs = T[:77], H[:77].contiguous()
    got = be.contrib_rows(X2, Ts, Hs, WA, WB, mean, rows=rows)
    _check_kernel(got, _formula(X2, Ts, Hs, WA, WB, mean, rows=rows), 6, 20, 10, f"{dtype} row list")
    sub = be.contrib_rows(X2[rows].contiguous(), Ts, Hs, WA, WB, mean)
    assert all(torch.equal(a, b) for a, b in zip(got, sub))


def test_contrib_rows_at_the_lds_limit_and_declines():
    be = HipBackend()
    # one row per workgroup: (2 A R + 2 A + 512 V) doubles; f32 vectors (V = 4), R = 16: A = 542 is the last shape that fits 160 KB
    X2, T, H, WA, WB, mean = _operands(6, 542, 4, 16, torch.float32, seed=5)
    _check_kernel(be.contrib_rows(X2, T, H, WA, WB, mean), _formula(X2, T, H, WA, WB, mean), 542, 4, 16, "LDS limit")
    X2, T, H, WA, WB, mean = _operands(6, 543, 4, 16, torch.float32, seed=6)
    assert be.contrib_rows(X2, T, H, WA, WB, mean) is None
    X2, T, H, WA, WB, mean = _operands(40, 4, 8, 17, torch.float32, seed=4)
    assert be.contrib_rows(X2, T, H, WA, WB, mean) is None


def test_contrib_rows_nan_score_row():
    be = HipBackend()
    X2, T, H, WA, WB, mean = _operands(40, 4, 8, 10, torch.float32, seed=3)
    T = T.contiguous()
    T[7] = float("nan")
    H[9] = float("nan")
    speA, speB, t2A, t2B = be.contrib_rows(X2, T, H, WA, WB, mean)
    other = torch.arange(40, device="cuda")
    assert torch.isnan(speA[7]).all() and torch.isnan(speB[7]).all() and not torch.isnan(speA[other != 7]).any()
    assert not torch.isnan(speB[other != 7]).any() and not torch.isnan(t2A[7]).any()
    assert torch.isnan(t2A[9]).all() and torch.isnan(t2B[9]).all() and not torch.isnan(t2B[other != 9]).any()


def _vec(dtype, B):
    return vec_width("f32" if dtype == torch.float32 else "f64", B)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("I,A,B", [(300, 5, 7), (257, 6, 8)])      # one element per thread; vector loads
def test_contrib_rows_register_chunk_boundaries(dtype, I, A, B):
    """R on both sides of 4 | 5, 8 | 9 and 12 | 13 (R = 5 and 16 run above): the chunks of 4, 8, 12 and 16 registers each at their
    last width and the next chunk at its first."""
    be = HipBackend()
    for R in (4, 8, 9, 12, 13):
        X2, T, H, WA, WB, mean = _operands(I, A, B, R, dtype, seed=I + R, nan_frac=0.05)
        got = be.contrib_rows(X2, T, H, WA, WB, mean)
        _check_kernel(got, _formula(X2, T, H, WA, WB, mean), A, B, R, f"{dtype} {(I, A, B)} R = {R}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_contrib_rows_without_a_mean_and_with_a_misaligned_one(dtype):
    """mean = NULL, and a mean one double into its storage while X is 16-byte aligned: the kernel then has to take the
    one-element path (a vector load of the mean would be misaligned).  Both against the formula; the run with the same mean
    aligned meets the same bounds."""
    be = HipBackend()
    I, A, B, R = 257, 6, 8, 10
    X2, T, H, WA, WB, mean = _operands(I, A, B, R, dtype, seed=31, nan_frac=0.05)
    assert X2.data_ptr() % 16 == 0 and mean.data_ptr() % 16 == 0 and _vec(dtype, B) > 1
    got = be.contrib_rows(X2, T, H, WA, WB, None)
    _check_kernel(got, _formula(X2, T, H, WA, WB, torch.zeros_like(mean)), A, B, R, f"{dtype} mean = NULL")
    buf = torch.zeros(A * B + 1, dtype=torch.float64, device="cuda")
    buf[1:] = mean
    shifted = buf[1:]
    assert shifted.data_ptr() % 16 == 8 and torch.equal(shifted, mean)
    want = _formula(X2, T, H, WA, WB, mean)
    one = be.contrib_rows(X2, T, H, WA, WB, shifted)
    _check_kernel(one, want, A, B, R, f"{dtype} misaligned mean")
    _check_kernel(be.contrib_rows(X2, T, H, WA, WB, mean), want, A, B, R, f"{dtype} aligned mean")
    assert all(torch.equal(a, b) for a, b in zip(one, be.contrib_rows(X2, T, H, WA, WB, shifted)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_contrib_rows_row_indices_outside_x(dtype):
    """Row indices -1 and I among valid ones: NaN in all four outputs of those rows (the guard is in the kernel, the backend
    passes the list through), every other row as the formula."""
    be = HipBackend()
    I, A, B, R, n = 50, 6, 20, 10, 23
    X2, T, H, WA, WB, mean = _operands(I, A, B, R, dtype, seed=41, nan_frac=0.05)
    rows = torch.randperm(I, generator=torch.Generator().manual_seed(3))[:n]
    bad = [0, 4, 11, n - 1]                                          # the first and last row of the list among them
    rows[bad] = torch.tensor([-1, I, I + 7, -(2 ** 40)])
    Ts, Hs = T[:n], H[:n].contiguous()
    got = be.contrib_rows(X2, Ts, Hs, WA, WB, mean, rows=rows.cuda())
    good = torch.ones(n, dtype=torch.bool)
    good[bad] = False
    assert all(bool(torch.isnan(g[bad]).all()) and not bool(torch.isnan(g[good]).any()) for g in got)
    g = good.cuda()
    want = _formula(X2, Ts[g], Hs[g], WA, WB, mean, rows=rows[good].cuda())
    _check_kernel(tuple(t[g] for t in got), want, A, B, R, f"{dtype} row indices outside X")


@pytest.mark.parametrize("case,plan", CONTRIB_LDS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_contrib_rows_group_halved_by_lds_pressure(case, plan):
    """16385 row indices into an X of 64 rows: 8 rows per workgroup wanted, halved until TH + accumulators + slab fit 160 KB."""
    be = HipBackend()
    n, A, B, R, st = case
    g_start, G, lg = plan
    assert contrib_g_start(n) == g_start == 8 and contrib_plan(n, R, A, B, vec_width(st, B))[:2] == (G, lg) and G < g_start
    assert contrib_plan(n, R, A, B, vec_width(st, B))[3] and n % G == 1 % G                      # a ragged last group where G > 1
    X2, _, _, WA, WB, mean = _operands(64, A, B, R, torch.float32, seed=51 + R, nan_frac=0.02)
    g = torch.Generator(device="cpu").manual_seed(52)
    rows = torch.randint(0, 64, (n,), generator=g).cuda()
    T = torch.randn(n, R, generator=g, dtype=torch.float64).cuda()
    H = torch.randn(n, R, generator=g, dtype=torch.float64).cuda()
    got = be.contrib_rows(X2, T, H, WA, WB, mean, rows=rows)
    _check_kernel(got, _formula(X2, T, H, WA, WB, mean, rows=rows), A, B, R, f"LDS pressure {case} G = {G}")
    again = be.contrib_rows(X2, T, H, WA, WB, mean, rows=rows)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case,plan", CONTRIB_ODD_G)
def test_contrib_rows_with_five_rows_per_workgroup(dtype, case, plan):
    """G = 5, not a power of two: 9000 rows are 1800 whole groups, 9001 leave a last group of one row."""
    be = HipBackend()
    n, A, B, R = case
    G, last = plan
    assert contrib_plan(n, R, A, B, _vec(dtype, B))[0] == G == 5 and n - (-(-n // G) - 1) * G == last
    X2, T, H, WA, WB, mean = _operands(n, A, B, R, dtype, seed=n, nan_frac=0.02)
    got = be.contrib_rows(X2, T, H, WA, WB, mean)
    _check_kernel(got, _formula(X2, T, H, WA, WB, mean), A, B, R, f"{dtype} {case} G = 5")
    again = be.contrib_rows(X2, T, H, WA, WB, mean)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


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
        xm[np.random.default_rng(seed + 3).random(xm.shape) < nan] = np.nan
        m = ctPLS(R, dtype=dtype)
        m.fit([x, xm], y)
        return m, [x, xm]
    m = tPLS(R, dtype=dtype)
    m.fit(x, y)
    return m, x


@pytest.mark.parametrize("dtype,rtol", [("float64", 1e-9), ("float32", 1e-5)])
@pytest.mark.parametrize("shape,R,nan,coupled", [
    ((60, 12), 3, 0.0, False),
    ((50, 8, 6), 1, 0.0, False),
    ((50, 8, 6), 3, 0.1, False),
    ((40, 5, 4, 3), 3, 0.0, False),
    ((45, 7, 6), 3, 0.1, True),
])
def test_estimator_against_restatement(dtype, rtol, shape, R, nan, coupled):
    m, X = _fit(shape, R, dtype, nan, coupled=coupled)
    nb = 2 if coupled else 1
    c = sample_contributions(m)
    rep = m.contributions_report_
    assert rep["form"] == ["contribution pass (cmtfpls_contrib_rows)"] * nb and rep["x_reads"] == [1] * nb and rep["why"] == [None] * nb, rep
    check(c, contributions(m, train=X), coupled, rtol)
    xn = O.import_synthetic((shape[0] // 2,) + shape[1:], 3, 3, error=0.2, seed=9)[0]
    if dtype == "float32":
        xn = xn.astype(np.float32).astype(np.float64)
    if nan:
        xn[np.random.default_rng(5).random(xn.shape) < nan] = np.nan
    Xn = [xn, (X[1][: xn.shape[0]] + 0.05)] if coupled else xn
    rows = np.random.default_rng(3).permutation(xn.shape[0])[:11]
    cn = sample_contributions(m, Xn, rows=rows)
    assert np.array_equal(cn["scores"], m.transform(Xn)[rows]) and m.contributions_report_["rows"] == 11
    check(cn, contributions(m, Xn, rows=rows), coupled, rtol)
    # the device form against the torch form of the same call: the kernel tolerances
    ct = sample_contributions(m, Xn, rows=rows, device=False)
    assert m.contributions_report_["form"] == ["torch fallback"] * nb and "switched off" in m.contributions_report_["why"][0]
    lst = (lambda v: v) if coupled else (lambda v: [v])
    full = contributions(m, Xn, rows=rows)
    for b in range(nb):
        absd = lst(full["abs_d"])[b]
        for k, (g, w) in enumerate(zip(lst(cn["spe_mode"])[b], lst(ct["spe_mode"])[b])):
            np.testing.assert_allclose(g, w, rtol=1e-11, atol=1e-9)
        P = int(np.prod([a.shape[1] for a in lst(cn["spe_mode"])[b]]))
        for g, w in zip(lst(cn["t2_mode"])[b], lst(ct["t2_mode"])[b]):
            terms = P // g.shape[1] + R + 2                  # the cells behind one entry of this mode, then as in the kernel test
            assert (np.abs(g - w) <= 1e-11 * np.abs(w) + terms * 2.0 ** -53 * absd[:, None]).all()


def test_report_read_counts_and_read_only():
    x, y, _ = O.import_synthetic((300, 16, 12), 3, 3, error=0.2, seed=4)
    xd = torch.from_numpy(x).float().cuda()
    m = tPLS(4, dtype="float32")
    m.fit(xd, y)
    before = xd.clone()
    sample_contributions(m, rows=[5, 1])
    rep = m.contributions_report_
    assert rep["x_reads"] == [1] and rep["training_stats"] == "computed" and rep["training_reads"] == 1 and rep["rows"] == 2, rep
    xn = torch.from_numpy(O.import_synthetic((100, 16, 12), 3, 3, error=0.2, seed=5)[0]).float().cuda()
    xn_before = xn.clone()
    c = sample_contributions(m, xn)
    rep = m.contributions_report_
    assert rep["x_reads"] == [2] and rep["training_stats"] == "cached" and rep["projection"].startswith("one-pass MTTKRP"), rep
    assert torch.equal(xd, before) and torch.equal(xn, xn_before)
    assert np.array_equal(c["scores"], m.transform(xn))


def test_more_than_16_components_fall_back_with_a_reason():
    x, y, _ = O.import_synthetic((80, 9, 8), 3, 3, error=0.2, seed=6)
    m = tPLS(17, dtype="float64")
    m.fit(x, y)
    c = sample_contributions(m)
    rep = m.contributions_report_
    assert rep["form"] == ["torch fallback"] and "16" in rep["why"][0], rep
    check(c, contributions(m, train=x), False, 1e-9)
